/* Host walk of the attempt schedule of feedback_gnn_amd/csrc/fgnn_attempts.h (host code, no GPU; built and run by
 * tests/test_attempt_schedule_cpu.py, once plain and once under the address and undefined-behaviour sanitizers).  For every
 * pre_iter, attempt_iter and attempts in 1 .. 4, restart in {0, 1}, and every test (a, k) at which the decision first reproduces the
 * syndrome (k in 1 .. T_a), and for "never" (a = -1), one codeword is walked through AttemptCtl exactly as the step loop of
 * mbp4_kernel, dsbp4_kernel and stbp4_kernel walks it, up to attempt_step_bound: qubit phase, break test on ndone, check phase,
 * control.  First line: the bound at pre_iter = attempt_iter = INT_MAX, attempts = 64.  Then one line per case:
 *   pre_iter attempt_iter attempts restart a k | found r its k | the step at which the codeword finished (0: never), the step at which
 *   the loop saw ndone complete (0: never), the bound | the steps whose qubit phase zeroed the messages */
#include <limits.h>
#include <stdio.h>

#include "fgnn_attempts.h"

static void walk(const int pre_iter, const int attempt_iter, const int attempts, const int restart, const int sa, const int sk)
{
    AttemptSched s = {};
    s.pre_iter = pre_iter;
    s.attempt_iter = attempt_iter;
    s.attempts = attempts;
    s.restart = restart;
    for (int i = 0; i < attempts; ++i) s.tab[i] = s.tab[ATTEMPT_MAX + i] = 1.0f;
    const int bound = attempt_step_bound(pre_iter, attempts - 1, attempt_iter), nact = 1;
    int stamp = 0, ndone = 0, stats[4] = {-1, -1, -1, -1}, finished = 0, seen = 0, zeroed[64], nz = 0;
    float used = 0.0f;
    AttemptCtl ctl(true);
    for (int step = 1; step <= bound; ++step) {
        const int T = ctl.T(s), k = ctl.k;
        if (!ctl.done) {  // qubits
            if (ctl.zero(s)) zeroed[nz++] = step;
            used += s.tab[ATTEMPT_MAX + ctl.r];
        }
        if (ndone == nact) {
            seen = step;
            break;
        }
        if (!ctl.done) {  // checks: a test (k > 0) sees odd parity unless it is the chosen one
            used += s.tab[ctl.r];
            if (k > 0 && !(ctl.r == sa && k == sk)) stamp = step;
        }
        if (!ctl.done) {  // control
            if (k == 0) {
                ctl.more();
            } else {
                const bool sat = stamp != step;
                if (sat || ctl.last(s, T)) {
                    stats[0] = sat ? 1 : 0;
                    stats[1] = ctl.r;
                    stats[2] = ctl.its;
                    stats[3] = k;
                    finished = step;
                    ++ndone;
                    ctl.done = true;
                } else if (k == T) {
                    ctl.again();
                } else {
                    ctl.more();
                }
            }
        }
    }
    printf("%d %d %d %d %d %d | %d %d %d %d | %d %d %d |", pre_iter, attempt_iter, attempts, restart, sa, sk, stats[0], stats[1], stats[2],
           stats[3], finished, seen, bound);
    for (int i = 0; i < nz; ++i) printf(" %d", zeroed[i]);
    printf("%s\n", used > 0.0f ? "" : " unused");
}

int main()
{
    printf("%d\n", attempt_step_bound(INT_MAX, ATTEMPT_MAX - 1, INT_MAX));
    for (int pre_iter = 1; pre_iter <= 4; ++pre_iter)
        for (int attempt_iter = 1; attempt_iter <= 4; ++attempt_iter)
            for (int attempts = 1; attempts <= 4; ++attempts)
                for (int restart = 0; restart <= 1; ++restart) {
                    for (int a = 0; a < attempts; ++a)
                        for (int k = 1; k <= (a == 0 ? pre_iter : attempt_iter); ++k) walk(pre_iter, attempt_iter, attempts, restart, a, k);
                    walk(pre_iter, attempt_iter, attempts, restart, -1, 0);
                }
    return 0;
}
