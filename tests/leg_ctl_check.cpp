/* Host walk of the leg control of feedback_gnn_amd/csrc/fgnn_legs.h (host code, no GPU; built and run by tests/test_leg_control_cpu.py,
 * once plain and once under the address and undefined-behaviour sanitizers).  For every pre_iter, leg_iter and num_legs in 1 .. 3,
 * stop_nconv in 1 .. 3, every plan of which tests (r, k) pass (bit t of `plan`: test t in the order leg 0: k = 1 .. pre_iter, leg 1:
 * k = 1 .. leg_iter, ..) and each of the weight rows below, one codeword is walked through LegCtl exactly as the step loops of
 * relay_kernel and relay4_kernel walk it, up to attempt_step_bound: qubit phase, settle, late stats, break on ndone, check phase,
 * control.  A decision is named by its test: the qubit phase of a step with k > 0 leaves test (r, k)'s decision in the buffer, and
 * what a settle writes out is whatever the buffer holds then.  First line: the bound at pre_iter = leg_iter = num_legs = INT_MAX.
 * Then one line per case:
 *   pre_iter leg_iter num_legs stop_nconv plan row | found best_w best_r best_k | the step at which the codeword finished (0: never),
 *   at which its stats were written, at which the loop saw ndone complete, the bound | the tests written out, in order, as r.k */
#include <limits.h>
#include <stdio.h>

#include "fgnn_attempts.h"
#include "fgnn_legs.h"

/* weights of tests 0 .. 8: ties, a strictly smaller later weight, a larger later weight, and a mix with zeros (no atomic is issued
 * for a weight of 0) and negative weights */
static const int WEIGHTS[4][9] = {{4, 4, 4, 4, 4, 4, 4, 4, 4}, {9, 8, 7, 6, 5, 4, 3, 2, 1}, {1, 2, 3, 4, 5, 6, 7, 8, 9}, {3, 0, 3, -2, 0, 5, -2, 3, 0}};

static int test_index(const LegSched& s, const int r, const int k) { return r == 0 ? k - 1 : s.pre_iter + (r - 1) * s.leg_iter + k - 1; }

static void walk(const LegSched& s, const unsigned plan, const int row)
{
    const int bound = attempt_step_bound(s.pre_iter, s.num_legs - 1, s.leg_iter), nact = 1;
    int stamp[1] = {0}, wacc[1] = {0}, ndone = 0, finished = 0, stats_at = 0, seen = 0, held_r = -1, held_k = -1, out[16][2], nout = 0;
    int32_t stats[4] = {-1, -1, -1, -1};
    LegCtl ctl(true);
    for (int step = 1; step <= bound; ++step) {
        const int T = ctl.T(s), r = ctl.r, k = ctl.k;
        if (!ctl.done && k > 0) {  // qubits: the decision after k check updates
            held_r = r;
            held_k = k;
        }
        if (ctl.pending)
            ctl.settle(wacc[0], [&] {
                out[nout][0] = held_r;
                out[nout++][1] = held_k;
            });
        if (ctl.stats_due()) {
            ctl.stats(stats);
            stats_at = step;
        }
        if (ndone == nact) {
            seen = step;
            break;
        }
        if (!ctl.done)  // checks: a test (k > 0) sees odd parity unless the plan lets it pass
            if (k > 0 && !((plan >> test_index(s, r, k)) & 1u)) stamp[0] = step;
        if (!ctl.done) {  // control
            if (k == 0) {
                ctl.more();
            } else {
                const LegTest t = ctl.test(s, T, stamp[0] != step);
                if (t.weigh) {
                    const int part = WEIGHTS[row][test_index(s, r, k)];
                    if (part) wacc[0] += part;
                    ctl.weighed();
                }
                if (t.fin) {
                    ctl.finish();
                    finished = step;
                    ++ndone;
                } else if (t.leg_end) {
                    ctl.next_leg();
                } else {
                    ctl.more();
                }
            }
        }
    }
    printf("%d %d %d %d %u %d | %d %d %d %d | %d %d %d %d |", s.pre_iter, s.leg_iter, s.num_legs, s.stop_nconv, plan, row, stats[0], stats[1],
           stats[2], stats[3], finished, stats_at, seen, bound);
    for (int i = 0; i < nout; ++i) printf(" %d.%d", out[i][0], out[i][1]);
    printf("\n");
}

int main()
{
    printf("%d\n", attempt_step_bound(INT_MAX, (long long)INT_MAX - 1, INT_MAX));
    for (int pre_iter = 1; pre_iter <= 3; ++pre_iter)
        for (int leg_iter = 1; leg_iter <= 3; ++leg_iter)
            for (int num_legs = 1; num_legs <= 3; ++num_legs)
                for (int stop_nconv = 1; stop_nconv <= 3; ++stop_nconv) {
                    const LegSched s = {pre_iter, num_legs, leg_iter, stop_nconv};
                    const int tests = pre_iter + (num_legs - 1) * leg_iter;
                    for (unsigned plan = 0; plan < (1u << tests); ++plan)
                        for (int row = 0; row < 4; ++row) walk(s, plan, row);
                }
    return 0;
}
