// fgnn_attempts.h — the attempt schedule of mbp4_kernel (fgnn_mbp4.hip), dsbp4_kernel (fgnn_dsbp4.hip) and stbp4_kernel
// (fgnn_stbp4.hip), stated once.  A codeword walks attempts r = 0 .. attempts - 1; attempt r runs up to T = pre_iter (r = 0) or
// attempt_iter check updates with factor[r] and own[r], the hard decision is tested after every update and the first test that
// passes ends the codeword; a restarting attempt starts from zero messages.  An attempt takes T + 1 workgroup steps, k = 0 .. T
// counting its finished check updates: step k = 0 sends the first messages, step k > 0 tests the decision after k updates and, for
// k < T, runs update k + 1.  Host and device (FG_FN), like fgnn_cn.h: tests/attempt_ctl_check.cpp walks the control on the CPU
// against the step bound below.
#ifndef FGNN_ATTEMPTS_H
#define FGNN_ATTEMPTS_H

#include "fgnn_math.h"

#if defined(__HIPCC__)
#define FG_METHOD __device__ __host__ __forceinline__
#else
#define FG_METHOD inline __attribute__((always_inline))
#endif

constexpr int ATTEMPT_MAX = 64;

struct AttemptSched {
    int pre_iter, attempt_iter, attempts, restart;
    float tab[2 * ATTEMPT_MAX];  // factor[0..63], own[0..63]; entries from `attempts` on are 0 and never read
};

// The steps a step loop must be given: a run (attempt, round, leg) of T check updates takes T + 1 steps, the first run has pre_iter
// updates and `later` more (attempts - 1 here) have `iter`; one more step lets the workgroup see its last codeword finished.
// Saturates below INT_MAX, so that `step <= bound` ends.
FG_FN int attempt_step_bound(int pre_iter, long long later, int iter)
{
    const long long steps = (long long)pre_iter + 1 + later * ((long long)iter + 1) + 1;
    return (int)(steps < INT32_MAX - 1 ? steps : INT32_MAX - 1);
}

// Where a codeword stands: attempt r, k finished check updates of it, `its` check updates in all.  r < attempts <= ATTEMPT_MAX
// throughout: the last attempt ends the codeword.  A step of the kernels is
//   T(), zero() -> qubit phase -> barrier -> break if every codeword is done -> check phase -> barrier ->
//   k == 0 ? more() : test passed || last() ? outputs : k == T ? again() : more()
struct AttemptCtl {
    int r, k, its;
    bool done;
    FG_METHOD explicit AttemptCtl(const bool active) : r(0), k(0), its(0), done(!active) {}
    // check updates of the current attempt
    FG_METHOD int T(const AttemptSched& s) const { return (r == 0) ? s.pre_iter : s.attempt_iter; }
    // this step's qubit phase starts a restarting attempt: from zero messages
    FG_METHOD bool zero(const AttemptSched& s) const { return s.restart && k == 0 && r > 0; }
    // after the check phase of a step that tested (k > 0): the test was the last of the last attempt.  The codeword is over when
    // the test passed or last(); r, its and k are then its stats words
    FG_METHOD bool last(const AttemptSched& s, const int T) const { return k == T && r == s.attempts - 1; }
    // else one more check update is done (also after an attempt's first step, k = 0, which tests nothing), or, at k == T, the
    // attempt is over and the next begins.  The branches on k == 0, on the test and on k == T stay in the kernels: folded into
    // one member (ends(sat), next(T)) they compile to selects there, and two (3,3,6) instantiations measured slower than before
    FG_METHOD void more() { ++k; ++its; }
    FG_METHOD void again() { ++r; k = 0; }
};

#endif
