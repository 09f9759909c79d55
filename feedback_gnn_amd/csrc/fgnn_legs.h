// fgnn_legs.h — the leg / stop / weight control of relay_kernel (fgnn_relay.hip) and relay4_kernel (fgnn_relay4.hip), stated once.
// A codeword walks legs r = 0 .. num_legs - 1; leg r runs up to T = pre_iter (r = 0) or leg_iter check updates, the decision is
// tested after every update and a test that passes ends the leg with a solution; the codeword ends with the leg in which it has
// stop_nconv solutions, or with the last leg.  A leg takes T + 1 workgroup steps at the most, k = 0 .. T counting its finished check
// updates, as an attempt of fgnn_attempts.h does; the step bound is attempt_step_bound(pre_iter, num_legs - 1, leg_iter).
//
// Solutions are compared by weight, and a weight is a sum over the threads of a codeword: it is started in the control section of
// the step that tested the decision (integer atomics into wacc[cw], LegCtl::weighed) and complete one barrier interval later, where
// settle() takes the running total and, where that decision is the codeword's output so far, has the kernel write it.  The first solution is taken, a
// later one only if strictly lighter; the last test of a codeword that found none is weighed too, and is then its output.  The
// kernel's decision buffer still holds the weighed decision when it settles: a test that is weighed ends its leg, and a leg's first
// step (k = 0) decides nothing.
//
// A step of the two kernels, with their own phases in brackets:
//   T() -> [qubit or bit phase] -> barrier -> pending ? settle(wacc[cw], [write the decision]) -> stats_due() ? stats() ->
//   break if every codeword is done -> [check phase: stamp[cw] = step on odd parity] -> barrier ->
//   k == 0 ? more() : { t = test(sat); t.weigh ? [weigh into wacc[cw]], weighed(); t.fin ? finish(), ++ndone : t.leg_end ? next_leg() : more() }
// The branches on k == 0, on weigh and on fin / leg_end stay in the kernels, around members that have none, as fgnn_attempts.h
// keeps its three for the reason given there; settle's one branch encloses the kernel's write, so that the three assignments and
// the write stay one region.  In this form the control sections branch as they did before the two kernels shared them.
// Host and device: tests/leg_ctl_check.cpp walks the control on the CPU.
// gdg_kernel (fgnn_gdg.hip) runs the same control with a decimation round as a leg: max_rounds + 1 legs, stop_nconv = 1, and the pick
// of the bit to fix where next_leg() is called.  It adds nothing here.
#ifndef FGNN_LEGS_H
#define FGNN_LEGS_H

#include <stdint.h>

#include "fgnn_attempts.h"

struct LegSched {
    int pre_iter, num_legs, leg_iter, stop_nconv;
};

// the ints a workgroup keeps behind its cpb codewords (leg_stage of fgnn_step.h lays them out): stamp[cpb], wacc[cpb], ndone
//   stamp[cw]  the number of the last workgroup step in which a check of the codeword saw odd parity (no reset needed)
//   wacc[cw]   running total of the weights of the decisions weighed so far (integer atomics; a thread keeps the previous total)
//   ndone      finished codewords; read by all threads in the same interval, so leaving the loop is a uniform decision
FG_FN int leg_lds_words(const int cpb) { return 2 * cpb + 1; }

// what the test of a step means for its codeword
struct LegTest {
    bool leg_end, fin, weigh;
};

// Where a codeword stands, in registers every thread of the codeword holds identically: leg r, k finished check updates of it,
// `found` solutions, the best of them (or the last test made) as weight, leg and k, the previous total of wacc[cw], and the test
// whose weight is under way (pend_r, pend_k, pending)
struct LegCtl {
    int r, k, found, best_w, best_r, best_k, wprev, pend_r, pend_k;
    bool done, written, pending;
    FG_METHOD explicit LegCtl(const bool active)
        : r(0), k(0), found(0), best_w(0), best_r(0), best_k(0), wprev(0), pend_r(0), pend_k(0), done(!active), written(!active), pending(false)
    {
    }
    // check updates of the current leg
    FG_METHOD int T(const LegSched& s) const { return (r == 0) ? s.pre_iter : s.leg_iter; }
    // with `pending`, after the barrier that completed the weight: total = wacc[cw].  Where the weighed decision is the best so far
    // (the first solution, a strictly lighter one, or the last test of a codeword without one) it becomes the output: write() is the
    // kernel's write of its decision buffer
    template <typename WRITE>
    FG_METHOD void settle(const int total, WRITE write)
    {
        const int w = total - wprev;
        wprev = total;
        if (found <= 1 || w < best_w) {
            best_w = w;
            best_r = pend_r;
            best_k = pend_k;
            write();
        }
        pending = false;
    }
    // the four stats words of a codeword, written once, in the step after its last: its last weight has settled by then
    FG_METHOD bool stats_due()
    {
        if (!done || written) return false;
        written = true;
        return true;
    }
    FG_METHOD void stats(int32_t* st) const
    {
        st[0] = found;
        st[1] = best_w;
        st[2] = best_r;
        st[3] = best_k;
    }
    // after the check phase of a step that tested (k > 0), sat: no check saw odd parity.  A solution ends the leg, as its last test
    // does; the leg's end is the codeword's in the last leg or with stop_nconv solutions; weighed are a solution and the last test
    // of a codeword that found none
    FG_METHOD LegTest test(const LegSched& s, const int T, const bool sat)
    {
        LegTest t;
        t.leg_end = sat || k == T;
        if (sat) ++found;
        t.fin = t.leg_end && (r == s.num_legs - 1 || found == s.stop_nconv);
        t.weigh = sat || (t.fin && found == 0);
        return t;
    }
    // the kernel has started this test's weight
    FG_METHOD void weighed()
    {
        pending = true;
        pend_r = r;
        pend_k = k;
    }
    FG_METHOD void finish() { done = true; }
    FG_METHOD void next_leg() { ++r; k = 0; }
    FG_METHOD void more() { ++k; }
};

#endif
