// fgnn_cn1.h — the single-output form of the check-node rules of fgnn_cn.h, for schedules that are serial along qubits
// (fgnn_mbp4_serial.hip): the qubit at the end of edge e asks for the one message its check would send it now, and the check's other
// slots must stay as they are.
//
// cn_output<CN_TYPE, PHI>(nu, slot, deg, j, synd, factor) returns the bits cn_update<CN_TYPE, PHI>(nu, slot, deg, synd, factor) writes
// to slot[j], and writes nothing.  It is the same float operation sequence: every loop of the rule runs over all deg inputs in the
// rule's order, what cn_update parks in a slot between its passes (the signed |.| of the phi and min-sum rules, the tanh of the boxplus
// rule) is formed again where pass 2 reads it, and only output j is evaluated.  A check of degree d therefore costs d evaluations of
// pass 1 where cn_update costs one: that is the price of the schedule, not of this form.
//
// Host and device (FG_FN): tests/cn_output_check.cpp compares it with cn_update on the CPU, output by output.
#ifndef FGNN_CN1_H
#define FGNN_CN1_H

#include "fgnn_cn.h"

template <int CN_TYPE, typename PHI>
FG_FN float cn_output(const float* nu, const int* __restrict__ slot, int deg, int j, unsigned synd, float factor)
{
    if constexpr (CN_TYPE == FGNN_CN_BOXPLUS_PHI) {
        unsigned neg = synd;
        float T = 0.0f;
        float w = 0.0f;  // what cn_update parks in slot[j]
        for (int i = 0; i < deg; ++i) {
            const float v = nu[slot[i]];
            const unsigned ng = v < 0.0f;
            neg ^= ng;
            const float a = PHI::phi(FG_ABS(v));
            T = T + a;
            if (i == j) w = with_sign(a, ng);
        }
        const float out = PHI::phi(T - FG_ABS(w));
        return with_sign(out, neg ^ sign_bit(w)) * factor;
    } else if constexpr (CN_TYPE == FGNN_CN_MINSUM) {
        const float LARGE = 10000.0f;
        unsigned neg = synd;
        float minv = 0.0f;
        float w = 0.0f;
        for (int i = 0; i < deg; ++i) {
            const float v = FG_MIN(FG_MAX(nu[slot[i]], -20.0f), 20.0f);
            const unsigned ng = v < 0.0f;
            neg ^= ng;
            const float a = FG_ABS(v);
            minv = (i == 0) ? a : FG_MIN(minv, a);
            if (i == j) w = with_sign(a, ng);
        }
        float min2 = 0.0f, nsum = 0.0f;
        for (int i = 0; i < deg; ++i) {
            // FG_ABS of the parked value: the magnitude of the clamped input
            float d = FG_ABS(FG_MIN(FG_MAX(nu[slot[i]], -20.0f), 20.0f)) - minv;
            d = (d == 0.0f) ? LARGE : d;
            min2 = (i == 0) ? d : FG_MIN(min2, d);
            nsum = nsum + d;
        }
        min2 = min2 + minv;
        nsum = nsum - (2.0f * LARGE - 1.0f);
        const float sg = (nsum > 0.0f) ? 1.0f : ((nsum < 0.0f) ? -1.0f : 0.0f);
        const float dm = 0.5f * (1.0f - sg);
        const float min_e = (1.0f - dm) * minv + dm * min2;
        const float d = FG_ABS(w) - minv;
        const float out = (d == 0.0f) ? min_e : minv;
        return with_sign(out, neg ^ sign_bit(w)) * factor;
    } else {
        float P = 1.0f;
        float tj = 1.0f;
        for (int i = 0; i < deg; ++i) {
            float t = fg_tanh(nu[slot[i]] / 2.0f);
            t = (t == 0.0f) ? 1e-12f : t;
            P = (i == 0) ? t : P * t;
            if (i == j) tj = t;
        }
        P = P * (synd ? -1.0f : 1.0f);
        const float clipv = 0.99999988f;
        float q = fg_rcp_unit(tj) * P;
        q = (FG_ABS(q) < 1e-7f) ? 0.0f : q;
        q = FG_MIN(FG_MAX(q, -clipv), clipv);
        return (2.0f * fg_atanh(q)) * factor;
    }
}

#endif
