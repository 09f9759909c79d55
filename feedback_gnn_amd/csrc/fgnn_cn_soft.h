// fgnn_cn_soft.h — check-node rules with a soft syndrome, for soft-syndrome BP4 (fgnn_dsbp4.hip).
//
// A check with d edges, syndrome bit s and syndrome LLR gamma is the rule of fgnn_cn.h on the d + 1 inputs (nu_1, .., nu_d, gamma) in
// that order, with the same float operations: the measured bit's own error is a degree-one variable on the check whose message to
// the check never changes, so it is one more constant input, held in a register.  Outputs 1 .. d (times factor) are the c->v messages
// and go back into the slots; output d + 1 (times factor) is w_c, the check's message to its syndrome-error variable, and is returned.
// The caller forms Gamma_c = gamma + w_c and u_hat_c = Gamma_c < 0 (soft_u_hat).  gamma = +inf (a perfect measurement) forms no NaN in
// any rule: every rule clamps its input before it evaluates anything (phi at 16.635532, min-sum at 20, tanh at 9).
//
// Two forms, as in fgnn_cn.h: cn_soft_update on runtime-degree rows (intermediates parked in the slots) and cn_soft_minsum_regular on a
// check of compile-time degree DC with the extra input in a register.  fgnn_cn.h itself is left alone: the hot kernels include it.
// Host and device (FG_FN), like fgnn_vn.h: tests/cn_soft_check.cpp runs every rule on the CPU.
#ifndef FGNN_CN_SOFT_H
#define FGNN_CN_SOFT_H

#include "fgnn_math.h"

// the values of FGNN_CN_* (include/fgnn.h), restated so that the header needs nothing but fgnn_math.h
#define FGNN_SOFT_BOXPLUS 0
#define FGNN_SOFT_BOXPLUS_PHI 1
#define FGNN_SOFT_MINSUM 2

FG_FN unsigned soft_sign_bit(float x) { return fg_f2u(x) >> 31; }
FG_FN float soft_with_sign(float mag, unsigned neg) { return fg_u2f(fg_f2u(mag) ^ (neg << 31)); }

// the message at BYTE offset `byte_off` from `msg` (the packed rows of g.cslot16 hold 4 * slot)
template <typename IDX>
FG_FN float& soft_slot_ref(float* msg, IDX byte_off)
{
    return *reinterpret_cast<float*>(reinterpret_cast<char*>(msg) + byte_off);
}

// the phi of BP4's check rule (decoding_q.py:365-373)
struct PhiSoft {
    FG_FN float phi(float x) { return fg_phi(x); }
};

// u_hat of a check: Gamma = gamma + w is one add
FG_FN unsigned soft_u_hat(float gamma, float w)
{
    const float G = gamma + w;
    return G < 0.0f ? 1u : 0u;
}

// Runtime-degree rows.  `msg` = this codeword's message array, `slot` = the check's slot list (ascending qubit).  Returns w_c.
template <int CN_TYPE, typename PHI>
FG_FN float cn_soft_update(float* msg, const int* slot, int deg, unsigned synd, float gamma, float factor)
{
    if (CN_TYPE == FGNN_SOFT_BOXPLUS_PHI) {
        unsigned neg = synd;
        float T = 0.0f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            const float v = msg[s];
            const unsigned ng = v < 0.0f;
            neg ^= ng;
            const float a = PHI::phi(FG_ABS(v));
            T = T + a;
            msg[s] = soft_with_sign(a, ng);
        }
        const unsigned ngg = gamma < 0.0f;
        neg ^= ngg;
        const float ag = PHI::phi(FG_ABS(gamma));
        T = T + ag;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            const float w = msg[s];
            const float out = PHI::phi(T - FG_ABS(w));
            msg[s] = soft_with_sign(out, neg ^ soft_sign_bit(w)) * factor;
        }
        return soft_with_sign(PHI::phi(T - ag), neg ^ ngg) * factor;
    } else if (CN_TYPE == FGNN_SOFT_MINSUM) {
        const float LARGE = 10000.0f;
        unsigned neg = synd;
        float minv = 0.0f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            const float v = FG_MIN(FG_MAX(msg[s], -20.0f), 20.0f);
            const unsigned ng = v < 0.0f;
            neg ^= ng;
            const float a = FG_ABS(v);
            minv = (j == 0) ? a : FG_MIN(minv, a);
            msg[s] = soft_with_sign(a, ng);
        }
        const float vg = FG_MIN(FG_MAX(gamma, -20.0f), 20.0f);
        const unsigned ngg = vg < 0.0f;
        neg ^= ngg;
        const float ag = FG_ABS(vg);
        minv = (deg == 0) ? ag : FG_MIN(minv, ag);
        float min2 = 0.0f, nsum = 0.0f;
        for (int j = 0; j < deg; ++j) {
            float d = FG_ABS(msg[slot[j]]) - minv;
            d = (d == 0.0f) ? LARGE : d;
            min2 = (j == 0) ? d : FG_MIN(min2, d);
            nsum = nsum + d;
        }
        float dg = ag - minv;
        dg = (dg == 0.0f) ? LARGE : dg;
        min2 = (deg == 0) ? dg : FG_MIN(min2, dg);
        nsum = nsum + dg;
        min2 = min2 + minv;
        nsum = nsum - (2.0f * LARGE - 1.0f);
        const float sg = (nsum > 0.0f) ? 1.0f : ((nsum < 0.0f) ? -1.0f : 0.0f);
        const float dm = 0.5f * (1.0f - sg);
        const float min_e = (1.0f - dm) * minv + dm * min2;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            const float w = msg[s];
            const float d = FG_ABS(w) - minv;
            const float out = (d == 0.0f) ? min_e : minv;
            msg[s] = soft_with_sign(out, neg ^ soft_sign_bit(w)) * factor;
        }
        const float outg = ((ag - minv) == 0.0f) ? min_e : minv;
        return soft_with_sign(outg, neg ^ ngg) * factor;
    } else {
        float P = 1.0f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            float t = fg_tanh(msg[s] / 2.0f);
            t = (t == 0.0f) ? 1e-12f : t;
            P = (j == 0) ? t : P * t;
            msg[s] = t;
        }
        float tg = fg_tanh(gamma / 2.0f);
        tg = (tg == 0.0f) ? 1e-12f : tg;
        P = (deg == 0) ? tg : P * tg;
        P = P * (synd ? -1.0f : 1.0f);
        const float clipv = 0.99999988f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            float q = fg_rcp_unit(msg[s]) * P;
            q = (FG_ABS(q) < 1e-7f) ? 0.0f : q;
            q = FG_MIN(FG_MAX(q, -clipv), clipv);
            msg[s] = (2.0f * fg_atanh(q)) * factor;
        }
        float q = fg_rcp_unit(tg) * P;
        q = (FG_ABS(q) < 1e-7f) ? 0.0f : q;
        q = FG_MIN(FG_MAX(q, -clipv), clipv);
        return (2.0f * fg_atanh(q)) * factor;
    }
}

// Min-sum on a check of compile-time degree DC, registers only, the extra input in a register: the DC messages are read once, each slot
// is written once; same float operations in the same order as cn_soft_update<FGNN_SOFT_MINSUM>.  `off` = BYTE offsets of the check's
// slots (soft_slot_ref).  deg < DC: edge j takes part iff j < deg; the guards fold away when deg == DC.  Returns w_c.
template <int DC, typename IDX>
FG_FN float cn_soft_minsum_regular(float* msg, const IDX (&off)[DC], int deg, unsigned synd, float gamma, float factor)
{
    const float LARGE = 10000.0f;
    float a[DC];
    unsigned ng[DC];
    unsigned neg = synd;
    float minv = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        const float v = (j < deg) ? FG_MIN(FG_MAX(soft_slot_ref(msg, off[j]), -20.0f), 20.0f) : 1.0f;
        ng[j] = v < 0.0f;
        neg ^= ng[j];
        a[j] = FG_ABS(v);
        minv = (j == 0) ? a[j] : ((j < deg) ? FG_MIN(minv, a[j]) : minv);
    }
    const float vg = FG_MIN(FG_MAX(gamma, -20.0f), 20.0f);
    const unsigned ngg = vg < 0.0f;
    neg ^= ngg;
    const float ag = FG_ABS(vg);
    minv = (deg == 0) ? ag : FG_MIN(minv, ag);
    float min2 = 0.0f, nsum = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        float d = a[j] - minv;
        d = (d == 0.0f) ? LARGE : d;
        min2 = (j == 0) ? d : ((j < deg) ? FG_MIN(min2, d) : min2);
        nsum = (j < deg) ? nsum + d : nsum;
    }
    float dg = ag - minv;
    dg = (dg == 0.0f) ? LARGE : dg;
    min2 = (deg == 0) ? dg : FG_MIN(min2, dg);
    nsum = nsum + dg;
    min2 = min2 + minv;
    nsum = nsum - (2.0f * LARGE - 1.0f);
    const float sg = (nsum > 0.0f) ? 1.0f : ((nsum < 0.0f) ? -1.0f : 0.0f);
    const float dm = 0.5f * (1.0f - sg);
    const float min_e = (1.0f - dm) * minv + dm * min2;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        const float out = ((a[j] - minv) == 0.0f) ? min_e : minv;
        if (j < deg) soft_slot_ref(msg, off[j]) = soft_with_sign(out, neg ^ ng[j]) * factor;
    }
    const float outg = ((ag - minv) == 0.0f) ? min_e : minv;
    return soft_with_sign(outg, neg ^ ngg) * factor;
}

#endif
