// fgnn_cn_st.h — check-node rules with one or two time-like inputs, for space-time BP4 (fgnn_stbp4.hip).
//
// Check (c,t) of a window of measurement rounds has d edges to the qubits of round t and NX further inputs: NX = 1 in round 0, the
// message b from time variable (c,0); NX = 2 in every later round, the message a from time variable (c,t-1) and then the message b
// from time variable (c,t).  It is the rule of fgnn_cn.h on the d + NX inputs (nu_1, .., nu_d, a, b) in that order, with the same float
// operations, and every extra input is treated exactly as fgnn_cn_soft.h treats its one extra input: with NX = 1 the float operations
// are those of cn_soft_update.  Outputs 1 .. d (times factor) are the c->v messages and go back into the slots; the outputs for the
// extra inputs (times factor) are returned in x[]: w_up towards time variable (c,t-1) in the place of a, w_dn towards time variable
// (c,t) in the place of b.  An infinite input forms no NaN in any rule: every rule clamps its input before it evaluates anything
// (phi at 16.635532, min-sum at 20, tanh at 9).
//
// Two forms, as in fgnn_cn_soft.h, NX a compile-time 1 or 2: cn_st_update on runtime-degree rows (intermediates parked in the slots)
// and cn_st_minsum_regular on a check of compile-time degree DC with the extra inputs in registers.  fgnn_cn.h and fgnn_cn_soft.h are
// left alone.  Host and device (FG_FN), like fgnn_cn_soft.h: tests/cn_st_check.cpp runs every rule on the CPU.
#ifndef FGNN_CN_ST_H
#define FGNN_CN_ST_H

#include "fgnn_cn_soft.h"

// `msg` = the message array of this round, `slot` = the check's slot list (ascending qubit).  x[0 .. NX) holds the extra inputs in
// order on entry and their outputs on return.
template <int CN_TYPE, int NX, typename PHI>
FG_FN void cn_st_update(float* msg, const int* slot, int deg, unsigned synd, float (&x)[NX], float factor)
{
    static_assert(NX == 1 || NX == 2, "a check has one or two time-like inputs");
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
        unsigned ngx[NX];
        float ax[NX];
        for (int e = 0; e < NX; ++e) {
            ngx[e] = x[e] < 0.0f;
            neg ^= ngx[e];
            ax[e] = PHI::phi(FG_ABS(x[e]));
            T = T + ax[e];
        }
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            const float w = msg[s];
            const float out = PHI::phi(T - FG_ABS(w));
            msg[s] = soft_with_sign(out, neg ^ soft_sign_bit(w)) * factor;
        }
        for (int e = 0; e < NX; ++e) x[e] = soft_with_sign(PHI::phi(T - ax[e]), neg ^ ngx[e]) * factor;
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
        unsigned ngx[NX];
        float ax[NX];
        for (int e = 0; e < NX; ++e) {
            const float vg = FG_MIN(FG_MAX(x[e], -20.0f), 20.0f);
            ngx[e] = vg < 0.0f;
            neg ^= ngx[e];
            ax[e] = FG_ABS(vg);
            minv = (deg == 0 && e == 0) ? ax[e] : FG_MIN(minv, ax[e]);
        }
        float min2 = 0.0f, nsum = 0.0f;
        for (int j = 0; j < deg; ++j) {
            float d = FG_ABS(msg[slot[j]]) - minv;
            d = (d == 0.0f) ? LARGE : d;
            min2 = (j == 0) ? d : FG_MIN(min2, d);
            nsum = nsum + d;
        }
        for (int e = 0; e < NX; ++e) {
            float dg = ax[e] - minv;
            dg = (dg == 0.0f) ? LARGE : dg;
            min2 = (deg == 0 && e == 0) ? dg : FG_MIN(min2, dg);
            nsum = nsum + dg;
        }
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
        for (int e = 0; e < NX; ++e) {
            const float outg = ((ax[e] - minv) == 0.0f) ? min_e : minv;
            x[e] = soft_with_sign(outg, neg ^ ngx[e]) * factor;
        }
    } else {
        float P = 1.0f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            float t = fg_tanh(msg[s] / 2.0f);
            t = (t == 0.0f) ? 1e-12f : t;
            P = (j == 0) ? t : P * t;
            msg[s] = t;
        }
        float tx[NX];
        for (int e = 0; e < NX; ++e) {
            float tg = fg_tanh(x[e] / 2.0f);
            tg = (tg == 0.0f) ? 1e-12f : tg;
            P = (deg == 0 && e == 0) ? tg : P * tg;
            tx[e] = tg;
        }
        P = P * (synd ? -1.0f : 1.0f);
        const float clipv = 0.99999988f;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j];
            float q = fg_rcp_unit(msg[s]) * P;
            q = (FG_ABS(q) < 1e-7f) ? 0.0f : q;
            q = FG_MIN(FG_MAX(q, -clipv), clipv);
            msg[s] = (2.0f * fg_atanh(q)) * factor;
        }
        for (int e = 0; e < NX; ++e) {
            float q = fg_rcp_unit(tx[e]) * P;
            q = (FG_ABS(q) < 1e-7f) ? 0.0f : q;
            q = FG_MIN(FG_MAX(q, -clipv), clipv);
            x[e] = (2.0f * fg_atanh(q)) * factor;
        }
    }
}

// Min-sum on a check of compile-time degree DC, registers only, the extra inputs in registers: the DC messages are read once, each slot
// is written once; same float operations in the same order as cn_st_update<FGNN_SOFT_MINSUM>.  `off` = BYTE offsets of the check's
// slots (soft_slot_ref).  deg < DC: edge j takes part iff j < deg; the guards fold away when deg == DC.
template <int DC, int NX, typename IDX>
FG_FN void cn_st_minsum_regular(float* msg, const IDX (&off)[DC], int deg, unsigned synd, float (&x)[NX], float factor)
{
    static_assert(NX == 1 || NX == 2, "a check has one or two time-like inputs");
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
    unsigned ngx[NX];
    float ax[NX];
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        const float vg = FG_MIN(FG_MAX(x[e], -20.0f), 20.0f);
        ngx[e] = vg < 0.0f;
        neg ^= ngx[e];
        ax[e] = FG_ABS(vg);
        minv = (deg == 0 && e == 0) ? ax[e] : FG_MIN(minv, ax[e]);
    }
    float min2 = 0.0f, nsum = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        float d = a[j] - minv;
        d = (d == 0.0f) ? LARGE : d;
        min2 = (j == 0) ? d : ((j < deg) ? FG_MIN(min2, d) : min2);
        nsum = (j < deg) ? nsum + d : nsum;
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        float dg = ax[e] - minv;
        dg = (dg == 0.0f) ? LARGE : dg;
        min2 = (deg == 0 && e == 0) ? dg : FG_MIN(min2, dg);
        nsum = nsum + dg;
    }
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
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        const float outg = ((ax[e] - minv) == 0.0f) ? min_e : minv;
        x[e] = soft_with_sign(outg, neg ^ ngx[e]) * factor;
    }
}

#endif
