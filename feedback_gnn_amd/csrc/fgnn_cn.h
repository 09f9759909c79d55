// fgnn_cn.h — check-node rules shared by binary BP (fgnn_bp2.hip), BP4 (fgnn_bp4.hip), the step-loop decoders (fgnn_step.h),
// soft-syndrome BP4 (fgnn_dsbp4.hip) and space-time BP4 (fgnn_stbp4.hip).
//
// Each rule is the oracle's float operation sequence in the oracle's order (oracle/fgnn_oracle.c restates them independently).
// The phi rule is parameterised by a policy PHI with a static PHI::phi(x): BP4 passes Mx<HWT> (fg_phi, or the opt-in hardware
// transcendentals), binary BP and GNN_BP4 pass PhiGnn (fg_phi_gnn, the log(exp(x)+1) - log(exp(x)-1) form of decoding.py:632-633).
// Line numbers: decoding_q.py (BP4) first, then decoding.py (binary BP).
//
// Extra inputs.  A check with d edges may have NX = 0, 1 or 2 further inputs held in registers: the syndrome LLR gamma of soft-syndrome
// BP4 (NX = 1: the measured bit's own error is a degree-one variable on the check whose message to the check never changes), the
// messages of the one or two time variables next to check (c,t) of space-time BP4 (NX = 1 in round 0, NX = 2 in every later round).
// It is the same rule on the d + NX inputs (nu_1, .., nu_d, x[0], .., x[NX-1]) in that order, with the same float operations.
// Outputs 1 .. d (times factor) are the c->v messages and go back into the slots; the outputs for the extra inputs (times factor)
// are returned in x[], each in the place of its input.  An infinite extra input forms no NaN in any rule: every rule clamps its input
// before it evaluates anything (phi at 16.635532, min-sum at 20, tanh at 9).  With NX = 0, x is not read.
//
// Host and device (FG_FN), like fgnn_vn.h: tests/cn_rule_check.cpp runs every rule on the CPU.
#ifndef FGNN_CN_H
#define FGNN_CN_H

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "../../include/fgnn.h"
#include "fgnn_math.h"

FG_FN unsigned sign_bit(float x) { return fg_f2u(x) >> 31; }
FG_FN float with_sign(float mag, unsigned neg) { return fg_u2f(fg_f2u(mag) ^ (neg << 31)); }

// the message at BYTE offset `byte_off` from `msg` (the packed rows of g.cslot16 hold 4 * slot).  IDX is the caller's offset type:
// int or unsigned, each kernel keeps the address arithmetic it was tuned with.
template <typename IDX>
FG_FN float& slot_ref(float* msg, IDX byte_off)
{
    return *reinterpret_cast<float*>(reinterpret_cast<char*>(msg) + byte_off);
}

struct PhiGnn {
    FG_FN float phi(float x) { return fg_phi_gnn(x); }
};
// the phi of BP4's check rule and soft syndromes (decoding_q.py:365-373): what bp4_kernel's exact policy evaluates; the step-loop decoders
// (fgnn_step.h) and the layered schedule pass it
struct PhiBp4 {
    FG_FN float phi(float x) { return fg_phi(x); }
};

// ---------------------------------------------------------------------------------------------
// Check-node rules on runtime-degree rows.  `msg` = this codeword's LDS message array, `slot` =
// the check's slot list.  Pass 1 parks |.|-type intermediates in the slots themselves (sign kept in
// the sign bit), pass 2 writes the c->v messages.  x[0 .. NX) holds the extra inputs in order on
// entry and their outputs on return.
// ---------------------------------------------------------------------------------------------
template <int CN_TYPE, typename PHI, int NX = 0>
FG_FN void cn_update(float* msg, const int* __restrict__ slot, int deg, unsigned synd, float factor, float* x = nullptr)
{
    static_assert(NX >= 0 && NX <= 2, "a check has at most two extra inputs");
    constexpr int AX = NX ? NX : 1;  // no zero-length arrays
    if constexpr (CN_TYPE == FGNN_CN_BOXPLUS_PHI) {  // _cn_update_phi (:376-431; decoding.py:637-693)
        unsigned neg = synd;
        float T = 0.0f;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float v = msg[s];
            unsigned ng = v < 0.0f;
            neg ^= ng;
            float a = PHI::phi(FG_ABS(v));
            T = T + a;
            msg[s] = with_sign(a, ng);
        }
        unsigned ngx[AX];
        float ax[AX];
        for (int e = 0; e < NX; ++e) {
            ngx[e] = x[e] < 0.0f;
            neg ^= ngx[e];
            ax[e] = PHI::phi(FG_ABS(x[e]));
            T = T + ax[e];
        }
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float w = msg[s];
            float out = PHI::phi(T - FG_ABS(w));
            msg[s] = with_sign(out, neg ^ sign_bit(w)) * factor;
        }
        for (int e = 0; e < NX; ++e) x[e] = with_sign(PHI::phi(T - ax[e]), neg ^ ngx[e]) * factor;
    } else if constexpr (CN_TYPE == FGNN_CN_MINSUM) {  // _cn_update_minsum (:539-644; decoding.py:744-850)
        const float LARGE = 10000.0f;
        unsigned neg = synd;
        float minv = 0.0f;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float v = FG_MIN(FG_MAX(msg[s], -20.0f), 20.0f);
            unsigned ng = v < 0.0f;
            neg ^= ng;
            float a = FG_ABS(v);
            minv = (j == 0) ? a : FG_MIN(minv, a);
            msg[s] = with_sign(a, ng);
        }
        unsigned ngx[AX];
        float ax[AX];
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
        float sg = (nsum > 0.0f) ? 1.0f : ((nsum < 0.0f) ? -1.0f : 0.0f);
        float dm = 0.5f * (1.0f - sg);
        float min_e = (1.0f - dm) * minv + dm * min2;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float w = msg[s];
            float d = FG_ABS(w) - minv;
            float out = (d == 0.0f) ? min_e : minv;
            msg[s] = with_sign(out, neg ^ sign_bit(w)) * factor;
        }
        for (int e = 0; e < NX; ++e) {
            const float outg = ((ax[e] - minv) == 0.0f) ? min_e : minv;
            x[e] = with_sign(outg, neg ^ ngx[e]) * factor;
        }
    } else {  // _cn_update_tanh (:313-363; decoding.py:575-623)
        float P = 1.0f;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float t = fg_tanh(msg[s] / 2.0f);
            t = (t == 0.0f) ? 1e-12f : t;
            P = (j == 0) ? t : P * t;
            msg[s] = t;
        }
        float tx[AX];
        for (int e = 0; e < NX; ++e) {
            float tg = fg_tanh(x[e] / 2.0f);
            tg = (tg == 0.0f) ? 1e-12f : tg;
            P = (deg == 0 && e == 0) ? tg : P * tg;
            tx[e] = tg;
        }
        P = P * (synd ? -1.0f : 1.0f);
        const float clipv = 0.99999988f;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
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

// _cn_update_minsum on a check of compile-time degree DC, registers only: the DC messages are read once, every intermediate that
// cn_update parks in the slots stays in registers, each slot is written once, the extra inputs stay in registers; same float
// operations in the same order as cn_update<FGNN_CN_MINSUM>.  `off` = BYTE offsets of the check's slots (slot_ref).  deg < DC
// (runtime-degree graphs compiled for a maximum degree): edge j takes part iff j < deg; the guards fold away when deg == DC.
template <int DC, int NX = 0, typename IDX>
FG_FN void cn_minsum_regular(float* msg, const IDX (&off)[DC], int deg, unsigned synd, float factor, float* x = nullptr)
{
    static_assert(NX >= 0 && NX <= 2, "a check has at most two extra inputs");
    constexpr int AX = NX ? NX : 1;
    const float LARGE = 10000.0f;
    float a[DC];
    unsigned ng[DC];
    unsigned neg = synd;
    float minv = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        const float v = (j < deg) ? FG_MIN(FG_MAX(slot_ref(msg, off[j]), -20.0f), 20.0f) : 1.0f;
        ng[j] = v < 0.0f;
        neg ^= ng[j];
        a[j] = FG_ABS(v);
        minv = (j == 0) ? a[j] : ((j < deg) ? FG_MIN(minv, a[j]) : minv);
    }
    unsigned ngx[AX];
    float ax[AX];
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
        if (j < deg) slot_ref(msg, off[j]) = with_sign(out, neg ^ ng[j]) * factor;
    }
#pragma unroll
    for (int e = 0; e < NX; ++e) {
        const float outg = ((ax[e] - minv) == 0.0f) ? min_e : minv;
        x[e] = with_sign(outg, neg ^ ngx[e]) * factor;
    }
}

// soft syndrome of one row, _cn_update_phi_loss (decoding_q.py:433-453)
template <typename PHI>
FG_FN float logit_row(const float* llr, const int* __restrict__ col, int deg)
{
    unsigned neg = 0;
    float T = 0.0f;
    for (int j = 0; j < deg; ++j) {
        float v = llr[col[j]];
        neg ^= (v < 0.0f);
        T = T + PHI::phi(FG_ABS(v));
    }
    return with_sign(PHI::phi(T), neg);
}

#endif
