// fgnn_cn.h — check-node rules shared by binary BP (fgnn_bp2.hip), BP4 (fgnn_bp4.hip) and GNN_BP4 (fgnn_gnnbp4.hip).
//
// Each rule is the oracle's float operation sequence in the oracle's order (oracle/fgnn_oracle.c restates them independently).
// The phi rule is parameterised by a policy PHI with a static PHI::phi(x): BP4 passes Mx<HWT> (fg_phi, or the opt-in hardware
// transcendentals), binary BP and GNN_BP4 pass PhiGnn (fg_phi_gnn, the log(exp(x)+1) - log(exp(x)-1) form of decoding.py:632-633).
// Line numbers: decoding_q.py (BP4) first, then decoding.py (binary BP).
#ifndef FGNN_CN_H
#define FGNN_CN_H

#include <hip/hip_runtime.h>

#include "../../include/fgnn.h"
#include "fgnn_math.h"

__device__ __forceinline__ unsigned sign_bit(float x) { return fg_f2u(x) >> 31; }
__device__ __forceinline__ float with_sign(float mag, unsigned neg) { return fg_u2f(fg_f2u(mag) ^ (neg << 31)); }

// the message at BYTE offset `byte_off` from `msg` (the packed rows of g.cslot16 hold 4 * slot).  IDX is the caller's offset type:
// int or unsigned, each kernel keeps the address arithmetic it was tuned with.
template <typename IDX>
__device__ __forceinline__ float& slot_ref(float* msg, IDX byte_off)
{
    return *reinterpret_cast<float*>(reinterpret_cast<char*>(msg) + byte_off);
}

struct PhiGnn {
    static __device__ __forceinline__ float phi(float x) { return fg_phi_gnn(x); }
};
// the phi of BP4's check rule and soft syndromes (decoding_q.py:365-373): what bp4_kernel's exact policy evaluates; the step-loop decoders
// (fgnn_step.h) and the layered schedule pass it
struct PhiBp4 {
    static __device__ __forceinline__ float phi(float x) { return fg_phi(x); }
};

// ---------------------------------------------------------------------------------------------
// Check-node rules on runtime-degree rows.  `msg` = this codeword's LDS message array, `slot` =
// the check's slot list.  Pass 1 parks |.|-type intermediates in the slots themselves (sign kept in
// the sign bit), pass 2 writes the c->v messages.
// ---------------------------------------------------------------------------------------------
template <int CN_TYPE, typename PHI>
__device__ __forceinline__ void cn_update(float* msg, const int* __restrict__ slot, int deg, unsigned synd, float factor)
{
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
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float w = msg[s];
            float out = PHI::phi(T - FG_ABS(w));
            msg[s] = with_sign(out, neg ^ sign_bit(w)) * factor;
        }
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
        float min2 = 0.0f, nsum = 0.0f;
        for (int j = 0; j < deg; ++j) {
            float d = FG_ABS(msg[slot[j]]) - minv;
            d = (d == 0.0f) ? LARGE : d;
            min2 = (j == 0) ? d : FG_MIN(min2, d);
            nsum = nsum + d;
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
    } else {  // _cn_update_tanh (:313-363; decoding.py:575-623)
        float P = 1.0f;
        for (int j = 0; j < deg; ++j) {
            int s = slot[j];
            float t = fg_tanh(msg[s] / 2.0f);
            t = (t == 0.0f) ? 1e-12f : t;
            P = (j == 0) ? t : P * t;
            msg[s] = t;
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
    }
}

// _cn_update_minsum on a check of compile-time degree DC, registers only: the DC messages are read once, every intermediate that
// cn_update parks in the slots stays in registers, each slot is written once; same float operations in the same order as
// cn_update<FGNN_CN_MINSUM>.  `off` = BYTE offsets of the check's slots (slot_ref).  deg < DC (runtime-degree graphs compiled for a
// maximum degree): edge j takes part iff j < deg; the guards fold away when deg == DC.
template <int DC, typename IDX>
__device__ __forceinline__ void cn_minsum_regular(float* msg, const IDX (&off)[DC], int deg, unsigned synd, float factor)
{
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
    float min2 = 0.0f, nsum = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        float d = a[j] - minv;
        d = (d == 0.0f) ? LARGE : d;
        min2 = (j == 0) ? d : ((j < deg) ? FG_MIN(min2, d) : min2);
        nsum = (j < deg) ? nsum + d : nsum;
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
}

// soft syndrome of one row, _cn_update_phi_loss (decoding_q.py:433-453)
template <typename PHI>
__device__ __forceinline__ float logit_row(const float* llr, const int* __restrict__ col, int deg)
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
