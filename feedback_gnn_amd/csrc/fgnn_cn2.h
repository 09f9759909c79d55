// fgnn_cn2.h — the register-resident phi rule of the binary decoders on compile-time check degrees: bp2_kernel (fgnn_bp2.hip) and
// bp2_layered_kernel (fgnn_bp2_layered.hip).  Device only (the table reads of fg_log_tab, the scheduling barriers).
#ifndef FGNN_CN2_H
#define FGNN_CN2_H

#include "fgnn_cn.h"

#ifndef FGNN_BP2_PHI_STAGE
#define FGNN_BP2_PHI_STAGE 2  // phi evaluations staged together in the regular check update, must divide DC
#endif

// N evaluations of fg_phi_gnn with the table reads of all 2N logarithms in flight together: the float operations of
// fg_phi_gnn (fg_exp, then fg_log(y + 1) - fg_log(y - 1)) in the same order, only the instruction schedule differs.
template <int N>
__device__ __forceinline__ void phi_gnn_n(const float (&x)[N], float (&out)[N])
{
    const float* tab = fg_log_tab();
    float yp[N], ym[N];
    uint32_t eb1[N], eb2[N], j1[N], j2[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float y = fg_exp(FG_CLAMP(x[k], FG_PHI_MIN, FG_PHI_MAX));
        yp[k] = y + 1.0f;
        ym[k] = y - 1.0f;
        const uint32_t w1 = fg_f2u(yp[k]) - FG_LOG_OFFS;
        const uint32_t w2 = fg_f2u(ym[k]) - FG_LOG_OFFS;
        eb1[k] = w1 & 0xff800000u;
        eb2[k] = w2 & 0xff800000u;
        j1[k] = (w1 >> 18) & 31u;
        j2[k] = (w2 >> 18) & 31u;
    }
    __builtin_amdgcn_sched_barrier(0);
    float rc1[N], lc1[N], rc2[N], lc2[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        rc1[k] = tab[j1[k]];
        lc1[k] = tab[32 + j1[k]];
        rc2[k] = tab[j2[k]];
        lc2[k] = tab[32 + j2[k]];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float r1 = FG_FMA(fg_u2f(fg_f2u(yp[k]) - eb1[k]), rc1[k], -1.0f);
        const float l1 = FG_FMA((float)(int32_t)eb1[k], FG_LN2_S23, lc1[k] + fg_log1p_small(r1));
        const float r2 = FG_FMA(fg_u2f(fg_f2u(ym[k]) - eb2[k]), rc2[k], -1.0f);
        const float l2 = FG_FMA((float)(int32_t)eb2[k], FG_LN2_S23, lc2[k] + fg_log1p_small(r2));
        out[k] = l1 - l2;
    }
}

// _cn_update_phi (decoding.py:637-693) for a check of compile-time degree DC: its DC messages are read once, live in registers
// between the two phi passes (cn_update parks phi(|v|) in LDS and reads it back) and are written once; signs travel as bit 31
// of integer words.  Same float operations in the same order as cn_update<FGNN_CN_BOXPLUS_PHI, PhiGnn> (fgnn_cn.h).
template <int DC>
__device__ __forceinline__ void cn2_phi_regular(float* msg, const unsigned (&off)[DC], unsigned synd, float factor, bool f1)
{
    float v[DC], aa[DC];
    uint32_t neg = synd << 31;
#pragma unroll
    for (int j = 0; j < DC; ++j) {
        v[j] = slot_ref(msg, off[j]);
        // cn_update tests v < 0: a message of -0 counts as positive there, and its parked copy carries no sign either
        neg ^= (v[j] < 0.0f) ? 0x80000000u : 0u;
    }
#pragma unroll
    for (int j = 0; j < DC; j += FGNN_BP2_PHI_STAGE) {
        float xa[FGNN_BP2_PHI_STAGE], oa[FGNN_BP2_PHI_STAGE];
#pragma unroll
        for (int k = 0; k < FGNN_BP2_PHI_STAGE; ++k) xa[k] = FG_ABS(v[j + k]);
        phi_gnn_n<FGNN_BP2_PHI_STAGE>(xa, oa);
#pragma unroll
        for (int k = 0; k < FGNN_BP2_PHI_STAGE; ++k) aa[j + k] = oa[k];
    }
    float T = 0.0f;
#pragma unroll
    for (int j = 0; j < DC; ++j) T = T + aa[j];
#pragma unroll
    for (int j = 0; j < DC; j += FGNN_BP2_PHI_STAGE) {
        float xa[FGNN_BP2_PHI_STAGE], oa[FGNN_BP2_PHI_STAGE];
#pragma unroll
        for (int k = 0; k < FGNN_BP2_PHI_STAGE; ++k) xa[k] = T - FG_ABS(aa[j + k]);
        phi_gnn_n<FGNN_BP2_PHI_STAGE>(xa, oa);
#pragma unroll
        for (int k = 0; k < FGNN_BP2_PHI_STAGE; ++k) {
            // sign of the parked word with_sign(phi(|v|), v < 0) that cn_update reads back
            const uint32_t sg = neg ^ ((v[j + k] < 0.0f) ? 0x80000000u : 0u) ^ (fg_f2u(aa[j + k]) & 0x80000000u);
            const float o = fg_u2f(fg_f2u(oa[k]) ^ sg);
            slot_ref(msg, off[j + k]) = f1 ? o : o * factor;
        }
    }
}

#endif
