// fgnn_mlp.h — MLP building blocks shared by the feedback GNN (fgnn_gnn.hip), its backward pass (fgnn_backward.hip) and GNN_BP4
// (fgnn_gnnbp4.hip): the runtime-shaped Dense layer of the general kernels, and the MFMA operand and lane maps of the fixed-shape
// 2-layer MLPs.
#ifndef FGNN_MLP_H
#define FGNN_MLP_H

#include "fgnn_internal.h"
#include "fgnn_math.h"

// ---------------------------------------------------------------------------------------------
// Runtime-shaped Dense layer, exactly as the oracle: fmaf chain in ascending k from 0, then (+ bias), then the activation.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float mlp_act(float a, int act)
{
    switch (act) {
    case FGNN_ACT_TANH: return fg_tanh(a);
    case FGNN_ACT_RELU: return FG_MAX(a, 0.0f);
    case FGNN_ACT_SIGMOID: return fg_sigmoid(a);
    default: return a;
    }
}

// Dense layer li of a runtime-shaped feedback GNN (fgnn_weights_create_general): out[j] = act(sum_k in[k] W[k][j] (+ b[j]))
__device__ __forceinline__ void gen_dense(const GnnGeneralDev& w, int li, const float* in, float* out)
{
    const int K = w.K[li], J = w.J[li], act = w.act_l[li];
    const float* W = w.W[li];
    const float* b = w.b[li];
    for (int j = 0; j < J; ++j) {
        float a = 0.0f;
        for (int k = 0; k < K; ++k) a = FG_FMA(in[k], W[k * J + j], a);
        if (b) a = a + b[j];
        out[j] = mlp_act(a, act);
    }
}

// ---------------------------------------------------------------------------------------------
// MFMA path of the fixed-shape 2-layer MLPs (fgnn_gnn.hip, fgnn_gnnbp4.hip): every Dense layer runs transposed on
// v_mfma_f32_16x16x4_f32, so a layer's accumulators are the next layer's B operand.  The lane maps below are the host side of that
// construction: the per-lane operand tables are written with them.  lane = 16 q + rho.
// ---------------------------------------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the unit that output row rho = 4q' + r' of row tile t carries: 16t + 4r' + q'.  Lane group q, register r of tile t then holds
// unit 4(4t + r) + q, element q of k-step 4t + r of the next layer.
inline int mfma_unit(int lane, int t)
{
    const int rho = lane & 15;
    return 16 * t + 4 * (rho & 3) + (rho >> 2);
}
// the same permutation for the 20 outputs of layer 2: the output column of row tile u (0: outputs 0..15, 1: 16..19), -1 = padding
inline int mfma_w2_col(int lane, int u)
{
    const int rho = lane & 15, rp = rho & 3, qp = rho >> 2;
    return (u == 0) ? 4 * rp + qp : (rp == 0 ? 16 + qp : -1);
}
// the output of layer 2 that lane group q holds in result register i (0..3: tile 0, 4: tile 1), i.e. the bias it adds there
inline int mfma_b2_row(int lane, int i) { return i < 4 ? 4 * i + (lane >> 4) : 16 + (lane >> 4); }

#endif
