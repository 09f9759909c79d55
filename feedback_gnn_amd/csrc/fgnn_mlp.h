// fgnn_mlp.h — MLP building blocks shared by the feedback GNN (fgnn_gnn.hip), its backward pass (fgnn_backward.hip) and GNN_BP4
// (fgnn_gnnbp4.hip): the syndrome sign and the check-feature staging of the feedback GNN, the runtime-shaped Dense layer and
// max / min / sum reduce of the general kernels, and the MFMA lane maps of the fixed-shape 2-layer MLPs with the host functions
// that write one per-lane operand-table entry each.
#ifndef FGNN_MLP_H
#define FGNN_MLP_H

#include "fgnn_internal.h"
#include "fgnn_math.h"

// 1 - 2 s of a syndrome bit
__device__ __forceinline__ float synd_sign(unsigned bit) { return (bit & 1) ? -1.0f : 1.0f; }

// The check features of codeword b, g_x | g_z = soft syndrome * (1 - 2 syndrome) (feedback_gnn.py:168-172), into gcn[m_x + m_z];
// the caller's threads lane, lane + stride, ... share the work and synchronise afterwards.
__device__ __forceinline__ void stage_check_features(const GraphDev& g, const float* logit_hx, const float* logit_hz, const uint8_t* synd_x,
                                                     const uint8_t* synd_z, int b, float* gcn, int lane, int stride)
{
    for (int c = lane; c < g.m_x; c += stride) gcn[c] = logit_hx[(size_t)b * g.m_x + c] * synd_sign(synd_x[(size_t)b * g.m_x + c]);
    for (int c = lane; c < g.m_z; c += stride)
        gcn[g.m_x + c] = logit_hz[(size_t)b * g.m_z + c] * synd_sign(synd_z[(size_t)b * g.m_z + c]);
}

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

// reduce_msg of the runtime-shaped kernels (feedback_gnn.py:130-150), one edge's message into acc: the first edge assigns, later ones
// take the max, the min or the sum; mean divides afterwards, in the caller
__device__ __forceinline__ void gg_reduce(float* acc, const float* msg, int D, bool first, int op)
{
    for (int i = 0; i < D; ++i) {
        const float m = msg[i];
        float r;
        if (first) r = m;
        else if (op == FGNN_REDUCE_MAX) r = FG_MAX(acc[i], m);
        else if (op == FGNN_REDUCE_MIN) r = FG_MIN(acc[i], m);
        else r = acc[i] + m;
        acc[i] = r;
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

// One 64-lane entry e[0..64) of a per-lane operand table each, from Keras-layout arrays (W[k][j]: input k, unit j).  Which entries a
// kernel's table holds, and in which order, is the kernel's own business (the T_* enum of fgnn_gnn.hip, the per-MLP order of fgnn_gnnbp4.hip).
// layer 1, row tile t, k-step s: A[rho][q] = W1[4s + q][unit(rho, t)]; units >= hid and inputs >= nin are padding
inline void mfma_fill_w1(float* e, const float* W1, int nin, int hid, int t, int s)
{
    for (int lane = 0; lane < 64; ++lane) {
        const int unit = mfma_unit(lane, t), k = 4 * s + (lane >> 4);
        e[lane] = (unit < hid && k < nin) ? W1[(size_t)k * hid + unit] : 0.0f;
    }
}
// element 4s + q of a vector on lane group q: the layer-1 bias of the unit that group holds in accumulator register s (and any other
// per-unit multiplier, such as one row of W1)
inline void mfma_fill_b1(float* e, const float* B1, int s)
{
    for (int lane = 0; lane < 64; ++lane) e[lane] = B1[4 * s + (lane >> 4)];
}
// layer 2 (dout = 20 outputs), row tile u, k-step s
inline void mfma_fill_w2(float* e, const float* W2, int dout, int u, int s)
{
    for (int lane = 0; lane < 64; ++lane) {
        const int mu = mfma_w2_col(lane, u);
        e[lane] = mu >= 0 ? W2[(size_t)(4 * s + (lane >> 4)) * dout + mu] : 0.0f;
    }
}
// the layer-2 bias of result register i
inline void mfma_fill_b2(float* e, const float* B2, int i)
{
    for (int lane = 0; lane < 64; ++lane) e[lane] = B2[mfma_b2_row(lane, i)];
}
// the 3-output inverse embedding, k-step s: rows 0..2 unpermuted, rows 3..15 padding
inline void mfma_fill_wout(float* e, const float* Wout, int s)
{
    for (int lane = 0; lane < 64; ++lane) e[lane] = (lane & 15) < 3 ? Wout[(size_t)(4 * s + (lane >> 4)) * 3 + (lane & 15)] : 0.0f;
}

#endif
