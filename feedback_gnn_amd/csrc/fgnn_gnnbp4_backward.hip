// fgnn_gnnbp4_backward.hip — training of GNN_BP4 on the GPU: a forward pass that records a tape, and the reverse pass.
//
// The forward (fgnn_gnnbp4_forward_tape) is GNN_BP4.call in the literal association: the float32 operations of
// gnn_bp4_general_kernel (fgnn_gnnbp4.hip) and og_gnn_bp4_general in the same order, so its soft syndromes are those of
// fgnn_gnnbp4_decode on a runtime-shaped handle bit for bit.  It needs no workspace: every node embedding it computes is a
// checkpoint, so the embeddings live in the tape and nothing is updated in place.  Per codeword and iteration k the tape holds
//     h_vn^(k) [n][D] after the VN update | h_cn^(k) [m][D] the VN update read | hlog^(k) [m] the hx then hz logits.
// MLP hidden activations are not kept; the reverse pass recomputes them.
//
// The reverse pass (fgnn_gnnbp4_backward) walks k = T-1 .. 0 through: the soft syndromes of iteration k (rows_logit -> softplus / lse2
// -> _llr_inv_embed -> h_vn^(k)), the VN update, and the CN update that produced h_cn^(k).  A workgroup owns a codeword at a time
// (codewords wg, wg + grid, ...), one thread per receiving node.  The gradient a per-edge message MLP sends to the OTHER end of its
// edge goes to a per-edge buffer (VN-major slots); the owning node gathers its slots in ascending order.  No floating-point atomics.
//
// Weight gradients: the threads of a workgroup leave, per Dense layer, their input row and the gradient at the layer's
// pre-activation in LDS (inputs k-major and padded, gradients row-major); after a barrier every thread owns entries (k, 4 j) of
// the layer's weight gradient and sums its entries over the staged rows in ascending row order, then adds the sum to the
// workgroup's own partial gradient in the workspace.  A second kernel adds the partials in ascending workgroup order.  Two calls
// with the same inputs therefore return the same bits.
//
// Two instantiations of both kernels.  FX = true: D = 20, H = 40, L = 2, tanh, mean, bias (the configuration bench.py --config c5
// runs) with compile-time widths — a node's vectors are registers, weights arrive as wave-uniform scalar loads, hidden activations
// go to LDS as they are made.  FX = false: runtime-shaped loops over per-thread buffers for every other supported setting.
//
// Gradient conventions are those of fgnn_backward.hip: the sign products are constants, the clip inside phi passes the gradient
// inside its interval and blocks it outside, |x|' = sign(x), softplus' = sigmoid, lse' = softmax.  GNN_BP4's phi
// (log(e^x + 1) - log(e^x - 1)) has the derivative -1 / sinh(x) of the decoder's.
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_mlp.h"
#include "fgnn_vn.h"

// The node loops are written once for both instantiations: `#pragma unroll` unrolls them where the width is a compile-time
// constant and is a request the optimizer declines, with a warning per loop, where it is a runtime value.
#pragma clang diagnostic ignored "-Wpass-failed"

namespace {

constexpr int SV_D = 20, SV_H = 40;  // the compile-time instantiation
constexpr int GW = 100, GD = 32;     // runtime-shaped instantiation: widest activation vector (3 D = H = 96), widest embedding

struct TrainDev {
    int D, H, L, act, mean, bias;
    const float* W[7][4];
    const float* b[7][4];
    int K[7][4], J[7][4];
    int oW[7][4], oB[7][4];  // offsets into grad_weights (order of host_arrays)
    const float* winv;       // [D][3]
    const float* binv;       // [3] or null
    int oWinv, oBinv, count;
};

template <bool FX> __device__ __forceinline__ int shD(const TrainDev& w) { if constexpr (FX) return SV_D; else return w.D; }
template <bool FX> __device__ __forceinline__ bool shMean(const TrainDev& w) { if constexpr (FX) return true; else return w.mean != 0; }

// ---- the scalar derivatives of fgnn_backward.hip (kept per file: the kernels of that file stay as they are) ----
__device__ __forceinline__ float tb_expm1(float t)
{
    t = FG_MIN(t, 60.0f);
    float tt = FG_FMA(t, FG_LOG2E, FG_RND_MAGIC);
    float k = tt - FG_RND_MAGIC;
    float r = FG_FMA(k, -FG_LN2_HI, t);
    r = FG_FMA(k, -FG_LN2_LO, r);
    float q = 1.381461043e-03f;
    q = FG_FMA(q, r, 8.368710056e-03f);
    q = FG_FMA(q, r, 4.166838899e-02f);
    q = FG_FMA(q, r, 1.666652113e-01f);
    q = FG_FMA(q, r, 4.999999404e-01f);
    float pm1 = FG_FMA(r * r, q, r);
    float sc = fg_u2f((fg_f2u(tt) << 23) + 0x3f800000u);
    return FG_FMA(sc, pm1, sc - 1.0f);
}
// d/dx of the clipped phi: -1/sinh(x) inside the clip interval, 0 outside
__device__ __forceinline__ float tb_dphi(float x)
{
    if (!(x >= FG_PHI_MIN && x <= FG_PHI_MAX)) return 0.0f;
    const float em1 = tb_expm1(x);
    return -(2.0f * (em1 + 1.0f)) / (em1 * (em1 + 2.0f));
}
__device__ __forceinline__ float tb_sigmoid(float x)
{
    const float e = fg_exp(-FG_MIN(FG_ABS(x), 87.0f));
    return x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}
__device__ __forceinline__ float tb_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ float tb_act_deriv(float h, int act)
{
    switch (act) {
    case FGNN_ACT_TANH: return 1.0f - h * h;
    case FGNN_ACT_RELU: return h > 0.0f ? 1.0f : 0.0f;
    case FGNN_ACT_SIGMOID: return h * (1.0f - h);
    default: return 1.0f;
    }
}

// logit_row_gnn of fgnn_gnnbp4.hip
__device__ __forceinline__ float tb_logit_row(const float* llr, const int* __restrict__ col, int deg)
{
    unsigned neg = 0;
    float T = 0.0f;
    for (int j = 0; j < deg; ++j) {
        float v = llr[col[j]];
        neg ^= (v < 0.0f);
        T = T + fg_phi_gnn(FG_ABS(v));
    }
    const float o = fg_phi_gnn(T);
    return neg ? -o : o;
}
// d loss / d T of a row times the row's sign, given d loss / d (row value)
__device__ __forceinline__ float tb_row_coef(const float* llr, const int* __restrict__ col, int deg, float up)
{
    unsigned neg = 0;
    float T = 0.0f;
    for (int j = 0; j < deg; ++j) {
        float v = llr[col[j]];
        neg ^= (v < 0.0f);
        T = T + fg_phi_gnn(FG_ABS(v));
    }
    return (neg ? -up : up) * tb_dphi(T);
}

// ---- one MLP, forward: the operations of gg_run (fgnn_gnnbp4.hip) ----
template <bool FX, int K0>
__device__ __forceinline__ void mlp_fwd(const TrainDev& w, int q, const float* x, float* out)
{
    if constexpr (FX) {
        scalar_fp W1 = as_scalar(w.W[q][0]), b1 = as_scalar(w.b[q][0]), W2 = as_scalar(w.W[q][1]), b2 = as_scalar(w.b[q][1]);
#pragma unroll
        for (int i = 0; i < SV_D; ++i) out[i] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < SV_H; ++j) {
            float a = 0.0f;
#pragma unroll
            for (int k = 0; k < K0; ++k) a = FG_FMA(x[k], W1[k * SV_H + j], a);
            const float h = fg_tanh(a + b1[j]);
#pragma unroll
            for (int i = 0; i < SV_D; ++i) out[i] = FG_FMA(h, W2[j * SV_D + i], out[i]);
        }
#pragma unroll
        for (int i = 0; i < SV_D; ++i) out[i] = out[i] + b2[i];
    } else {
        float bufA[GW], bufB[GW];
        const float* cur = x;
        for (int l = 0; l < w.L; ++l) {
            float* nxt = (l == w.L - 1) ? out : ((l & 1) ? bufB : bufA);
            const int K = w.K[q][l], J = w.J[q][l];
            const int act = l == w.L - 1 ? FGNN_ACT_LINEAR : w.act;
            const float* W = w.W[q][l];
            const float* bb = w.b[q][l];
            for (int j = 0; j < J; ++j) {
                float a = 0.0f;
                for (int kk = 0; kk < K; ++kk) a = FG_FMA(cur[kk], W[kk * J + j], a);
                if (bb) a = a + bb[j];
                nxt[j] = mlp_act(a, act);
            }
            cur = nxt;
        }
    }
}

// ---- weight-gradient staging ----
struct Stage {
    float* SA;   // [KA][lda] layer inputs, k-major: entry (k, row r) at k * lda + r, lda = threads + 1 (bank = k + r)
    float* SD;   // [threads][ldd] gradients at the pre-activations, row-major, ldd a multiple of 4
    int lda, ldd, nt, tid;
    int rows;    // staged rows of the chunk at hand (threads 0 .. rows-1; an idle one stages zeros)
    float* part; // the workgroup's partial gradient [count]
};

// pW[k][j] += sum_r SA[k][r] SD[r][j],  pB[j] += sum_r SD[r][j]; rows in ascending order, one owner per entry
__device__ __forceinline__ void accum_dw(const Stage& st, const float* SD, int K, int J, float* pW, float* pB)
{
    const int JQ = (J + 3) >> 2;
    for (int it = st.tid; it < K * JQ; it += st.nt) {
        const int k = it / JQ, j0 = (it - k * JQ) * 4;
        const float* ap = st.SA + k * st.lda;
        const float* dp = SD + j0;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        for (int r = 0; r < st.rows; ++r) {
            const float a = ap[r];
            const float4 d = *reinterpret_cast<const float4*>(dp + r * st.ldd);
            a0 = FG_FMA(a, d.x, a0);
            a1 = FG_FMA(a, d.y, a1);
            a2 = FG_FMA(a, d.z, a2);
            a3 = FG_FMA(a, d.w, a3);
        }
        float* o = pW + k * J + j0;
        o[0] += a0;
        if (j0 + 1 < J) o[1] += a1;
        if (j0 + 2 < J) o[2] += a2;
        if (j0 + 3 < J) o[3] += a3;
    }
    if (pB)
        for (int j = st.tid; j < J; j += st.nt) {
            float s = 0.0f;
            for (int r = 0; r < st.rows; ++r) s = s + SD[r * st.ldd + j];
            pB[j] += s;
        }
}

// ---- one MLP, reverse: dx = d loss / d x given dy = d loss / d (output), and the weight gradients of its layers.  Called by
// every thread of the workgroup (it synchronises); an idle thread (active = false) stages zero rows. ----
template <bool FX, int K0>
__device__ __forceinline__ void mlp_bwd(const TrainDev& w, int q, const float* x, const float* dy, float* dx, bool active, const Stage& st)
{
    const int r = st.tid;
    if constexpr (FX) {
        scalar_fp W1 = as_scalar(w.W[q][0]), b1 = as_scalar(w.b[q][0]), W2 = as_scalar(w.W[q][1]);
#pragma unroll
        for (int k = 0; k < K0; ++k) dx[k] = 0.0f;
        float* sd = st.SD + r * st.ldd;  // [delta of layer 1: SV_H | dy: SV_D]
        if (active) {
#pragma unroll 1
            for (int j = 0; j < SV_H; ++j) {
                float a = 0.0f;
#pragma unroll
                for (int k = 0; k < K0; ++k) a = FG_FMA(x[k], W1[k * SV_H + j], a);
                const float h = fg_tanh(a + b1[j]);
                float dh = 0.0f;
#pragma unroll
                for (int i = 0; i < SV_D; ++i) dh = FG_FMA(W2[j * SV_D + i], dy[i], dh);
                const float d1 = dh * (1.0f - h * h);
                st.SA[j * st.lda + r] = h;
                sd[j] = d1;
#pragma unroll
                for (int k = 0; k < K0; ++k) dx[k] = FG_FMA(W1[k * SV_H + j], d1, dx[k]);
            }
#pragma unroll
            for (int i = 0; i < SV_D; ++i) sd[SV_H + i] = dy[i];
        } else {
            for (int j = 0; j < SV_H; ++j) st.SA[j * st.lda + r] = 0.0f;
            for (int j = 0; j < SV_H + SV_D; ++j) sd[j] = 0.0f;
        }
        __syncthreads();
        accum_dw(st, st.SD + SV_H, SV_H, SV_D, st.part + w.oW[q][1], st.part + w.oB[q][1]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K0; ++k) st.SA[k * st.lda + r] = active ? x[k] : 0.0f;
        __syncthreads();
        accum_dw(st, st.SD, K0, SV_H, st.part + w.oW[q][0], st.part + w.oB[q][0]);
        __syncthreads();
    } else {
        float ha[4][GW];  // ha[l] = input of layer l
        float dA[GW], dB[GW];
        const int L = w.L;
        if (active) {
            const int Kin = w.K[q][0];
            for (int k = 0; k < Kin; ++k) ha[0][k] = x[k];
            for (int l = 0; l + 1 < L; ++l) {
                const int K = w.K[q][l], J = w.J[q][l];
                const float* W = w.W[q][l];
                const float* bb = w.b[q][l];
                for (int j = 0; j < J; ++j) {
                    float a = 0.0f;
                    for (int kk = 0; kk < K; ++kk) a = FG_FMA(ha[l][kk], W[kk * J + j], a);
                    if (bb) a = a + bb[j];
                    ha[l + 1][j] = mlp_act(a, w.act);
                }
            }
            for (int j = 0; j < w.J[q][L - 1]; ++j) dA[j] = dy[j];
        }
        float* dc = dA;
        float* dn = dB;
        for (int l = L - 1; l >= 0; --l) {
            const int K = w.K[q][l], J = w.J[q][l], Jp = (J + 3) & ~3;
            if (active && l < L - 1)
                for (int j = 0; j < J; ++j) dc[j] = dc[j] * tb_act_deriv(ha[l + 1][j], w.act);
            for (int k = 0; k < K; ++k) st.SA[k * st.lda + r] = active ? ha[l][k] : 0.0f;
            for (int j = 0; j < Jp; ++j) st.SD[r * st.ldd + j] = (active && j < J) ? dc[j] : 0.0f;
            __syncthreads();
            accum_dw(st, st.SD, K, J, st.part + w.oW[q][l], w.bias ? st.part + w.oB[q][l] : nullptr);
            __syncthreads();
            if (active) {
                const float* W = w.W[q][l];
                for (int k = 0; k < K; ++k) {
                    float a = 0.0f;
                    for (int j = 0; j < J; ++j) a = FG_FMA(W[k * J + j], dc[j], a);
                    dn[k] = a;
                }
            }
            float* t = dc;
            dc = dn;
            dn = t;
        }
        if (active)
            for (int k = 0; k < w.K[q][0]; ++k) dx[k] = dc[k];
    }
}

// ---- tape layout: codeword b, iteration k at tape + (b T + k) S, S = (n + m) D + m ----
struct TapeView {
    float *hv, *hc, *hl;
};
__device__ __forceinline__ TapeView tape_at(float* tape, const GraphDev& g, int D, int T, int b, int k)
{
    const size_t S = (size_t)(g.n + g.m) * D + g.m;
    TapeView t;
    t.hv = tape + ((size_t)b * T + k) * S;
    t.hc = t.hv + (size_t)g.n * D;
    t.hl = t.hc + (size_t)g.m * D;
    return t;
}

struct FwdArgs {
    int B, T;
    const uint8_t* synd_x;
    const uint8_t* synd_z;
    float* xlog_all;  // [T,B,m_z+rows(lz)]
    float* zlog_all;  // [T,B,m_x+rows(lx)]
    float* tape;
};

// the three LLRs of a qubit from its embedding (embed_to_llr) — the chain of gnn_bp4_general_kernel
template <bool FX>
__device__ __forceinline__ void llr_of(const TrainDev& w, const float* hv, float (&Lv)[3])
{
    const int D = shD<FX>(w);
    Lv[0] = Lv[1] = Lv[2] = 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        Lv[0] = FG_FMA(hv[k], w.winv[k * 3 + 0], Lv[0]);
        Lv[1] = FG_FMA(hv[k], w.winv[k * 3 + 1], Lv[1]);
        Lv[2] = FG_FMA(hv[k], w.winv[k * 3 + 2], Lv[2]);
    }
    if (w.binv) {
        Lv[0] = Lv[0] + w.binv[0];
        Lv[1] = Lv[1] + w.binv[1];
        Lv[2] = Lv[2] + w.binv[2];
    }
}

// the (signed) reduced message of one side of qubit v: sum_e sg_e MLP([hc[c_e] | own]) (/ deg)
template <bool FX>
__device__ __forceinline__ void vn_side_fwd(const GraphDev& g, const TrainDev& w, int s, int v, const float* hc, const float* ssg,
                                            const float* own, float* acc)
{
    constexpr int MW = FX ? 3 * SV_D : GW, MD = FX ? SV_D : GD;
    const int D = shD<FX>(w);
    const int* vptr = s ? g.vptr_z : g.vptr_x;
    const int e0 = vptr[v], e1 = vptr[v + 1];
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] = 0.0f;
    for (int e = e0; e < e1; ++e) {
        const int c = (s ? g.m_x : 0) + g.vchk[e];
        const float* src = hc + (size_t)c * D;
        float feat[MW], msg[MD];
#pragma unroll
        for (int i = 0; i < D; ++i) { feat[i] = src[i]; feat[D + i] = own[i]; }
        mlp_fwd<FX, 2 * SV_D>(w, 4 + s, feat, msg);
        const float sg = ssg[c];
#pragma unroll
        for (int i = 0; i < D; ++i) { const float mv = msg[i] * sg; acc[i] = (e == e0) ? mv : acc[i] + mv; }
    }
    if (shMean<FX>(w) && e1 > e0) {
        const float fd = (float)(e1 - e0);
#pragma unroll
        for (int i = 0; i < D; ++i) acc[i] = acc[i] / fd;
    }
}
// the reduced message of check c (combined id): sum_e MLP([hv[v_e] | own]) (/ deg); hv null = the initial embeddings (ones)
template <bool FX>
__device__ __forceinline__ void cn_side_fwd(const GraphDev& g, const TrainDev& w, int s, int c, const float* hv, const float* own, float* acc)
{
    constexpr int MW = FX ? 3 * SV_D : GW, MD = FX ? SV_D : GD;
    const int D = shD<FX>(w);
    const int p0 = g.cptr[c], p1 = g.cptr[c + 1];
#pragma unroll
    for (int i = 0; i < D; ++i) acc[i] = 0.0f;
    for (int p = p0; p < p1; ++p) {
        float feat[MW], msg[MD];
        if (hv) {
            const float* src = hv + (size_t)g.cvn[p] * D;
#pragma unroll
            for (int i = 0; i < D; ++i) feat[i] = src[i];
        } else {
#pragma unroll
            for (int i = 0; i < D; ++i) feat[i] = 1.0f;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) feat[D + i] = own[i];
        mlp_fwd<FX, 2 * SV_D>(w, s, feat, msg);
#pragma unroll
        for (int i = 0; i < D; ++i) acc[i] = (p == p0) ? msg[i] : acc[i] + msg[i];
    }
    if (shMean<FX>(w) && p1 > p0) {
        const float fd = (float)(p1 - p0);
#pragma unroll
        for (int i = 0; i < D; ++i) acc[i] = acc[i] / fd;
    }
}

template <bool FX>
__global__ void __launch_bounds__(256) gnn_bp4_tape_kernel(GraphDev g, TrainDev w, FwdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ float lds[];
    constexpr int MW = FX ? 3 * SV_D : GW, MD = FX ? SV_D : GD;
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int n = g.n, mx = g.m_x, mz = g.m_z, m = g.m, D = shD<FX>(w), T = a.T;
    float* lx = lds;
    float* lz = lx + n;
    float* ssg = lz + n;
    const uint8_t* sx = a.synd_x + (size_t)b * mx;
    const uint8_t* sz = a.synd_z + (size_t)b * mz;
    for (int c = tid; c < m; c += NT) ssg[c] = synd_sign(c < mx ? sx[c] : sz[c - mx]);
    __syncthreads();
    for (int it = -1; it < T; ++it) {
        if (it >= 0) {
            const TapeView tk = tape_at(a.tape, g, D, T, b, it);
            const float* hvp = it > 0 ? tape_at(a.tape, g, D, T, b, it - 1).hv : nullptr;
            // ---- UpdateVNEmbeddings + embed_to_llr + the binary LLRs of cal_logit ----
            for (int v = tid; v < n; v += NT) {
                float own[MD], feat[MW], nh[MD];
#pragma unroll
                for (int i = 0; i < D; ++i) own[i] = hvp ? hvp[(size_t)v * D + i] : 1.0f;
                vn_side_fwd<FX>(g, w, 0, v, tk.hc, ssg, own, feat);
                vn_side_fwd<FX>(g, w, 1, v, tk.hc, ssg, own, feat + D);
#pragma unroll
                for (int i = 0; i < D; ++i) feat[2 * D + i] = own[i];
                mlp_fwd<FX, 3 * SV_D>(w, 6, feat, nh);
#pragma unroll
                for (int i = 0; i < D; ++i) tk.hv[(size_t)v * D + i] = nh[i];
                float Lv[3];
                llr_of<FX>(w, nh, Lv);
                vn_binary_llrs<VnMath>(Lv[0], Lv[1], Lv[2], lx[v], lz[v]);
            }
            __syncthreads();
            // ---- soft syndromes: hx rows on llr_z, hz rows on llr_x, logical rows appended ----
            float* xl = a.xlog_all + ((size_t)it * a.B + b) * (mz + g.rows[5]);
            float* zl = a.zlog_all + ((size_t)it * a.B + b) * (mx + g.rows[4]);
            for (int c = tid; c < m; c += NT) {
                const int p0 = g.cptr[c];
                const float vq = tb_logit_row(c < mx ? lz : lx, g.cvn + p0, g.cptr[c + 1] - p0);
                tk.hl[c] = vq;
                if (c < mx) zl[c] = vq;
                else xl[c - mx] = vq;
            }
            for (int r = tid; r < g.rows[5]; r += NT) xl[mz + r] = tb_logit_row(lx, g.rcol[5] + g.rptr[5][r], g.rptr[5][r + 1] - g.rptr[5][r]);
            for (int r = tid; r < g.rows[4]; r += NT) zl[mx + r] = tb_logit_row(lz, g.rcol[4] + g.rptr[4][r], g.rptr[4][r + 1] - g.rptr[4][r]);
            __syncthreads();
            if (it == T - 1) break;
        }
        // ---- UpdateCNEmbeddings: h_cn^(it+1) from h_vn^(it), h_cn^(it), hlog^(it) (it = -1: ones, zeros, zero logits) ----
        const TapeView tn = tape_at(a.tape, g, D, T, b, it + 1);
        const float* hvp = it >= 0 ? tape_at(a.tape, g, D, T, b, it).hv : nullptr;
        const float* hcp = it >= 0 ? tape_at(a.tape, g, D, T, b, it).hc : nullptr;
        const float* hlp = it >= 0 ? tape_at(a.tape, g, D, T, b, it).hl : nullptr;
        auto side = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const int c0 = s ? mx : 0, cnt = s ? mz : mx;
            for (int cl = tid; cl < cnt; cl += NT) {
                const int c = c0 + cl;
                float own[MD], feat[MW], nh[MD];
#pragma unroll
                for (int i = 0; i < D; ++i) own[i] = hcp ? hcp[(size_t)c * D + i] : 0.0f;
                cn_side_fwd<FX>(g, w, s, c, hvp, own, feat);
#pragma unroll
                for (int i = 0; i < D; ++i) feat[D + i] = own[i];
                feat[2 * D] = hlp ? hlp[c] * ssg[c] : 0.0f;
                mlp_fwd<FX, 2 * SV_D + 1>(w, 2 + s, feat, nh);
#pragma unroll
                for (int i = 0; i < D; ++i) tn.hc[(size_t)c * D + i] = nh[i];
            }
        };
        side(std::integral_constant<int, 0>{});
        side(std::integral_constant<int, 1>{});
        __syncthreads();
    }
}

struct BwdArgs {
    int B, T;
    const uint8_t* synd_x;
    const uint8_t* synd_z;
    float* tape;       // read only here
    const float* gx;   // [T,B,m_z+rows(lz)] or null
    const float* gz;   // [T,B,m_x+rows(lx)] or null
    float* work;       // per workgroup: gV [n][D] | gC [m][D] | gE [E][D] | glog [m] | partial gradient [count]
    size_t wg_floats;
    int lds_sa;        // floats of the SA region
    int ldd;
};

template <bool FX>
__global__ void __launch_bounds__(256) gnn_bp4_backward_kernel(GraphDev g, TrainDev w, BwdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ float lds[];
    constexpr int MW = FX ? 3 * SV_D : GW, MD = FX ? SV_D : GD;
    const int tid = threadIdx.x, NT = blockDim.x;
    const int n = g.n, mx = g.m_x, mz = g.m_z, m = g.m, D = shD<FX>(w), T = a.T;
    const int R5 = g.rows[5], R4 = g.rows[4];
    float* lx = lds;
    float* lz = lx + n;
    float* dlx = lz + n;
    float* dlz = dlx + n;
    float* ssg = dlz + n;
    float* coef = ssg + m;
    float* coefL = coef + m;  // [R5 lz rows | R4 lx rows]
    const int misc = (4 * n + 2 * m + R5 + R4 + 3) & ~3;
    float* gV = a.work + (size_t)blockIdx.x * a.wg_floats;
    float* gC = gV + (size_t)n * D;
    float* gE = gC + (size_t)m * D;
    float* glog = gE + (size_t)g.E * D;
    Stage st;
    st.SA = lds + misc;
    st.SD = st.SA + a.lds_sa;
    st.lda = NT + 1;
    st.ldd = a.ldd;
    st.nt = NT;
    st.tid = tid;
    st.rows = 0;
    st.part = glog + m;
    for (int i = tid; i < w.count; i += NT) st.part[i] = 0.0f;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        __syncthreads();
        const uint8_t* sx = a.synd_x + (size_t)b * mx;
        const uint8_t* sz = a.synd_z + (size_t)b * mz;
        for (int c = tid; c < m; c += NT) ssg[c] = synd_sign(c < mx ? sx[c] : sz[c - mx]);
        for (int k = T - 1; k >= 0; --k) {
            const bool last = k == T - 1;
            const TapeView tk = tape_at(a.tape, g, D, T, b, k);
            const TapeView tp = tape_at(a.tape, g, D, T, b, k > 0 ? k - 1 : 0);
            const float* hvp = k > 0 ? tp.hv : nullptr;  // h_vn^(k-1): null = ones
            const float* hcp = k > 0 ? tp.hc : nullptr;  // h_cn^(k-1): null = zeros
            const float* hlp = k > 0 ? tp.hl : nullptr;  // hlog^(k-1): null = zero logits
            __syncthreads();
            // ---- S: soft syndromes of iteration k ----
            for (int v = tid; v < n; v += NT) {
                float hv[MD], Lv[3];
#pragma unroll
                for (int i = 0; i < D; ++i) hv[i] = tk.hv[(size_t)v * D + i];
                llr_of<FX>(w, hv, Lv);
                vn_binary_llrs<VnMath>(Lv[0], Lv[1], Lv[2], lx[v], lz[v]);
                dlx[v] = 0.0f;
                dlz[v] = 0.0f;
            }
            __syncthreads();
            {
                const float* gxk = a.gx ? a.gx + ((size_t)k * a.B + b) * (mz + R5) : nullptr;
                const float* gzk = a.gz ? a.gz + ((size_t)k * a.B + b) * (mx + R4) : nullptr;
                for (int c = tid; c < m; c += NT) {
                    float up = c < mx ? (gzk ? gzk[c] : 0.0f) : (gxk ? gxk[c - mx] : 0.0f);
                    if (!last) up = up + glog[c] * ssg[c];  // the logit that entered the next CN update, times the syndrome sign
                    const int p0 = g.cptr[c];
                    coef[c] = tb_row_coef(c < mx ? lz : lx, g.cvn + p0, g.cptr[c + 1] - p0, up);
                }
                for (int r = tid; r < R5; r += NT)
                    coefL[r] = tb_row_coef(lx, g.rcol[5] + g.rptr[5][r], g.rptr[5][r + 1] - g.rptr[5][r], gxk ? gxk[mz + r] : 0.0f);
                for (int r = tid; r < R4; r += NT)
                    coefL[R5 + r] = tb_row_coef(lz, g.rcol[4] + g.rptr[4][r], g.rptr[4][r + 1] - g.rptr[4][r], gzk ? gzk[mx + r] : 0.0f);
            }
            __syncthreads();
            // logical rows into their qubits, one row at a time (a row's qubits are distinct)
            for (int r = 0; r < R5; ++r) {
                for (int p = g.rptr[5][r] + tid; p < g.rptr[5][r + 1]; p += NT) dlx[g.rcol[5][p]] += coefL[r];
                __syncthreads();
            }
            for (int r = 0; r < R4; ++r) {
                for (int p = g.rptr[4][r] + tid; p < g.rptr[4][r + 1]; p += NT) dlz[g.rcol[4][p]] += coefL[R5 + r];
                __syncthreads();
            }
            for (int c0 = 0; c0 < n; c0 += NT) {
                const int v = c0 + tid;
                const bool active = v < n;
                st.rows = min(NT, n - c0);
                float hv[MD], dL[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (active) {
                    float Lv[3];
#pragma unroll
                    for (int i = 0; i < D; ++i) hv[i] = tk.hv[(size_t)v * D + i];
                    llr_of<FX>(w, hv, Lv);
                    const float X = Lv[0], Y = Lv[1], Z = Lv[2], lxv = lx[v], lzv = lz[v];
                    float gxl = dlx[v], gzl = dlz[v];
                    for (int e = g.vptr_z[v]; e < g.vptr_z[v + 1]; ++e) gxl = gxl + coef[mx + g.vchk[e]];
                    for (int e = g.vptr_x[v]; e < g.vptr_x[v + 1]; ++e) gzl = gzl + coef[g.vchk[e]];
                    gxl = gxl * tb_dphi(FG_ABS(lxv)) * tb_sign(lxv);
                    gzl = gzl * tb_dphi(FG_ABS(lzv)) * tb_sign(lzv);
                    // llr_x = softplus(-Z) - lse(-X,-Y);  llr_z = softplus(-X) - lse(-Z,-Y)
                    const float wx = tb_sigmoid(Y - X), wz = tb_sigmoid(Y - Z);
                    dL[0] = gxl * wx - gzl * tb_sigmoid(-X);
                    dL[2] = gzl * wz - gxl * tb_sigmoid(-Z);
                    dL[1] = gxl * (1.0f - wx) + gzl * (1.0f - wz);
                    float gv[MD];
#pragma unroll
                    for (int i = 0; i < D; ++i)
                        gv[i] = FG_FMA(w.winv[i * 3 + 2], dL[2], FG_FMA(w.winv[i * 3 + 1], dL[1], w.winv[i * 3 + 0] * dL[0]));
                    if (!last) {  // + what the VN update of iteration k+1 left for its own input, + the CN update's edges
#pragma unroll
                        for (int i = 0; i < D; ++i) gv[i] = gv[i] + gV[(size_t)v * D + i];
                        for (int e = g.vptr_x[v]; e < g.vptr_x[v + 1]; ++e)
#pragma unroll
                            for (int i = 0; i < D; ++i) gv[i] = gv[i] + gE[(size_t)e * D + i];
                        for (int e = g.vptr_z[v]; e < g.vptr_z[v + 1]; ++e)
#pragma unroll
                            for (int i = 0; i < D; ++i) gv[i] = gv[i] + gE[(size_t)e * D + i];
                    }
#pragma unroll
                    for (int i = 0; i < D; ++i) gV[(size_t)v * D + i] = gv[i];
                }
#pragma unroll
                for (int i = 0; i < D; ++i) st.SA[i * st.lda + tid] = active ? hv[i] : 0.0f;
#pragma unroll
                for (int j = 0; j < 4; ++j) st.SD[tid * st.ldd + j] = dL[j];
                __syncthreads();
                accum_dw(st, st.SD, D, 3, st.part + w.oWinv, w.binv ? st.part + w.oBinv : nullptr);
                __syncthreads();
            }
            // ---- V: the VN update of iteration k ----
            for (int c0 = 0; c0 < n; c0 += NT) {
                const int v = c0 + tid;
                const bool active = v < n;
                st.rows = min(NT, n - c0);
                float own[MD], down[MD], feat[MW], dfeat[MW];
#pragma unroll
                for (int i = 0; i < D; ++i) own[i] = 0.0f;
                {
                    float dy[MD];
#pragma unroll
                    for (int i = 0; i < D; ++i) dy[i] = 0.0f;
                    if (active) {
#pragma unroll
                        for (int i = 0; i < D; ++i) {
                            own[i] = hvp ? hvp[(size_t)v * D + i] : 1.0f;
                            dy[i] = gV[(size_t)v * D + i];
                        }
                        vn_side_fwd<FX>(g, w, 0, v, tk.hc, ssg, own, feat);
                        vn_side_fwd<FX>(g, w, 1, v, tk.hc, ssg, own, feat + D);
#pragma unroll
                        for (int i = 0; i < D; ++i) feat[2 * D + i] = own[i];
                    }
                    mlp_bwd<FX, 3 * SV_D>(w, 6, feat, dy, dfeat, active, st);
                }
#pragma unroll
                for (int i = 0; i < D; ++i) down[i] = dfeat[2 * D + i];
                auto side = [&](auto sc) {
                    constexpr int s = decltype(sc)::value;
                    const int* vptr = s ? g.vptr_z : g.vptr_x;
                    const int e0 = active ? vptr[v] : 0, e1 = active ? vptr[v + 1] : 0;
                    const float fd = (float)(e1 - e0);
                    for (int es = 0; __syncthreads_or(e0 + es < e1); ++es) {
                        const int e = e0 + es;
                        const bool ea = e < e1;
                        float fe[MW], dm[MD], dfe[MW];
#pragma unroll
                        for (int i = 0; i < D; ++i) dm[i] = 0.0f;
                        if (ea) {
                            const int c = (s ? mx : 0) + g.vchk[e];
                            const float* src = tk.hc + (size_t)c * D;
                            const float sg = ssg[c];
#pragma unroll
                            for (int i = 0; i < D; ++i) {
                                fe[i] = src[i];
                                fe[D + i] = own[i];
                                const float da = dfeat[s * D + i];
                                dm[i] = (shMean<FX>(w) ? da / fd : da) * sg;
                            }
                        }
                        mlp_bwd<FX, 2 * SV_D>(w, 4 + s, fe, dm, dfe, ea, st);
                        if (ea) {
#pragma unroll
                            for (int i = 0; i < D; ++i) {
                                gE[(size_t)e * D + i] = dfe[i];  // to the check at the other end
                                down[i] = down[i] + dfe[D + i];
                            }
                        }
                    }
                };
                side(std::integral_constant<int, 0>{});
                side(std::integral_constant<int, 1>{});
                if (active) {
#pragma unroll
                    for (int i = 0; i < D; ++i) gV[(size_t)v * D + i] = down[i];  // d loss / d h_vn^(k-1), this path
                }
            }
            __syncthreads();
            // ---- C: the CN update that produced h_cn^(k) ----
            auto cside = [&](auto sc) {
                constexpr int s = decltype(sc)::value;
                const int cb = s ? mx : 0, cnt = s ? mz : mx;
                for (int c0 = 0; c0 < cnt; c0 += NT) {
                    const int c = cb + c0 + tid;
                    const bool active = c0 + tid < cnt;
                    st.rows = min(NT, cnt - c0);
                    const int p0 = active ? g.cptr[c] : 0, p1 = active ? g.cptr[c + 1] : 0;
                    const float fd = (float)(p1 - p0);
                    float own[MD], down[MD], feat[MW], dfeat[MW];
#pragma unroll
                    for (int i = 0; i < D; ++i) own[i] = 0.0f;
                    {
                        float dy[MD];
#pragma unroll
                        for (int i = 0; i < D; ++i) dy[i] = 0.0f;
                        if (active) {
#pragma unroll
                            for (int i = 0; i < D; ++i) {
                                own[i] = hcp ? hcp[(size_t)c * D + i] : 0.0f;
                                dy[i] = last ? 0.0f : gC[(size_t)c * D + i];
                            }
                            for (int p = p0; p < p1; ++p) {
                                const float* ge = gE + (size_t)g.cslot[p] * D;
#pragma unroll
                                for (int i = 0; i < D; ++i) dy[i] = dy[i] + ge[i];
                            }
                            cn_side_fwd<FX>(g, w, s, c, hvp, own, feat);
#pragma unroll
                            for (int i = 0; i < D; ++i) feat[D + i] = own[i];
                            feat[2 * D] = hlp ? hlp[c] * ssg[c] : 0.0f;
                        }
                        mlp_bwd<FX, 2 * SV_D + 1>(w, 2 + s, feat, dy, dfeat, active, st);
                    }
#pragma unroll
                    for (int i = 0; i < D; ++i) down[i] = dfeat[D + i];
                    if (active) glog[c] = dfeat[2 * D];
                    for (int es = 0; __syncthreads_or(p0 + es < p1); ++es) {
                        const int p = p0 + es;
                        const bool ea = p < p1;
                        float fe[MW], dm[MD], dfe[MW];
#pragma unroll
                        for (int i = 0; i < D; ++i) dm[i] = 0.0f;
                        if (ea) {
                            const float* src = hvp ? hvp + (size_t)g.cvn[p] * D : nullptr;
#pragma unroll
                            for (int i = 0; i < D; ++i) {
                                fe[i] = src ? src[i] : 1.0f;
                                fe[D + i] = own[i];
                                dm[i] = shMean<FX>(w) ? dfeat[i] / fd : dfeat[i];
                            }
                        }
                        mlp_bwd<FX, 2 * SV_D>(w, s, fe, dm, dfe, ea, st);
                        if (ea) {
                            float* ge = gE + (size_t)g.cslot[p] * D;
#pragma unroll
                            for (int i = 0; i < D; ++i) {
                                ge[i] = dfe[i];  // to the qubit at the other end
                                down[i] = down[i] + dfe[D + i];
                            }
                        }
                    }
                    if (active) {
#pragma unroll
                        for (int i = 0; i < D; ++i) gC[(size_t)c * D + i] = down[i];  // d loss / d h_cn^(k-1), this path
                    }
                }
            };
            cside(std::integral_constant<int, 0>{});
            cside(std::integral_constant<int, 1>{});
        }
    }
}

// grad[p] = sum over workgroups, ascending
__global__ void __launch_bounds__(256) gnn_bp4_grad_reduce_kernel(const float* work, size_t wg_floats, size_t part_off, int nwg, int count,
                                                                   float* grad)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= count) return;
    float s = 0.0f;
    for (int wg = 0; wg < nwg; ++wg) s = s + work[(size_t)wg * wg_floats + part_off + p];
    grad[p] = s;
}

constexpr int BWD_MAX_WG = 512;  // workgroups of the reverse pass: codeword b goes to workgroup b mod this

// The device view of a runtime-shaped handle, or the reason it cannot be trained here
int train_view(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, TrainDev* t)
{
    if (!g || !w) return fgnn_fail(FGNN_ERR_ARG, "graph or weights is NULL");
    fgnn_gnnbp4_train_view v;
    if (!fgnn_gnnbp4_weights_train_view(w, &v))
        return fgnn_fail(FGNN_ERR_ARG, "the GNN_BP4 tape and reverse pass take weights made by fgnn_gnnbp4_weights_create_general");
    if (v.device != g->device) return fgnn_fail(FGNN_ERR_ARG, "weights and graph live on different devices");
    if (v.use_attributes) return fgnn_fail(FGNN_ERR_ARG, "use_attributes=True has no reverse pass");
    if (v.reduce_op != FGNN_REDUCE_SUM && v.reduce_op != FGNN_REDUCE_MEAN)
        return fgnn_fail(FGNN_ERR_ARG, "reduce_op max / min has no reverse pass (sum and mean do)");
    std::memset(t, 0, sizeof(*t));
    t->D = v.D; t->H = v.H; t->L = v.L; t->act = v.act; t->mean = v.reduce_op == FGNN_REDUCE_MEAN; t->bias = v.bias;
    int pos = 0;
    for (int q = 0; q < 7; ++q)
        for (int l = 0; l < v.L; ++l) {
            t->W[q][l] = v.W[q][l];
            t->b[q][l] = v.b[q][l];
            t->K[q][l] = v.K[q][l];
            t->J[q][l] = v.J[q][l];
            t->oW[q][l] = pos;
            pos += v.K[q][l] * v.J[q][l];
            t->oB[q][l] = pos;
            if (v.bias) pos += v.J[q][l];
        }
    t->winv = v.winv;
    t->binv = v.binv;
    t->oWinv = pos;
    pos += v.D * 3;
    t->oBinv = pos;
    if (v.bias) pos += 3;
    t->count = pos;
    return FGNN_OK;
}

bool is_survey(const fgnn_graph* g, const TrainDev& t)
{
    return !g->force_generic && t.D == SV_D && t.H == SV_H && t.L == 2 && t.act == FGNN_ACT_TANH && t.mean && t.bias;
}

size_t tape_floats(const fgnn_graph* g, const TrainDev& t, int T, int B)
{
    return (size_t)B * T * ((size_t)(g->d.n + g->d.m) * t.D + g->d.m);
}

struct BwdPlan {
    int nwg, threads, lds_sa, ldd;
    size_t wg_floats, part_off, lds_bytes;
};
// launch shape of the reverse pass: the largest workgroup whose staged rows fit in LDS next to the soft-syndrome state
int bwd_plan(const fgnn_graph* g, const TrainDev& t, int B, BwdPlan* p)
{
    const GraphDev& d = g->d;
    int KA = t.D, JD = 4;
    if (is_survey(g, t)) {
        KA = 3 * SV_D;
        JD = SV_H + SV_D;
    } else
        for (int q = 0; q < 7; ++q)
            for (int l = 0; l < t.L; ++l) {
                KA = std::max(KA, t.K[q][l]);
                JD = std::max(JD, (t.J[q][l] + 3) & ~3);
            }
    const size_t misc = (size_t)((4 * d.n + 2 * d.m + d.rows[4] + d.rows[5] + 3) & ~3);
    p->threads = 0;
    for (int nt : {256, 128, 64}) {
        const size_t sa = ((size_t)KA * (nt + 1) + 3) & ~size_t(3);
        const size_t bytes = (misc + sa + (size_t)nt * JD) * sizeof(float);
        if (bytes <= FGNN_LDS_BUDGET) {
            p->threads = nt;
            p->lds_sa = (int)sa;
            p->lds_bytes = bytes;
            break;
        }
    }
    if (!p->threads) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident part of the GNN_BP4 reverse pass");
    p->ldd = JD;
    p->nwg = std::min(B, BWD_MAX_WG);
    p->part_off = (size_t)(d.n + d.m + d.E) * t.D + d.m;
    p->wg_floats = (p->part_off + t.count + 3) & ~size_t(3);
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_gnnbp4_grad_count(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int* count)
{
    TrainDev t;
    if (!count) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    if (int rc = train_view(g, w, &t)) return rc;
    *count = t.count;
    return FGNN_OK;
}

extern "C" int fgnn_gnnbp4_tape_bytes(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, int B, size_t* bytes)
{
    TrainDev t;
    if (!bytes) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    if (num_iter < 1 || B < 0) return fgnn_fail(FGNN_ERR_ARG, "num_iter must be >= 1 and B >= 0");
    if (int rc = train_view(g, w, &t)) return rc;
    *bytes = tape_floats(g, t, num_iter, B) * sizeof(float);
    return FGNN_OK;
}

extern "C" int fgnn_gnnbp4_backward_workspace_bytes(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int B, size_t* bytes)
{
    TrainDev t;
    BwdPlan p;
    if (!bytes) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (int rc = train_view(g, w, &t)) return rc;
    if (int rc = bwd_plan(g, t, B, &p)) return rc;
    *bytes = (size_t)p.nwg * p.wg_floats * sizeof(float);
    return FGNN_OK;
}

extern "C" int fgnn_gnnbp4_forward_tape(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, const uint8_t* synd_x,
                                        const uint8_t* synd_z, int B, float* x_logit_all, float* z_logit_all, float* tape,
                                        size_t tape_bytes, void* stream)
{
    TrainDev t;
    if (int rc = train_view(g, w, &t)) return rc;
    if (num_iter < 1 || B < 0) return fgnn_fail(FGNN_ERR_ARG, "num_iter must be >= 1 and B >= 0");
    if (!g->d.rptr[4] || !g->d.rptr[5]) return fgnn_fail(FGNN_ERR_STATE, "lx / lz row sets not installed (fgnn_graph_set_rows 4, 5)");
    if (B == 0) return FGNN_OK;
    if (!synd_x || !synd_z || !x_logit_all || !z_logit_all || !tape) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    const size_t need = tape_floats(g, t, num_iter, B) * sizeof(float);
    if (tape_bytes < need)
        return fgnn_fail(FGNN_ERR_ARG, "tape too small: " + std::to_string(tape_bytes) + " bytes given, " + std::to_string(need) + " needed");
    const size_t lds_bytes = (size_t)(2 * g->d.n + g->d.m) * sizeof(float);
    if (lds_bytes > FGNN_LDS_BUDGET) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident part of the GNN_BP4 tape forward");
    FGNN_DEVICE_GUARD(g->device);
    const FwdArgs a{B, num_iter, synd_x, synd_z, x_logit_all, z_logit_all, tape};
    auto kern = is_survey(g, t) ? gnn_bp4_tape_kernel<true> : gnn_bp4_tape_kernel<false>;
    return fgnn_launch(kern, dim3(B), dim3(256), lds_bytes, static_cast<hipStream_t>(stream), g->d, t, a);
}

extern "C" int fgnn_gnnbp4_backward(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, const uint8_t* synd_x,
                                    const uint8_t* synd_z, int B, const float* tape, size_t tape_bytes, const float* grad_x_logit_all,
                                    const float* grad_z_logit_all, float* grad_weights, int grad_count, void* workspace,
                                    size_t ws_bytes, void* stream)
{
    TrainDev t;
    BwdPlan p;
    if (int rc = train_view(g, w, &t)) return rc;
    if (num_iter < 1 || B < 0) return fgnn_fail(FGNN_ERR_ARG, "num_iter must be >= 1 and B >= 0");
    if (!g->d.rptr[4] || !g->d.rptr[5]) return fgnn_fail(FGNN_ERR_STATE, "lx / lz row sets not installed (fgnn_graph_set_rows 4, 5)");
    if (!grad_weights) return fgnn_fail(FGNN_ERR_ARG, "grad_weights is NULL");
    if (grad_count != t.count)
        return fgnn_fail(FGNN_ERR_ARG, "grad_weights holds " + std::to_string(grad_count) + " floats, this configuration has " +
                                           std::to_string(t.count));
    FGNN_DEVICE_GUARD(g->device);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (B == 0) {
        FGNN_HIP_CHECK(hipMemsetAsync(grad_weights, 0, (size_t)t.count * sizeof(float), s));
        return FGNN_OK;
    }
    if (!synd_x || !synd_z || !tape || !workspace) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    const size_t need_tape = tape_floats(g, t, num_iter, B) * sizeof(float);
    if (tape_bytes < need_tape)
        return fgnn_fail(FGNN_ERR_ARG, "tape too small: " + std::to_string(tape_bytes) + " bytes given, " + std::to_string(need_tape) + " needed");
    if (int rc = bwd_plan(g, t, B, &p)) return rc;
    const size_t need_ws = (size_t)p.nwg * p.wg_floats * sizeof(float);
    if (ws_bytes < need_ws)
        return fgnn_fail(FGNN_ERR_ARG, "workspace too small: " + std::to_string(ws_bytes) + " bytes given, " + std::to_string(need_ws) + " needed");
    BwdArgs a;
    a.B = B;
    a.T = num_iter;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.tape = const_cast<float*>(tape);
    a.gx = grad_x_logit_all;
    a.gz = grad_z_logit_all;
    a.work = static_cast<float*>(workspace);
    a.wg_floats = p.wg_floats;
    a.lds_sa = p.lds_sa;
    a.ldd = p.ldd;
    auto kern = is_survey(g, t) ? gnn_bp4_backward_kernel<true> : gnn_bp4_backward_kernel<false>;
    if (int rc = fgnn_launch(kern, dim3(p.nwg), dim3(p.threads), p.lds_bytes, s, g->d, t, a)) return rc;
    return fgnn_launch(gnn_bp4_grad_reduce_kernel, dim3((t.count + 255) / 256), dim3(256), 0, s, static_cast<const float*>(workspace),
                       p.wg_floats, p.part_off, p.nwg, t.count, grad_weights);
}
