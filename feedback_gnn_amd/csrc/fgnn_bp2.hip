// fgnn_bp2.hip — binary syndrome belief propagation on one Tanner graph, LDS-resident.
//
// Replaces LDPCBPDecoder.call with is_syndrome=True of /root/reference sionna/fec/ldpc/decoding.py:874-1048
// (the fork's additions to upstream Sionna: syndrome sign :905-908 applied inside the check-node rules :595, :658,
// :767; normalization_factor :991) and the BSC draw of BP_BSC_Model.call (feedback_gnn.py:213-214).  SURVEY.md §8(f)
// rank 1: same check-node rules as BP4 with one LLR per bit and a linear variable-node update.
//
// The parity-check matrix is side 0 (hx) of an fgnn_graph.  One workgroup holds the E_x messages of its codeword(s)
// in LDS for all iterations; the variable-node phase is a sum and a subtraction per edge, the check-node phase is
// the phi / min-sum / tanh rule (phi in its log(exp(x)+1) - log(exp(x)-1) form, decoding.py:632-633).
// Bit-identical to oracle/fgnn_oracle.c: og_bp2_decode.
#include <cstdlib>

#include "fgnn_step.h"
#include "fgnn_cn.h"
#include "fgnn_cn2.h"
#include "fgnn_rng.h"

#ifndef FGNN_BP2_WAVES
#define FGNN_BP2_WAVES 6  // waves per SIMD the register allocation aims at
#endif

namespace {

struct Bp2Args {
    int B, num_iter, tpc, cpb, lds_per_cw;
    float factor, llr_const;
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null (all-zero syndrome)
    float* soft_out;       // [B,n] or null
    uint8_t* hard_out;     // [B,n] or null
};

// DV/DC > 0 (phi and min-sum rules): every bit has DV edges at slots v*DV .. v*DV+DV-1 and every check DC edges whose slot byte offsets
// come as one packed 16-byte row of g.cslot16 (the hx rows are the first m_x of it); DV = 0: runtime degrees through the CSR tables.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_BP2_WAVES))) bp2_kernel(GraphDev g, Bp2Args a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    extern __shared__ float lds[];
    const StepCw cw(a.B, a.tpc, a.cpb);
    const int lane = cw.lane;
    const BitRows rows(g, a.llr_ch, a.llr_const, a.synd, cw);
    float* msg = lds + (size_t)cw.cwl * a.lds_per_cw;
    const int n = g.n, m = g.m_x;
    if (cw.active)
        for (int e = lane; e < g.E_x; e += a.tpc) msg[e] = 0.0f;
    const StepSynd synd(g, rows, cw, a.tpc, m, a.synd != nullptr);  // the syndrome bits of the lane's checks, one register for all iterations
    const bool f1 = a.factor == 1.0f;
    __syncthreads();
    for (int it = 0; it <= a.num_iter; ++it) {
        if (cw.active)
            for (int v = lane; v < n; v += a.tpc) {
                const float L = rows.prior(v);
                BitSlots<DV> q(g, msg, v);
                const float S = q.fetch();
                if (it == a.num_iter) {
                    const float o = -1.0f * (L + S);
                    if (a.soft_out) a.soft_out[rows.at(v)] = o;
                    if (a.hard_out) a.hard_out[rows.at(v)] = (uint8_t)(0.0f < o);
                    continue;
                }
                q.store(S + L);
            }
        if (it == a.num_iter) break;
        __syncthreads();
        if (cw.active) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd.at(g, rows, i, c);
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if constexpr (CN_TYPE == FGNN_CN_MINSUM) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                    else cn2_phi_regular<DC>(msg, off, sy, a.factor, f1);
                } else if constexpr (DC > 0 && CN_TYPE == FGNN_CN_MINSUM) {
                    // runtime degrees up to DC: the slot list is read once (all loads in flight together), then the regular update with
                    // edge j masked out where j >= deg — no intermediate parked in LDS, no second walk through the index list
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    unsigned off[DC];
#pragma unroll
                    for (int j = 0; j < DC; ++j) off[j] = (j < deg) ? 4u * (unsigned)g.cslot[c0 + j] : 0u;
                    cn_minsum_regular<DC>(msg, off, deg, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    cn_update<CN_TYPE, PhiGnn>(msg, g.cslot + c0, deg, sy, a.factor);
                }
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) bsc_kernel(uint64_t seed, float p, uint64_t first, int B, int n, int nblk,
                                                  uint8_t* __restrict__ noise)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * nblk) return;
    const int b = (int)(t / nblk), blk = (int)(t - (long long)b * nblk);
    float u[4];
    fg_uniform4(seed, first + (uint64_t)b, (uint32_t)blk, u);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (blk * 4 + k < n) noise[(size_t)b * n + blk * 4 + k] = (uint8_t)(u[k] < p);
}

}  // namespace

extern "C" int fgnn_bp2_decode(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                               float llr_const, const uint8_t* synd, int B, float* soft_out, uint8_t* hard_out, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (B < 0 || num_iter < 0) return fgnn_fail(FGNN_ERR_ARG, "B and num_iter must be >= 0");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!soft_out && !hard_out) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    LaunchGeom L = fgnn_geom(g, B);
    Bp2Args a;
    a.B = B;
    a.num_iter = num_iter;
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.llr_ch = llr_ch;
    a.synd = synd;
    a.soft_out = soft_out;
    a.hard_out = hard_out;
    a.lds_per_cw = (int)lds_round4(g->d.E_x);
    const size_t lds_bytes = (size_t)a.lds_per_cw * sizeof(float) * (size_t)L.cpb;
    if (lds_bytes > FGNN_LDS_BUDGET) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident kernel");
    hipStream_t st = static_cast<hipStream_t>(stream);
    // FGNN_BP2_NO_PRED (tests): a graph forced onto the generic kernels runs min-sum on the loop too
    const bool predicated = !(g->force_generic && getenv("FGNN_BP2_NO_PRED"));
    return bit_dispatch(g, cn_type, predicated, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(bp2_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, st, g->d, a);
    });
}

extern "C" int fgnn_bsc_noise(uint64_t seed, float p, uint64_t first_sample, int B, int n, uint8_t* noise, void* stream)
{
    if (B < 0 || n <= 0) return fgnn_fail(FGNN_ERR_ARG, "bad noise arguments");
    if (B == 0) return FGNN_OK;
    if (!noise) return fgnn_fail(FGNN_ERR_ARG, "bad noise arguments");
    const int nblk = (n + 3) / 4;
    const long long total = (long long)B * nblk;
    return fgnn_launch(bsc_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), seed, p,
                       first_sample, B, n, nblk, noise);
}
