// fgnn_bp4_layered.hip — BP4 in the layered (serial) check schedule, LDS-resident: the checks are updated one layer at a time and every
// update sees the results of the layers before it.  include/fgnn.h states the semantics at fgnn_bp4_decode_layered.
//
// A layer holds checks that share no qubit, across hx and hz (fgnn_graph_set_layers validates it).  So inside a layer
//   - the thread of edge (c, v) reads only v's slots and writes only slot (c, v): no other edge of the layer touches v;
//   - the thread of check c reads and writes only c's slots.
// Two phases per layer, each closed by a workgroup barrier, no atomics:
//   edges:   nu_e in place — the qubit's sums over its slots (vn_sums), its totals (vn_totals), one softplus and one log-sum-exp
//            (vn_edge, the literal form of fgnn_vn.h) with mu_e as the edge's own message;
//   checks:  cn_update of fgnn_cn.h on the check's slots with its syndrome bit, times the normalisation factor.
// Every float operation is the one bp4_kernel's runtime-degree path executes for one flooding iteration whose new messages are kept
// on that layer's checks only; the epilogue is bp4_kernel's (marginals, decision, binary LLRs, soft syndromes), on VnMath and fg_phi.
// No saturation shortcut, no early exit, no hardware transcendentals, no shared log-sum-exp: options 1, 2, 3 and 5 are not read.
// Runtime degrees only: there is no (3,3,6) instantiation.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (layered_lds_bytes in tests/test_gpu_bp4_layered.py mirrors it):
//   msg [E_x + E_z]  c->v / v->c messages, slot e in [0,E_x) = hx edges, [E_x,E) = hz edges, sorted by (qubit, check): bp4_kernel's layout
//   T   [3n]         the channel LLRs lam^X [0,n), lam^Y [n,2n), lam^Z [2n,3n) (read only with llr_ch != null); in the epilogue the
//                    thread of qubit v, done with its three, parks llr_x at T[v] and llr_z at T[n+v] for the soft syndromes
// [[882,24]]: 5292 + 2648 floats = 31 760 bytes per codeword; [[1270,28]]: 7620 + 3812 floats = 45 728 bytes.
//
// Barriers.  The loop bounds (num_iter, num_layers) and the conditions around the barriers are launch arguments: every thread of the
// workgroup reaches every barrier.  Padded codewords of the last workgroup and threads beyond a layer's edges or checks skip the
// work, never a barrier.
//
// Occupancy.  With 256 threads (4 waves) per codeword the LDS above admits 5 workgroups of [[882,24]] on a CU (5 x (31 760 + the 256
// bytes of the log table) fit 160 KiB, 6 do not) and 3 of [[1270,28]]: 5 waves per SIMD at the most, and fewer with fewer threads per
// codeword.  The kernels are therefore compiled for 5 waves per SIMD (a budget of 96 VGPRs): each of the three
// instantiations (one per check rule) takes 60 VGPRs, no spills, no scratch.
#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"

#ifndef FGNN_LAYERED_WAVES
#define FGNN_LAYERED_WAVES 5  // waves per SIMD the register allocation aims at: what the LDS of [[882,24]] admits
#endif
#ifndef FGNN_LAYERED_TPC
#define FGNN_LAYERED_TPC 256  // most threads per codeword without fgnn_graph_set_launch: see fgnn_bp4_decode_layered below
#endif

namespace {

struct LayArgs {
    int B, num_iter, num_layers, tpc, cpb, lds_per_cw, t_off;
    float factor, llr_const;
    const int* lay_cptr;      // [num_layers+1] first entry of layer l in lay_chk
    const int* lay_chk;       // [m] checks by layer, ascending inside a layer
    const int* lay_eptr;      // [num_layers+1] first entry of layer l in lay_edge
    const int2* lay_edge;     // [E] (slot, qubit) of the edges of a layer's checks
    const float* llr_ch;      // [B,3,n] or null
    const uint8_t* synd_x;    // [B,m_x] or null (all-zero syndrome)
    const uint8_t* synd_z;    // [B,m_z] or null
    const float* msg_init_x;  // [B,E_x] or null
    const float* msg_init_z;
    float* llr_out;           // [B,3,n]
    uint8_t* x_hat;
    uint8_t* z_hat;
    float* x_logit;           // [B,rows0] or null
    float* z_logit;           // [B,rows1] or null
    float* msg_out_x;
    float* msg_out_z;
};

template <int CN_TYPE>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_LAYERED_WAVES))) bp4_layered_kernel(GraphDev g, LayArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ float lds[];
    const int cwl = threadIdx.x / a.tpc;
    const int lane = threadIdx.x - cwl * a.tpc;
    const int b = blockIdx.x * a.cpb + cwl;
    const bool active = b < a.B;  // padding codewords of the last workgroup only keep the barriers company
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* T = msg + a.t_off;
    const int n = g.n;
    const size_t bb = active ? (size_t)b : 0;
    const uint8_t* sx = a.synd_x ? a.synd_x + bb * g.m_x : nullptr;
    const uint8_t* sz = a.synd_z ? a.synd_z + bb * g.m_z : nullptr;
    const bool per_qubit = a.llr_ch != nullptr;

    if (active) {
        for (int e = lane; e < g.E_x; e += a.tpc) msg[e] = a.msg_init_x ? a.msg_init_x[bb * g.E_x + e] : 0.0f;
        for (int e = lane; e < g.E_z; e += a.tpc) msg[g.E_x + e] = a.msg_init_z ? a.msg_init_z[bb * g.E_z + e] : 0.0f;
        if (per_qubit)
            for (int i = lane; i < 3 * n; i += a.tpc) T[i] = a.llr_ch[bb * 3 * n + i];
    }
    __syncthreads();

    for (int it = 0; it < a.num_iter; ++it) {
        for (int l = 0; l < a.num_layers; ++l) {
            // ---- the edges of the layer's checks: v->c in place (_vn_update :227-275, for this edge alone) ----
            if (active) {
                const int e1 = a.lay_eptr[l + 1];
                for (int i = a.lay_eptr[l] + lane; i < e1; i += a.tpc) {
                    const int2 sv = a.lay_edge[i];
                    const int s = sv.x, v = sv.y;
                    const float lx = per_qubit ? T[v] : a.llr_const, ly = per_qubit ? T[n + v] : a.llr_const,
                                lz = per_qubit ? T[2 * n + v] : a.llr_const;
                    float Sz, Sx, X, Y, Z;
                    vn_sums(msg, g.vptr_z[v], g.vptr_z[v + 1], g.vptr_x[v], g.vptr_x[v + 1], Sz, Sx);
                    vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
                    const bool hx_edge = s < g.E_x;  // num = softplus(-X), A = Z on an hx edge; softplus(-Z), X on an hz edge
                    const float num = VnMath::softplus(hx_edge ? -X : -Z);
                    msg[s] = vn_edge<VnMath>(num, hx_edge ? Z : X, Y, msg[s]);
                }
            }
            __syncthreads();
            // ---- the layer's checks (:752-767) ----
            if (active) {
                const int c1 = a.lay_cptr[l + 1];
                for (int i = a.lay_cptr[l] + lane; i < c1; i += a.tpc) {
                    const int c = a.lay_chk[i];
                    const uint8_t* sp = c < g.m_x ? sx : sz;
                    const unsigned synd = sp ? (sp[c < g.m_x ? c : c - g.m_x] & 1u) : 0u;
                    const int c0 = g.cptr[c];
                    cn_update<CN_TYPE, PhiBp4>(msg, g.cslot + c0, g.cptr[c + 1] - c0, synd, a.factor);
                }
            }
            __syncthreads();
        }
    }

    // ---- marginals (:777), hard decision (:783-790), binary LLRs of cal_logit (:455-464): bp4_kernel's epilogue ----
    const bool logits = a.x_logit || a.z_logit;
    if (active) {
        if (a.msg_out_x)
            for (int e = lane; e < g.E_x; e += a.tpc) a.msg_out_x[bb * g.E_x + e] = msg[e];
        if (a.msg_out_z)
            for (int e = lane; e < g.E_z; e += a.tpc) a.msg_out_z[bb * g.E_z + e] = msg[g.E_x + e];
        for (int v = lane; v < n; v += a.tpc) {
            const float lx = per_qubit ? T[v] : a.llr_const, ly = per_qubit ? T[n + v] : a.llr_const,
                        lz = per_qubit ? T[2 * n + v] : a.llr_const;
            float Sz, Sx, X, Y, Z;
            vn_sums(msg, g.vptr_z[v], g.vptr_z[v + 1], g.vptr_x[v], g.vptr_x[v + 1], Sz, Sx);
            vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
            float* o = a.llr_out + bb * 3 * n;
            o[v] = X;
            o[n + v] = Y;
            o[2 * n + v] = Z;
            const int d = vn_decide(X, Y, Z);
            a.x_hat[bb * n + v] = (uint8_t)(d & 1);
            a.z_hat[bb * n + v] = (uint8_t)(d >> 1);
            // the qubit's channel LLRs were read above by this thread and by no other: llr_x and llr_z take their place
            if (logits) vn_binary_llrs<VnMath>(X, Y, Z, T[v], T[n + v]);
        }
    }
    if (!logits) return;  // a launch argument: the same for every thread
    __syncthreads();
    if (active) {
        const float* llx = T;
        const float* llz = T + n;
        if (a.x_logit)
            for (int r = lane; r < g.rows[0]; r += a.tpc) {
                const int p0 = g.rptr[0][r];
                a.x_logit[bb * g.rows[0] + r] = logit_row<PhiBp4>(llx, g.rcol[0] + p0, g.rptr[0][r + 1] - p0);
            }
        if (a.z_logit)
            for (int r = lane; r < g.rows[1]; r += a.tpc) {
                const int p0 = g.rptr[1][r];
                a.z_logit[bb * g.rows[1] + r] = logit_row<PhiBp4>(llz, g.rcol[1] + p0, g.rptr[1][r + 1] - p0);
            }
    }
}

}  // namespace

extern "C" int fgnn_bp4_decode_layered(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                                       float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, const float* msg_init_x,
                                       const float* msg_init_z, float* llr_out, uint8_t* x_hat, uint8_t* z_hat, float* x_logit,
                                       float* z_logit, float* msg_out_x, float* msg_out_z, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (B < 0 || num_iter < 0) return fgnn_fail(FGNN_ERR_ARG, "B and num_iter must be >= 0");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");  // decoding_q.py:107
    if ((x_logit && !g->d.rptr[0]) || (z_logit && !g->d.rptr[1]))
        return fgnn_fail(FGNN_ERR_STATE, "logit row sets not installed (fgnn_graph_set_rows)");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!llr_out || !x_hat || !z_hat) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    if ((msg_init_x == nullptr) != (msg_init_z == nullptr)) return fgnn_fail(FGNN_ERR_ARG, "msg_init_x and msg_init_z go together");
    LaunchGeom L = fgnn_geom(g, B);
    // Threads per codeword.  A layer holds a fraction of the checks ([[882,24]]: 13 layers of 6 to 96 checks, 36 to 576 edges), so
    // the thread per node that fgnn_geom deals a codeword of a small batch (up to 1024) would mostly wait at the barriers: without
    // fgnn_graph_set_launch a codeword gets at most FGNN_LAYERED_TPC threads.  256 is the fastest of tools/bench_layered.py's sweep on
    // [[882,24]] at 16 384 codewords (profiles/layered_bench.json: 64 / 128 / 192 / 256 / 384 / 512 threads take 29.5 / 18.2 / 15.6 /
    // 15.2 / 17.5 / 18.2 ms for 16 min-sum iterations); small batches have not been swept.
    if (!g->user_launch && L.cpb == 1 && L.tpc > FGNN_LAYERED_TPC) {
        L.tpc = FGNN_LAYERED_TPC;
        L.threads = L.tpc;
    }
    const size_t t_off = ((size_t)g->d.E + 3) & ~(size_t)3;
    const size_t per_cw = t_off + (((size_t)3 * g->d.n + 3) & ~(size_t)3);
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb;
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident layered BP4 kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    int rc = fgnn_graph_ensure_layers(g);
    if (rc) return rc;
    FGNN_DEVICE_GUARD(g->device);
    LayArgs a;
    a.B = B;
    a.num_iter = num_iter;
    a.num_layers = g->check_layers.num;
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.lds_per_cw = (int)per_cw;
    a.t_off = (int)t_off;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.lay_cptr = g->check_layers.table<int>(LAY_CPTR);
    a.lay_chk = g->check_layers.table<int>(LAY_CHK);
    a.lay_eptr = g->check_layers.table<int>(LAY_EPTR);
    a.lay_edge = g->check_layers.table<int2>(LAY_EDGE);
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.msg_init_x = msg_init_x;
    a.msg_init_z = msg_init_z;
    a.llr_out = llr_out;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.x_logit = x_logit;
    a.z_logit = z_logit;
    a.msg_out_x = msg_out_x;
    a.msg_out_z = msg_out_z;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(L.blocks), block(L.threads);
    switch (cn_type) {
    case FGNN_CN_BOXPLUS_PHI: return fgnn_launch(bp4_layered_kernel<FGNN_CN_BOXPLUS_PHI>, grid, block, lds_bytes, st, g->d, a);
    case FGNN_CN_MINSUM: return fgnn_launch(bp4_layered_kernel<FGNN_CN_MINSUM>, grid, block, lds_bytes, st, g->d, a);
    default: return fgnn_launch(bp4_layered_kernel<FGNN_CN_BOXPLUS>, grid, block, lds_bytes, st, g->d, a);
    }
}
