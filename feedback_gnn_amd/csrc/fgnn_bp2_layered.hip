// fgnn_bp2_layered.hip — binary syndrome BP in the layered (serial) check schedule, LDS-resident: the checks of side 0 (hx) are updated
// one layer at a time and every update sees the results of the layers before it.  include/fgnn.h states the semantics at
// fgnn_bp2_decode_layered.
//
// With one LLR per bit the schedule runs on an accumulator: next to the messages mu_e the codeword keeps the running posteriors P_v.
// A layer holds checks that share no bit (fgnn_graph_set_bit_layers validates it), so the thread of check c reads and writes only c's
// slots and the posteriors of c's bits, and no other thread of the layer touches either:
//     nu_e = P_v - mu_e   (one subtraction per edge, written into the slot)
//     mu_e = the check rule of fgnn_cn.h / fgnn_cn2.h on the slots, in place, unchanged
//     P_v  = nu_e + mu_e  (one addition per edge)
// No bit is re-summed, and one workgroup barrier closes a layer.  The compile-time-degree forms keep nu in registers across the rule;
// the loop form parks it in P[v], which nobody else reads until the layer's barrier.  The three lines are layer_check of fgnn_layer.h,
// shared with relay_layered_kernel (fgnn_relay_layered.hip).
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   msg [E_x]  the c->v messages, slot e sorted by (bit, check): bp2_kernel's layout, so the packed rows of g.cslot16 index it directly
//   P   [n]    the running posteriors
// and, with `stop` or `stats`, one word per codeword of the workgroup behind them (stamp[cw] = the number of the last parity sweep in
// which a check of the codeword saw odd parity).  [[882,24]]: 2648 + 884 floats = 14 128 bytes per codeword.
//
// Barriers.  The loop bounds (num_iter, num_layers), `stop` and `stats` are launch arguments: every thread of the workgroup reaches
// every barrier.  A codeword that has stopped, a padding codeword of the last workgroup and a thread beyond a layer's checks skip the
// work, never a barrier.  The whole workgroup leaves the iteration loop early only on the stamp words: written in the sweep before a
// barrier, read by every thread after it, and not written again before the next layer's barrier.
//
// Instantiations (bit_dispatch of fgnn_step.h, as bp2_kernel) and what hipcc gives them for gfx950 at FGNN_BP2L_WAVES = 5 (a budget of
// 96 VGPRs; the predicated degree-16 form at 4, a budget of 128), as VGPRs / spilled VGPRs / scratch bytes:
//   phi     (3,6) 75/0/0   (4,8) 85/0/0   loop 40/0/0
//   min-sum (3,6) 53/0/0   (4,8) 63/0/0   predicated <= 8: 63/0/0   predicated <= 16: 102/0/0   loop 38/0/0
//   boxplus loop 38/0/0
// No instantiation spills a VGPR or uses scratch.  The two predicated forms park 8 and 50 SGPRs in VGPR lanes (the j < deg masks of
// the three passes over a check's edges; relay_kernel<0,16> parks 35 the same way): lane writes, no memory.
// Occupancy is set by LDS, not by registers: with 128 threads (2 waves) per codeword 11 workgroups of [[882,24]] fit a CU, 5.5 waves per
// SIMD.
#include <cstdlib>

#include "fgnn_layer.h"

#ifndef FGNN_BP2L_WAVES
#define FGNN_BP2L_WAVES 5  // waves per SIMD the register allocation aims at: what the LDS of [[882,24]] admits at 128 threads per codeword
#endif
#define FGNN_BP2L_WAVES_OF(DC) ((DC) >= 16 ? FGNN_BP2L_WAVES - 1 : FGNN_BP2L_WAVES)
#ifndef FGNN_BP2L_TPC
#define FGNN_BP2L_TPC 128  // most threads per codeword without fgnn_graph_set_launch: see fgnn_bp2_decode_layered below
#endif

namespace {

struct Bp2LayArgs {
    int B, num_iter, num_layers, tpc, cpb, lds_per_cw, p_off, stop;
    float factor, llr_const;
    const int* lay_cptr;   // [num_layers+1] first entry of layer l in lay_chk
    const int* lay_chk;    // [m_x] checks by layer, ascending inside a layer
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null (all-zero syndrome)
    float* soft_out;       // [B,n] or null
    uint8_t* hard_out;     // [B,n] or null
    int32_t* stats;        // [B,2] or null
};

// DV/DC as bp2_kernel: DV > 0 the packed rows of a (DV,DC)-regular hx; DV = 0, DC > 0 min-sum on runtime degrees up to DC, predicated;
// DV = DC = 0 the loop over the CSR tables
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_BP2L_WAVES_OF(DC)))) bp2_layered_kernel(GraphDev g, Bp2LayArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ float lds[];
    const StepCw cw(a.B, a.tpc, a.cpb);
    const int lane = cw.lane;
    const BitRows rows(g, a.llr_ch, a.llr_const, a.synd, cw);
    float* msg = lds + (size_t)cw.cwl * a.lds_per_cw;
    float* P = msg + a.p_off;
    const int n = g.n, m = g.m_x;
    const bool tests = a.stop || a.stats != nullptr;  // a launch with parity sweeps: it has the stamp words
    int* stamp = reinterpret_cast<int*>(lds + (size_t)a.cpb * a.lds_per_cw);

    if (cw.active) {
        for (int e = lane; e < g.E_x; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) P[v] = rows.prior(v) + 0.0f;  // what bp2_kernel's L + S gives with no message yet
    }
    if (tests)
        for (int i = threadIdx.x; i < a.cpb; i += blockDim.x) stamp[i] = 0;
    // the syndrome bits of the lane's checks in the order of the parity sweep; the layers read theirs where they use them
    const StepSynd synd(g, rows, cw, a.tpc, m, tests && a.synd != nullptr);
    const bool f1 = a.factor == 1.0f;
    __syncthreads();

    bool run = cw.active, sat = false;
    int it_run = 0;
    // the parity sweep of a running codeword over all checks of hx, d_v = (P_v < 0): stamp[cw] = mark where a check sees odd parity
    const auto sweep = [&](const int mark) {
        if (!run) return;
        int i = 0;
        for (int c = lane; c < m; c += a.tpc, ++i) {
            unsigned par = synd.at(g, rows, i, c);
            if constexpr (DV > 0) {
                unsigned off[DC];
                row_unpack(g, c, off);
#pragma unroll
                for (int j = 0; j < DC; ++j) par ^= (unsigned)(P[row_qubit<DV>(off[j], 0u)] < 0.0f);
            } else {
                const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                for (int j = 0; j < deg; ++j) par ^= (unsigned)(P[g.cvn[c0 + j]] < 0.0f);
            }
            if (par) stamp[cw.cwl] = mark;
        }
    };

    for (int it = 1; it <= a.num_iter; ++it) {
        for (int l = 0; l < a.num_layers; ++l) {
            if (run) {
                const int c1 = a.lay_cptr[l + 1];
                for (int i = a.lay_cptr[l] + lane; i < c1; i += a.tpc) {
                    const int c = a.lay_chk[i];
                    const unsigned sy = a.synd ? rows.synd_of(g, c) : 0u;
                    layer_check<CN_TYPE, DV, DC>(g, msg, P, c, sy, a.factor, f1);
                }
            }
            __syncthreads();
        }
        if (run) it_run = it;
        if (a.stop) {
            sweep(it);
            __syncthreads();
            if (run && stamp[cw.cwl] != it) {
                run = false;
                sat = true;
            }
            // a codeword that has stopped writes its word no more: every thread reads the same words here, and the next sweep writes
            // them only after the next layer's barrier
            bool all = true;
            for (int j = 0; j < cw.nact; ++j) all = all && stamp[j] != it;
            if (all) break;
        }
    }
    if (a.stats && !(a.stop && a.num_iter > 0)) {  // the one test of a launch without `stop`, or of the prior's decision
        const int mark = a.num_iter + 1;
        sweep(mark);
        __syncthreads();
        sat = stamp[cw.cwl] != mark;
    }

    if (cw.active) {
        for (int v = lane; v < n; v += a.tpc) {
            const float o = -1.0f * P[v];
            if (a.soft_out) a.soft_out[rows.at(v)] = o;
            if (a.hard_out) a.hard_out[rows.at(v)] = (uint8_t)(0.0f < o);
        }
        if (a.stats && lane == 0) {
            a.stats[(size_t)cw.b * 2] = sat ? 1 : 0;
            a.stats[(size_t)cw.b * 2 + 1] = it_run;
        }
    }
}

}  // namespace

extern "C" int fgnn_bp2_decode_layered(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                                       float llr_const, const uint8_t* synd, int B, int stop, float* soft_out, uint8_t* hard_out,
                                       int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (B < 0 || num_iter < 0) return fgnn_fail(FGNN_ERR_ARG, "B and num_iter must be >= 0");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");
    if (stop != 0 && stop != 1) return fgnn_fail(FGNN_ERR_ARG, "stop must be 0 or 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!soft_out && !hard_out) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    LaunchGeom L = fgnn_geom(g, B);
    // Threads per codeword.  One thread takes a check of the layer, and a layer holds a fraction of the checks (hx of [[882,24]]: 9
    // layers of 3 to 91 checks), so most of the thread per node that fgnn_geom deals a codeword would only wait at the barriers:
    // without fgnn_graph_set_launch a codeword gets at most FGNN_BP2L_TPC threads.  128 is the fastest of tools/bench_bp2_layered.py's
    // sweep on hx of [[882,24]] at 10 000 codewords, one codeword per workgroup (profiles/bp2_layered_bench.json: 64 / 128 / 192 / 256 /
    // 384 / 512 threads take 1.00 / 0.85 / 0.89 / 1.00 / 1.85 / 1.98 ms for 16 min-sum iterations); fewer than 64 threads, small
    // batches and other codes have not been swept.
    if (!g->user_launch && L.cpb == 1 && L.tpc > FGNN_BP2L_TPC) {
        L.tpc = FGNN_BP2L_TPC;
        L.threads = L.tpc;
    }
    const size_t p_off = lds_round4(g->d.E_x);
    const size_t per_cw = p_off + lds_round4(g->d.n);
    const bool tests = stop || stats;
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb + (tests ? lds_round4(L.cpb) * sizeof(int) : 0);
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident layered binary BP kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    int rc = fgnn_graph_ensure_bit_layers(g);
    if (rc) return rc;
    FGNN_DEVICE_GUARD(g->device);
    Bp2LayArgs a;
    a.B = B;
    a.num_iter = num_iter;
    a.num_layers = g->bit_layers.num;
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.lds_per_cw = (int)per_cw;
    a.p_off = (int)p_off;
    a.stop = stop;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.lay_cptr = g->bit_layers.table<int>(LAY_CPTR);
    a.lay_chk = g->bit_layers.table<int>(LAY_CHK);
    a.llr_ch = llr_ch;
    a.synd = synd;
    a.soft_out = soft_out;
    a.hard_out = hard_out;
    a.stats = stats;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // FGNN_BP2_NO_PRED (tests): a graph forced onto the generic kernels runs min-sum on the loop too, as in fgnn_bp2_decode
    const bool predicated = !(g->force_generic && getenv("FGNN_BP2_NO_PRED"));
    return bit_dispatch(g, cn_type, predicated, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(bp2_layered_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, st, g->d, a);
    });
}
