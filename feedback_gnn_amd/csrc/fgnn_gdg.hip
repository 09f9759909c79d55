// fgnn_gdg.hip — binary BP with guided decimation guessing (BP-GDG) on one Tanner graph, LDS-resident: min-sum BP runs, the least
// reliable free bit is fixed, and for the first `depth` fixes both values are tried, so that a sample becomes P = 2^depth paths; each
// path then goes on greedily, and the lightest solution among the paths is the sample's output.
//
// Gong, Cammerer, Renes, "Toward low-latency iterative decoding of QLDPC codes under circuit-level noise" (2024), in the form
// include/fgnn.h states at fgnn_gdg_decode (the bits are ranked by the posterior of the last test, not by a history of posteriors).
// The parity-check matrix is side 0 (hx) of an fgnn_graph.  The paths of a sample never interact, so a path is a codeword of its own to
// the kernel: virtual codeword vb = (position in the index list) * P + path, StepCw is built on nact * P, the input rows are the
// sample's, and the decisions and the four result words of a path go to row vb of the workspace.  Several paths of one sample may share a
// workgroup, or lie in two.  gdg_select_kernel then reads a sample's P results, picks the path and copies its row to hard_out.
//
// The step is that of the binary leg decoders in fgnn_step.h (StepCw, BitRows, StepSynd, BitSlots; bit_check for the check phase,
// bit_weigh for the weight of a decision, bit_sample for the sample's rows, BitArgs on the host), which relay_kernel (fgnn_relay.hip)
// and si_kernel (fgnn_si.hip) run too; its own is the bit phase, relay_kernel's with the memory term taken out and the fix marks put
// in, and the pick.  The control is that of fgnn_legs.h with a round as a leg: R + 1 legs, stop at the first solution.  LegCtl weighs
// the test that ends a path (integer atomics into wacc[cw], complete one barrier interval later) and has the kernel write that
// decision.  A round differs from a leg in that the messages are kept: at k = 0 of a round r > 0 the bit phase fetches them as they
// are and sends x - mu with the new Lhat.
//
// The pick is bp4gd_kernel's (fgnn_bp4gd.hip): at the last test of a round (k = T) every free bit posts a 64-bit key into the
// codeword's LDS word of that round's parity, and the control section of the same step, two barriers later, reads the winner; its owner
// sets the fix mark.  |P_v| >= +0, so its float bits order as unsigned integers:
//   least reliable   key = bits(|P_v|) << 32 | v,                atomicMin, the word starts at all ones
//   most reliable    key = bits(|P_v|) << 32 | (0xFFFFFFFF - v), atomicMax, the word starts at 0
// both give the lowest index on ties, an integer extremum of a total order whatever the arrival order: no float atomics.  The other
// word is reset, to the start value of the pick that will use it, one round after it was read: at least two barriers before its next post.
//
// LDS of one virtual codeword, in floats, each area rounded up to 4 floats (gdg_lds_bytes in tests/test_gpu_gdg.py mirrors it):
//   msg [E_x]      c->v / v->c messages of hx, sorted by (bit, check): bp2_kernel's layout
//   P   [n]        posteriors of the last test: the parity test gathers their signs in the same sweep as the check update
//   fix [n] bytes  0 = free, 1 + d = fixed to d; written and read by the thread that owns the bit only: no barrier orders them
// and per workgroup
//   key[2 cpb]     (64-bit) the selection keys, two per codeword, used alternately by round parity
//   stamp[cpb], wacc[cpb], ndone   the words of the leg control (leg_stage)
// hx of [[882,24]]: 2648 + 884 + 224 floats = 15 024 bytes per path.
#include "fgnn_step.h"

#ifndef FGNN_GDG_WAVES
#define FGNN_GDG_WAVES 6  // waves per SIMD the register allocation aims at (relay_kernel's target)
#endif
// the predicated update for degrees up to 16 holds 16 magnitudes and signs next to the control state: relay_kernel's takes 95 VGPRs
// at five waves; with the fix marks, the key and the path next to them this one spills 3 VGPRs to scratch there (16 bytes per lane),
// so it runs at four waves per SIMD
#define FGNN_GDG_WAVES_OF(DC) ((DC) >= 16 ? FGNN_GDG_WAVES - 2 : FGNN_GDG_WAVES)

namespace {

struct GdgArgs : BitArgs {   // B = nact * P virtual codewords
    int f_off, max_steps;
    int depth, rounds, tail_least;
    LegSched legs;           // a round is a leg: pre_iter, rounds + 1, round_iter, 1
    float factor, llr_const, decim;
    const float* llr_ch;     // [.,n] logits or null
    const uint8_t* synd;     // [.,m_x] or null (all-zero syndrome)
    const int32_t* index;    // [nact] samples or null (sample i is i)
    uint8_t* dec;            // workspace: [B,n] decisions
    int32_t* res;            // workspace: [B,4] found, w or 0, bits fixed, its
};

__device__ __forceinline__ unsigned long long gdg_key_start(const bool least) { return least ? ~0ull : 0ull; }

// DV/DC > 0: (DV,DC)-regular hx with the packed slot rows of g.cslot16; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_GDG_WAVES_OF(DC)))) gdg_kernel(GraphDev g, GdgArgs a)
{
    FG_LOG_TAB_SETUP();  // cn_update names the phi policy: the table every kernel of that family installs
    extern __shared__ float lds[];
    const StepCw cw(a.B, a.tpc, a.cpb);
    const int cwl = cw.cwl, lane = cw.lane;
    const int path = cw.b & ((1 << a.depth) - 1);
    const StepCw in = bit_sample(cw, a.index, cw.b >> a.depth);  // the input rows are the sample's
    const BitRows rows(g, a.llr_ch, a.llr_const, a.synd, in);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* P = msg + a.p_off;
    uint8_t* fix = reinterpret_cast<uint8_t*>(msg + a.f_off);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(lds + (size_t)a.cpb * a.lds_per_cw);  // 16-byte aligned
    const int n = g.n, m = g.m_x;

    const LegLds ws = leg_stage(lds + 4 * a.cpb, a.cpb, a.lds_per_cw);  // behind the 2 cpb keys
    if (cw.active) {
        for (int v = lane; v < n; v += a.tpc) {
            P[v] = rows.prior(v);
            fix[v] = 0;
        }
        if (lane == 0) {
            key[2 * cwl] = gdg_key_start(0 < a.depth || a.tail_least);
            key[2 * cwl + 1] = gdg_key_start(1 < a.depth || a.tail_least);
        }
    }
    const StepSynd synd(g, rows, in, a.tpc, m, a.synd != nullptr);
    __syncthreads();

    LegCtl ctl(cw.active);
    int its = 0;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.legs), r = ctl.r, k = ctl.k;
        const bool least = r < a.depth || a.tail_least;
        // ---- bits: posterior after k check updates, selection key at the end of a round, messages to the checks ----
        if (!ctl.done) {
            const bool post = k == T && r < a.rounds;
            for (int v = lane; v < n; v += a.tpc) {
                const int f = fix[v];
                const float L = f ? (f == 1 ? a.decim : -a.decim) : rows.prior(v);
                // the bit's c->v messages: zeros before the first check update of the first round; a later round keeps them
                BitSlots<DV> q(g, msg, v);
                float S = 0.0f;
                if (k > 0 || r > 0) {
                    S = q.fetch();
                    if (k > 0) {
                        const float Pv = L + S;
                        P[v] = Pv;
                        if (k == T) {
                            if (post && !f) {
                                const unsigned long long hi = (unsigned long long)fg_f2u(__builtin_fabsf(Pv)) << 32;
                                if (least) atomicMin(&key[2 * cwl + (r & 1)], hi | (unsigned long long)(unsigned)v);
                                else atomicMax(&key[2 * cwl + (r & 1)], hi | (unsigned long long)(0xFFFFFFFFu - (unsigned)v));
                            }
                            continue;
                        }
                    }
                } else {
                    q.zeros();
                }
                const float x = S + L;
                if (k > 0 || r > 0) q.store(x);
                else q.store_zeros(x);
            }
        }
        __syncthreads();
        // ---- the decision weighed in the previous step: its weight is complete now, P still holds it ----
        if (ctl.pending)
            ctl.settle(ws.wacc[cwl], [&] {
                for (int v = lane; v < n; v += a.tpc) a.dec[(size_t)cw.b * n + v] = (uint8_t)(P[v] < 0.0f);
            });
        if (ctl.stats_due() && lane == 0) {
            int32_t* st = a.res + (size_t)cw.b * 4;
            st[0] = ctl.found;
            st[1] = ctl.found ? ctl.best_w : 0;
            st[2] = ctl.best_r;
            st[3] = its;
        }
        if (*ws.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks: parity of the decisions (k > 0), then the min-sum update (k < T) ----
        if (!ctl.done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i)
                bit_check<DV, DC>(g, msg, P, c, synd.at(g, rows, i, c), k > 0, k < T, a.factor, [&] { ws.stamp[cwl] = step; });
        }
        __syncthreads();
        // ---- per virtual codeword: solution found, round over (the pick), path finished (fgnn_legs.h) ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();
                ++its;
            } else {
                const LegTest t = ctl.test(a.legs, T, ws.stamp[cwl] != step);
                if (t.weigh) {
                    const int part = bit_weigh(P, rows, n, lane, a.tpc);
                    if (part) atomicAdd(&ws.wacc[cwl], part);
                    ctl.weighed();
                }
                if (t.fin) {
                    ctl.finish();
                    if (lane == 0) atomicAdd(ws.ndone, 1);
                } else if (t.leg_end) {
                    // the winner of this round's bids: every thread of the codeword reads it, the bit's owner fixes it
                    const unsigned lo = (unsigned)(key[2 * cwl + (r & 1)] & 0xFFFFFFFFull);
                    const unsigned vs = least ? lo : 0xFFFFFFFFu - lo;
                    if (vs < (unsigned)n && (int)(vs % (unsigned)a.tpc) == lane) {
                        unsigned val = (unsigned)(P[vs] < 0.0f);
                        if (r < a.depth) val ^= ((unsigned)path >> r) & 1u;
                        fix[vs] = (uint8_t)(1u + val);
                    }
                    // the other word: read a round ago, posted to a round from now, by the pick of round r + 1
                    if (lane == 0) key[2 * cwl + ((r + 1) & 1)] = gdg_key_start(r + 1 < a.depth || a.tail_least);
                    ctl.next_leg();
                } else {
                    ctl.more();
                    ++its;
                }
            }
        }
    }
}

struct GdgSelArgs {
    int nact, n, depth;
    const int32_t* index;   // [nact] or null
    const uint8_t* dec;     // [nact P, n]
    const int32_t* res;     // [nact P, 4]
    uint8_t* hard_out;      // [B,n]
    int32_t* stats;         // [B,4]
    int32_t* path_stats;    // [nact,P,4] or null
};

// one workgroup per listed sample: the path with found = 1 of smallest w (signed), lowest path on ties; path 0 if none found.  Every
// thread walks the P <= 64 result rows itself (the same 1 KiB for the whole workgroup), then the workgroup copies the chosen row
__global__ void __launch_bounds__(256) gdg_select_kernel(GdgSelArgs a)
{
    const int i = blockIdx.x;
    const int P = 1 << a.depth;
    const int32_t* res = a.res + (size_t)i * P * 4;
    int nfound = 0, best = 0, best_w = 0;
    for (int p = 0; p < P; ++p) {
        const int f = res[4 * p], w = res[4 * p + 1];
        if (f && (nfound == 0 || w < best_w)) {
            best = p;
            best_w = w;
        }
        nfound += f;
    }
    const size_t b = a.index ? (size_t)a.index[i] : (size_t)i;
    const uint8_t* row = a.dec + ((size_t)i * P + best) * a.n;
    for (int v = threadIdx.x; v < a.n; v += blockDim.x) a.hard_out[b * a.n + v] = row[v];
    if (threadIdx.x == 0) {
        int32_t* st = a.stats + b * 4;
        st[0] = nfound;
        st[1] = nfound ? best_w : 0;
        st[2] = best;
        st[3] = res[4 * best + 2];
    }
    if (a.path_stats)
        for (int j = threadIdx.x; j < 4 * P; j += blockDim.x) a.path_stats[(size_t)i * P * 4 + j] = res[j];
}

// the workspace of nact samples at `depth`: the result words of the nact P paths, then their decision rows
size_t gdg_ws_bytes(const fgnn_graph* g, int depth, int nact)
{
    return (size_t)nact * ((size_t)1 << depth) * (4 * sizeof(int32_t) + (size_t)g->d.n);
}

}  // namespace

extern "C" int fgnn_gdg_workspace_bytes(const fgnn_graph* g, int depth, int nact, size_t* bytes)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (!bytes) return fgnn_fail(FGNN_ERR_ARG, "bytes is NULL");
    if (depth < 0 || depth > FGNN_GDG_MAX_DEPTH) return fgnn_fail(FGNN_ERR_ARG, "depth must be in 0 .. 6");
    if (nact < 0) return fgnn_fail(FGNN_ERR_ARG, "nact must be >= 0");
    *bytes = gdg_ws_bytes(g, depth, nact);
    return FGNN_OK;
}

extern "C" int fgnn_gdg_decode(const fgnn_graph* g, float normalization_factor, int pre_iter, int round_iter, int max_rounds, int depth,
                               int tail_pick, float decim_llr, const float* llr_ch, float llr_const, const uint8_t* synd, int B,
                               const int32_t* index, int nact, uint8_t* hard_out, int32_t* stats, int32_t* path_stats, void* workspace,
                               size_t ws_bytes, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || round_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and round_iter must be >= 1");
    if (max_rounds < 0) return fgnn_fail(FGNN_ERR_ARG, "max_rounds must be >= 0");
    if (depth < 0 || depth > FGNN_GDG_MAX_DEPTH) return fgnn_fail(FGNN_ERR_ARG, "depth must be in 0 .. 6");
    if (tail_pick != FGNN_GDG_MOST && tail_pick != FGNN_GDG_LEAST) return fgnn_fail(FGNN_ERR_ARG, "tail_pick must be FGNN_GDG_MOST or FGNN_GDG_LEAST");
    if (!(decim_llr > 0.0f)) return fgnn_fail(FGNN_ERR_ARG, "decim_llr must be > 0");
    if (int err = bit_check_list(index, B, nact)) return err;  // as fgnn_osd0: no list = all B samples
    if (B == 0 || nact == 0) return FGNN_OK;  // nothing to decode needs no buffers
    if (!hard_out || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    if ((size_t)nact << depth > (size_t)INT_MAX) return fgnn_fail(FGNN_ERR_ARG, "nact * 2^depth must fit an int");
    const size_t need = gdg_ws_bytes(g, depth, nact);
    if (!workspace || ws_bytes < need)
        return fgnn_fail(FGNN_ERR_ARG, "workspace too small: fgnn_gdg_decode needs " + std::to_string(need) + " bytes");
    if (reinterpret_cast<uintptr_t>(workspace) % 4) return fgnn_fail(FGNN_ERR_ARG, "workspace must be 4-byte aligned");
    FGNN_DEVICE_GUARD(g->device);
    const int VB = nact << depth;
    const LaunchGeom L = fgnn_geom(g, VB);
    GdgArgs a;
    a.depth = depth;
    a.rounds = std::min(max_rounds, g->d.n);
    a.tail_least = tail_pick == FGNN_GDG_LEAST;
    bit_args_fill(a, VB, {pre_iter, a.rounds + 1, round_iter, 1}, normalization_factor, llr_ch, llr_const, synd);
    a.index = index;
    a.decim = decim_llr;
    a.res = static_cast<int32_t*>(workspace);
    a.dec = reinterpret_cast<uint8_t*>(a.res + (size_t)VB * 4);
    // per virtual codeword: E_x messages, n posteriors and n fix bytes; per workgroup: two 64-bit keys per codeword, the leg words
    size_t lds_bytes;
    if (int err = bit_lds_bytes(a, g, L, "BP-GDG", {{(size_t)g->d.n, &a.f_off}}, 2, &lds_bytes)) return err;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int err = bit_dispatch(g, FGNN_CN_MINSUM, true, [&](auto, auto dv, auto dc) {
            return fgnn_launch(gdg_kernel<decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
        }))
        return err;
    GdgSelArgs s;
    s.nact = nact;
    s.n = g->d.n;
    s.depth = depth;
    s.index = index;
    s.dec = a.dec;
    s.res = a.res;
    s.hard_out = hard_out;
    s.stats = stats;
    s.path_stats = path_stats;
    return fgnn_launch(gdg_select_kernel, dim3(nact), dim3(256), 0, st, s);
}
