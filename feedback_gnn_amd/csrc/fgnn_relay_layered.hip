// fgnn_relay_layered.hip — Relay-BP whose legs run in the layered (serial) check schedule, LDS-resident: relay_kernel's chain of
// min-sum legs with per-bit memory strengths (fgnn_relay.hip), each iteration of a leg updating the checks of side 0 (hx) one layer at
// a time on running posteriors as bp2_layered_kernel does (fgnn_bp2_layered.hip).  include/fgnn.h states the semantics at
// fgnn_relay_decode_layered.
//
// LDS is relay_kernel's (bit_lds_bytes of fgnn_step.h).  Per codeword, in floats, each area rounded up to 4 floats:
//   msg [E_x]  the c->v messages, slot e sorted by (bit, check), so a bit's slots are one run and the packed rows of g.cslot16 index it
//   P   [n]    the running posteriors: what the memory term reads, what a layer corrects, what the parity sweep and the output decide on
// and per workgroup the words of the leg control (leg_stage: stamp[cpb], wacc[cpb], ndone).  [[882,24]]: 14 128 bytes per codeword.
//
// A workgroup step is one iteration k = 1 .. T of a codeword's current leg (a leg here has no k = 0 step: LegCtl is unchanged, the
// kernel calls more() once after the constructor and after every next_leg()):
//   bit phase    Lam_v = (1 - gam_v) L_v + gam_v P_v;  P_v = Lam_v + S_v, S_v re-summed over the bit's slots (k = 1: the owner zeroes
//                them and S_v = 0.0f).  A thread touches only its own bits and their slots.
//   barrier
//   layers       layer_check<FGNN_CN_MINSUM, DV, DC> of fgnn_layer.h on the checks of layer l, one barrier behind every layer
//   sweep        parity of the signs of P over every check of hx (bit_check with update = false): stamp[cw] = step on odd parity
//   barrier
//   control      LegCtl::test; a weighed decision starts its weight (bit_weigh, integer atomics into wacc[cw]); fin: ++ndone
//   barrier
//   settle       the weight is complete: LegCtl::settle takes it and, where the decision is the output so far, the lane writes the signs
//                of its own bits of P to hard_out; stats of a codeword that finished; leave if ndone == the workgroup's codewords
// num_layers + 3 barriers per step.
//
// The hazard of the weighed decision.  relay_kernel settles a decision one step later, behind the bit-phase barrier of the next step,
// because P still holds it there (a leg's k = 0 step decides nothing).  Here the next bit phase overwrites P.  This kernel settles
// before that bit phase, behind one barrier more per step (one in num_layers + 3; on hx of [[882,24]] one in 12), instead of keeping
// the tested decision in a byte area: that area would add n bytes of LDS per codeword, and LDS is what sets this kernel's occupancy;
// it would also cost a write of n bytes on every test, where the barrier is paid once per step whatever the codewords do.  The write
// in settle reads P[v] for the lane's own bits v = lane, lane + tpc, ..: the bits the same lane overwrites in the next bit phase, so
// no barrier is needed between the two.
//
// Barriers.  The loop bounds (max_steps, num_layers) are launch arguments: every thread of the workgroup reaches every barrier.  A
// finished codeword, a padding codeword of the last workgroup and a thread beyond a layer's checks skip the work, never a barrier:
// no barrier stands inside an `if (!ctl.done)`.  The whole workgroup leaves the step loop early only on ndone == nact: ndone is
// written in the control section (atomics), read by every thread behind the barrier that follows it, and not written again before
// three more barriers.  stamp[cw] is written in the sweep and read in the control section behind the barrier between them; wacc[cw]
// is added to in the control section and read in settle behind the barrier between them.  max_steps = pre_iter + (num_legs - 1) *
// leg_iter, the most iterations a codeword can run, so every codeword has finished, settled and written its stats when the loop ends.
//
// Instantiations (bit_dispatch of fgnn_step.h, as relay_kernel) and what hipcc gives them for gfx950 at FGNN_RELAYL_WAVES = 5 (a budget
// of 96 VGPRs; the predicated degree-16 form at 4, a budget of 128), as VGPRs / spilled VGPRs / scratch bytes:
//   (3,6) 88/0/0   (4,8) 88/0/0   predicated <= 8: 86/0/0   predicated <= 16: 126/0/0   loop 81/0/0
// No instantiation spills a VGPR or uses scratch.  The two predicated forms park 7 and 41 SGPRs in VGPR lanes (the j < deg masks, as
// in bp2_layered_kernel): lane writes, no memory.  At the budget of six waves (80 VGPRs) the regular forms would have to give registers
// back for nothing: occupancy is set by LDS, as for bp2_layered_kernel (with 128 threads per codeword 11 workgroups of [[882,24]] fit a
// CU, 5.5 waves per SIMD).
#include "fgnn_layer.h"

#ifndef FGNN_RELAYL_WAVES
#define FGNN_RELAYL_WAVES 5  // waves per SIMD the register allocation aims at (bp2_layered_kernel's: what the LDS of [[882,24]] admits)
#endif
#define FGNN_RELAYL_WAVES_OF(DC) ((DC) >= 16 ? FGNN_RELAYL_WAVES - 1 : FGNN_RELAYL_WAVES)
#ifndef FGNN_RELAYL_TPC
#define FGNN_RELAYL_TPC 128  // most threads per codeword without fgnn_graph_set_launch: see fgnn_relay_decode_layered below
#endif

namespace {

struct RelayLayArgs : BitArgs {
    int max_steps;
    LegSched legs;
    float factor, llr_const;
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null (all-zero syndrome)
    int num_layers;
    const int* lay_cptr;   // [num_layers+1] first entry of layer l in lay_chk
    const int* lay_chk;    // [m_x] checks by layer, ascending inside a layer
    const float* gamma;    // [num_legs,n]
    uint8_t* hard_out;     // [B,n]
    int32_t* stats;        // [B,4]
};

// DV/DC > 0: (DV,DC)-regular hx with the packed slot rows of g.cslot16; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_RELAYL_WAVES_OF(DC)))) relay_layered_kernel(GraphDev g, RelayLayArgs a)
{
    FG_LOG_TAB_SETUP();  // cn_update names the phi policy: the table every kernel of that family installs (FGNN_LDS_BUDGET leaves its 256 bytes)
    extern __shared__ float lds[];
    const StepCw cw(a.B, a.tpc, a.cpb);
    const int cwl = cw.cwl, lane = cw.lane;
    const BitRows rows(g, a.llr_ch, a.llr_const, a.synd, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* P = msg + a.p_off;
    const int n = g.n, m = g.m_x;

    const LegLds ws = leg_stage(lds, a.cpb, a.lds_per_cw);
    if (cw.active)
        for (int v = lane; v < n; v += a.tpc) P[v] = rows.prior(v);
    // the syndrome bits of the lane's checks in the order of the parity sweep; the layers read theirs where they use them
    const StepSynd synd(g, rows, cw, a.tpc, m, a.synd != nullptr);
    __syncthreads();

    LegCtl ctl(cw.active);
    ctl.more();  // k = 1: the first iteration of leg 0
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.legs), k = ctl.k;
        // ---- bits: memory term on the posteriors of the previous iteration (or leg), posteriors re-summed ----
        if (!ctl.done) {
            const float* gam = a.gamma + (size_t)ctl.r * n;
            for (int v = lane; v < n; v += a.tpc) {
                const float L = rows.prior(v);
                const float gv = gam[v];
                const float om = 1.0f - gv;
                const float lam = om * L + gv * P[v];
                BitSlots<DV> q(g, msg, v);
                float S = 0.0f;
                if (k > 1) {
                    S = q.fetch();
                } else {
                    // a leg starts from zero messages, whatever the last leg left in the slots
                    for (int e = q.e0; e < q.e1; ++e) msg[e] = 0.0f;
                }
                P[v] = lam + S;
            }
        }
        __syncthreads();
        // ---- checks, layer by layer ----
        for (int l = 0; l < a.num_layers; ++l) {
            if (!ctl.done) {
                const int c1 = a.lay_cptr[l + 1];
                for (int i = a.lay_cptr[l] + lane; i < c1; i += a.tpc) {
                    const int c = a.lay_chk[i];
                    const unsigned sy = a.synd ? rows.synd_of(g, c) : 0u;
                    layer_check<FGNN_CN_MINSUM, DV, DC>(g, msg, P, c, sy, a.factor, false);
                }
            }
            __syncthreads();
        }
        // ---- parity of the decisions, the signs of P ----
        if (!ctl.done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i)
                bit_check<DV, DC>(g, msg, P, c, synd.at(g, rows, i, c), true, false, a.factor, [&] { ws.stamp[cwl] = step; });
        }
        __syncthreads();
        // ---- per codeword: solution found, leg over, decoder finished (fgnn_legs.h) ----
        if (!ctl.done) {
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
                ctl.next_leg();
                ctl.more();  // k = 1: a leg has no k = 0 step here
            } else {
                ctl.more();
            }
        }
        __syncthreads();
        // ---- the decision weighed above: its weight is complete now, and P holds it until the lane's own next bit phase ----
        if (ctl.pending)
            ctl.settle(ws.wacc[cwl], [&] {
                for (int v = lane; v < n; v += a.tpc) a.hard_out[rows.at(v)] = (uint8_t)(P[v] < 0.0f);
            });
        if (ctl.stats_due() && lane == 0) ctl.stats(a.stats + (size_t)cw.b * 4);
        if (*ws.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
    }
}

}  // namespace

extern "C" int fgnn_relay_decode_layered(const fgnn_graph* g, float normalization_factor, int pre_iter, int num_legs, int leg_iter,
                                         int stop_nconv, const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd,
                                         int B, uint8_t* hard_out, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || num_legs < 1 || leg_iter < 1 || stop_nconv < 1)
        return fgnn_fail(FGNN_ERR_ARG, "pre_iter, num_legs, leg_iter and stop_nconv must be >= 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!gamma) return fgnn_fail(FGNN_ERR_ARG, "gamma is NULL");
    if (!hard_out || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    LaunchGeom L = fgnn_geom(g, B);
    // Threads per codeword, as fgnn_bp2_decode_layered: one thread takes a check of the layer and a layer holds a fraction of the
    // checks, so without fgnn_graph_set_launch a codeword gets at most FGNN_RELAYL_TPC threads.  tools/bench_relay_layered.py sweeps
    // the value on hx of [[882,24]] at 10 000 codewords (profiles/relay_layered_bench.json): 64 / 128 / 192 / 256 threads take 5.62 /
    // 3.99 / 4.00 / 3.95 ms at the default schedule and 5.04 / 4.00 / 5.38 / 6.02 ms for one leg of 64 iterations that never stops
    if (!g->user_launch && L.cpb == 1 && L.tpc > FGNN_RELAYL_TPC) {
        L.tpc = FGNN_RELAYL_TPC;
        L.threads = L.tpc;
    }
    RelayLayArgs a;
    bit_args_fill(a, B, {pre_iter, num_legs, leg_iter, stop_nconv}, normalization_factor, llr_ch, llr_const, synd);
    // a leg of T iterations takes T steps here, and the step of a codeword's last test settles it: no step more
    const long long steps = (long long)pre_iter + (long long)(num_legs - 1) * (long long)leg_iter;
    a.max_steps = (int)(steps < INT32_MAX - 1 ? steps : INT32_MAX - 1);
    a.gamma = gamma;
    a.hard_out = hard_out;
    a.stats = stats;
    // per codeword: E_x messages and n posteriors; per workgroup: stamp and wacc per codeword, ndone
    size_t lds_bytes;
    if (int err = bit_lds_bytes(a, g, L, nullptr, {}, 0, &lds_bytes)) return err;
    if (int err = fgnn_graph_ensure_bit_layers(g)) return err;
    FGNN_DEVICE_GUARD(g->device);
    a.num_layers = g->bit_layers.num;
    a.lay_cptr = g->bit_layers.table<int>(LAY_CPTR);
    a.lay_chk = g->bit_layers.table<int>(LAY_CHK);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return bit_dispatch(g, FGNN_CN_MINSUM, true, [&](auto, auto dv, auto dc) {
        return fgnn_launch(relay_layered_kernel<decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads), lds_bytes, st,
                           g->d, a);
    });
}
