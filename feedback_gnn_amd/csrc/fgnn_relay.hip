// fgnn_relay.hip — Relay-BP on one Tanner graph: a chain of min-sum BP runs ("legs") with per-bit memory strengths, LDS-resident.
//
// Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories" (2025), in the form
// include/fgnn.h states at fgnn_relay_decode.  The layout is bp2_kernel's (fgnn_bp2.hip): the parity-check matrix is side 0 (hx) of an
// fgnn_graph, one workgroup holds the E_x messages of its codeword(s) in LDS, the check update is the shared min-sum rule of fgnn_cn.h.
// Added per codeword: the posteriors P[n] in LDS (the memory term reads them, the next leg starts from them, the parity test gathers
// their signs in the same sweep as the check update), and per workgroup the words of the leg control.  All legs run in one
// launch; the messages never leave LDS.
//
// Codewords of one workgroup stop at different steps.  The leg / stop / weight control is the shared one of fgnn_legs.h (LegCtl:
// registers every thread of a codeword holds identically; stamp[cw], wacc[cw] and ndone in LDS, laid out by leg_stage, written in
// one barrier interval and read in the next); the kernel stands on the frame of fgnn_step.h (StepCw, BitRows, StepSynd, BitSlots,
// row_unpack) and shares its check phase (bit_check), the weight of a decision (bit_weigh: the bits with P < 0, each the rounded
// 1024-fold of its prior) and its host frame (BitArgs) with gdg_kernel and si_kernel there.  Its own are the memory term on the
// posteriors and the write of the decisions from the signs of P.
#include "fgnn_step.h"

#ifndef FGNN_RELAY_WAVES
#define FGNN_RELAY_WAVES 6  // waves per SIMD the register allocation aims at (bp2_kernel's target)
#endif
// the predicated update for degrees up to 16 holds 16 magnitudes and signs next to the decoder's control state: it takes 95 VGPRs
// spill-free (the 80 of six waves leave 21 spilled), so it runs at one wave per SIMD fewer
#define FGNN_RELAY_WAVES_OF(DC) ((DC) >= 16 ? FGNN_RELAY_WAVES - 1 : FGNN_RELAY_WAVES)

namespace {

struct RelayArgs : BitArgs {
    int max_steps;
    LegSched legs;
    float factor, llr_const;
    const float* gamma;    // [num_legs,n]
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null (all-zero syndrome)
    uint8_t* hard_out;     // [B,n]
    int32_t* stats;        // [B,4]
};

// DV/DC > 0: (DV,DC)-regular hx with the packed slot rows of g.cslot16; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_RELAY_WAVES_OF(DC)))) relay_kernel(GraphDev g, RelayArgs a)
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
    const StepSynd synd(g, rows, cw, a.tpc, m, a.synd != nullptr);
    __syncthreads();

    LegCtl ctl(cw.active);
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.legs), r = ctl.r, k = ctl.k;
        // ---- bits: posterior after k check updates, memory term, messages to the checks ----
        if (!ctl.done) {
            const float* gam = a.gamma + (size_t)r * n;
            for (int v = lane; v < n; v += a.tpc) {
                const float L = rows.prior(v);
                const float gv = gam[v];
                const float om = 1.0f - gv;
                float Pv = P[v];
                // the bit's c->v messages: zeros before the first check update of a leg, whatever the last leg left in the slots
                BitSlots<DV> q(g, msg, v);
                float S = 0.0f;
                if (k > 0) {
                    S = q.fetch();
                    const float lam0 = om * L + gv * Pv;
                    Pv = lam0 + S;
                    P[v] = Pv;
                    if (k == T) continue;
                } else {
                    q.zeros();
                }
                const float lam = om * L + gv * Pv;
                const float x = S + lam;
                if (k > 0) q.store(x);
                else q.store_zeros(x);
            }
        }
        __syncthreads();
        // ---- the decision weighed in the previous step: its weight is complete now, P still holds it ----
        if (ctl.pending)
            ctl.settle(ws.wacc[cwl], [&] {
                for (int v = lane; v < n; v += a.tpc) a.hard_out[rows.at(v)] = (uint8_t)(P[v] < 0.0f);
            });
        if (ctl.stats_due() && lane == 0) ctl.stats(a.stats + (size_t)cw.b * 4);
        if (*ws.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks: parity of the decisions (k > 0), then the min-sum update (k < T) ----
        if (!ctl.done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i)
                bit_check<DV, DC>(g, msg, P, c, synd.at(g, rows, i, c), k > 0, k < T, a.factor, [&] { ws.stamp[cwl] = step; });
        }
        __syncthreads();
        // ---- per codeword: solution found, leg over, decoder finished (fgnn_legs.h) ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();
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
                    ctl.next_leg();
                } else {
                    ctl.more();
                }
            }
        }
    }
}

}  // namespace

extern "C" int fgnn_relay_decode(const fgnn_graph* g, float normalization_factor, int pre_iter, int num_legs, int leg_iter,
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
    FGNN_DEVICE_GUARD(g->device);
    LaunchGeom L = fgnn_geom(g, B);
    RelayArgs a;
    bit_args_fill(a, B, {pre_iter, num_legs, leg_iter, stop_nconv}, normalization_factor, llr_ch, llr_const, synd);
    a.gamma = gamma;
    a.hard_out = hard_out;
    a.stats = stats;
    // per codeword: E_x messages and n posteriors; per workgroup: stamp and wacc per codeword, ndone
    size_t lds_bytes;
    if (int err = bit_lds_bytes(a, g, L, nullptr, {}, 0, &lds_bytes)) return err;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return bit_dispatch(g, FGNN_CN_MINSUM, true, [&](auto, auto dv, auto dc) {
        return fgnn_launch(relay_kernel<decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
    });
}
