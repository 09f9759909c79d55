// fgnn_relay4.hip — Relay-BP4: a chain of min-sum BP4 runs ("legs") with per-qubit memory strengths on both Tanner graphs, LDS-resident.
//
// Relay-BP's memory term (Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories", 2025)
// applied to each of a qubit's three LLRs, in the form include/fgnn.h states at fgnn_relay4_decode.  The qubit update is the literal
// form of fgnn_vn.h (one log-sum-exp per edge, fgnn_math.h) with the memory-weighted LLRs Lam in place of the channel LLRs,
// the check update is the shared min-sum rule of fgnn_cn.h, the leg / stop / weight control is the shared one of fgnn_legs.h (LegCtl).
// The kernel stands on the frame of the step-loop decoders (fgnn_step.h): codeword rows, staged syndrome bits, a qubit's slots (counted
// as zeros before a leg's first check update), a check's row and parity, the write of the decisions, the staging of the control's LDS
// words; its own are the memory term on the posteriors M and the weight of a decision.  No
// saturation shortcuts, no register-resident channel LLRs, no hardware transcendentals: the channel LLRs are re-read from global
// memory (L2) by the thread that owns the qubit, every float operation is the one bp4_kernel and cn_update execute, in their order.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (relay4_lds_bytes in tests/test_gpu_relay4.py mirrors it):
//   msg [E_x + E_z]  c->v / v->c messages, slot e in [0,E_x) = hx edges, [E_x,E) = hz edges, sorted by (qubit, check): bp4_kernel's layout
//   M   [3n]         posteriors M^X [0,n), M^Y [n,2n), M^Z [2n,3n): the memory term reads them, the next leg starts from them
//   dec [n] bytes    decisions d_v = x_v | z_v << 1 of the last test: the parity test gathers them in the same sweep as the check update
// and per workgroup the ints of the leg control, stamp[cpb], wacc[cpb], ndone (leg_lds_words of fgnn_legs.h, laid out by leg_stage).
// [[882,24]]: 5292 + 2648 + 224 floats = 32 656 bytes per codeword; [[1270,28]]: 7620 + 3812 + 320 floats = 47 008 bytes.
//
// Codewords of one workgroup stop at different steps: leg, step of the leg, solutions found and best weight are registers every thread of
// a codeword holds identically; what crosses threads goes through the LDS words above, written in one barrier interval and read in the next.
//
// Occupancy.  With 256 threads (4 waves) per codeword the LDS above admits 4 workgroups of [[882,24]] on a CU (5 x (32 672 + the 256
// bytes of the log table) exceed 160 KiB) and 3 of [[1270,28]]: 4 waves per SIMD at the most, whatever the registers allow.  The kernels
// are therefore compiled for 4 waves per SIMD (a budget of 128 VGPRs): the (3,3,6) instantiation takes 89 VGPRs and the loop 69, no
// spills, no scratch.  Asking for more waves would only squeeze the allocation of a kernel whose residency LDS decides.
#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_RELAY4_WAVES
#define FGNN_RELAY4_WAVES 4  // waves per SIMD the register allocation aims at: what the LDS of the benchmark codes admits
#endif

namespace {

struct Relay4Args : StepArgs {
    LegSched legs;
    int m_off;
    float factor;
    const float* gamma;      // [num_legs,n]
};

// the weight of deciding Pauli d (1 = X, 2 = Z, 3 = Y) at a qubit with channel LLRs (lx, ly, lz)
__device__ __forceinline__ int relay4_weight(int d, float lx, float ly, float lz)
{
    const float l = d == 1 ? lx : (d == 2 ? lz : ly);
    return (int)__builtin_rintf(1024.0f * FG_MIN(FG_MAX(l, -20.0f), 20.0f));
}

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16; DV = DC = 0: runtime degrees, the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_RELAY4_WAVES))) relay4_kernel(GraphDev g, Relay4Args a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepRows rows(g, a, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* M = msg + a.m_off;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    const int n = g.n, m = g.m;

    const LegLds ws = leg_stage(lds, a.cpb, a.lds_per_cw);
    if (cw.active)
        for (int v = lane; v < n; v += a.tpc) {
            rows.llrs(n, v, a.llr_const, M[v], M[n + v], M[2 * n + v]);
            dec[v] = 0;
        }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    LegCtl ctl(cw.active);
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.legs), r = ctl.r, k = ctl.k;
        // ---- qubits: marginals after k check updates and their decision, memory term, messages to the checks ----
        if (!ctl.done) {
            const float* gam = a.gamma + (size_t)r * n;
            for (int v = lane; v < n; v += a.tpc) {
                float lx, ly, lz;
                rows.llrs(n, v, a.llr_const, lx, ly, lz);
                const float gv = gam[v];
                const float om = 1.0f - gv;
                float MX = M[v], MY = M[n + v], MZ = M[2 * n + v];
                // the qubit's c->v messages: zeros before the first check update of a leg, whatever the last leg left in the slots
                QubitSlots<DV> q(g, msg, v);
                float Sz, Sx;
                q.fetch(Sz, Sx, k > 0);
                if (k > 0) {  // posteriors of the memory-weighted LLRs, kept for the next memory term, and their decision (fgnn_vn.h)
                    vn_totals(Sz, Sx, om * lx + gv * MX, om * ly + gv * MY, om * lz + gv * MZ, MX, MY, MZ);
                    M[v] = MX;
                    M[n + v] = MY;
                    M[2 * n + v] = MZ;
                    dec[v] = (uint8_t)vn_decide(MX, MY, MZ);
                    if (k == T) continue;
                }
                float X, Y, Z;
                vn_totals(Sz, Sx, om * lx + gv * MX, om * ly + gv * MY, om * lz + gv * MZ, X, Y, Z);
                q.store(X, Y, Z, vn_edge<VnMath>, k > 0);
            }
        }
        __syncthreads();
        // ---- the decision weighed in the previous step: its weight is complete now, dec still holds it ----
        if (ctl.pending) ctl.settle(ws.wacc[cwl], [&] { step_write_decisions(a, dec, rows.bb, n, lane); });
        if (ctl.stats_due() && lane == 0) ctl.stats(a.stats + (size_t)cw.b * 4);
        if (*ws.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the min-sum update (k < T) ----
        if (!ctl.done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd.at(g, rows, i, c);
                const bool is_x = c < g.m_x;
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0 && parity_regular<DV>(g, dec, off, is_x, sy)) ws.stamp[cwl] = step;
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0 && parity_csr(g, dec, c0, deg, is_x, sy)) ws.stamp[cwl] = step;
                    if (k < T) cn_update<FGNN_CN_MINSUM, PhiGnn>(msg, g.cslot + c0, deg, sy, a.factor);
                }
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, leg over, decoder finished (fgnn_legs.h) ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();
            } else {
                const LegTest t = ctl.test(a.legs, T, ws.stamp[cwl] != step);
                if (t.weigh) {
                    int part = 0;
                    for (int v = lane; v < n; v += a.tpc) {
                        const int d = dec[v];
                        if (d) {
                            float lx, ly, lz;
                            rows.llrs(n, v, a.llr_const, lx, ly, lz);
                            part += relay4_weight(d, lx, ly, lz);
                        }
                    }
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

extern "C" int fgnn_relay4_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int num_legs, int leg_iter,
                                  int stop_nconv, const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                                  const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (cn_type != FGNN_CN_MINSUM) return fgnn_fail(FGNN_ERR_ARG, "fgnn_relay4_decode runs the min-sum check rule only (cn_type FGNN_CN_MINSUM)");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || num_legs < 1 || leg_iter < 1 || stop_nconv < 1)
        return fgnn_fail(FGNN_ERR_ARG, "pre_iter, num_legs, leg_iter and stop_nconv must be >= 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!gamma) return fgnn_fail(FGNN_ERR_ARG, "gamma is NULL");
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    Relay4Args a;
    // the step after a codeword's last weighs its last decision
    step_args_fill(a, L, B, pre_iter, num_legs - 1, leg_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.legs = {pre_iter, num_legs, leg_iter, stop_nconv};
    a.factor = normalization_factor;
    a.gamma = gamma;
    // per codeword: E messages, 3n posteriors and n decision bytes; per workgroup: stamp and wacc per codeword, ndone
    const size_t m_off = lds_round4(g->d.E), d_off = m_off + lds_round4((size_t)3 * g->d.n);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "Relay-BP4", d_off + lds_bytes_as_floats(g->d.n), 0, leg_lds_words(L.cpb), &lds_bytes)) return err;
    a.m_off = (int)m_off;
    a.d_off = (int)d_off;
    const auto kernel = step_regular_336(g) ? relay4_kernel<3, 6> : relay4_kernel<0, 0>;
    return fgnn_launch(kernel, dim3(L.blocks), dim3(L.threads), lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
}
