// fgnn_mbp4.hip — BP4 with message-strength control (MBP4 / AMBP4; Kuo, Lai, "Exploiting degeneracy in belief propagation decoding of
// quantum codes", 2022), flooding schedule, LDS-resident.  A codeword walks a list of attempts; attempt a multiplies every check output
// by factor[a] and takes an edge's own message out of the qubit totals multiplied by own[a] (vn_edge_own, fgnn_vn.h): with
// own[a] = alpha_a and factor[a] = base / alpha_a that is MBP4 at strength alpha_a, and a descending list of alphas is AMBP4.  The
// algorithm is stated to the float operation at fgnn_mbp4_decode in include/fgnn.h.  The kernel stands on the frame of the step-loop
// decoders (fgnn_step.h): codeword rows, staged syndrome bits, a qubit's slots, a check's row and parity, the output write; the check
// rule is the shared one (fgnn_cn.h).  The attempt walk, the `tab` table and the qubit phase with the own-weight edge rule (vn_edge_own)
// are the ones it shares with dsbp4_kernel and stbp4_kernel (fgnn_attempts.h, attempt_stage and attempt_qubit of fgnn_step.h); lamhat
// is always the channel LLRs.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   msg  [E_x + E_z]  c->v / v->c messages, bp4_kernel's layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last test
// and per workgroup tab[128], stamp[cpb] and ndone (AttemptLds, fgnn_step.h).
//
// A step of an attempt with T check updates, k = 0 .. T counting the finished ones (the walk: AttemptCtl, fgnn_attempts.h):
//   qubits   k > 0: marginals, decision into dec;  k = T: no messages;  k < T: v->c messages with own[r] (k = 0 of a restarting
//            attempt: the owner zeroes the qubit's slots first)
//   barrier
//   checks   k > 0: parity of the decisions against the syndrome bit (stamp);  k < T: check update, * factor[r]
//   barrier
//   control  solved / out of attempts: outputs, done;  k = T: the next attempt
// No float atomics; no result depends on the order in which threads arrive.
//
// Registers.  Compiled for FGNN_MBP4_WAVES waves per SIMD, the most at which no instantiation needs scratch (DESIGN.md section 4,
// "Message-strength control", lists what each instantiation takes).
#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_MBP4_WAVES
#define FGNN_MBP4_WAVES 7  // waves per SIMD the register allocation aims at
#endif

namespace {

using MbArgs = AttemptArgs;  // the frame's arguments and the schedule, nothing else

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_MBP4_WAVES))) mbp4_kernel(GraphDev g, MbArgs a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    static_assert(!REGULAR || CN_TYPE == FGNN_CN_MINSUM, "the regular rows are compiled for min-sum");
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepRows rows(g, a, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    const int n = g.n, m = g.m;
    const AttemptLds w = attempt_stage(lds, a);
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    AttemptCtl ctl(cw.active);
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.sched), k = ctl.k;
        // ---- qubits: marginals after k check updates and their decision, messages to the checks ----
        if (!ctl.done) {
            const bool zero = ctl.zero(a.sched);
            const float ow = w.tab[ATTEMPT_MAX + ctl.r];
            for (int v = lane; v < n; v += a.tpc) {
                float lx, ly, lz;
                rows.llrs(n, v, a.llr_const, lx, ly, lz);
                attempt_qubit<DV>(g, msg, v, lx, ly, lz, k, T, zero, ow, dec + v);
            }
        }
        __syncthreads();
        if (*w.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the check update (k < T) ----
        if (!ctl.done) {
            const float fac = w.tab[ctl.r];
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd.at(g, rows, i, c);
                const bool is_x = c < g.m_x;
                bool odd = false;
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0) odd = parity_regular<DV>(g, dec, off, is_x, sy) != 0u;
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, fac);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) odd = parity_csr(g, dec, c0, deg, is_x, sy) != 0u;
                    if (k < T) cn_update<CN_TYPE, PhiBp4>(msg, g.cslot + c0, deg, sy, fac);
                }
                if (odd) w.stamp[cwl] = step;
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, attempt over, decoder finished ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();  // an attempt's first step tests nothing
            } else {
                const bool sat = w.stamp[cwl] != step;
                if (sat || ctl.last(a.sched, T)) {
                    step_write_decisions(a, dec, rows.bb, n, lane);
                    if (lane == 0) step_finish(a, (size_t)cw.b, sat, ctl.r, ctl.its, k, w.ndone);
                    ctl.done = true;
                } else if (k == T) {
                    ctl.again();
                } else {
                    ctl.more();
                }
            }
        }
    }
}

}  // namespace

extern "C" int fgnn_mbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                                int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                                const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (int err = attempt_check_sched(num_attempts, pre_iter, attempt_iter, restart)) return err;
    if (int err = attempt_check_tables(num_attempts, factor, own)) return err;
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    MbArgs a;
    attempt_args_fill(a, L, B, num_attempts, factor, own, pre_iter, attempt_iter, restart, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat,
                      stats);
    // per codeword: E messages and n decision bytes; per workgroup: the two 64-float tables, a stamp per codeword and ndone
    const size_t d_off = lds_round4(g->d.E);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "MBP4", d_off + lds_bytes_as_floats(g->d.n), 2 * ATTEMPT_MAX, L.cpb + 1, &lds_bytes)) return err;
    a.d_off = (int)d_off;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(mbp4_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
