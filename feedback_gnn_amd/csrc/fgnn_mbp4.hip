// fgnn_mbp4.hip — BP4 with message-strength control (MBP4 / AMBP4; Kuo, Lai, "Exploiting degeneracy in belief propagation decoding of
// quantum codes", 2022), flooding schedule, LDS-resident.  A codeword walks a list of attempts; attempt a multiplies every check output
// by factor[a] and takes an edge's own message out of the qubit totals multiplied by own[a] (vn_edge_own, fgnn_vn.h): with
// own[a] = alpha_a and factor[a] = base / alpha_a that is MBP4 at strength alpha_a, and a descending list of alphas is AMBP4.  The
// algorithm is stated to the float operation at fgnn_mbp4_decode in include/fgnn.h.  The kernel stands on the frame of the step-loop
// decoders (fgnn_step.h): codeword rows, staged syndrome bits, a qubit's slots, a check's row and parity, the output write; the check
// rule is the shared one (fgnn_cn.h).  Its own are the attempt walk below, the `tab` table and the own-weight edge rule (vn_edge_own);
// lamhat is always the channel LLRs.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   msg  [E_x + E_z]  c->v / v->c messages, bp4_kernel's layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last test
// and per workgroup
//   tab[128]     factor[0..63], then own[0..63]: the codewords of a workgroup sit at different attempts, so the two are indexed per
//                lane; staged from the kernel arguments once, before the first barrier
//   stamp[cpb]   the number of the last workgroup step in which a check of the codeword saw odd parity
//   ndone        finished codewords
//
// A codeword walks attempts r = 0 .. A-1 of T = pre_iter or attempt_iter check updates; an attempt takes T + 1 workgroup steps,
// k = 0 .. T counting its finished check updates:
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
#include <cmath>

#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_MBP4_WAVES
#define FGNN_MBP4_WAVES 7  // waves per SIMD the register allocation aims at
#endif

namespace {

constexpr int MBP4_MAX_ATTEMPTS = 64;

struct MbArgs : StepArgs {
    int pre_iter, attempt_iter, attempts, restart;
    float tab[2 * MBP4_MAX_ATTEMPTS];  // factor[0..63], own[0..63]; entries from `attempts` on are 0 and never read
};

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
    float* tab = lds + (size_t)a.cpb * a.lds_per_cw;
    int* stamp = reinterpret_cast<int*>(tab + 2 * MBP4_MAX_ATTEMPTS);
    int* ndone = stamp + a.cpb;
    const int n = g.n, m = g.m;

    for (int i = threadIdx.x; i < 2 * MBP4_MAX_ATTEMPTS; i += blockDim.x) tab[i] = a.tab[i];
    for (int i = threadIdx.x; i < a.cpb + 1; i += blockDim.x) stamp[i] = 0;  // stamp, ndone
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    int r = 0, k = 0, its = 0;  // r < a.attempts <= 64 throughout: the last attempt ends the codeword
    bool done = !cw.active;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.attempt_iter;
        // ---- qubits: marginals after k check updates and their decision, messages to the checks ----
        if (!done) {
            const bool zero = a.restart && k == 0 && r > 0;  // a restarting attempt starts from zero messages
            const float ow = tab[MBP4_MAX_ATTEMPTS + r];
            for (int v = lane; v < n; v += a.tpc) {
                float lx, ly, lz;
                rows.llrs(n, v, a.llr_const, lx, ly, lz);
                QubitSlots<DV> q(g, msg, v);
                if (zero) q.clear();
                float Sz, Sx;
                q.fetch(Sz, Sx);
                float X, Y, Z;
                vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
                if (k > 0) {  // the test's decision; an attempt's last test sends no messages
                    dec[v] = (uint8_t)vn_decide(X, Y, Z);
                    if (k == T) continue;
                }
                q.store(X, Y, Z, [&](float num, float A, float Ye, float mu) { return vn_edge_own<VnMath>(num, A, Ye, mu, ow); });
            }
        }
        __syncthreads();
        if (*ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the check update (k < T) ----
        if (!done) {
            const float fac = tab[r];
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
                if (odd) stamp[cwl] = step;
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, attempt over, decoder finished ----
        if (!done) {
            if (k == 0) {
                k = 1;
                ++its;
            } else {
                const bool sat = stamp[cwl] != step;
                if (sat || (k == T && r == a.attempts - 1)) {
                    step_write_decisions(a, dec, rows.bb, n, lane);
                    if (lane == 0) step_finish(a, (size_t)cw.b, sat, r, its, k, ndone);
                    done = true;
                } else if (k == T) {
                    ++r;
                    k = 0;
                } else {
                    ++k;
                    ++its;
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
    if (num_attempts < 1 || num_attempts > MBP4_MAX_ATTEMPTS) return fgnn_fail(FGNN_ERR_ARG, "num_attempts must be in 1 .. 64");
    if (pre_iter < 1 || attempt_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and attempt_iter must be >= 1");
    if (restart != 0 && restart != 1) return fgnn_fail(FGNN_ERR_ARG, "restart must be 0 or 1");
    if (!factor || !own) return fgnn_fail(FGNN_ERR_ARG, "factor and own must hold num_attempts floats each");
    for (int i = 0; i < num_attempts; ++i) {
        if (!std::isfinite(factor[i]) || !(factor[i] > 0.0f)) return fgnn_fail(FGNN_ERR_ARG, "every factor must be finite and > 0");
        if (!std::isfinite(own[i]) || own[i] < 0.0f) return fgnn_fail(FGNN_ERR_ARG, "every own weight must be finite and >= 0");
    }
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    MbArgs a;
    step_args_fill(a, L, B, pre_iter, num_attempts - 1, attempt_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.pre_iter = pre_iter;
    a.attempt_iter = attempt_iter;
    a.attempts = num_attempts;
    a.restart = restart;
    for (int i = 0; i < MBP4_MAX_ATTEMPTS; ++i) {
        a.tab[i] = i < num_attempts ? factor[i] : 0.0f;
        a.tab[MBP4_MAX_ATTEMPTS + i] = i < num_attempts ? own[i] : 0.0f;
    }
    // per codeword: E messages and n decision bytes; per workgroup: the two 64-float tables, a stamp per codeword and ndone
    const size_t d_off = lds_round4(g->d.E);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "MBP4", d_off + lds_bytes_as_floats(g->d.n), 2 * MBP4_MAX_ATTEMPTS, L.cpb + 1, &lds_bytes)) return err;
    a.d_off = (int)d_off;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(mbp4_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
