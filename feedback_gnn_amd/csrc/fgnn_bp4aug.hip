// fgnn_bp4aug.hip — augmented BP4, LDS-resident (Rigby, Olivier, Jarvis, "Modified belief propagation decoders for quantum low-density
// parity-check codes", Phys. Rev. A 100, 012330, 2019): when BP4 has run its iterations without a solution, a random fraction of the
// check rows is written into the matrix a second time and BP4 runs again, with fresh draws until an estimate reproduces the syndrome.
// The algorithm is stated to the float operation at fgnn_bp4aug_decode in include/fgnn.h.  The copy of a row stands directly after its
// original; in flooding BP from zero messages its messages then equal the original's bit for bit, so the augmented matrix is never
// built: a qubit adds the message of a duplicated check twice in a row (vn_sums_dup of fgnn_vn.h), everything else is BP4.
//
// The kernel stands on the frame of the step-loop decoders (fgnn_step.h) and is bp4fb_kernel (fgnn_bp4fb.hip) without marks, keys
// and feedback.  Its own are the duplicate marks and the duplicated sums.  The mark of a check is re-derived from one Philox block
// (fgnn_rng.h, integer instructions only) by the owner of every qubit on it, for the qubit's own slots, at the first qubit phase of an
// attempt: no thread reads a mark that another thread wrote, so the marks need no barrier and no atomic.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   msg  [E_x + E_z]  c->v / v->c messages, bp4_kernel's layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last test
//   dup  the marks of the attempt: the loop keeps a byte per slot, [E] bytes indexed as msg is; the (3,3,6) instantiation one byte per
//        qubit, [n] bytes, bit j = hx slot j, bit 3 + j = hz slot j, which is the per-codeword byte count of fgnn_bp4gd_decode
// and per workgroup
//   stamp[cpb]   the number of the last workgroup step in which a check of the codeword saw odd parity
//   ndone        finished codewords
//
// A codeword walks attempts r = 0 .. A of T = pre_iter or attempt_iter check updates; an attempt takes T + 1 workgroup steps,
// k = 0 .. T counting its finished check updates:
//   qubits   k = 0 of attempt r > 0: the owner draws the marks of the qubit's slots (and, restarting, zeroes the slots);  duplicated
//            sums;  k > 0: marginals, decision into dec;  k < T: v->c messages, the edge's own message taken out once
//   barrier
//   checks   k > 0: parity of the decisions against the syndrome bit (stamp);  k < T: check update
//   barrier
//   control  solved / out of attempts: outputs, done;  k = T: the next attempt
// Attempt 0 has no mark set: its sums are vn_sums's, and with max_attempts = 0 the result is that of fgnn_bp4gd_decode without rounds.
//
// Registers.  Compiled for FGNN_BP4AUG_WAVES waves per SIMD, the value of bp4fb_kernel and the most at which no instantiation needs
// scratch ("Augmentation", lists what each instantiation takes).
#include <cmath>

#include "fgnn_step.h"
#include "fgnn_rng.h"
#include "fgnn_cn.h"

#ifndef FGNN_BP4AUG_WAVES
#define FGNN_BP4AUG_WAVES 6  // waves per SIMD the register allocation aims at
#endif

namespace {

constexpr uint32_t AUG_STREAM = 5;  // streams 0-2 of fgnn_rng.h keep the fourth counter word below 256; 3 and 4 are fgnn_bp4fb_decode's

struct AugArgs : StepArgs {
    int pre_iter, attempt_iter, attempts, restart, m_off, mark_bytes;
    float factor, density;
    uint32_t seed_lo, seed_hi;
    uint64_t first_sample;
};

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_BP4AUG_WAVES))) bp4aug_kernel(GraphDev g, AugArgs a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    static_assert(!REGULAR || CN_TYPE == FGNN_CN_MINSUM, "the regular rows are compiled for min-sum");
    static_assert(2 * DV <= 8, "a qubit's marks are the bits of one byte");
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepRows rows(g, a, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    uint8_t* dup = reinterpret_cast<uint8_t*>(msg + a.m_off);
    int* stamp = reinterpret_cast<int*>(lds + (size_t)a.cpb * a.lds_per_cw);
    int* ndone = stamp + a.cpb;
    const int n = g.n, m = g.m;
    const uint64_t sample = a.first_sample + (uint64_t)rows.bb;
    const uint32_t s_lo = (uint32_t)sample, s_hi = (uint32_t)(sample >> 32);

    // dup_c of attempt att: unit(w(c, att, 5)[0]) < density, w of include/fgnn.h
    auto marked = [&](const int c, const int att) __attribute__((always_inline)) {
        uint32_t w[4];
        fg_philox4x32_10(s_lo, s_hi, (uint32_t)c, ((uint32_t)att << 8) | AUG_STREAM, a.seed_lo, a.seed_hi, w);
        return fg_u32_to_unit(w[0]) < a.density;
    };

    for (int i = threadIdx.x; i < a.cpb + 1; i += blockDim.x) stamp[i] = 0;  // stamp, ndone
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
        for (int i = lane; i < a.mark_bytes; i += a.tpc) dup[i] = 0;
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    int r = 0, k = 0, its = 0;
    bool done = !cw.active;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.attempt_iter;
        // ---- qubits: the attempt's marks, marginals after k check updates and their decision, messages to the checks ----
        if (!done) {
            const bool first = k == 0 && r > 0;  // an attempt after the first begins: fresh marks
            const bool zero = a.restart && first;  // a restarting attempt starts from zero messages
            for (int v = lane; v < n; v += a.tpc) {
                float lx, ly, lz;
                rows.llrs(n, v, a.llr_const, lx, ly, lz);
                QubitSlots<DV> q(g, msg, v);
                unsigned bits = 0u;
                if constexpr (REGULAR) {
                    if (first) {
#pragma unroll
                        for (int j = 0; j < DV; ++j) bits |= (marked(g.vchk[q.x0 + j], r) ? 1u : 0u) << j;
#pragma unroll
                        for (int j = 0; j < DV; ++j) bits |= (marked(g.m_x + g.vchk[q.z0 + j], r) ? 1u : 0u) << (DV + j);
                        dup[v] = (uint8_t)bits;
                    } else {
                        bits = dup[v];
                    }
                } else if (first) {
                    for (int e = q.x0; e < q.x1; ++e) dup[e] = marked(g.vchk[e], r) ? 1 : 0;
                    for (int e = q.z0; e < q.z1; ++e) dup[e] = marked(g.m_x + g.vchk[e], r) ? 1 : 0;
                }
                if (zero) q.clear();
                float Sz, Sx;
                q.fetch_dup(Sz, Sx, bits, dup);
                float X, Y, Z;
                vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
                if (k > 0) {  // the test's decision; an attempt's last test sends no messages
                    dec[v] = (uint8_t)vn_decide(X, Y, Z);
                    if (k == T) continue;
                }
                q.store(X, Y, Z, vn_edge<VnMath>);
            }
        }
        __syncthreads();
        if (*ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the check update (k < T) ----
        if (!done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd.at(g, rows, i, c);
                const bool is_x = c < g.m_x;
                bool odd = false;
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0) odd = parity_regular<DV>(g, dec, off, is_x, sy) != 0u;
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) odd = parity_csr(g, dec, c0, deg, is_x, sy) != 0u;
                    if (k < T) cn_update<CN_TYPE, PhiBp4>(msg, g.cslot + c0, deg, sy, a.factor);
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
                if (sat || (k == T && r == a.attempts)) {
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

extern "C" int fgnn_bp4aug_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int attempt_iter,
                                  int max_attempts, float density, int restart, uint64_t seed, uint64_t first_sample, const float* llr_ch,
                                  float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat,
                                  int32_t* stats, void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (pre_iter < 1 || attempt_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and attempt_iter must be >= 1");
    if (max_attempts < 0 || max_attempts > 65535) return fgnn_fail(FGNN_ERR_ARG, "max_attempts must be in 0 .. 65535");
    if (!std::isfinite(density) || density < 0.0f || density > 1.0f) return fgnn_fail(FGNN_ERR_ARG, "density must be finite and in [0, 1]");
    if (restart != 0 && restart != 1) return fgnn_fail(FGNN_ERR_ARG, "restart must be 0 or 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    AugArgs a;
    step_args_fill(a, L, B, pre_iter, max_attempts, attempt_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.pre_iter = pre_iter;
    a.attempt_iter = attempt_iter;
    a.attempts = max_attempts;
    a.restart = restart;
    a.factor = normalization_factor;
    a.density = density;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    a.first_sample = first_sample;
    // per codeword: E messages, n decision bytes and the marks, a byte per qubit on the (3,3,6) rows and a byte per slot in the loop;
    // per workgroup: a stamp per codeword and ndone
    const bool regular = cn_type == FGNN_CN_MINSUM && step_regular_336(g);  // step_dispatch's choice
    const size_t mark_bytes = regular ? g->d.n : g->d.E;
    const size_t d_off = lds_round4(g->d.E), m_off = d_off + lds_bytes_as_floats(g->d.n);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "augmented BP4", m_off + lds_bytes_as_floats(mark_bytes), 0, L.cpb + 1, &lds_bytes)) return err;
    a.d_off = (int)d_off;
    a.m_off = (int)m_off;
    a.mark_bytes = (int)mark_bytes;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(bp4aug_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
