// fgnn_bp4fb.hip — BP4 with prior feedback, LDS-resident: when BP4 has run its iterations without a solution, the unsatisfied checks of
// its last estimate choose qubits whose channel LLRs are changed, and BP4 runs again.  Two hand-written rules:
//   FGNN_FB_PERTURB   random perturbation (Poulin, Chung, "On the iterative decoding of sparse quantum codes", 2008): every qubit on an
//                     unsatisfied check gets three seeded random reductions of its LLRs;
//   FGNN_FB_ENHANCED  enhanced feedback (Wang, Sanders, Poulin, "Enhanced feedback iterative decoding of sparse quantum codes", 2012):
//                     one qubit of one unsatisfied check gets the two Paulis that anticommute with the check made likelier or less likely.
// The algorithm is stated to the float operation at fgnn_bp4fb_decode in include/fgnn.h.  The kernel stands on the frame of the
// step-loop decoders (fgnn_step.h): codeword rows, staged syndrome bits, a qubit's slots with the literal edge rule (fgnn_vn.h), a
// check's row and parity, the output write; the check rule is the shared one (fgnn_cn.h).  Its own are the attempt walk below, the
// `mark` bytes, the keys and the Philox draws.  lamhat is never stored: the thread that owns a qubit re-reads
// the channel LLRs from global memory (L2) and, for a marked qubit only, re-derives the change, for PERTURB from one Philox block
// (fgnn_rng.h, integer instructions only).  Feedback never accumulates: every attempt's lamhat is the channel LLRs plus one change.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (the byte count of fgnn_bp4gd_decode):
//   msg  [E_x + E_z]  c->v / v->c messages, bp4_kernel's layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last test
//   mark [n] bytes    0 = lamhat_v is the channel LLRs; 1 + 2 side + s = enhanced feedback from a check of side 0 (hx) / 1 (hz) with
//                     syndrome bit s; 5 = perturbed
// and per workgroup
//   key[2 cpb]   (64-bit) the ENHANCED selection keys, two per codeword, used alternately by attempt parity
//   stamp[cpb]   the number of the last workgroup step in which a check of the codeword saw odd parity
//   ndone        finished codewords
//
// A codeword walks attempts r = 0 .. A (r = feedback steps made so far) of T = pre_iter or attempt_iter check updates; an attempt takes
// T + 1 workgroup steps, k = 0 .. T counting its finished check updates:
//   qubits   lamhat from the channel LLRs and mark[v];  k > 0: marginals, decision into dec;  k = T: the owner clears mark[v], no
//            messages;  k < T: v->c messages (k = 0 of a restarting attempt: the owner zeroes the qubit's slots first)
//   barrier
//   checks   k > 0: parity of the decisions against the syndrome bit (stamp);  k = T and attempts left: a check of odd parity marks its
//            qubits (PERTURB: several checks may store the same byte 5) or posts its key with a 64-bit atomicMax (ENHANCED);
//            k < T: check update
//   barrier
//   control  solved / out of attempts: outputs, done.  k = T, ENHANCED: every thread reads the winning check, recomputes its Philox
//            block for the qubit v*, the owner of v* stores the mark, the other key word is cleared
// mark[v] is read and cleared by the owner of v in qubit phases and written in the check phase / control section of step k = T only:
// a barrier lies between the clearing and the marking, and between the marking and the next read (ENHANCED: both by the owner itself).
// The key of check c is (uint64) w[0] << 32 | (0xFFFFFFFF - c), never 0: the maximum of a total order, whatever the arrival order.
// No float atomics; no result depends on the order in which threads arrive.
//
// Registers.  Compiled for FGNN_BP4FB_WAVES waves per SIMD, the most at which no instantiation needs scratch (DESIGN.md section 4,
// "Prior feedback", lists what each instantiation takes).
#include <cmath>

#include "fgnn_step.h"
#include "fgnn_rng.h"
#include "fgnn_cn.h"

#ifndef FGNN_BP4FB_WAVES
#define FGNN_BP4FB_WAVES 6  // waves per SIMD the register allocation aims at
#endif

namespace {

constexpr int FB_MARK_PERTURB = 5;
constexpr uint32_t FB_STREAM_PERTURB = 3, FB_STREAM_ENHANCED = 4;  // streams 0-2 of fgnn_rng.h keep the fourth counter word below 256

struct FbArgs : StepArgs {
    int rule, pre_iter, attempt_iter, attempts, restart, m_off;
    float factor, strength;
    uint32_t seed_lo, seed_hi;
    uint64_t first_sample;
};

// lamhat of a marked qubit from its channel LLRs (order X, Y, Z).  f = 5: lam - F * u, one product, then one subtraction, per LLR;
// f = 1 + 2 side + s: t = s ? -F : +F added to Y and to Z (hx check) or X (hz check)
__device__ __forceinline__ void fb_lamhat(int f, float F, const uint32_t w[4], float& lx, float& ly, float& lz)
{
    if (f == FB_MARK_PERTURB) {
        lx = lx - F * fg_u32_to_unit(w[0]);
        ly = ly - F * fg_u32_to_unit(w[1]);
        lz = lz - F * fg_u32_to_unit(w[2]);
    } else {
        const float t = ((f - 1) & 1) ? -F : F;
        ly = ly + t;
        if (f <= 2)
            lz = lz + t;
        else
            lx = lx + t;
    }
}

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_BP4FB_WAVES))) bp4fb_kernel(GraphDev g, FbArgs a)
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
    uint8_t* mark = reinterpret_cast<uint8_t*>(msg + a.m_off);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(lds + (size_t)a.cpb * a.lds_per_cw);  // 16-byte aligned
    int* stamp = reinterpret_cast<int*>(key + 2 * a.cpb);
    int* ndone = stamp + a.cpb;
    const int n = g.n, m = g.m;
    const uint64_t sample = a.first_sample + (uint64_t)rows.bb;
    const uint32_t s_lo = (uint32_t)sample, s_hi = (uint32_t)(sample >> 32);

    // w(idx, att, s) of include/fgnn.h
    auto draw = [&](const uint32_t idx, const int att, const uint32_t stream, uint32_t w[4]) __attribute__((always_inline)) {
        fg_philox4x32_10(s_lo, s_hi, idx, ((uint32_t)att << 8) | stream, a.seed_lo, a.seed_hi, w);
    };

    for (int i = threadIdx.x; i < 5 * a.cpb + 1; i += blockDim.x) stamp[i - 4 * a.cpb] = 0;  // key words, stamp, ndone
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) {
            dec[v] = 0;
            mark[v] = 0;
        }
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    int r = 0, k = 0, its = 0;
    bool done = !cw.active;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.attempt_iter;
        const bool post = k == T && r < a.attempts;  // this step's test may be followed by a feedback step
        // ---- qubits: lamhat, marginals after k check updates and their decision, messages to the checks ----
        if (!done) {
            const bool zero = a.restart && k == 0 && r > 0;  // a restarting attempt starts from zero messages
            for (int v = lane; v < n; v += a.tpc) {
                const int f = mark[v];
                float lx, ly, lz;
                rows.llrs(n, v, a.llr_const, lx, ly, lz);
                if (f) {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    if (f == FB_MARK_PERTURB) draw((uint32_t)v, r, FB_STREAM_PERTURB, w);
                    fb_lamhat(f, a.strength, w, lx, ly, lz);
                }
                QubitSlots<DV> q(g, msg, v);
                if (zero) q.clear();
                float Sz, Sx;
                q.fetch(Sz, Sx);
                float X, Y, Z;
                vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
                if (k > 0) {  // the test's decision; after an attempt's last test the mark has served
                    dec[v] = (uint8_t)vn_decide(X, Y, Z);
                    if (k == T) {
                        if (f) mark[v] = 0;
                        continue;
                    }
                }
                q.store(X, Y, Z, vn_edge<VnMath>);
            }
        }
        __syncthreads();
        if (*ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0) and what an unsatisfied check feeds back, then the check update (k < T) ----
        if (!done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd.at(g, rows, i, c);
                const bool is_x = c < g.m_x;
                bool odd = false;
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0) {
                        odd = parity_regular<DV>(g, dec, off, is_x, sy) != 0u;
                        if (odd && post && a.rule == FGNN_FB_PERTURB) {
#pragma unroll
                            for (int j = 0; j < DC; ++j) mark[row_qubit<DV>(off[j], row_base(g, is_x))] = (uint8_t)FB_MARK_PERTURB;
                        }
                    }
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {
                        odd = parity_csr(g, dec, c0, deg, is_x, sy) != 0u;
                        if (odd && post && a.rule == FGNN_FB_PERTURB)
                            for (int j = 0; j < deg; ++j) mark[g.cvn[c0 + j]] = (uint8_t)FB_MARK_PERTURB;
                    }
                    if (k < T) cn_update<CN_TYPE, PhiBp4>(msg, g.cslot + c0, deg, sy, a.factor);
                }
                if (odd) {
                    stamp[cwl] = step;
                    if (post && a.rule == FGNN_FB_ENHANCED) {
                        uint32_t w[4];
                        draw((uint32_t)c, r + 1, FB_STREAM_ENHANCED, w);
                        atomicMax(&key[2 * cwl + (r & 1)], ((unsigned long long)w[0] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)c));
                    }
                }
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
                    if (a.rule == FGNN_FB_ENHANCED) {
                        // the winning check: every thread of the codeword reads it and finds its qubit v*, the owner of v* marks it
                        const unsigned cs = 0xFFFFFFFFu - (unsigned)(key[2 * cwl + (r & 1)] & 0xFFFFFFFFull);
                        const int c0 = cs < (unsigned)m ? g.cptr[cs] : 0, deg = cs < (unsigned)m ? g.cptr[cs + 1] - c0 : 0;
                        if (deg > 0) {  // a check without qubits changes nothing
                            uint32_t w[4];
                            draw(cs, r + 1, FB_STREAM_ENHANCED, w);
                            const int vs = g.cvn[c0 + fg_fy_pick(fg_u32_to_unit(w[1]), deg)];  // a check's qubits ascend
                            if (vs % a.tpc == lane) mark[vs] = (uint8_t)(1u + ((int)cs < g.m_x ? 0u : 2u) + rows.synd_of(g, (int)cs));
                        }
                        if (lane == 0) key[2 * cwl + ((r + 1) & 1)] = 0ull;  // read an attempt ago, posted to an attempt from now
                    }
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

extern "C" int fgnn_bp4fb_decode(const fgnn_graph* g, int rule, int cn_type, float normalization_factor, int pre_iter, int attempt_iter,
                                 int max_attempts, float strength, int restart, uint64_t seed, uint64_t first_sample, const float* llr_ch,
                                 float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat,
                                 int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (rule != FGNN_FB_PERTURB && rule != FGNN_FB_ENHANCED) return fgnn_fail(FGNN_ERR_ARG, "rule must be FGNN_FB_PERTURB or FGNN_FB_ENHANCED");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");  // decoding_q.py:107
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || attempt_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and attempt_iter must be >= 1");
    if (max_attempts < 0 || max_attempts > 65535) return fgnn_fail(FGNN_ERR_ARG, "max_attempts must be in 0 .. 65535");
    if (!std::isfinite(strength) || strength < 0.0f) return fgnn_fail(FGNN_ERR_ARG, "strength must be finite and >= 0");
    if (restart != 0 && restart != 1) return fgnn_fail(FGNN_ERR_ARG, "restart must be 0 or 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    FbArgs a;
    step_args_fill(a, L, B, pre_iter, max_attempts, attempt_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.rule = rule;
    a.pre_iter = pre_iter;
    a.attempt_iter = attempt_iter;
    a.attempts = max_attempts;
    a.restart = restart;
    a.factor = normalization_factor;
    a.strength = strength;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    a.first_sample = first_sample;
    // per codeword: E messages, n decision bytes and n mark bytes; per workgroup: two 64-bit keys and a stamp per codeword, ndone:
    // the byte count of fgnn_bp4gd_decode
    const size_t d_off = lds_round4(g->d.E), m_off = d_off + lds_bytes_as_floats(g->d.n);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "BP4 feedback", m_off + lds_bytes_as_floats(g->d.n), 0, 5 * L.cpb + 1, &lds_bytes)) return err;
    a.d_off = (int)d_off;
    a.m_off = (int)m_off;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(bp4fb_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
