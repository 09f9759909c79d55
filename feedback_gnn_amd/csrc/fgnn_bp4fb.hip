// fgnn_bp4fb.hip — BP4 with prior feedback, LDS-resident: when BP4 has run its iterations without a solution, the unsatisfied checks of
// its last estimate choose qubits whose channel LLRs are changed, and BP4 runs again.  Two hand-written rules:
//   FGNN_FB_PERTURB   random perturbation (Poulin, Chung, "On the iterative decoding of sparse quantum codes", 2008): every qubit on an
//                     unsatisfied check gets three seeded random reductions of its LLRs;
//   FGNN_FB_ENHANCED  enhanced feedback (Wang, Sanders, Poulin, "Enhanced feedback iterative decoding of sparse quantum codes", 2012):
//                     one qubit of one unsatisfied check gets the two Paulis that anticommute with the check made likelier or less likely.
// The algorithm is stated to the float operation at fgnn_bp4fb_decode in include/fgnn.h.  The kernel is bp4gd_kernel (fgnn_bp4gd.hip)
// with its `fix` bytes turned into `mark` bytes: the same message layout, literal qubit update (fgnn_vn.h), shared check rule
// (fgnn_cn.h), step / stop control, parity-by-stamp test and ndone exit.  lamhat is never stored: the thread that owns a qubit re-reads
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
#include <climits>
#include <cmath>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_rng.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"

#ifndef FGNN_BP4FB_WAVES
#define FGNN_BP4FB_WAVES 6  // waves per SIMD the register allocation aims at
#endif

namespace {

constexpr int FB_MARK_PERTURB = 5;
constexpr uint32_t FB_STREAM_PERTURB = 3, FB_STREAM_ENHANCED = 4;  // streams 0-2 of fgnn_rng.h keep the fourth counter word below 256

struct FbArgs {
    int B, rule, pre_iter, attempt_iter, attempts, restart, max_steps, tpc, cpb, lds_per_cw, d_off, m_off;
    float factor, llr_const, strength;
    uint32_t seed_lo, seed_hi;
    uint64_t first_sample;
    const float* llr_ch;     // [B,3,n] or null
    const uint8_t* synd_x;   // [B,m_x] or null (all-zero syndrome)
    const uint8_t* synd_z;   // [B,m_z] or null
    uint8_t* x_hat;          // [B,n]
    uint8_t* z_hat;          // [B,n]
    int32_t* stats;          // [B,4]
};

// the phi of BP4's check rule (decoding_q.py:365-373): what bp4_kernel's exact policy evaluates
struct PhiBp4 {
    static __device__ __forceinline__ float phi(float x) { return fg_phi(x); }
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
    const int cwl = threadIdx.x / a.tpc;
    const int lane = threadIdx.x - cwl * a.tpc;
    const int b = blockIdx.x * a.cpb + cwl;
    const bool active = b < a.B;
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    uint8_t* mark = reinterpret_cast<uint8_t*>(msg + a.m_off);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(lds + (size_t)a.cpb * a.lds_per_cw);  // 16-byte aligned
    int* stamp = reinterpret_cast<int*>(key + 2 * a.cpb);
    int* ndone = stamp + a.cpb;
    const int n = g.n, m = g.m;
    const size_t bb = active ? (size_t)b : 0;
    const float* lch = a.llr_ch ? a.llr_ch + bb * 3 * n : nullptr;
    const uint8_t* sx = a.synd_x ? a.synd_x + bb * g.m_x : nullptr;
    const uint8_t* sz = a.synd_z ? a.synd_z + bb * g.m_z : nullptr;
    const int nact = min(a.cpb, a.B - (int)blockIdx.x * a.cpb);
    const uint64_t sample = a.first_sample + (uint64_t)bb;
    const uint32_t s_lo = (uint32_t)sample, s_hi = (uint32_t)(sample >> 32);

    auto synd_of = [&](const int c) __attribute__((always_inline)) -> unsigned {
        const uint8_t* s = c < g.m_x ? sx : sz;
        return s ? (s[c < g.m_x ? c : c - g.m_x] & 1u) : 0u;
    };
    // w(idx, att, s) of include/fgnn.h
    auto draw = [&](const uint32_t idx, const int att, const uint32_t stream, uint32_t w[4]) __attribute__((always_inline)) {
        fg_philox4x32_10(s_lo, s_hi, idx, ((uint32_t)att << 8) | stream, a.seed_lo, a.seed_hi, w);
    };

    for (int i = threadIdx.x; i < 5 * a.cpb + 1; i += blockDim.x) stamp[i - 4 * a.cpb] = 0;  // key words, stamp, ndone
    if (active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) {
            dec[v] = 0;
            mark[v] = 0;
        }
    }
    const bool synd_in_reg = (m + a.tpc - 1) / a.tpc <= 32;
    unsigned synd_bits = 0;
    if (active && synd_in_reg) {
        int i = 0;
        for (int c = lane; c < m; c += a.tpc, ++i) synd_bits |= synd_of(c) << i;
    }
    __syncthreads();

    int r = 0, k = 0, its = 0;
    bool done = !active;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.attempt_iter;
        const bool post = k == T && r < a.attempts;  // this step's test may be followed by a feedback step
        // ---- qubits: lamhat, marginals after k check updates and their decision, messages to the checks ----
        if (!done) {
            const bool zero = a.restart && k == 0 && r > 0;  // a restarting attempt starts from zero messages
            for (int v = lane; v < n; v += a.tpc) {
                const int f = mark[v];
                float lx = lch ? lch[v] : a.llr_const;
                float ly = lch ? lch[n + v] : a.llr_const;
                float lz = lch ? lch[2 * n + v] : a.llr_const;
                if (f) {
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
                    if (f == FB_MARK_PERTURB) draw((uint32_t)v, r, FB_STREAM_PERTURB, w);
                    fb_lamhat(f, a.strength, w, lx, ly, lz);
                }
                // the qubit's c->v messages (zeros before the first check update) and their sums: only this fetch and the store
                // below differ between the regular rows, which keep the messages in registers, and the runtime degrees
                const int x0 = REGULAR ? v * DV : g.vptr_x[v], z0 = REGULAR ? g.E_x + v * DV : g.vptr_z[v];
                const int dx = REGULAR ? DV : g.vptr_x[v + 1] - x0, dz = REGULAR ? DV : g.vptr_z[v + 1] - z0;
                float* px = msg + x0;
                float* pz = msg + z0;
                if (zero) {  // the slots of a qubit are its owner's in this phase
                    for (int j = 0; j < dx; ++j) px[j] = 0.0f;
                    for (int j = 0; j < dz; ++j) pz[j] = 0.0f;
                }
                float mx[REGULAR ? DV : 1], mz[REGULAR ? DV : 1];
                float Sz = 0.0f, Sx = 0.0f;
                if constexpr (REGULAR) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) { mz[j] = pz[j]; Sz = Sz + mz[j]; }
#pragma unroll
                    for (int j = 0; j < DV; ++j) { mx[j] = px[j]; Sx = Sx + mx[j]; }
                } else {
                    vn_sums(msg, z0, z0 + dz, x0, x0 + dx, Sz, Sx);
                }
                float X, Y, Z;
                vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
                if (k > 0) {  // the test's decision; after an attempt's last test the mark has served
                    dec[v] = (uint8_t)vn_decide(X, Y, Z);
                    if (k == T) {
                        if (f) mark[v] = 0;
                        continue;
                    }
                }
                const float numx = VnMath::softplus(-X);
                const float numz = VnMath::softplus(-Z);
                if constexpr (REGULAR) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) px[j] = vn_edge<VnMath>(numx, Z, Y, mx[j]);
#pragma unroll
                    for (int j = 0; j < DV; ++j) pz[j] = vn_edge<VnMath>(numz, X, Y, mz[j]);
                } else {
                    for (int j = 0; j < dx; ++j) px[j] = vn_edge<VnMath>(numx, Z, Y, px[j]);
                    for (int j = 0; j < dz; ++j) pz[j] = vn_edge<VnMath>(numz, X, Y, pz[j]);
                }
            }
        }
        __syncthreads();
        if (*ndone == nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0) and what an unsatisfied check feeds back, then the check update (k < T) ----
        if (!done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd_in_reg ? ((synd_bits >> i) & 1u) : synd_of(c);
                const bool is_x = c < g.m_x;
                const int sh = is_x ? 1 : 0;  // hx rows test z_hat (bit 1 of the decision), hz rows x_hat (bit 0)
                bool odd = false;
                if constexpr (REGULAR) {
                    const uint4 pk = reinterpret_cast<const uint4*>(g.cslot16)[c];
                    const unsigned w[4] = {pk.x, pk.y, pk.z, pk.w};
                    unsigned off[DC];
#pragma unroll
                    for (int j = 0; j < DC; ++j) off[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                    if (k > 0) {
                        const unsigned base = is_x ? 0u : (unsigned)g.E_x;  // slot base + v * DV + j belongs to qubit v
                        unsigned par = sy;
#pragma unroll
                        for (int j = 0; j < DC; ++j) par ^= ((unsigned)dec[((off[j] >> 2) - base) / DV] >> sh) & 1u;
                        odd = par != 0u;
                        if (odd && post && a.rule == FGNN_FB_PERTURB) {
#pragma unroll
                            for (int j = 0; j < DC; ++j) mark[((off[j] >> 2) - base) / DV] = (uint8_t)FB_MARK_PERTURB;
                        }
                    }
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {
                        unsigned par = sy;
                        for (int j = 0; j < deg; ++j) par ^= ((unsigned)dec[g.cvn[c0 + j]] >> sh) & 1u;
                        odd = par != 0u;
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
                    for (int v = lane; v < n; v += a.tpc) {
                        const unsigned d = dec[v];
                        a.x_hat[bb * n + v] = (uint8_t)(d & 1u);
                        a.z_hat[bb * n + v] = (uint8_t)(d >> 1);
                    }
                    if (lane == 0) {
                        int32_t* st = a.stats + (size_t)b * 4;
                        st[0] = sat ? 1 : 0;
                        st[1] = r;
                        st[2] = its;
                        st[3] = k;
                        atomicAdd(ndone, 1);
                    }
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
                            if (vs % a.tpc == lane) mark[vs] = (uint8_t)(1u + ((int)cs < g.m_x ? 0u : 2u) + synd_of((int)cs));
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

template <int CN_TYPE, int DV, int DC>
int launch(const fgnn_graph* g, const FbArgs& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    return fgnn_launch(bp4fb_kernel<CN_TYPE, DV, DC>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
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
    LaunchGeom L = fgnn_geom(g, B);
    FbArgs a;
    a.B = B;
    a.rule = rule;
    a.pre_iter = pre_iter;
    a.attempt_iter = attempt_iter;
    a.attempts = max_attempts;
    a.restart = restart;
    // a codeword takes T + 1 steps per attempt; one more step lets the workgroup see its last codeword finished
    const long long steps = (long long)pre_iter + 1 + (long long)max_attempts * ((long long)attempt_iter + 1) + 1;
    a.max_steps = (int)std::min<long long>(steps, INT_MAX - 1);
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.strength = strength;
    a.seed_lo = (uint32_t)seed;
    a.seed_hi = (uint32_t)(seed >> 32);
    a.first_sample = first_sample;
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.stats = stats;
    // per codeword: E messages, n decision bytes and n mark bytes, each rounded up to 4 floats; per workgroup: two 64-bit keys and a
    // stamp per codeword, ndone: the byte count of fgnn_bp4gd_decode
    const size_t bytes_area = (((size_t)g->d.n + 3) / 4 + 3) & ~(size_t)3;
    const size_t d_off = ((size_t)g->d.E + 3) & ~(size_t)3;
    const size_t m_off = d_off + bytes_area;
    const size_t per_cw = m_off + bytes_area;
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb + (((size_t)5 * L.cpb + 1 + 3) & ~(size_t)3) * sizeof(int);
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident BP4 feedback kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    a.d_off = (int)d_off;
    a.m_off = (int)m_off;
    a.lds_per_cw = (int)per_cw;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch (cn_type) {
    case FGNN_CN_BOXPLUS: return launch<FGNN_CN_BOXPLUS, 0, 0>(g, a, L, lds_bytes, st);
    case FGNN_CN_BOXPLUS_PHI: return launch<FGNN_CN_BOXPLUS_PHI, 0, 0>(g, a, L, lds_bytes, st);
    default: break;
    }
    if (g->d.cslot16 && !g->force_generic && g->d.dvx == 3 && g->d.dvz == 3 && g->d.dc == 6)
        return launch<FGNN_CN_MINSUM, 3, 6>(g, a, L, lds_bytes, st);
    return launch<FGNN_CN_MINSUM, 0, 0>(g, a, L, lds_bytes, st);
}
