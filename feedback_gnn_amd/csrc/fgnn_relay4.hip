// fgnn_relay4.hip — Relay-BP4: a chain of min-sum BP4 runs ("legs") with per-qubit memory strengths on both Tanner graphs, LDS-resident.
//
// Relay-BP's memory term (Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories", 2025)
// applied to each of a qubit's three LLRs, in the form include/fgnn.h states at fgnn_relay4_decode.  The qubit update is the literal
// form of fgnn_vn.h (one log-sum-exp per edge, fgnn_math.h) with the memory-weighted LLRs Lam in place of the channel LLRs,
// the check update is the shared min-sum rule of fgnn_cn.h, the leg / stop / weight control is relay_kernel's (fgnn_relay.hip).  No
// saturation shortcuts, no register-resident channel LLRs, no hardware transcendentals: the channel LLRs are re-read from global
// memory (L2) by the thread that owns the qubit, every float operation is the one bp4_kernel and cn_update execute, in their order.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (relay4_lds_bytes in tests/test_gpu_relay4.py mirrors it):
//   msg [E_x + E_z]  c->v / v->c messages, slot e in [0,E_x) = hx edges, [E_x,E) = hz edges, sorted by (qubit, check): bp4_kernel's layout
//   M   [3n]         posteriors M^X [0,n), M^Y [n,2n), M^Z [2n,3n): the memory term reads them, the next leg starts from them
//   dec [n] bytes    decisions d_v = x_v | z_v << 1 of the last test: the parity test gathers them in the same sweep as the check update
// and per workgroup stamp[cpb], wacc[cpb], ndone (ints), as relay_kernel:
//   stamp[cw]  the number of the last workgroup step in which a check of the codeword saw odd parity (no reset needed)
//   wacc[cw]   running total of the weights of the decisions weighed so far (integer atomics; a thread keeps the previous total)
//   ndone      finished codewords; read by all threads in the same interval, so leaving the loop is a uniform decision
// [[882,24]]: 5292 + 2648 + 224 floats = 32 656 bytes per codeword; [[1270,28]]: 7620 + 3812 + 320 floats = 47 008 bytes.
//
// Codewords of one workgroup stop at different steps: leg, step of the leg, solutions found and best weight are registers every thread of
// a codeword holds identically; what crosses threads goes through the LDS words above, written in one barrier interval and read in the next.
//
// Occupancy.  With 256 threads (4 waves) per codeword the LDS above admits 4 workgroups of [[882,24]] on a CU (5 x (32 672 + the 256
// bytes of the log table) exceed 160 KiB) and 3 of [[1270,28]]: 4 waves per SIMD at the most, whatever the registers allow.  The kernels
// are therefore compiled for 4 waves per SIMD (a budget of 128 VGPRs): the (3,3,6) instantiation takes 88 VGPRs and the loop 67, no
// spills, no scratch.  Asking for more waves would only squeeze the allocation of a kernel whose residency LDS decides.
#include <climits>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"

#ifndef FGNN_RELAY4_WAVES
#define FGNN_RELAY4_WAVES 4  // waves per SIMD the register allocation aims at: what the LDS of the benchmark codes admits
#endif

namespace {

struct Relay4Args {
    int B, pre_iter, num_legs, leg_iter, stop_nconv, max_steps, tpc, cpb, lds_per_cw, m_off, d_off;
    float factor, llr_const;
    const float* gamma;      // [num_legs,n]
    const float* llr_ch;     // [B,3,n] or null
    const uint8_t* synd_x;   // [B,m_x] or null (all-zero syndrome)
    const uint8_t* synd_z;   // [B,m_z] or null
    uint8_t* x_hat;          // [B,n]
    uint8_t* z_hat;          // [B,n]
    int32_t* stats;          // [B,4]
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
    const int cwl = threadIdx.x / a.tpc;
    const int lane = threadIdx.x - cwl * a.tpc;
    const int b = blockIdx.x * a.cpb + cwl;
    const bool active = b < a.B;
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* M = msg + a.m_off;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    int* stamp = reinterpret_cast<int*>(lds + (size_t)a.cpb * a.lds_per_cw);
    int* wacc = stamp + a.cpb;
    int* ndone = wacc + a.cpb;
    const int n = g.n, m = g.m;
    const size_t bb = active ? (size_t)b : 0;
    const float* lch = a.llr_ch ? a.llr_ch + bb * 3 * n : nullptr;
    const uint8_t* sx = a.synd_x ? a.synd_x + bb * g.m_x : nullptr;
    const uint8_t* sz = a.synd_z ? a.synd_z + bb * g.m_z : nullptr;
    const int nact = min(a.cpb, a.B - (int)blockIdx.x * a.cpb);

    auto synd_of = [&](const int c) __attribute__((always_inline)) -> unsigned {
        const uint8_t* s = c < g.m_x ? sx : sz;
        return s ? (s[c < g.m_x ? c : c - g.m_x] & 1u) : 0u;
    };

    for (int i = threadIdx.x; i < 2 * a.cpb + 1; i += blockDim.x) stamp[i] = 0;
    if (active)
        for (int v = lane; v < n; v += a.tpc) {
            M[v] = lch ? lch[v] : a.llr_const;
            M[n + v] = lch ? lch[n + v] : a.llr_const;
            M[2 * n + v] = lch ? lch[2 * n + v] : a.llr_const;
            dec[v] = 0;
        }
    const bool synd_in_reg = (m + a.tpc - 1) / a.tpc <= 32;
    unsigned synd_bits = 0;
    if (active && synd_in_reg) {
        int i = 0;
        for (int c = lane; c < m; c += a.tpc, ++i) synd_bits |= synd_of(c) << i;
    }
    __syncthreads();

    int r = 0, k = 0, found = 0, best_w = 0, best_r = 0, best_k = 0, wprev = 0, pend_r = 0, pend_k = 0;
    bool done = !active, written = !active, pending = false;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.leg_iter;
        // ---- qubits: marginals after k check updates and their decision, memory term, messages to the checks ----
        if (!done) {
            const float* gam = a.gamma + (size_t)r * n;
            for (int v = lane; v < n; v += a.tpc) {
                const float lx = lch ? lch[v] : a.llr_const, ly = lch ? lch[n + v] : a.llr_const, lz = lch ? lch[2 * n + v] : a.llr_const;
                const float gv = gam[v];
                const float om = 1.0f - gv;
                float MX = M[v], MY = M[n + v], MZ = M[2 * n + v];
                // the qubit's c->v messages (zeros before the first check update of a leg) and their sums: only this fetch and the
                // store below differ between the regular rows, which keep the messages in registers, and the runtime degrees
                const int x0 = REGULAR ? v * DV : g.vptr_x[v], z0 = REGULAR ? g.E_x + v * DV : g.vptr_z[v];
                const int dx = REGULAR ? DV : g.vptr_x[v + 1] - x0, dz = REGULAR ? DV : g.vptr_z[v + 1] - z0;
                float* px = msg + x0;
                float* pz = msg + z0;
                float mx[REGULAR ? DV : 1], mz[REGULAR ? DV : 1];
                float Sz = 0.0f, Sx = 0.0f;
                if constexpr (REGULAR) {
                    if (k > 0) {
#pragma unroll
                        for (int j = 0; j < DV; ++j) { mz[j] = pz[j]; Sz = Sz + mz[j]; }
#pragma unroll
                        for (int j = 0; j < DV; ++j) { mx[j] = px[j]; Sx = Sx + mx[j]; }
                    } else {
#pragma unroll
                        for (int j = 0; j < DV; ++j) mz[j] = mx[j] = 0.0f;
                    }
                } else if (k > 0) {
                    vn_sums(msg, z0, z0 + dz, x0, x0 + dx, Sz, Sx);
                }
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
                const float numx = VnMath::softplus(-X);
                const float numz = VnMath::softplus(-Z);
                if constexpr (REGULAR) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) px[j] = vn_edge<VnMath>(numx, Z, Y, mx[j]);
#pragma unroll
                    for (int j = 0; j < DV; ++j) pz[j] = vn_edge<VnMath>(numz, X, Y, mz[j]);
                } else {
                    for (int j = 0; j < dx; ++j) px[j] = vn_edge<VnMath>(numx, Z, Y, k > 0 ? px[j] : 0.0f);
                    for (int j = 0; j < dz; ++j) pz[j] = vn_edge<VnMath>(numz, X, Y, k > 0 ? pz[j] : 0.0f);
                }
            }
        }
        __syncthreads();
        // ---- the decision weighed in the previous step: its weight is complete now, dec still holds it ----
        if (pending) {
            const int total = wacc[cwl];
            const int w = total - wprev;
            wprev = total;
            if (found <= 1 || w < best_w) {
                best_w = w;
                best_r = pend_r;
                best_k = pend_k;
                for (int v = lane; v < n; v += a.tpc) {
                    const unsigned d = dec[v];
                    a.x_hat[bb * n + v] = (uint8_t)(d & 1u);
                    a.z_hat[bb * n + v] = (uint8_t)(d >> 1);
                }
            }
            pending = false;
        }
        if (done && !written) {
            if (lane == 0) {
                int32_t* st = a.stats + (size_t)b * 4;
                st[0] = found;
                st[1] = best_w;
                st[2] = best_r;
                st[3] = best_k;
            }
            written = true;
        }
        if (*ndone == nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the min-sum update (k < T) ----
        if (!done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = synd_in_reg ? ((synd_bits >> i) & 1u) : synd_of(c);
                const bool is_x = c < g.m_x;
                const int sh = is_x ? 1 : 0;  // hx rows test z_hat (bit 1 of the decision), hz rows x_hat (bit 0)
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
                        if (par) stamp[cwl] = step;
                    }
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {
                        unsigned par = sy;
                        for (int j = 0; j < deg; ++j) par ^= ((unsigned)dec[g.cvn[c0 + j]] >> sh) & 1u;
                        if (par) stamp[cwl] = step;
                    }
                    if (k < T) cn_update<FGNN_CN_MINSUM, PhiGnn>(msg, g.cslot + c0, deg, sy, a.factor);
                }
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, leg over, decoder finished ----
        if (!done) {
            if (k == 0) {
                k = 1;
            } else {
                const bool sat = stamp[cwl] != step;
                const bool leg_end = sat || k == T;
                if (sat) ++found;
                const bool fin = leg_end && (r == a.num_legs - 1 || found == a.stop_nconv);
                if (sat || (fin && found == 0)) {  // weigh this decision: a solution, or the last test of a decoder that found none
                    int part = 0;
                    for (int v = lane; v < n; v += a.tpc) {
                        const int d = dec[v];
                        if (d) part += relay4_weight(d, lch ? lch[v] : a.llr_const, lch ? lch[n + v] : a.llr_const,
                                                     lch ? lch[2 * n + v] : a.llr_const);
                    }
                    if (part) atomicAdd(&wacc[cwl], part);
                    pending = true;
                    pend_r = r;
                    pend_k = k;
                }
                if (fin) {
                    done = true;
                    if (lane == 0) atomicAdd(ndone, 1);
                } else if (leg_end) {
                    ++r;
                    k = 0;
                } else {
                    ++k;
                }
            }
        }
    }
}

template <int DV, int DC>
int launch(const fgnn_graph* g, const Relay4Args& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    return fgnn_launch(relay4_kernel<DV, DC>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
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
    LaunchGeom L = fgnn_geom(g, B);
    Relay4Args a;
    a.B = B;
    a.pre_iter = pre_iter;
    a.num_legs = num_legs;
    a.leg_iter = leg_iter;
    a.stop_nconv = stop_nconv;
    // a codeword takes T + 1 steps per leg; one more step weighs its last decision
    const long long steps = (long long)pre_iter + 1 + (long long)(num_legs - 1) * ((long long)leg_iter + 1) + 1;
    a.max_steps = (int)std::min<long long>(steps, INT_MAX - 1);
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.gamma = gamma;
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.stats = stats;
    // per codeword: E messages, 3n posteriors and n decision bytes, each rounded up to 4 floats; per workgroup: stamp and wacc per
    // codeword, ndone
    const size_t m_off = ((size_t)g->d.E + 3) & ~(size_t)3;
    const size_t d_off = m_off + (((size_t)3 * g->d.n + 3) & ~(size_t)3);
    const size_t per_cw = d_off + ((((size_t)g->d.n + 3) / 4 + 3) & ~(size_t)3);
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb + (((size_t)2 * L.cpb + 1 + 3) & ~(size_t)3) * sizeof(int);
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident Relay-BP4 kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    a.m_off = (int)m_off;
    a.d_off = (int)d_off;
    a.lds_per_cw = (int)per_cw;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    if (g->d.cslot16 && !g->force_generic && g->d.dvx == 3 && g->d.dvz == 3 && g->d.dc == 6) return launch<3, 6>(g, a, L, lds_bytes, st);
    return launch<0, 0>(g, a, L, lds_bytes, st);
}
