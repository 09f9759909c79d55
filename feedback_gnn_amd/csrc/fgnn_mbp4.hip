// fgnn_mbp4.hip — BP4 with message-strength control (MBP4 / AMBP4; Kuo, Lai, "Exploiting degeneracy in belief propagation decoding of
// quantum codes", 2022), flooding schedule, LDS-resident.  A codeword walks a list of attempts; attempt a multiplies every check output
// by factor[a] and takes an edge's own message out of the qubit totals multiplied by own[a] (vn_edge_own, fgnn_vn.h): with
// own[a] = alpha_a and factor[a] = base / alpha_a that is MBP4 at strength alpha_a, and a descending list of alphas is AMBP4.  The
// algorithm is stated to the float operation at fgnn_mbp4_decode in include/fgnn.h.  The kernel is a sibling of bp4fb_kernel
// (fgnn_bp4fb.hip): the same message layout, literal qubit update, shared check rule (fgnn_cn.h), step / stop control,
// parity-by-stamp test and ndone exit; it has no mark bytes and no random draws, and lamhat is always the channel LLRs.
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
#include <climits>
#include <cmath>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"

#ifndef FGNN_MBP4_WAVES
#define FGNN_MBP4_WAVES 7  // waves per SIMD the register allocation aims at
#endif

namespace {

constexpr int MBP4_MAX_ATTEMPTS = 64;

struct MbArgs {
    int B, pre_iter, attempt_iter, attempts, restart, max_steps, tpc, cpb, lds_per_cw, d_off;
    float llr_const;
    const float* llr_ch;     // [B,3,n] or null
    const uint8_t* synd_x;   // [B,m_x] or null (all-zero syndrome)
    const uint8_t* synd_z;   // [B,m_z] or null
    uint8_t* x_hat;          // [B,n]
    uint8_t* z_hat;          // [B,n]
    int32_t* stats;          // [B,4]
    float tab[2 * MBP4_MAX_ATTEMPTS];  // factor[0..63], own[0..63]; entries from `attempts` on are 0 and never read
};

// the phi of BP4's check rule (decoding_q.py:365-373): what bp4_kernel's exact policy evaluates
struct PhiBp4 {
    static __device__ __forceinline__ float phi(float x) { return fg_phi(x); }
};

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_MBP4_WAVES))) mbp4_kernel(GraphDev g, MbArgs a)
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
    float* tab = lds + (size_t)a.cpb * a.lds_per_cw;
    int* stamp = reinterpret_cast<int*>(tab + 2 * MBP4_MAX_ATTEMPTS);
    int* ndone = stamp + a.cpb;
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

    for (int i = threadIdx.x; i < 2 * MBP4_MAX_ATTEMPTS; i += blockDim.x) tab[i] = a.tab[i];
    for (int i = threadIdx.x; i < a.cpb + 1; i += blockDim.x) stamp[i] = 0;  // stamp, ndone
    if (active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
    }
    const bool synd_in_reg = (m + a.tpc - 1) / a.tpc <= 32;
    unsigned synd_bits = 0;
    if (active && synd_in_reg) {
        int i = 0;
        for (int c = lane; c < m; c += a.tpc, ++i) synd_bits |= synd_of(c) << i;
    }
    __syncthreads();

    int r = 0, k = 0, its = 0;  // r < a.attempts <= 64 throughout: the last attempt ends the codeword
    bool done = !active;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.attempt_iter;
        // ---- qubits: marginals after k check updates and their decision, messages to the checks ----
        if (!done) {
            const bool zero = a.restart && k == 0 && r > 0;  // a restarting attempt starts from zero messages
            const float ow = tab[MBP4_MAX_ATTEMPTS + r];
            for (int v = lane; v < n; v += a.tpc) {
                const float lx = lch ? lch[v] : a.llr_const;
                const float ly = lch ? lch[n + v] : a.llr_const;
                const float lz = lch ? lch[2 * n + v] : a.llr_const;
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
                if (k > 0) {  // the test's decision; an attempt's last test sends no messages
                    dec[v] = (uint8_t)vn_decide(X, Y, Z);
                    if (k == T) continue;
                }
                const float numx = VnMath::softplus(-X);
                const float numz = VnMath::softplus(-Z);
                if constexpr (REGULAR) {
#pragma unroll
                    for (int j = 0; j < DV; ++j) px[j] = vn_edge_own<VnMath>(numx, Z, Y, mx[j], ow);
#pragma unroll
                    for (int j = 0; j < DV; ++j) pz[j] = vn_edge_own<VnMath>(numz, X, Y, mz[j], ow);
                } else {
                    for (int j = 0; j < dx; ++j) px[j] = vn_edge_own<VnMath>(numx, Z, Y, px[j], ow);
                    for (int j = 0; j < dz; ++j) pz[j] = vn_edge_own<VnMath>(numz, X, Y, pz[j], ow);
                }
            }
        }
        __syncthreads();
        if (*ndone == nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs: parity of the decisions (k > 0), then the check update (k < T) ----
        if (!done) {
            const float fac = tab[r];
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
                    }
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, fac);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {
                        unsigned par = sy;
                        for (int j = 0; j < deg; ++j) par ^= ((unsigned)dec[g.cvn[c0 + j]] >> sh) & 1u;
                        odd = par != 0u;
                    }
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
int launch(const fgnn_graph* g, const MbArgs& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    return fgnn_launch(mbp4_kernel<CN_TYPE, DV, DC>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
}

}  // namespace

extern "C" int fgnn_mbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                                int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                                const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");  // decoding_q.py:107
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
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
    LaunchGeom L = fgnn_geom(g, B);
    MbArgs a;
    a.B = B;
    a.pre_iter = pre_iter;
    a.attempt_iter = attempt_iter;
    a.attempts = num_attempts;
    a.restart = restart;
    // a codeword takes T + 1 steps per attempt; one more step lets the workgroup see its last codeword finished
    const long long steps = (long long)pre_iter + 1 + (long long)(num_attempts - 1) * ((long long)attempt_iter + 1) + 1;
    a.max_steps = (int)std::min<long long>(steps, INT_MAX - 1);
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.llr_const = llr_const;
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.stats = stats;
    for (int i = 0; i < MBP4_MAX_ATTEMPTS; ++i) {
        a.tab[i] = i < num_attempts ? factor[i] : 0.0f;
        a.tab[MBP4_MAX_ATTEMPTS + i] = i < num_attempts ? own[i] : 0.0f;
    }
    // per codeword: E messages and n decision bytes, each rounded up to 4 floats; per workgroup: the two 64-float tables, a stamp per
    // codeword and ndone
    const size_t bytes_area = (((size_t)g->d.n + 3) / 4 + 3) & ~(size_t)3;
    const size_t d_off = ((size_t)g->d.E + 3) & ~(size_t)3;
    const size_t per_cw = d_off + bytes_area;
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb + (size_t)2 * MBP4_MAX_ATTEMPTS * sizeof(float) +
                             (((size_t)L.cpb + 1 + 3) & ~(size_t)3) * sizeof(int);
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident MBP4 kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    a.d_off = (int)d_off;
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
