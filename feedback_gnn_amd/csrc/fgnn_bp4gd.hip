// fgnn_bp4gd.hip — BP4 with guided decimation (BP4-GD), LDS-resident: when BP4 has run its iterations without a solution, the most
// reliable undecided qubit is fixed to its current decision and BP4 goes on from the messages it has.
//
// Yao, Abu Laban, Haeger, Amat, Pfister, "Belief propagation decoding of quantum LDPC codes with guided decimation" (2023), quaternary
// variant, in the form include/fgnn.h states at fgnn_bp4gd_decode.  The qubit update is the literal form of fgnn_vn.h (one log-sum-exp
// per edge, fgnn_math.h) with the decimated LLRs lamhat in place of the channel LLRs, the check update is the shared rule of fgnn_cn.h,
// the step / stop control is relay4_kernel's (fgnn_relay4.hip).  No saturation shortcuts, no register-resident channel LLRs, no
// hardware transcendentals: the channel LLRs are re-read from global memory (L2) by the thread that owns the qubit and overridden
// where the qubit is fixed; every float operation is the one bp4_kernel and cn_update execute, in their order.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (bp4gd_lds_bytes in tests/test_gpu_bp4gd.py mirrors it):
//   msg [E_x + E_z]  c->v / v->c messages, slot e in [0,E_x) = hx edges, [E_x,E) = hz edges, sorted by (qubit, check): bp4_kernel's layout
//   dec [n] bytes    decisions d_v = x_v | z_v << 1 of the last test: the parity test gathers them in the same sweep as the check update
//   fix [n] bytes    0 = free, 1 + d = fixed to d; written and read by the thread that owns the qubit only: no barrier orders them
// and per workgroup
//   key[2 cpb]   (64-bit) the selection keys, two per codeword, used alternately by round parity: margin bits << 32 | ~v
//   stamp[cpb]   the number of the last workgroup step in which a check of the codeword saw odd parity (no reset needed)
//   ndone        finished codewords; read by all threads in the same interval, so leaving the loop is a uniform decision
// [[882,24]]: 5292 + 224 + 224 floats = 22 960 bytes per codeword; [[1270,28]]: 7620 + 320 + 320 floats = 33 040 bytes.
//
// A codeword walks rounds r = 0 .. R (r = qubits fixed so far) of T = pre_iter or round_iter check updates; a round takes T + 1
// workgroup steps, k = 0 .. T counting its finished check updates:
//   qubits   k > 0: marginals of the messages, decision into dec; k = T: the free qubits post their selection key, no messages;
//            k < T: v->c messages from the same totals (k = 0: totals on the lamhat that holds the qubit fixed at the end of the last round)
//   barrier
//   checks   k > 0: parity of the decisions against the syndrome bit (stamp); k < T: check update
//   barrier
//   control  solved / out of rounds: outputs, done.  k = T: read the winning key, its owner sets fix, the other key word is cleared
// The key of qubit v is (float bits of margin_v) << 32 | (0xFFFFFFFF - v): the margin is >= +0 (the marginals are sums that start from
// +0.0f, so none is -0), its bits order as unsigned integers, and the low word makes the lowest index win a tie.  A 64-bit integer
// atomicMax per free qubit finds the maximum of a total order, whatever the arrival order: no float atomics.  A key word is cleared one
// round after it was read, by one thread, in the control section that reads the other word: at least two barriers before its next post.
//
// Codewords of one workgroup stop at different steps: round, step of the round and iteration count are registers every thread of a
// codeword holds identically; what crosses threads goes through the LDS words above, written in one barrier interval and read in a later one.
//
// Occupancy.  With 256 threads (4 waves) per codeword the LDS above admits 7 workgroups of [[882,24]] on a CU by the byte count
// (7 x (22 992 + the 256 bytes of the log table) = 162 736 of 163 840 bytes) and 4 of [[1270,28]].  Seven waves per SIMD leave a budget
// of 72 VGPRs, at which three of the four instantiations spill to scratch; at six (a budget of 80 VGPRs) none does.  The kernels are
// therefore compiled for 6 waves per SIMD: the registers, not the LDS, hold [[882,24]] to six workgroups per CU.  DESIGN.md section 4
// lists what each instantiation takes.
#include <climits>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"

#ifndef FGNN_BP4GD_WAVES
#define FGNN_BP4GD_WAVES 6  // waves per SIMD the register allocation aims at: the most at which no instantiation needs scratch
#endif

namespace {

struct GdArgs {
    int B, pre_iter, round_iter, rounds, max_steps, tpc, cpb, lds_per_cw, d_off, f_off;
    float factor, llr_const, decim;
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

// lamhat of a qubit fixed to d (f = 1 + d), order X, Y, Z: the fixed Pauli's LLR is -D and the others +0; the identity holds all three at +D
__device__ __forceinline__ void gd_fixed_llrs(int f, float D, float& lx, float& ly, float& lz)
{
    lx = f == 1 ? D : (f == 2 ? -D : 0.0f);
    ly = f == 1 ? D : (f == 4 ? -D : 0.0f);
    lz = f == 1 ? D : (f == 3 ? -D : 0.0f);
}

// margin of decision d over the runner-up among c = (0, X, Z, Y): min(c_j, j != d) - c_d, one subtraction
__device__ __forceinline__ float gd_margin(int d, float X, float Y, float Z)
{
    const float cd = d == 0 ? 0.0f : (d == 1 ? X : (d == 2 ? Z : Y));
    const float a = d == 0 ? X : 0.0f;           // c_0, or c_1 when d = 0
    const float b = (d == 0 || d == 1) ? Z : X;  // the two others
    const float c = d == 3 ? Z : Y;
    return FG_MIN(FG_MIN(a, b), c) - cd;
}

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_BP4GD_WAVES))) bp4gd_kernel(GraphDev g, GdArgs a)
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
    uint8_t* fix = reinterpret_cast<uint8_t*>(msg + a.f_off);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(lds + (size_t)a.cpb * a.lds_per_cw);  // 16-byte aligned
    int* stamp = reinterpret_cast<int*>(key + 2 * a.cpb);
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

    for (int i = threadIdx.x; i < 5 * a.cpb + 1; i += blockDim.x) stamp[i - 4 * a.cpb] = 0;  // key words, stamp, ndone
    if (active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) {
            dec[v] = 0;
            fix[v] = 0;
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
        const int T = (r == 0) ? a.pre_iter : a.round_iter;
        // ---- qubits: marginals after k check updates and their decision, selection key, messages to the checks ----
        if (!done) {
            const bool post = k == T && r < a.rounds;
            for (int v = lane; v < n; v += a.tpc) {
                const int f = fix[v];
                float lx, ly, lz;
                if (f) {
                    gd_fixed_llrs(f, a.decim, lx, ly, lz);
                } else {
                    lx = lch ? lch[v] : a.llr_const;
                    ly = lch ? lch[n + v] : a.llr_const;
                    lz = lch ? lch[2 * n + v] : a.llr_const;
                }
                // the qubit's c->v messages (zeros before the first check update) and their sums: only this fetch and the store
                // below differ between the regular rows, which keep the messages in registers, and the runtime degrees
                const int x0 = REGULAR ? v * DV : g.vptr_x[v], z0 = REGULAR ? g.E_x + v * DV : g.vptr_z[v];
                const int dx = REGULAR ? DV : g.vptr_x[v + 1] - x0, dz = REGULAR ? DV : g.vptr_z[v + 1] - z0;
                float* px = msg + x0;
                float* pz = msg + z0;
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
                if (k > 0) {  // the test's decision; at the end of a round the free qubits bid for the next fix
                    const int d = vn_decide(X, Y, Z);
                    dec[v] = (uint8_t)d;
                    if (k == T) {
                        if (post && !f)
                            atomicMax(&key[2 * cwl + (r & 1)],
                                      ((unsigned long long)fg_f2u(gd_margin(d, X, Y, Z)) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v));
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
        // ---- checks of both graphs: parity of the decisions (k > 0), then the check update (k < T) ----
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
                    if (k < T) cn_update<CN_TYPE, PhiBp4>(msg, g.cslot + c0, deg, sy, a.factor);
                }
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, round over, decoder finished ----
        if (!done) {
            if (k == 0) {
                k = 1;
                ++its;
            } else {
                const bool sat = stamp[cwl] != step;
                if (sat || (k == T && r == a.rounds)) {
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
                    // the winner of this round's bids: every thread of the codeword reads it, the qubit's owner fixes it to its decision
                    const unsigned vs = 0xFFFFFFFFu - (unsigned)(key[2 * cwl + (r & 1)] & 0xFFFFFFFFull);
                    if (vs < (unsigned)n && (int)(vs % (unsigned)a.tpc) == lane) fix[vs] = (uint8_t)(1u + dec[vs]);
                    if (lane == 0) key[2 * cwl + ((r + 1) & 1)] = 0ull;  // read a round ago, posted to a round from now
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
int launch(const fgnn_graph* g, const GdArgs& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    return fgnn_launch(bp4gd_kernel<CN_TYPE, DV, DC>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
}

}  // namespace

extern "C" int fgnn_bp4gd_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int round_iter, int max_rounds,
                                 float decim_llr, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B,
                                 uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");  // decoding_q.py:107
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || round_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and round_iter must be >= 1");
    if (max_rounds < 0) return fgnn_fail(FGNN_ERR_ARG, "max_rounds must be >= 0");
    if (!(decim_llr > 0.0f)) return fgnn_fail(FGNN_ERR_ARG, "decim_llr must be > 0");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    LaunchGeom L = fgnn_geom(g, B);
    GdArgs a;
    a.B = B;
    a.pre_iter = pre_iter;
    a.round_iter = round_iter;
    a.rounds = std::min(max_rounds, g->d.n);
    // a codeword takes T + 1 steps per round; one more step lets the workgroup see its last codeword finished
    const long long steps = (long long)pre_iter + 1 + (long long)a.rounds * ((long long)round_iter + 1) + 1;
    a.max_steps = (int)std::min<long long>(steps, INT_MAX - 1);
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.factor = normalization_factor;
    a.llr_const = llr_const;
    a.decim = decim_llr;
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.stats = stats;
    // per codeword: E messages, n decision bytes and n fix bytes, each rounded up to 4 floats; per workgroup: two 64-bit keys and a
    // stamp per codeword, ndone
    const size_t bytes_area = (((size_t)g->d.n + 3) / 4 + 3) & ~(size_t)3;
    const size_t d_off = ((size_t)g->d.E + 3) & ~(size_t)3;
    const size_t f_off = d_off + bytes_area;
    const size_t per_cw = f_off + bytes_area;
    const size_t lds_bytes = per_cw * sizeof(float) * (size_t)L.cpb + (((size_t)5 * L.cpb + 1 + 3) & ~(size_t)3) * sizeof(int);
    if (lds_bytes > FGNN_LDS_BUDGET)
        return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident BP4-GD kernel: " + std::to_string(lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    a.d_off = (int)d_off;
    a.f_off = (int)f_off;
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
