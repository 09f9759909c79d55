// fgnn_bp4gd.hip — BP4 with guided decimation (BP4-GD), LDS-resident: when BP4 has run its iterations without a solution, the most
// reliable undecided qubit is fixed to its current decision and BP4 goes on from the messages it has.
//
// Yao, Abu Laban, Haeger, Amat, Pfister, "Belief propagation decoding of quantum LDPC codes with guided decimation" (2023), quaternary
// variant, in the form include/fgnn.h states at fgnn_bp4gd_decode.  The qubit update is the literal form of fgnn_vn.h (one log-sum-exp
// per edge, fgnn_math.h) with the decimated LLRs lamhat in place of the channel LLRs, the check update is the shared rule of fgnn_cn.h.
// The kernel stands on the frame of the step-loop decoders (fgnn_step.h): codeword rows, staged syndrome bits, a qubit's slots, a
// check's row and parity, the output write; its own are the round walk below, the `fix` bytes and the bids.  No saturation shortcuts,
// no register-resident channel LLRs, no hardware transcendentals: the channel LLRs are re-read from global memory (L2) by the thread
// that owns the qubit and overridden where the qubit is fixed; every float operation is the one bp4_kernel and cn_update execute, in
// their order.
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
#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_BP4GD_WAVES
#define FGNN_BP4GD_WAVES 6  // waves per SIMD the register allocation aims at: the most at which no instantiation needs scratch
#endif

namespace {

struct GdArgs : StepArgs {
    int pre_iter, round_iter, rounds, f_off;
    float factor, decim;
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
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepRows rows(g, a, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    uint8_t* fix = reinterpret_cast<uint8_t*>(msg + a.f_off);
    unsigned long long* key = reinterpret_cast<unsigned long long*>(lds + (size_t)a.cpb * a.lds_per_cw);  // 16-byte aligned
    int* stamp = reinterpret_cast<int*>(key + 2 * a.cpb);
    int* ndone = stamp + a.cpb;
    const int n = g.n, m = g.m;

    for (int i = threadIdx.x; i < 5 * a.cpb + 1; i += blockDim.x) stamp[i - 4 * a.cpb] = 0;  // key words, stamp, ndone
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) {
            dec[v] = 0;
            fix[v] = 0;
        }
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    int r = 0, k = 0, its = 0;
    bool done = !cw.active;
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
                    rows.llrs(n, v, a.llr_const, lx, ly, lz);
                }
                QubitSlots<DV> q(g, msg, v);
                float Sz, Sx;
                q.fetch(Sz, Sx);
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
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0 && parity_regular<DV>(g, dec, off, is_x, sy)) stamp[cwl] = step;
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0 && parity_csr(g, dec, c0, deg, is_x, sy)) stamp[cwl] = step;
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
                    step_write_decisions(a, dec, rows.bb, n, lane);
                    if (lane == 0) step_finish(a, (size_t)cw.b, sat, r, its, k, ndone);
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

}  // namespace

extern "C" int fgnn_bp4gd_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int round_iter, int max_rounds,
                                 float decim_llr, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B,
                                 uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (pre_iter < 1 || round_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and round_iter must be >= 1");
    if (max_rounds < 0) return fgnn_fail(FGNN_ERR_ARG, "max_rounds must be >= 0");
    if (!(decim_llr > 0.0f)) return fgnn_fail(FGNN_ERR_ARG, "decim_llr must be > 0");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    GdArgs a;
    a.rounds = std::min(max_rounds, g->d.n);
    step_args_fill(a, L, B, pre_iter, a.rounds, round_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.pre_iter = pre_iter;
    a.round_iter = round_iter;
    a.factor = normalization_factor;
    a.decim = decim_llr;
    // per codeword: E messages, n decision bytes and n fix bytes; per workgroup: two 64-bit keys and a stamp per codeword, ndone
    const size_t d_off = lds_round4(g->d.E), f_off = d_off + lds_bytes_as_floats(g->d.n);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "BP4-GD", f_off + lds_bytes_as_floats(g->d.n), 0, 5 * L.cpb + 1, &lds_bytes)) return err;
    a.d_off = (int)d_off;
    a.f_off = (int)f_off;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(bp4gd_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
