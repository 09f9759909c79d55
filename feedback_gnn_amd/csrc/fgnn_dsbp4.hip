// fgnn_dsbp4.hip — soft-syndrome BP4 (Kuo, Chern, Lai, "Decoding of quantum data-syndrome codes via belief propagation", 2021;
// Raveendran et al., "Soft syndrome decoding of quantum LDPC codes for joint correction of data and syndrome errors", 2022), flooding
// schedule, LDS-resident, with the attempt list of AMBP4 kept.  Check c carries a syndrome LLR gamma_c: the error u_c of its measured
// bit is a degree-one variable on the check, so it is one more constant input of the check rule (fgnn_cn.h, NX = 1), held in a register,
// and the decoder returns u_hat next to the data error.  A sample is solved when H e_hat == s ^ u_hat on both graphs.  The algorithm is
// stated to the float operation at fgnn_dsbp4_decode in include/fgnn.h.  The kernel stands on the frame of the step-loop decoders
// (fgnn_step.h): staged syndrome bits, a qubit's slots, a check's row and parity (started from s ^ u_hat), the output write; its
// attempt walk, `tab` table and qubit phase are mbp4_kernel's and stbp4_kernel's too (fgnn_attempts.h, fgnn_step.h).  Its own are the
// `uh` bytes, the soft check rule and its input addressing (DsRows; bp4gd, bp4fb, mbp4 and relay4 use StepRows, stbp4 its StIn).
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   msg  [E_x + E_z]  c->v / v->c messages, bp4_kernel's layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last test
//   uh   [m] bytes    bit 0: u_hat of the last check update, bit 1: the u_hat the last test used
// and per workgroup tab[128], stamp[cpb] and ndone as in mbp4_kernel.
//
// u_hat.  A check's byte is written by the lane that updates the check, read by that same lane in the next step's parity test, and
// read by the output loop, which walks the checks with the same lane assignment; no other thread touches it.  A step that tests and
// then updates (0 < k < T) would overwrite the tested bit before the control phase can write it out, so the test moves it to bit 1.
//
// gamma_c is loop-invariant and the same lane owns check c in every step, so it stays out of LDS: the lane reads it again from global
// memory in every check update, next to the check's row, which it also reads again.  Keeping a lane's values in registers instead
// was measured on MI355X and gained nothing ("Soft syndromes"), and its registers cost a wave per SIMD.
//
// A step of an attempt with T check updates, k = 0 .. T counting the finished ones:
//   qubits   as mbp4_kernel
//   barrier
//   checks   k > 0: parity of the decisions against s ^ u_hat (stamp);  k < T: soft check update * factor[r], u_hat = gamma + w < 0
//   barrier
//   control  solved / out of attempts: outputs, done;  k = T: the next attempt
// No float atomics; no result depends on the order in which threads arrive.
//
// Registers.  Compiled for FGNN_DSBP4_WAVES waves per SIMD, the most at which no instantiation needs scratch (DESIGN.md section 4,
// "Soft syndromes", lists what each instantiation takes).
#include <cmath>

#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_DSBP4_WAVES
#define FGNN_DSBP4_WAVES 7  // waves per SIMD the register allocation aims at
#endif

namespace {

struct DsArgs : AttemptArgs {
    int u_off;
    float gamma_x, gamma_z;
    const float* synd_llr_x;  // [B,m_x] or null (gamma_x for every hx check)
    const float* synd_llr_z;  // [B,m_z] or null
    uint8_t* u_x_hat;         // [B,m_x]
    uint8_t* u_z_hat;         // [B,m_z]
};

// This kernel's form of StepRows (fgnn_step.h): the inputs are addressed as the rows of the workgroup's first codeword, the same for
// every lane, plus a 32-bit offset per lane (a workgroup's codewords fit the LDS, so cpb * 3 n is small): no per-lane pointer lives
// through the kernel, which takes 71 of the 72 VGPRs of seven waves
struct DsRows {
    const float* lch0;
    const uint8_t* sx0;
    const uint8_t* sz0;
    unsigned lo;
    int cwl;
    __device__ __forceinline__ DsRows(const GraphDev& g, const StepArgs& a, const StepCw& cw)
    {
        const size_t b0 = (size_t)blockIdx.x * a.cpb;
        lch0 = a.llr_ch ? a.llr_ch + b0 * 3 * g.n : nullptr;
        sx0 = a.synd_x ? a.synd_x + b0 * g.m_x : nullptr;
        sz0 = a.synd_z ? a.synd_z + b0 * g.m_z : nullptr;
        lo = (unsigned)(cw.cwl * 3 * g.n);
        cwl = cw.cwl;
    }
    __device__ __forceinline__ unsigned synd_of(const GraphDev& g, const int c) const
    {
        const bool is_x = c < g.m_x;
        const uint8_t* s = is_x ? sx0 : sz0;
        const unsigned o = is_x ? (unsigned)(cwl * g.m_x + c) : (unsigned)(cwl * g.m_z + (c - g.m_x));
        return s ? (s[o] & 1u) : 0u;
    }
    __device__ __forceinline__ void llrs(const int n, const int v, const float llr_const, float& lx, float& ly, float& lz) const
    {
        lx = lch0 ? lch0[lo + (unsigned)v] : llr_const;
        ly = lch0 ? lch0[lo + (unsigned)(n + v)] : llr_const;
        lz = lch0 ? lch0[lo + (unsigned)(2 * n + v)] : llr_const;
    }
};

// gamma of check c of the workgroup's codeword cwl: the side's array, or its scalar.  gx0 / gz0 are the rows of the workgroup's first
// codeword, the same for every lane, and the lane adds a 32-bit offset: no per-lane pointer lives through the qubit phase.
__device__ __forceinline__ float gamma_at(const float* gx0, const float* gz0, float gamma_x, float gamma_z, int cwl, int m_x, int m_z, int c)
{
    const bool is_x = c < m_x;
    const float* gl = is_x ? gx0 : gz0;
    const unsigned o = is_x ? (unsigned)(cwl * m_x + c) : (unsigned)(cwl * m_z + (c - m_x));
    return gl ? gl[o] : (is_x ? gamma_x : gamma_z);
}

// u_hat of a check: Gamma = gamma + w is one add
FG_FN unsigned soft_u_hat(float gamma, float w)
{
    const float G = gamma + w;
    return G < 0.0f ? 1u : 0u;
}

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
template <int CN_TYPE, int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_DSBP4_WAVES))) dsbp4_kernel(GraphDev g, DsArgs a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    static_assert(!REGULAR || CN_TYPE == FGNN_CN_MINSUM, "the regular rows are compiled for min-sum");
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const DsRows rows(g, a, cw);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    uint8_t* dec = reinterpret_cast<uint8_t*>(msg + a.d_off);
    uint8_t* uh = reinterpret_cast<uint8_t*>(msg + a.u_off);
    const int n = g.n, m = g.m;
    const size_t b0 = (size_t)blockIdx.x * a.cpb;
    const float* gx0 = a.synd_llr_x ? a.synd_llr_x + b0 * g.m_x : nullptr;
    const float* gz0 = a.synd_llr_z ? a.synd_llr_z + b0 * g.m_z : nullptr;
    const float gamma_x = a.gamma_x, gamma_z = a.gamma_z;
#define GAMMA_OF(c) gamma_at(gx0, gz0, gamma_x, gamma_z, cwl, g.m_x, g.m_z, (c))

    const AttemptLds w = attempt_stage(lds, a);
    if (cw.active) {
        for (int e = lane; e < g.E; e += a.tpc) msg[e] = 0.0f;
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
        for (int c = lane; c < m; c += a.tpc) uh[c] = 0;
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
        // ---- checks of both graphs: parity of the decisions against s ^ u_hat (k > 0), then the soft check update (k < T) ----
        if (!ctl.done) {
            const float fac = w.tab[ctl.r];
            // one check: c, its index i among the lane's checks, its syndrome LLR
            auto one_check = [&](const int c, const int i, const float gm) __attribute__((always_inline)) {
                const unsigned sy = synd.at(g, rows, i, c);
                const bool is_x = c < g.m_x;
                const unsigned ut = (unsigned)uh[c] & 1u;  // u_hat of the check update before this step: this lane wrote it
                unsigned un = ut;
                bool odd = false;
                float x[1] = {gm};  // the extra input of the check rule; w_c on return
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0) odd = parity_regular<DV>(g, dec, off, is_x, sy ^ ut) != 0u;
                    if (k < T) {
                        cn_minsum_regular<DC, 1>(msg, off, DC, sy, fac, x);
                        un = soft_u_hat(gm, x[0]);
                    }
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) odd = parity_csr(g, dec, c0, deg, is_x, sy ^ ut) != 0u;
                    if (k < T) {
                        cn_update<CN_TYPE, PhiBp4, 1>(msg, g.cslot + c0, deg, sy, fac, x);
                        un = soft_u_hat(gm, x[0]);
                    }
                }
                uh[c] = (uint8_t)(un | (ut << 1));
                if (odd) w.stamp[cwl] = step;
            };
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) one_check(c, i, k < T ? GAMMA_OF(c) : 0.0f);
        }
        __syncthreads();
        // ---- per codeword: solution found, attempt over, decoder finished ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();  // an attempt's first step tests nothing
            } else {
                const bool sat = w.stamp[cwl] != step;
                if (sat || ctl.last(a.sched, T)) {
                    // the output rows are addressed from a laundered copy of b: formed here, once per codeword, instead of living in
                    // per-lane 64-bit registers through every step
                    int bo = cw.b;
                    asm volatile("" : "+v"(bo));
                    const size_t ob = (size_t)bo;
                    step_write_decisions(a, dec, ob, n, lane);
                    for (int c = lane; c < m; c += a.tpc) {  // the lane that wrote the byte
                        const uint8_t u = (uint8_t)((uh[c] >> 1) & 1u);
                        if (c < g.m_x) a.u_x_hat[ob * g.m_x + c] = u;
                        else a.u_z_hat[ob * g.m_z + (c - g.m_x)] = u;
                    }
                    if (lane == 0) step_finish(a, ob, sat, ctl.r, ctl.its, k, w.ndone);
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

#undef GAMMA_OF

}  // namespace

extern "C" int fgnn_dsbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                                 int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                                 const uint8_t* synd_z, const float* synd_llr_x, float gamma_x, const float* synd_llr_z, float gamma_z,
                                 int B, uint8_t* x_hat, uint8_t* z_hat, uint8_t* u_x_hat, uint8_t* u_z_hat, int32_t* stats, void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (int err = attempt_check_sched(num_attempts, pre_iter, attempt_iter, restart)) return err;
    if (int err = attempt_check_tables(num_attempts, factor, own)) return err;
    if (std::isnan(gamma_x) || std::isnan(gamma_z)) return fgnn_fail(FGNN_ERR_ARG, "gamma_x and gamma_z must not be NaN");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !u_x_hat || !u_z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = fgnn_geom(g, B);
    DsArgs a;
    attempt_args_fill(a, L, B, num_attempts, factor, own, pre_iter, attempt_iter, restart, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat,
                      stats);
    a.gamma_x = gamma_x;
    a.gamma_z = gamma_z;
    a.synd_llr_x = synd_llr_x;
    a.synd_llr_z = synd_llr_z;
    a.u_x_hat = u_x_hat;
    a.u_z_hat = u_z_hat;
    // per codeword: E messages, n decision bytes and m u_hat bytes; per workgroup: the two 64-float tables, a stamp per codeword and
    // ndone
    const size_t d_off = lds_round4(g->d.E), u_off = d_off + lds_bytes_as_floats(g->d.n);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "soft-syndrome BP4", u_off + lds_bytes_as_floats(g->d.m), 2 * ATTEMPT_MAX, L.cpb + 1, &lds_bytes))
        return err;
    a.d_off = (int)d_off;
    a.u_off = (int)u_off;
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        return fgnn_launch(dsbp4_kernel<decltype(cn)::value, decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads),
                           lds_bytes, static_cast<hipStream_t>(stream), g->d, a);
    });
}
