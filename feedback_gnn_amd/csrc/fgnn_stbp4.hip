// fgnn_stbp4.hip — space-time BP4: a window of R repeated, noisy syndrome measurements decoded in one launch (the phenomenological
// noise model), flooding schedule, LDS-resident, with the attempt list of AMBP4 kept.  Over R rounds the differences of consecutive
// syndromes satisfy d_t = s_t ^ s_{t-1} = H e_t ^ u_t ^ u_{t-1}: R copies of the code's two Tanner graphs, coupled only by binary
// "time" variables u_{c,t} between check c of round t and check c of round t + 1; the time variable of the last round has degree one,
// which is soft-syndrome BP4's extra input, so R = 1 is fgnn_dsbp4_decode bit for bit.  The algorithm is stated to the float operation
// at fgnn_stbp4_decode in include/fgnn.h.  The kernel is a sibling of dsbp4_kernel (fgnn_dsbp4.hip) on the frame of the step-loop
// decoders (fgnn_step.h): the parity of a check's row, the stats words; its attempt walk, `tab` table and the qubit phase of a round's
// qubit are the ones mbp4_kernel and dsbp4_kernel run (fgnn_attempts.h, fgnn_step.h).  Its own are the window, the time variables and
// the check rule with one or two time-like inputs (fgnn_cn.h, NX = 1 and 2).  Instantiations and dispatch as dsbp4_kernel: the runtime-degree loop
// for each check rule, and min-sum on the packed rows of a (3,3,6)-regular graph, whose BYTE offsets are taken from the round's area.
//
// LDS of one window, in floats, each area rounded up to 4 floats:
//   msg  R x [E_x + E_z]   c->v / v->c messages of round t at msg + t * area, bp4_kernel's slot layout
//   b    [R m]             b(c,t) at t m + c: between check (c,t) and time variable (c,t)
//   a    [(R-1) m]         a(c,t) at (t-1) m + c, t >= 1: between check (c,t) and time variable (c,t-1)
//   dec  [R n] bytes       decisions d_v = x_v | z_v << 1 of the last test, round t at t n
//   uh   [R m] bytes       u_hat of the last test, round t at t m
// and per workgroup tab[128], stamp[cpb] and ndone as in mbp4_kernel.  An a or b slot holds the check's output after the check phase
// and the time variable's message after the qubit phase, as the edge slots do.
//
// Who touches what.  Time variable (c,t) is worked by the lane of flat index t m + c in the qubit phase: it is the only reader and
// writer of b(c,t) and a(c,t+1) there, and the only writer of uh(c,t).  Check (c,t) is worked by the lane of the same flat index in
// the check phase: it is the only one touching a(c,t) and b(c,t) there, and it reads uh(c,t), uh(c,t-1) and the decisions, which
// nobody writes in that phase.  So the two barriers per step of dsbp4_kernel suffice.  u_hat is formed in the qubit phase together
// with the decisions and is not overwritten before the control section writes it out: one bit per byte, where dsbp4_kernel needs two.
//
// gamma is loop-invariant and read again from global memory by the time variable's lane in every qubit phase, as dsbp4_kernel reads
// it again in every check update ("Soft syndromes", measured the alternative).  The syndrome differences are
// formed once, while the bits are staged: bit i of a register is d of the lane's i-th check where a lane has 32 checks at the most.
//
// A step of an attempt with T check updates, k = 0 .. T counting the finished ones:
//   qubits   as mbp4_kernel on every round; time variables: u_hat = Gamma < 0 (k > 0), messages a and b (k < T)
//   barrier
//   checks   k > 0: parity of the round's decisions against d ^ u_hat_t ^ u_hat_{t-1} (stamp);  k < T: check update * factor[r]
//   barrier
//   control  solved / out of attempts: outputs, done;  k = T: the next attempt
// No float atomics; no result depends on the order in which threads arrive, nor on the launch geometry.
//
// Soft outputs.  fgnn_stbp4_decode_soft launches the same kernel with the compile-time flag SOFT: where a window's outputs are
// written, the totals of its qubits and the Gamma of its time variables are formed again from the LDS (st_soft_out below says why
// that is exact for an unsolved window) and written next to them; no LDS is added and the plain instantiations keep their code.
//
// Registers.  Compiled for FGNN_STBP4_WAVES waves per SIMD, the most at which no instantiation needs scratch (DESIGN.md section 4,
// "Repeated measurements" and "Window post-processing", lists what each instantiation takes).
#include <cmath>

#include "fgnn_step.h"
#include "fgnn_cn.h"

#ifndef FGNN_STBP4_WAVES
#define FGNN_STBP4_WAVES 6  // waves per SIMD the register allocation aims at
#endif

namespace {

struct StArgs : AttemptArgs {  // synd_x [B,R,m_x], synd_z [B,R,m_z], x_hat and z_hat [B,R,n]
    int rounds;
    int area, b_off, a_off, u_off;  // floats: a round's message area; the b, a and uh areas from the window's start (dec: d_off)
    float gamma_x, gamma_z, gamma_last_x, gamma_last_z;
    const float* synd_llr_x;  // [B,R,m_x] or null
    const float* synd_llr_z;  // [B,R,m_z] or null
    const uint8_t* prev_x;    // [B,m_x] or null
    const uint8_t* prev_z;    // [B,m_z] or null
    uint8_t* u_x_hat;         // [B,R,m_x]
    uint8_t* u_z_hat;         // [B,R,m_z]
};

// fgnn_stbp4_decode_soft: StArgs and the three soft outputs.  A struct of its own, so that the plain instantiations keep their
// kernel arguments and with them their code
struct StSoftArgs : StArgs {
    float* marg;   // [B,R,3,n]
    float* gam_x;  // [B,R,m_x]
    float* gam_z;  // [B,R,m_z]
};

// What the lanes read of the arguments beside the frame's, copied out once by value: a select between a field of the argument struct
// and anything else may be formed as a select between two addresses, and the whole struct then lives in scratch.
struct StIn {
    const uint8_t *sx, *sz, *px, *pz;
    const float *glx, *glz;
    float gx, gz, gxl, gzl;
    int R;
    __device__ __forceinline__ StIn(const StArgs& a)
        : sx(a.synd_x), sz(a.synd_z), px(a.prev_x), pz(a.prev_z), glx(a.synd_llr_x), glz(a.synd_llr_z), gx(a.gamma_x), gz(a.gamma_z),
          gxl(a.gamma_last_x), gzl(a.gamma_last_z), R(a.rounds)
    {
    }
};

// d_{c,t} of window `row`: s_{c,t} ^ s_{c,t-1}, with s_{c,-1} = prev_c; a null array is all zero
__device__ __forceinline__ unsigned st_diff(const GraphDev& g, const StIn& in, const size_t row, const int t, const int c)
{
    const bool is_x = c < g.m_x;
    const uint8_t* s = is_x ? in.sx : in.sz;
    const uint8_t* pv = is_x ? in.px : in.pz;
    const size_t ms = (size_t)(is_x ? g.m_x : g.m_z), cs = (size_t)(is_x ? c : c - g.m_x);
    const unsigned cur = s ? (s[(row * in.R + t) * ms + cs] & 1u) : 0u;
    unsigned before;
    if (t > 0) before = s ? (s[(row * in.R + (t - 1)) * ms + cs] & 1u) : 0u;
    else before = pv ? (pv[row * ms + cs] & 1u) : 0u;
    return cur ^ before;
}

// the differences of a lane's checks j = lane, lane + tpc, .. of the flat (t,c) space: bit i of a register where a lane has 32
// checks at the most, else formed again from the rows
struct StSynd {
    bool in_reg;
    unsigned bits;
    __device__ __forceinline__ StSynd(const GraphDev& g, const StIn& in, const StepCw& cw, const size_t row, const int tpc)
    {
        const int NC = in.R * g.m;
        in_reg = (NC + tpc - 1) / tpc <= 32;
        bits = 0;
        if (cw.active && in_reg) {
            int i = 0;
            for (int j = cw.lane, c = cw.lane, t = 0; j < NC; j += tpc, c += tpc, ++i) {
                while (c >= g.m) { c -= g.m; ++t; }
                bits |= st_diff(g, in, row, t, c) << i;
            }
        }
    }
    __device__ __forceinline__ unsigned at(const GraphDev& g, const StIn& in, const size_t row, const int i, const int t, const int c) const
    {
        return in_reg ? ((bits >> i) & 1u) : st_diff(g, in, row, t, c);
    }
};

// gamma_{c,t} of window `row`: the side's array, or its scalar (the last round has its own)
__device__ __forceinline__ float st_gamma(const GraphDev& g, const StIn& in, const size_t row, const int t, const int c)
{
    const bool is_x = c < g.m_x;
    const float* gl = is_x ? in.glx : in.glz;
    if (gl) return gl[(row * in.R + t) * (size_t)(is_x ? g.m_x : g.m_z) + (size_t)(is_x ? c : c - g.m_x)];
    const bool last = t == in.R - 1;
    return is_x ? (last ? in.gxl : in.gx) : (last ? in.gzl : in.gz);
}

// The soft outputs of a finished window, from its LDS (SOFT instantiations, control section).  An unsolved window ends at k = T of its
// last attempt: that step's qubit phase sent no messages (attempt_qubit returns after the decision, the time variables `continue`
// before they write a / b) and its check phase made no update, so the edge slots still hold the c->v messages of update T and the
// b / a slots w_dn / w_up.  The totals and Gamma are formed again from them, by the routines and in the order of the qubit phase:
// the values the decisions and u_hat of the last test were taken from.  A window solved at k < T has had its slots overwritten by
// update k + 1: the rows of every solved window are +0.0f
template <int DV>
__device__ __forceinline__ void st_soft_out(const GraphDev& g, const StSoftArgs& a, const StIn& in, float* win, const float* bsl,
                                            const float* asl, const float* lch, const float llr_const, const size_t row, const int lane,
                                            const bool unsolved)
{
    const int n = g.n, m = g.m, R = a.rounds, NQ = R * n, NC = R * m;
    float* const marg = a.marg;
    float* const gam_x = a.gam_x;
    float* const gam_z = a.gam_z;
    // the four scalar gammas as values the compiler takes for new here: left to it, the selects among them in this second place
    // that reads them become an indexed read of a four-float table in scratch
    float gx = in.gx, gz = in.gz, gxl = in.gxl, gzl = in.gzl;
    asm volatile("" : "+s"(gx), "+s"(gz), "+s"(gxl), "+s"(gzl));
    for (int i = lane, v = lane, t = 0; i < NQ; i += a.tpc, v += a.tpc) {
        while (v >= n) { v -= n; ++t; }
        float X = 0.0f, Y = 0.0f, Z = 0.0f;
        if (unsolved) {
            const float lx = lch ? lch[v] : llr_const;
            const float ly = lch ? lch[n + v] : llr_const;
            const float lz = lch ? lch[2 * n + v] : llr_const;
            QubitSlots<DV> q(g, win + t * a.area, v);
            float Sz, Sx;
            q.fetch(Sz, Sx);
            vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
        }
        float* mg = marg + (row * R + t) * 3 * n + v;
        mg[0] = X;
        mg[n] = Y;
        mg[2 * (size_t)n] = Z;
    }
    for (int j = lane, c = lane, t = 0; j < NC; j += a.tpc, c += a.tpc) {
        while (c >= m) { c -= m; ++t; }
        float G = 0.0f;
        if (unsolved) {
            const bool is_x = c < g.m_x, last = t == R - 1;
            const float* gl = is_x ? in.glx : in.glz;  // st_gamma on the values above
            float gm = is_x ? (last ? gxl : gx) : (last ? gzl : gz);
            if (gl) gm = gl[(row * R + t) * (size_t)(is_x ? g.m_x : g.m_z) + (size_t)(is_x ? c : c - g.m_x)];
            const float s1 = gm + bsl[j];
            G = last ? s1 : s1 + asl[j];
        }
        if (c < g.m_x) gam_x[(row * R + t) * g.m_x + c] = G;
        else gam_z[(row * R + t) * g.m_z + (c - g.m_x)] = G;
    }
}

// DV/DC > 0: (DV,DV,DC)-regular graphs with the packed slot rows of g.cslot16 (min-sum); DV = DC = 0: runtime degrees, the loop.
// SOFT: fgnn_stbp4_decode_soft, the same steps, and st_soft_out where a window's outputs are written.
template <int CN_TYPE, int DV, int DC, bool SOFT = false>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_STBP4_WAVES)))
stbp4_kernel(GraphDev g, std::conditional_t<SOFT, StSoftArgs, StArgs> a)
{
    FG_LOG_TAB_SETUP();
    constexpr bool REGULAR = DV > 0;
    static_assert(!REGULAR || CN_TYPE == FGNN_CN_MINSUM, "the regular rows are compiled for min-sum");
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    float* win = lds + (size_t)cwl * a.lds_per_cw;
    float* bsl = win + a.b_off;
    float* asl = win + a.a_off;
    uint8_t* dec = reinterpret_cast<uint8_t*>(win + a.d_off);
    uint8_t* uh = reinterpret_cast<uint8_t*>(win + a.u_off);
    const int n = g.n, m = g.m, R = a.rounds, NQ = R * n, NC = R * m;
    const size_t row = cw.active ? (size_t)cw.b : 0;
    const StIn in(a);
    const float llr_const = a.llr_const;  // by value: lch ? lch[v] : a.llr_const would select between two addresses
    const float* lch = a.llr_ch ? a.llr_ch + row * 3 * n : nullptr;

    const AttemptLds w = attempt_stage(lds, a);
    if (cw.active) {
        for (int e = lane; e < a.d_off; e += a.tpc) win[e] = 0.0f;  // the messages of every round, b and a
        for (int i = lane; i < NQ; i += a.tpc) dec[i] = 0;
        for (int j = lane; j < NC; j += a.tpc) uh[j] = 0;
    }
    const StSynd synd(g, in, cw, row, a.tpc);
    __syncthreads();

    AttemptCtl ctl(cw.active);
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.sched), k = ctl.k;
        // ---- qubits of every round, then the time variables: marginals after k check updates, their decisions, messages to the checks ----
        if (!ctl.done) {
            const bool zero = ctl.zero(a.sched);
            const float ow = w.tab[ATTEMPT_MAX + ctl.r];
            for (int i = lane, v = lane, t = 0; i < NQ; i += a.tpc, v += a.tpc) {
                while (v >= n) { v -= n; ++t; }
                const float lx = lch ? lch[v] : llr_const;
                const float ly = lch ? lch[n + v] : llr_const;
                const float lz = lch ? lch[2 * n + v] : llr_const;
                attempt_qubit<DV>(g, win + t * a.area, v, lx, ly, lz, k, T, zero, ow, dec + i);
            }
            for (int j = lane, c = lane, t = 0; j < NC; j += a.tpc, c += a.tpc) {
                while (c >= m) { c -= m; ++t; }
                const float gm = st_gamma(g, in, row, t, c);
                const bool inner = t < R - 1;  // j < (R-1) m: a(c,t+1) is asl[j]
                const float w_dn = zero ? 0.0f : bsl[j];
                const float w_up = (inner && !zero) ? asl[j] : 0.0f;
                const float s1 = gm + w_dn;
                if (k > 0) {
                    const float G = inner ? s1 + w_up : s1;
                    uh[j] = (uint8_t)(G < 0.0f ? 1 : 0);
                    if (k == T) continue;
                }
                if (inner) {
                    asl[j] = s1;
                    bsl[j] = gm + w_up;
                } else {
                    bsl[j] = gm;
                }
            }
        }
        __syncthreads();
        if (*w.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        // ---- checks of both graphs in every round: parity of the decisions against d ^ u_hat_t ^ u_hat_{t-1} (k > 0), update (k < T) ----
        if (!ctl.done) {
            const float fac = w.tab[ctl.r];
            int idx = 0;
            for (int j = lane, c = lane, t = 0; j < NC; j += a.tpc, c += a.tpc, ++idx) {
                while (c >= m) { c -= m; ++t; }
                const unsigned sy = synd.at(g, in, row, idx, t, c);
                unsigned par = sy;  // against d ^ u_hat_t ^ u_hat_{t-1}
                if (k > 0) {
                    par ^= (unsigned)uh[j];
                    if (t > 0) par ^= (unsigned)uh[j - m];
                }
                float* msg = win + t * a.area;
                if constexpr (REGULAR) {
                    unsigned off[DC];
                    row_unpack(g, c, off);
                    if (k > 0 && parity_regular<DV>(g, dec + t * n, off, c < g.m_x, par) != 0u) w.stamp[cwl] = step;
                    if (k < T) {
                        if (t == 0) {
                            float x[1] = {bsl[j]};
                            cn_minsum_regular<DC, 1>(msg, off, DC, sy, fac, x);
                            bsl[j] = x[0];
                        } else {
                            float x[2] = {asl[j - m], bsl[j]};
                            cn_minsum_regular<DC, 2>(msg, off, DC, sy, fac, x);
                            asl[j - m] = x[0];
                            bsl[j] = x[1];
                        }
                    }
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0 && parity_csr(g, dec + t * n, c0, deg, c < g.m_x, par) != 0u) w.stamp[cwl] = step;
                    if (k < T) {
                        if (t == 0) {
                            float x[1] = {bsl[j]};
                            cn_update<CN_TYPE, PhiBp4, 1>(msg, g.cslot + c0, deg, sy, fac, x);
                            bsl[j] = x[0];
                        } else {
                            float x[2] = {asl[j - m], bsl[j]};
                            cn_update<CN_TYPE, PhiBp4, 2>(msg, g.cslot + c0, deg, sy, fac, x);
                            asl[j - m] = x[0];
                            bsl[j] = x[1];
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- per window: solution found, attempt over, decoder finished ----
        if (!ctl.done) {
            if (k == 0) {
                ctl.more();  // an attempt's first step tests nothing
            } else {
                const bool sat = w.stamp[cwl] != step;
                if (sat || ctl.last(a.sched, T)) {
                    step_write_decisions(a, dec, row, NQ, lane);  // the window's R rows of n as one row of R n
                    for (int j = lane, c = lane, t = 0; j < NC; j += a.tpc, c += a.tpc) {
                        while (c >= m) { c -= m; ++t; }
                        if (c < g.m_x) a.u_x_hat[(row * R + t) * g.m_x + c] = uh[j];
                        else a.u_z_hat[(row * R + t) * g.m_z + (c - g.m_x)] = uh[j];
                    }
                    if constexpr (SOFT) st_soft_out<DV>(g, a, in, win, bsl, asl, lch, llr_const, row, lane, !sat);
                    if (lane == 0) step_finish(a, row, sat, ctl.r, ctl.its, k, w.ndone);
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

// the floats of one window of R rounds, and the offsets of its areas
struct StLayout {
    size_t area, b_off, a_off, d_off, u_off, per_win;
    StLayout(const GraphDev& d, int R)
    {
        area = lds_round4(d.E);
        b_off = area * R;
        a_off = b_off + lds_round4((size_t)R * d.m);
        d_off = a_off + lds_round4((size_t)(R - 1) * d.m);
        u_off = d_off + lds_bytes_as_floats((size_t)R * d.n);
        per_win = u_off + lds_bytes_as_floats((size_t)R * d.m);
    }
};

// per window: the layout above; per workgroup: the two 64-float tables, a stamp per window and ndone
size_t st_lds_bytes(const GraphDev& d, int R, int cpb)
{
    return StLayout(d, R).per_win * sizeof(float) * (size_t)cpb + 2 * ATTEMPT_MAX * sizeof(float) + lds_round4((size_t)cpb + 1) * sizeof(int);
}

// The launch of a window: R n qubits and R m checks per "codeword".  A caller's fgnn_graph_set_launch is taken as it is; else the
// plan of a codeword (fgnn_graph.hip, default_launch) on the window's nodes: a thread per four nodes in groups of four waves up to a
// full workgroup, small windows share a workgroup while they fit the LDS, and a batch below one window per CU gets a thread per node.
LaunchGeom st_geom(const fgnn_graph* g, int B, int R)
{
    LaunchGeom L;
    if (g->user_launch) {
        L.tpc = g->tpc;
        L.cpb = g->cpb;
    } else {
        const long long nodes = (long long)R * std::max(g->d.n, g->d.m);
        L.cpb = 1;
        if (nodes >= 256) {
            L.tpc = (int)std::min<long long>(1024, (nodes + 1023) / 1024 * 256);
        } else if (nodes >= 64) {
            L.tpc = (int)((nodes + 63) / 64 * 64);
        } else {
            int p2 = 1;
            while (p2 < nodes) p2 <<= 1;
            L.tpc = p2;
            L.cpb = 256 / p2;
            while (L.cpb > 1 && st_lds_bytes(g->d, R, L.cpb) > FGNN_LDS_BUDGET) L.cpb >>= 1;
        }
        if (L.cpb == 1 && B <= 256) L.tpc = (int)std::min<long long>(1024, std::max<long long>(L.tpc, (nodes + 63) / 64 * 64));
    }
    L.threads = L.tpc * L.cpb;
    L.blocks = (B + L.cpb - 1) / L.cpb;
    return L;
}

// fgnn_stbp4_decode and fgnn_stbp4_decode_soft: one set of checks and one launch; soft: the three soft arrays are asked for
int st_decode(const bool soft, const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
              int attempt_iter, int restart, int rounds, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z,
              const uint8_t* prev_x, const uint8_t* prev_z, const float* synd_llr_x, float gamma_x, float gamma_last_x,
              const float* synd_llr_z, float gamma_z, float gamma_last_z, int B, uint8_t* x_hat, uint8_t* z_hat, uint8_t* u_x_hat,
              uint8_t* u_z_hat, int32_t* stats, float* marg, float* gam_x, float* gam_z, void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (int err = attempt_check_sched(num_attempts, pre_iter, attempt_iter, restart)) return err;
    if (rounds < 1) return fgnn_fail(FGNN_ERR_ARG, "rounds must be >= 1");
    if (int err = attempt_check_tables(num_attempts, factor, own)) return err;
    if (std::isnan(gamma_x) || std::isnan(gamma_z) || std::isnan(gamma_last_x) || std::isnan(gamma_last_z))
        return fgnn_fail(FGNN_ERR_ARG, "gamma_x, gamma_z, gamma_last_x and gamma_last_z must not be NaN");
    // the window must fit the LDS, whatever the batch: one window per workgroup is the least a launch can ask for
    const int cpb_least = g->user_launch ? g->cpb : 1;
    if (st_lds_bytes(g->d, rounds, cpb_least) > FGNN_LDS_BUDGET) {
        int fit = 0;
        while (fit < rounds && st_lds_bytes(g->d, fit + 1, cpb_least) <= FGNN_LDS_BUDGET) ++fit;
        return fgnn_fail(FGNN_ERR_ARG, "window too large for the LDS-resident space-time BP4 kernel: " + std::to_string(rounds) + " rounds need " +
                                           std::to_string(st_lds_bytes(g->d, rounds, cpb_least)) + " bytes of LDS per workgroup, the limit is " +
                                           std::to_string(FGNN_LDS_BUDGET) + "; the largest number of rounds that fits is " + std::to_string(fit));
    }
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !u_x_hat || !u_z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    if (soft && (!marg || !gam_x || !gam_z)) return fgnn_fail(FGNN_ERR_ARG, "no soft output buffer");
    FGNN_DEVICE_GUARD(g->device);
    const LaunchGeom L = st_geom(g, B, rounds);
    StSoftArgs a;
    attempt_args_fill(a, L, B, num_attempts, factor, own, pre_iter, attempt_iter, restart, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat,
                      stats);
    a.rounds = rounds;
    a.gamma_x = gamma_x;
    a.gamma_z = gamma_z;
    a.gamma_last_x = gamma_last_x;
    a.gamma_last_z = gamma_last_z;
    a.synd_llr_x = synd_llr_x;
    a.synd_llr_z = synd_llr_z;
    a.prev_x = prev_x;
    a.prev_z = prev_z;
    a.u_x_hat = u_x_hat;
    a.u_z_hat = u_z_hat;
    const StLayout lay(g->d, rounds);
    a.area = (int)lay.area;
    a.b_off = (int)lay.b_off;
    a.a_off = (int)lay.a_off;
    a.d_off = (int)lay.d_off;
    a.u_off = (int)lay.u_off;
    a.lds_per_cw = (int)lay.per_win;
    a.marg = marg;
    a.gam_x = gam_x;
    a.gam_z = gam_z;
    const size_t lds_bytes = st_lds_bytes(g->d, rounds, L.cpb);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    return step_dispatch(g, cn_type, [&](auto cn, auto dv, auto dc) {
        constexpr int CN = decltype(cn)::value, DV = decltype(dv)::value, DC = decltype(dc)::value;
        if (soft) return fgnn_launch(stbp4_kernel<CN, DV, DC, true>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
        return fgnn_launch(stbp4_kernel<CN, DV, DC, false>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, StArgs(a));
    });
}

}  // namespace

extern "C" int fgnn_stbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                                 int attempt_iter, int restart, int rounds, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                                 const uint8_t* synd_z, const uint8_t* prev_x, const uint8_t* prev_z, const float* synd_llr_x, float gamma_x,
                                 float gamma_last_x, const float* synd_llr_z, float gamma_z, float gamma_last_z, int B, uint8_t* x_hat,
                                 uint8_t* z_hat, uint8_t* u_x_hat, uint8_t* u_z_hat, int32_t* stats, void* stream)
{
    return st_decode(false, g, cn_type, num_attempts, factor, own, pre_iter, attempt_iter, restart, rounds, llr_ch, llr_const, synd_x, synd_z,
                     prev_x, prev_z, synd_llr_x, gamma_x, gamma_last_x, synd_llr_z, gamma_z, gamma_last_z, B, x_hat, z_hat, u_x_hat, u_z_hat,
                     stats, nullptr, nullptr, nullptr, stream);
}

extern "C" int fgnn_stbp4_decode_soft(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                                      int attempt_iter, int restart, int rounds, const float* llr_ch, float llr_const,
                                      const uint8_t* synd_x, const uint8_t* synd_z, const uint8_t* prev_x, const uint8_t* prev_z,
                                      const float* synd_llr_x, float gamma_x, float gamma_last_x, const float* synd_llr_z, float gamma_z,
                                      float gamma_last_z, int B, uint8_t* x_hat, uint8_t* z_hat, uint8_t* u_x_hat, uint8_t* u_z_hat,
                                      int32_t* stats, float* marg, float* gam_x, float* gam_z, void* stream)
{
    return st_decode(true, g, cn_type, num_attempts, factor, own, pre_iter, attempt_iter, restart, rounds, llr_ch, llr_const, synd_x, synd_z,
                     prev_x, prev_z, synd_llr_x, gamma_x, gamma_last_x, synd_llr_z, gamma_z, gamma_last_z, B, x_hat, z_hat, u_x_hat, u_z_hat,
                     stats, marg, gam_x, gam_z, stream);
}
