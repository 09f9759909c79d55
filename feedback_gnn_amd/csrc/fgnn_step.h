// fgnn_step.h — the frame of the step-loop BP4 decoders: bp4gd_kernel (fgnn_bp4gd.hip), bp4fb_kernel (fgnn_bp4fb.hip), bp4aug_kernel
// (fgnn_bp4aug.hip), mbp4_kernel (fgnn_mbp4.hip), dsbp4_kernel (fgnn_dsbp4.hip), stbp4_kernel (fgnn_stbp4.hip) and relay4_kernel
// (fgnn_relay4.hip).
//
// The seven kernels keep several codewords in the LDS of a workgroup and walk each through workgroup steps of one qubit phase, one
// check phase and a control section.  What is the same in all of them has its one statement here:
//   StepCw / StepRows / StepSynd   which codeword a thread works on, the codeword's input rows, its syndrome bits staged in a register
//   QubitSlots<DV>                 a qubit's message slots: pre-clear, fetch with the sums Sz and Sx (or, for bp4aug_kernel, the sums
//                                  with duplicated checks), store through the kernel's edge rule
//   row_unpack / parity_*          a check's packed row, and the parity of the decisions over a check's qubits
//   step_write_decisions / step_finish   dec -> x_hat | z_hat, the four stats words and ndone
// and on the host StepArgs (the head of every kernel's argument struct), the LDS arithmetic, the LDS refusal and the dispatch over
// (check rule, regular 3-3-6).  Each kernel keeps its own step loop, barriers, LDS order, waves-per-SIMD value and whatever makes it
// that decoder.  bp4gd_kernel, bp4fb_kernel and bp4aug_kernel have a control section each.  mbp4_kernel, dsbp4_kernel and stbp4_kernel share
// one, the attempt schedule of fgnn_attempts.h (AttemptSched, AttemptCtl, the step bound), and with it
//   AttemptArgs, attempt_check_* / attempt_args_fill   the schedule in the argument struct, its argument checks and its fill
//   attempt_stage                  tab, stamp and ndone staged into LDS behind the codewords
//   attempt_qubit<DV>              the qubit phase of one qubit: decision after k updates, messages with own[r]
// relay4_kernel shares its control with the binary relay_kernel (fgnn_relay.hip): the leg control of fgnn_legs.h (LegSched, LegCtl),
// whose LDS words leg_stage lays out here.
// Every float operation stays where it was: the sums run hz before hx, each ascending from 0.
//
// The binary decoders on side 0 (hx), bp2_kernel (fgnn_bp2.hip), bp2_layered_kernel (fgnn_bp2_layered.hip), relay_kernel
// (fgnn_relay.hip), gdg_kernel (fgnn_gdg.hip, whose codewords are the paths of its samples) and si_kernel (fgnn_si.hip), take StepCw
// (from B, tpc, cpb), StepSynd (over the m_x checks of hx) and row_unpack from the frame, and have their own part at the end:
//   BitRows                        the llr_ch / output row and the syndrome row of a codeword, synd_of, the prior
//   BitSlots<DV>                   a bit's message slots: fetch with the ascending sum (or zeros), store x - m_j; QubitSlots' binary sibling
// and on the host bit_dispatch over (check rule, regular (3,6) / (4,8), predicated runtime degrees up to 8 / 16, loop).  The three on
// the leg control, relay_kernel, gdg_kernel and si_kernel, keep their bit phases and share
//   bit_check<DV, DC>              one check of a step: parity of the signs of P, the caller's action where it is odd, the min-sum update
//   bit_weigh / bit_sample         a lane's part of the weight of the decision in P; the codeword with the rows of a listed sample
// and on the host BitArgs (the head of their argument structs), bit_args_fill (the inputs, max_steps from the legs), bit_lds_bytes
// (geometry, offsets, LDS bytes or the refusal, through step_lds_bytes) and bit_check_list (index / nact).
#ifndef FGNN_STEP_H
#define FGNN_STEP_H

#include <algorithm>
#include <climits>
#include <cmath>
#include <initializer_list>
#include <type_traits>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"
#include "fgnn_vn.h"
#include "fgnn_attempts.h"
#include "fgnn_legs.h"

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------

// what every step-loop kernel is told; a kernel's own argument struct derives from it and is passed by value
struct StepArgs {
    int B, tpc, cpb, lds_per_cw, d_off, max_steps;  // d_off: the dec bytes of a codeword, in floats from its msg
    float llr_const;
    const float* llr_ch;     // [B,3,n] or null
    const uint8_t* synd_x;   // [B,m_x] or null (all-zero syndrome)
    const uint8_t* synd_z;   // [B,m_z] or null
    uint8_t* x_hat;          // [B,n]
    uint8_t* z_hat;          // [B,n]
    int32_t* stats;          // [B,4]
};

// the first run (round, attempt, leg) of a codeword has pre_iter check updates, `later` more have `iter`: max_steps is
// attempt_step_bound (fgnn_attempts.h)
inline void step_args_fill(StepArgs& a, const LaunchGeom& L, int B, int pre_iter, long long later, int iter, const float* llr_ch,
                           float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats)
{
    a.B = B;
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.max_steps = attempt_step_bound(pre_iter, later, iter);
    a.llr_const = llr_const;
    a.llr_ch = llr_ch;
    a.synd_x = synd_x;
    a.synd_z = synd_z;
    a.x_hat = x_hat;
    a.z_hat = z_hat;
    a.stats = stats;
}

// LDS areas are counted in floats and rounded up to 4 of them; an area of bytes is counted as the floats that hold it
inline size_t lds_round4(size_t floats) { return (floats + 3) & ~(size_t)3; }
inline size_t lds_bytes_as_floats(size_t bytes) { return lds_round4((bytes + 3) / 4); }

// the LDS of a launch: per_cw floats for each of the cpb codewords, `table_floats` floats and `words` ints per workgroup.  Sets
// a.lds_per_cw; a launch over the budget is refused under the decoder's name (Relay-BP gives none).  ARGS: StepArgs or BitArgs
template <typename ARGS>
int step_lds_bytes(ARGS& a, const char* decoder, size_t per_cw, size_t table_floats, size_t words, size_t* lds_bytes)
{
    *lds_bytes = per_cw * sizeof(float) * (size_t)a.cpb + table_floats * sizeof(float) + lds_round4(words) * sizeof(int);
    if (*lds_bytes > FGNN_LDS_BUDGET) {
        if (!decoder) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident kernel");
        return fgnn_fail(FGNN_ERR_ARG, std::string("code too large for the LDS-resident ") + decoder + " kernel: " + std::to_string(*lds_bytes) +
                                           " bytes of LDS per workgroup, the limit is " + std::to_string(FGNN_LDS_BUDGET));
    }
    a.lds_per_cw = (int)per_cw;
    return FGNN_OK;
}

// the checks every CN_TYPE decoder begins with
inline int step_check_args(const fgnn_graph* g, int cn_type, int B)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (cn_type < 0 || cn_type > 2) return fgnn_fail(FGNN_ERR_ARG, "Unknown node type.");  // decoding_q.py:107
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    return FGNN_OK;
}

// what a kernel on the attempt schedule is told; MbArgs, DsArgs and StArgs derive from it
struct AttemptArgs : StepArgs {
    AttemptSched sched;
};

// the checks of the schedule that follow step_check_args, in two parts: a decoder may test arguments of its own between the numbers
// and the tables (fgnn_stbp4_decode: rounds) and after the tables (the gammas)
inline int attempt_check_sched(int num_attempts, int pre_iter, int attempt_iter, int restart)
{
    if (num_attempts < 1 || num_attempts > ATTEMPT_MAX) return fgnn_fail(FGNN_ERR_ARG, "num_attempts must be in 1 .. 64");
    if (pre_iter < 1 || attempt_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "pre_iter and attempt_iter must be >= 1");
    if (restart != 0 && restart != 1) return fgnn_fail(FGNN_ERR_ARG, "restart must be 0 or 1");
    return FGNN_OK;
}
inline int attempt_check_tables(int num_attempts, const float* factor, const float* own)
{
    if (!factor || !own) return fgnn_fail(FGNN_ERR_ARG, "factor and own must hold num_attempts floats each");
    for (int i = 0; i < num_attempts; ++i) {
        if (!std::isfinite(factor[i]) || !(factor[i] > 0.0f)) return fgnn_fail(FGNN_ERR_ARG, "every factor must be finite and > 0");
        if (!std::isfinite(own[i]) || own[i] < 0.0f) return fgnn_fail(FGNN_ERR_ARG, "every own weight must be finite and >= 0");
    }
    return FGNN_OK;
}

// step_args_fill and the schedule of a checked call
inline void attempt_args_fill(AttemptArgs& a, const LaunchGeom& L, int B, int num_attempts, const float* factor, const float* own, int pre_iter,
                              int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                              const uint8_t* synd_z, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats)
{
    step_args_fill(a, L, B, pre_iter, num_attempts - 1, attempt_iter, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat, stats);
    a.sched.pre_iter = pre_iter;
    a.sched.attempt_iter = attempt_iter;
    a.sched.attempts = num_attempts;
    a.sched.restart = restart;
    for (int i = 0; i < ATTEMPT_MAX; ++i) {
        a.sched.tab[i] = i < num_attempts ? factor[i] : 0.0f;
        a.sched.tab[ATTEMPT_MAX + i] = i < num_attempts ? own[i] : 0.0f;
    }
}

// the graphs the (3,3,6) instantiations run: (3,3,6)-regular with packed check rows, unless the tests force the loop
inline bool step_regular_336(const fgnn_graph* g)
{
    return g->d.cslot16 && !g->force_generic && g->d.dvx == 3 && g->d.dvz == 3 && g->d.dc == 6;
}

// kernel<CN_TYPE, DV, DC> of a launch: boxplus and boxplus-phi run the loop, min-sum the (3,3,6) rows where the graph has them.
// `launch` is called with the three values as std::integral_constant arguments.
template <typename LAUNCH>
int step_dispatch(const fgnn_graph* g, int cn_type, LAUNCH launch)
{
    using std::integral_constant;
    const integral_constant<int, 0> loop;
    switch (cn_type) {
    case FGNN_CN_BOXPLUS: return launch(integral_constant<int, FGNN_CN_BOXPLUS>(), loop, loop);
    case FGNN_CN_BOXPLUS_PHI: return launch(integral_constant<int, FGNN_CN_BOXPLUS_PHI>(), loop, loop);
    default: break;
    }
    if (step_regular_336(g)) return launch(integral_constant<int, FGNN_CN_MINSUM>(), integral_constant<int, 3>(), integral_constant<int, 6>());
    return launch(integral_constant<int, FGNN_CN_MINSUM>(), loop, loop);
}

// kernel<CN_TYPE, DV, DC> of a launch of the binary decoders on side 0 (hx): boxplus-phi and min-sum run the register-resident
// check update on (3,6)- and (4,8)-regular hx with packed check rows (the GHP and GB families; cslot16 exists for check degrees up
// to 8, and the slots of side 0 come first in the combined numbering, so its byte offsets index a binary kernel's message area
// directly), unless the tests force the loop.  On other graphs min-sum runs the predicated update for runtime degrees up to 8 / 16
// where `predicated` allows it (its compare/select work is cheap, what the loop over the slot list pays for is latency: 17.7 ->
// 13.0 ms on [[882,24]], 202 -> 153 ms on the 1000-row over-complete GB matrix, per 65 536 x 64).  The phi rule stays on the loop:
// masked-out edges would still cost a phi (measured: 26.2 against 20.8 ms); so does boxplus.  `launch` as for step_dispatch
template <typename LAUNCH>
int bit_dispatch(const fgnn_graph* g, int cn_type, bool predicated, LAUNCH launch)
{
    using std::integral_constant;
    const integral_constant<int, 0> loop;
    const bool regular = g->d.cslot16 && !g->force_generic;
    const bool r36 = regular && g->d.dvx == 3 && g->d.dc == 6, r48 = regular && g->d.dvx == 4 && g->d.dc == 8;
    const bool phi = cn_type == FGNN_CN_BOXPLUS_PHI, minsum = cn_type == FGNN_CN_MINSUM;
    const integral_constant<int, FGNN_CN_BOXPLUS_PHI> PHI;
    const integral_constant<int, FGNN_CN_MINSUM> MINSUM;
    if (r36 && phi) return launch(PHI, integral_constant<int, 3>(), integral_constant<int, 6>());
    if (r36 && minsum) return launch(MINSUM, integral_constant<int, 3>(), integral_constant<int, 6>());
    if (r48 && phi) return launch(PHI, integral_constant<int, 4>(), integral_constant<int, 8>());
    if (r48 && minsum) return launch(MINSUM, integral_constant<int, 4>(), integral_constant<int, 8>());
    const int md = predicated ? g->d.max_cdeg_x : 1 << 30;
    if (minsum && md <= 8) return launch(MINSUM, loop, integral_constant<int, 8>());
    if (minsum && md <= 16) return launch(MINSUM, loop, integral_constant<int, 16>());
    if (phi) return launch(PHI, loop, loop);
    if (minsum) return launch(MINSUM, loop, loop);
    return launch(integral_constant<int, FGNN_CN_BOXPLUS>(), loop, loop);
}

// The head of what a binary decoder on the leg control is told: the codewords of the launch and what bit_lds_bytes lays out (p_off:
// the posteriors, in floats from msg).  RelayArgs, GdgArgs and SiArgs derive from it.  Required of each of them, behind the head and
// in its own order (the struct is the kernel's argument; DESIGN.md has what moving them costs): int max_steps; LegSched legs;
// float factor, llr_const; const float* llr_ch; const uint8_t* synd.  bit_args_fill writes these by name
struct BitArgs {
    int B, tpc, cpb, lds_per_cw, p_off;
};

// the inputs of a checked call, into B and the fields BitArgs requires of ARGS
template <typename ARGS>
void bit_args_fill(ARGS& a, int B, const LegSched& legs, float factor, const float* llr_ch, float llr_const, const uint8_t* synd)
{
    a.B = B;
    a.legs = legs;
    a.max_steps = attempt_step_bound(legs.pre_iter, legs.num_legs - 1, legs.leg_iter);  // the step after a codeword's last weighs its last decision
    a.factor = factor;
    a.llr_const = llr_const;
    a.llr_ch = llr_ch;
    a.synd = synd;
}

// The geometry and the LDS of a launch.  Per codeword: E_x messages, n posteriors at a.p_off, then the decoder's own areas of so many
// bytes, whose offsets are written through `off`, each area rounded up to 4 floats; per workgroup: words64 64-bit words per codeword
// (keys, residuals: 16-byte aligned), then the words of the leg control, which leg_stage finds at lds + 2 * words64 * cpb
struct BitArea {
    size_t bytes;
    int* off;
};
inline int bit_lds_bytes(BitArgs& a, const fgnn_graph* g, const LaunchGeom& L, const char* decoder, std::initializer_list<BitArea> behind_p,
                         size_t words64, size_t* lds_bytes)
{
    a.tpc = L.tpc;
    a.cpb = L.cpb;
    a.p_off = (int)lds_round4(g->d.E_x);
    size_t per_cw = a.p_off + lds_round4(g->d.n);
    for (const BitArea& area : behind_p) {
        *area.off = (int)per_cw;
        per_cw += lds_bytes_as_floats(area.bytes);
    }
    return step_lds_bytes(a, decoder, per_cw, 2 * words64 * (size_t)L.cpb, leg_lds_words(L.cpb), lds_bytes);
}

// the sample list of a call: nact of the B samples, or without a list all of them
inline int bit_check_list(const int32_t* index, int B, int& nact)
{
    if (index && (nact < 0 || nact > B)) return fgnn_fail(FGNN_ERR_ARG, "nact must be in 0 .. B");
    if (!index) nact = B;
    return FGNN_OK;
}

// ---------------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------------

// the codeword of a thread: cwl-th of the workgroup, b-th of the batch (active iff b < B), lane of its tpc threads; nact = the
// workgroup's active codewords
struct StepCw {
    int cwl, lane, b, nact;
    bool active;
    __device__ __forceinline__ StepCw(const int B, const int tpc, const int cpb)
    {
        cwl = threadIdx.x / tpc;
        lane = threadIdx.x - cwl * tpc;
        b = blockIdx.x * cpb + cwl;
        active = b < B;
        nact = min(cpb, B - (int)blockIdx.x * cpb);
    }
    __device__ __forceinline__ StepCw(const StepArgs& a) : StepCw(a.B, a.tpc, a.cpb) {}
};

// the input rows of a thread's codeword (row 0 for an inactive one, which reads nothing), one pointer each
struct StepRows {
    size_t bb;
    const float* lch;
    const uint8_t* sx;
    const uint8_t* sz;
    __device__ __forceinline__ StepRows(const GraphDev& g, const StepArgs& a, const StepCw& cw)
    {
        bb = cw.active ? (size_t)cw.b : 0;
        lch = a.llr_ch ? a.llr_ch + bb * 3 * g.n : nullptr;
        sx = a.synd_x ? a.synd_x + bb * g.m_x : nullptr;
        sz = a.synd_z ? a.synd_z + bb * g.m_z : nullptr;
    }
    // syndrome bit of combined check c (hx rows first)
    __device__ __forceinline__ unsigned synd_of(const GraphDev& g, const int c) const
    {
        const uint8_t* s = c < g.m_x ? sx : sz;
        return s ? (s[c < g.m_x ? c : c - g.m_x] & 1u) : 0u;
    }
    // channel LLRs of qubit v, order X, Y, Z
    __device__ __forceinline__ void llrs(const int n, const int v, const float llr_const, float& lx, float& ly, float& lz) const
    {
        lx = lch ? lch[v] : llr_const;
        ly = lch ? lch[n + v] : llr_const;
        lz = lch ? lch[2 * n + v] : llr_const;
    }
};

// the syndrome bits of a lane's checks c = lane, lane + tpc, ..: bit i of a register where a lane has 32 checks at the most, else
// read again from the rows.  ROWS: StepRows, or a kernel's own rows with the same synd_of; m: the checks of the codeword, g.m
// unless the kernel says otherwise (the binary decoders: g.m_x).  any = false: the syndrome is null, that is all-zero; no bit is
// staged and none is asked of the rows (the binary decoders again; StepRows answers 0 for a null side by itself)
struct StepSynd {
    bool any, in_reg;
    unsigned bits;
    template <typename ROWS>
    __device__ __forceinline__ StepSynd(const GraphDev& g, const ROWS& rows, const StepCw& cw, const int tpc, const int m, const bool any_ = true)
        : any(any_)
    {
        in_reg = (m + tpc - 1) / tpc <= 32;
        bits = 0;
        if (cw.active && any && in_reg) {
            int i = 0;
            for (int c = cw.lane; c < m; c += tpc, ++i) bits |= rows.synd_of(g, c) << i;
        }
    }
    template <typename ROWS>
    __device__ __forceinline__ StepSynd(const GraphDev& g, const ROWS& rows, const StepCw& cw, const int tpc) : StepSynd(g, rows, cw, tpc, g.m)
    {
    }
    // of the lane's i-th check, which is c
    template <typename ROWS>
    __device__ __forceinline__ unsigned at(const GraphDev& g, const ROWS& rows, const int i, const int c) const
    {
        return !any ? 0u : in_reg ? ((bits >> i) & 1u) : rows.synd_of(g, c);
    }
};

// The message slots of qubit v in the codeword's msg: the hx run [x0, x1) at px, the hz run [z0, z1) at pz.  DV > 0: a
// (DV,DV,.)-regular graph, the messages are fetched into registers once; DV = 0: runtime degrees, they are read where they are used.
// Only the fetch and the store differ between the two.  The runs are kept by their ends, as vn_sums takes them, and the two pointers
// are formed once: with degrees kept instead, or the pointers formed again in the store, bp4gd_kernel's boxplus-phi loop takes 75
// VGPRs instead of 72 (and relay4_kernel<3,6> took one more, measured before it moved onto the leg control of fgnn_legs.h).
template <int DV>
struct QubitSlots {
    static constexpr bool REGULAR = DV > 0;
    float* msg;
    float* px;
    float* pz;
    int x0, z0, x1, z1;
    float mx[REGULAR ? DV : 1], mz[REGULAR ? DV : 1];

    __device__ __forceinline__ QubitSlots(const GraphDev& g, float* msg_, const int v) : msg(msg_)
    {
        x0 = REGULAR ? v * DV : g.vptr_x[v];
        z0 = REGULAR ? g.E_x + v * DV : g.vptr_z[v];
        x1 = REGULAR ? x0 + DV : g.vptr_x[v + 1];
        z1 = REGULAR ? z0 + DV : g.vptr_z[v + 1];
        px = msg + x0;
        pz = msg + z0;
    }
    // a restarting attempt starts from zero messages: the slots of a qubit are its owner's in the qubit phase
    __device__ __forceinline__ void clear()
    {
        const int dx = x1 - x0, dz = z1 - z0;
        for (int j = 0; j < dx; ++j) px[j] = 0.0f;
        for (int j = 0; j < dz; ++j) pz[j] = 0.0f;
    }
    // the qubit's c->v messages and their sums, the hz run before the hx run, each ascending.  live = false: no check update has
    // written the slots yet and the messages count as zeros, whatever the slots hold
    __device__ __forceinline__ void fetch(float& Sz, float& Sx, const bool live = true)
    {
        Sz = 0.0f;
        Sx = 0.0f;
        if constexpr (REGULAR) {
            if (live) {
#pragma unroll
                for (int j = 0; j < DV; ++j) { mz[j] = pz[j]; Sz = Sz + mz[j]; }
#pragma unroll
                for (int j = 0; j < DV; ++j) { mx[j] = px[j]; Sx = Sx + mx[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < DV; ++j) mz[j] = mx[j] = 0.0f;
            }
        } else if (live) {
            vn_sums(msg, z0, z1, x0, x1, Sz, Sx);
        }
    }
    // the fetch on the code with duplicated check rows (vn_sums_dup of fgnn_vn.h): a marked slot's message is added twice in a row.
    // DV > 0: bit j of `bits` marks hx slot j, bit DV + j hz slot j; DV = 0: dup[e] marks slot e of msg.  With no mark set the sums
    // are those of fetch(), bit for bit
    __device__ __forceinline__ void fetch_dup(float& Sz, float& Sx, const unsigned bits, const uint8_t* dup)
    {
        if constexpr (REGULAR) {
            Sz = 0.0f;
            Sx = 0.0f;
#pragma unroll
            for (int j = 0; j < DV; ++j) {
                mz[j] = pz[j];
                Sz = Sz + mz[j];
                if ((bits >> (DV + j)) & 1u) Sz = Sz + mz[j];
            }
#pragma unroll
            for (int j = 0; j < DV; ++j) {
                mx[j] = px[j];
                Sx = Sx + mx[j];
                if ((bits >> j) & 1u) Sx = Sx + mx[j];
            }
        } else {
            vn_sums_dup(msg, dup, z0, z1, x0, x1, Sz, Sx);
        }
    }
    // the v->c messages from the totals X, Y, Z: edge(num, A, Y, mu) is the kernel's edge rule (vn_edge, vn_edge_own of fgnn_vn.h),
    // mu the edge's own c->v message as fetched
    template <typename EDGE>
    __device__ __forceinline__ void store(const float X, const float Y, const float Z, EDGE edge, const bool live = true)
    {
        const float numx = VnMath::softplus(-X);
        const float numz = VnMath::softplus(-Z);
        if constexpr (REGULAR) {
#pragma unroll
            for (int j = 0; j < DV; ++j) px[j] = edge(numx, Z, Y, mx[j]);
#pragma unroll
            for (int j = 0; j < DV; ++j) pz[j] = edge(numz, X, Y, mz[j]);
        } else {
            const int dx = x1 - x0, dz = z1 - z0;
            for (int j = 0; j < dx; ++j) px[j] = edge(numx, Z, Y, live ? px[j] : 0.0f);
            for (int j = 0; j < dz; ++j) pz[j] = edge(numz, X, Y, live ? pz[j] : 0.0f);
        }
    }
};

// The per-workgroup words of a kernel on the attempt schedule, behind the cpb codewords: tab[128] = factor[0..63], own[0..63] (the
// codewords of a workgroup sit at different attempts, so the two are indexed per lane), stamp[cpb] = the number of the last
// workgroup step in which a check of the codeword saw odd parity, ndone = finished codewords.  Staged by the whole workgroup,
// before the kernel's first barrier
struct AttemptLds {
    float* tab;
    int* stamp;
    int* ndone;
};
__device__ __forceinline__ AttemptLds attempt_stage(float* lds, const AttemptArgs& a)
{
    float* tab = lds + (size_t)a.cpb * a.lds_per_cw;
    int* stamp = reinterpret_cast<int*>(tab + 2 * ATTEMPT_MAX);
    for (int i = threadIdx.x; i < 2 * ATTEMPT_MAX; i += blockDim.x) tab[i] = a.sched.tab[i];
    for (int i = threadIdx.x; i < a.cpb + 1; i += blockDim.x) stamp[i] = 0;  // stamp, ndone
    return {tab, stamp, stamp + a.cpb};
}

// The per-workgroup words of a kernel on the leg control (fgnn_legs.h), behind the cpb codewords of lds_per_cw floats each:
// stamp[cpb], wacc[cpb], ndone, leg_lds_words(cpb) ints.  Zeroed by the whole workgroup, before the kernel's first barrier
struct LegLds {
    int* stamp;
    int* wacc;
    int* ndone;
};
__device__ __forceinline__ LegLds leg_stage(float* lds, const int cpb, const int lds_per_cw)
{
    int* stamp = reinterpret_cast<int*>(lds + (size_t)cpb * lds_per_cw);
    for (int i = threadIdx.x; i < leg_lds_words(cpb); i += blockDim.x) stamp[i] = 0;
    return {stamp, stamp + cpb, stamp + 2 * cpb};
}

// The qubit phase of qubit v at step k of an attempt of T check updates, on the slots of `msg` and the channel LLRs lx, ly, lz:
// the marginals after k updates, for k > 0 the test's decision into *d, for k < T the messages to the checks with the own weight ow
// (an attempt's last test sends none); zero: a restarting attempt's first step, the owner zeroes the qubit's slots first
template <int DV>
__device__ __forceinline__ void attempt_qubit(const GraphDev& g, float* msg, const int v, const float lx, const float ly, const float lz,
                                              const int k, const int T, const bool zero, const float ow, uint8_t* d)
{
    QubitSlots<DV> q(g, msg, v);
    if (zero) q.clear();
    float Sz, Sx;
    q.fetch(Sz, Sx);
    float X, Y, Z;
    vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
    if (k > 0) {
        *d = (uint8_t)vn_decide(X, Y, Z);
        if (k == T) return;
    }
    q.store(X, Y, Z, [&](float num, float A, float Ye, float mu) { return vn_edge_own<VnMath>(num, A, Ye, mu, ow); });
}

// the BYTE offsets of check c's slots from its packed row of g.cslot16
template <int DC>
__device__ __forceinline__ void row_unpack(const GraphDev& g, const int c, unsigned (&off)[DC])
{
    const uint4 pk = reinterpret_cast<const uint4*>(g.cslot16)[c];
    const unsigned w[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
    for (int j = 0; j < DC; ++j) off[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
}

// the qubit of a slot of a (DV,DV,.)-regular graph: slot base + v * DV + j belongs to qubit v, base = 0 (hx) or E_x (hz)
template <int DV>
__device__ __forceinline__ unsigned row_qubit(const unsigned byte_off, const unsigned base)
{
    return ((byte_off >> 2) - base) / DV;
}
__device__ __forceinline__ unsigned row_base(const GraphDev& g, const bool is_x) { return is_x ? 0u : (unsigned)g.E_x; }

// parity of the decisions dec over a check's qubits, starting from `par`: hx rows test z_hat (bit 1 of the decision), hz rows x_hat
// (bit 0).  On the unpacked row of a regular graph, and on the CSR row [c0, c0 + deg) of g.cvn
template <int DV, int DC>
__device__ __forceinline__ unsigned parity_regular(const GraphDev& g, const uint8_t* dec, const unsigned (&off)[DC], const bool is_x, unsigned par)
{
    const int sh = is_x ? 1 : 0;
    const unsigned base = row_base(g, is_x);
#pragma unroll
    for (int j = 0; j < DC; ++j) par ^= ((unsigned)dec[row_qubit<DV>(off[j], base)] >> sh) & 1u;
    return par;
}
__device__ __forceinline__ unsigned parity_csr(const GraphDev& g, const uint8_t* dec, const int c0, const int deg, const bool is_x, unsigned par)
{
    const int sh = is_x ? 1 : 0;
    for (int j = 0; j < deg; ++j) par ^= ((unsigned)dec[g.cvn[c0 + j]] >> sh) & 1u;
    return par;
}

// the decisions of a codeword into row `row` of x_hat and z_hat
__device__ __forceinline__ void step_write_decisions(const StepArgs& a, const uint8_t* dec, const size_t row, const int n, const int lane)
{
    for (int v = lane; v < n; v += a.tpc) {
        const unsigned d = dec[v];
        a.x_hat[row * n + v] = (uint8_t)(d & 1u);
        a.z_hat[row * n + v] = (uint8_t)(d >> 1);
    }
}

// one thread of a finished codeword: its four stats words, and the workgroup counts it
__device__ __forceinline__ void step_finish(const StepArgs& a, const size_t row, const bool sat, const int r, const int its, const int k, int* ndone)
{
    int32_t* st = a.stats + row * 4;
    st[0] = sat ? 1 : 0;
    st[1] = r;
    st[2] = its;
    st[3] = k;
    atomicAdd(ndone, 1);
}

// ---------------------------------------------------------------------------------------------
// The binary decoders on side 0 (hx): the rows and slots of all five, then the check, weight and sample of the three on the leg control
// ---------------------------------------------------------------------------------------------

// the rows of a thread's codeword b: element v of its llr_ch and output rows is at(v), its syndrome bits are synd_of; the pointers are
// the launch's.  The products are formed where they are used, as an index and not a pointer (an inactive codeword's lie beyond the
// arrays, and it reads and writes nothing): kept as a row pointer per lane, or formed once ahead of the loops, bp2_kernel's min-sum
// instantiations measured 0.4 to 0.7 % slower
struct BitRows {
    int b, n, m;
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null
    float llr_const;
    __device__ __forceinline__ BitRows(const GraphDev& g, const float* llr_ch_, const float llr_const_, const uint8_t* synd_, const StepCw& cw)
        : b(cw.b), n(g.n), m(g.m_x), llr_ch(llr_ch_), synd(synd_), llr_const(llr_const_)
    {
    }
    __device__ __forceinline__ size_t at(const int v) const { return (size_t)b * n + v; }
    // of a syndrome that is not null: StepSynd is told of a null one (any = false) and then asks for no bit
    __device__ __forceinline__ unsigned synd_of(const GraphDev&, const int c) const { return synd[(size_t)b * m + c] & 1u; }
    // the prior of bit v: the channel logit clamped to +-20, as an LLR
    __device__ __forceinline__ float prior(const int v) const
    {
        float lc = llr_ch ? llr_ch[at(v)] : llr_const;
        lc = FG_MIN(FG_MAX(lc, -20.0f), 20.0f);
        return -1.0f * lc;
    }
};

// The message slots [e0, e1) of bit v in the codeword's msg, the binary sibling of QubitSlots: DV > 0: a (DV,.)-regular hx, the
// messages are fetched into registers once; DV = 0: runtime degrees through g.vptr_x, they are read where they are used
template <int DV>
struct BitSlots {
    static constexpr bool REGULAR = DV > 0;
    float* msg;
    int e0, e1;
    float mi[REGULAR ? DV : 1];

    __device__ __forceinline__ BitSlots(const GraphDev& g, float* msg_, const int v) : msg(msg_)
    {
        e0 = REGULAR ? v * DV : g.vptr_x[v];
        e1 = REGULAR ? e0 + DV : g.vptr_x[v + 1];
    }
    // the sum of the bit's c->v messages, ascending from 0
    __device__ __forceinline__ float fetch()
    {
        float S = 0.0f;
        if constexpr (REGULAR) {
            float* mv = msg + e0;
#pragma unroll
            for (int j = 0; j < DV; ++j) mi[j] = mv[j];
#pragma unroll
            for (int j = 0; j < DV; ++j) S = S + mi[j];
        } else {
            for (int e = e0; e < e1; ++e) S = S + msg[e];
        }
        return S;
    }
    // in place of fetch() where no check update has written the slots yet: the messages count as zeros, whatever the slots hold,
    // and their sum is 0.  The caller branches between the two (relay_kernel, on k > 0): folded into fetch(live), the regular bit
    // loop compiled to two exec regions where the branch gives one
    __device__ __forceinline__ void zeros()
    {
        if constexpr (REGULAR) {
#pragma unroll
            for (int j = 0; j < DV; ++j) mi[j] = 0.0f;
        }
    }
    // the v->c messages from the total x: x minus the edge's own c->v message, as fetched, or after zeros() as zero
    __device__ __forceinline__ void store(const float x)
    {
        if constexpr (REGULAR) {
            float* mv = msg + e0;
#pragma unroll
            for (int j = 0; j < DV; ++j) mv[j] = x - mi[j];
        } else {
            for (int e = e0; e < e1; ++e) msg[e] = x - msg[e];
        }
    }
    __device__ __forceinline__ void store_zeros(const float x)
    {
        if constexpr (REGULAR) {
            store(x);
        } else {
            for (int e = e0; e < e1; ++e) msg[e] = x - 0.0f;
        }
    }
};

// codeword cw reads and writes the rows of the pos-th listed sample, index[pos] (pos without a list): StepCw with that b.  An inactive
// codeword reads nothing, the index list included
__device__ __forceinline__ StepCw bit_sample(const StepCw& cw, const int32_t* index, const int pos)
{
    StepCw in = cw;
    in.b = cw.active ? (index ? index[pos] : pos) : 0;
    return in;
}

// One check c of a step of the leg decoders, syndrome bit sy: with `test` (k > 0) the parity of the decisions, the signs of the
// posteriors P, over the check's bits, and odd() where it is odd; with `update` (k < T) the min-sum update of the check's slots.
// DV/DC > 0: the packed row; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop
template <int DV, int DC, typename ODD>
__device__ __forceinline__ void bit_check(const GraphDev& g, float* msg, const float* P, const int c, const unsigned sy, const bool test,
                                          const bool update, const float factor, ODD odd)
{
    if constexpr (DV > 0) {
        unsigned off[DC];
        row_unpack(g, c, off);
        if (test) {
            unsigned par = sy;
#pragma unroll
            for (int j = 0; j < DC; ++j) par ^= (unsigned)(P[row_qubit<DV>(off[j], 0u)] < 0.0f);
            if (par) odd();
        }
        if (update) cn_minsum_regular<DC>(msg, off, DC, sy, factor);
    } else if constexpr (DC > 0) {
        const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
        if (test) {  // before the slot list is loaded: the two index lists are never live together
            int vn[DC];
#pragma unroll
            for (int j = 0; j < DC; ++j) vn[j] = (j < deg) ? g.cvn[c0 + j] : 0;
            unsigned par = sy;
#pragma unroll
            for (int j = 0; j < DC; ++j) par ^= (unsigned)((j < deg) && (P[vn[j]] < 0.0f));
            if (par) odd();
        }
        if (update) {
            unsigned off[DC];
#pragma unroll
            for (int j = 0; j < DC; ++j) off[j] = (j < deg) ? 4u * (unsigned)g.cslot[c0 + j] : 0u;
            cn_minsum_regular<DC>(msg, off, deg, sy, factor);
        }
    } else {
        const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
        if (test) {
            unsigned par = sy;
            for (int j = 0; j < deg; ++j) par ^= (unsigned)(P[g.cvn[c0 + j]] < 0.0f);
            if (par) odd();
        }
        if (update) cn_update<FGNN_CN_MINSUM, PhiGnn>(msg, g.cslot + c0, deg, sy, factor);
    }
}

// a lane's part of the weight of the decision in P: over its bits with P < 0, the rounded 1024-fold of the prior
__device__ __forceinline__ int bit_weigh(const float* P, const BitRows& rows, const int n, const int lane, const int tpc)
{
    int part = 0;
    for (int v = lane; v < n; v += tpc)
        if (P[v] < 0.0f) part += (int)__builtin_rintf(1024.0f * rows.prior(v));
    return part;
}

#endif
