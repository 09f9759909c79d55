// fgnn_relay.hip — Relay-BP on one Tanner graph: a chain of min-sum BP runs ("legs") with per-bit memory strengths, LDS-resident.
//
// Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories" (2025), in the form
// include/fgnn.h states at fgnn_relay_decode.  The layout is bp2_kernel's (fgnn_bp2.hip): the parity-check matrix is side 0 (hx) of an
// fgnn_graph, one workgroup holds the E_x messages of its codeword(s) in LDS, the check update is the shared min-sum rule of fgnn_cn.h.
// Added per codeword: the posteriors P[n] in LDS (the memory term reads them, the next leg starts from them, the parity test gathers
// their signs in the same sweep as the check update), and three words per codeword of convergence state.  All legs run in one
// launch; the messages never leave LDS.
//
// Codewords of one workgroup stop at different steps.  Every piece of control state (leg, step of the leg, solutions found, best
// weight) is a register every thread of a codeword holds identically; what crosses threads goes through LDS words that are written in
// one barrier interval and read in the next:
//   stamp[cw]  the number of the last workgroup step in which a check of the codeword saw odd parity (no reset needed)
//   wacc[cw]   running total of the weights of the decisions weighed so far (integer atomics; a thread keeps the previous total)
//   ndone      finished codewords; read by all threads in the same interval, so leaving the loop is a uniform decision
#include <climits>

#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_cn.h"

#ifndef FGNN_RELAY_WAVES
#define FGNN_RELAY_WAVES 6  // waves per SIMD the register allocation aims at (bp2_kernel's target)
#endif
// the predicated update for degrees up to 16 holds 16 magnitudes and signs next to the decoder's control state: it takes 95 VGPRs
// spill-free (the 80 of six waves leave 21 spilled), so it runs at one wave per SIMD fewer
#define FGNN_RELAY_WAVES_OF(DC) ((DC) >= 16 ? FGNN_RELAY_WAVES - 1 : FGNN_RELAY_WAVES)

namespace {

struct RelayArgs {
    int B, pre_iter, num_legs, leg_iter, stop_nconv, max_steps, tpc, cpb, lds_per_cw, p_off;
    float factor, llr_const;
    const float* gamma;    // [num_legs,n]
    const float* llr_ch;   // [B,n] logits or null
    const uint8_t* synd;   // [B,m_x] or null (all-zero syndrome)
    uint8_t* hard_out;     // [B,n]
    int32_t* stats;        // [B,4]
};

__device__ __forceinline__ float relay_prior(const RelayArgs& a, size_t row, int v)
{
    float lc = a.llr_ch ? a.llr_ch[row + v] : a.llr_const;
    lc = FG_MIN(FG_MAX(lc, -20.0f), 20.0f);
    return -1.0f * lc;
}

// DV/DC > 0: (DV,DC)-regular hx with the packed slot rows of g.cslot16; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_RELAY_WAVES_OF(DC)))) relay_kernel(GraphDev g, RelayArgs a)
{
    FG_LOG_TAB_SETUP();  // cn_update names the phi policy: the table every kernel of that family installs (FGNN_LDS_BUDGET leaves its 256 bytes)
    constexpr bool REGULAR = DV > 0;
    extern __shared__ float lds[];
    const int cwl = threadIdx.x / a.tpc;
    const int lane = threadIdx.x - cwl * a.tpc;
    const int b = blockIdx.x * a.cpb + cwl;
    const bool active = b < a.B;
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* P = msg + a.p_off;
    int* stamp = reinterpret_cast<int*>(lds + (size_t)a.cpb * a.lds_per_cw);
    int* wacc = stamp + a.cpb;
    int* ndone = wacc + a.cpb;
    const int n = g.n, m = g.m_x;
    const size_t row = (size_t)(active ? b : 0) * n;
    const int nact = min(a.cpb, a.B - (int)blockIdx.x * a.cpb);

    for (int i = threadIdx.x; i < 2 * a.cpb + 1; i += blockDim.x) stamp[i] = 0;
    if (active)
        for (int v = lane; v < n; v += a.tpc) P[v] = relay_prior(a, row, v);
    const bool synd_in_reg = (m + a.tpc - 1) / a.tpc <= 32;
    unsigned synd_bits = 0;
    if (active && a.synd && synd_in_reg) {
        int i = 0;
        for (int c = lane; c < m; c += a.tpc, ++i) synd_bits |= (unsigned)(a.synd[(size_t)b * m + c] & 1u) << i;
    }
    __syncthreads();

    int r = 0, k = 0, found = 0, best_w = 0, best_r = 0, best_k = 0, wprev = 0, pend_r = 0, pend_k = 0;
    bool done = !active, written = !active, pending = false;
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = (r == 0) ? a.pre_iter : a.leg_iter;
        // ---- bits: posterior after k check updates, memory term, messages to the checks ----
        if (!done) {
            const float* gam = a.gamma + (size_t)r * n;
            for (int v = lane; v < n; v += a.tpc) {
                const float L = relay_prior(a, row, v);
                const float gv = gam[v];
                const float om = 1.0f - gv;
                float Pv = P[v];
                if constexpr (REGULAR) {
                    float* mv = msg + v * DV;
                    float mi[DV];
                    float S = 0.0f;
                    if (k > 0) {
#pragma unroll
                        for (int j = 0; j < DV; ++j) mi[j] = mv[j];
#pragma unroll
                        for (int j = 0; j < DV; ++j) S = S + mi[j];
                        const float lam0 = om * L + gv * Pv;
                        Pv = lam0 + S;
                        P[v] = Pv;
                        if (k == T) continue;
                    } else {
#pragma unroll
                        for (int j = 0; j < DV; ++j) mi[j] = 0.0f;
                    }
                    const float lam = om * L + gv * Pv;
                    const float x = S + lam;
#pragma unroll
                    for (int j = 0; j < DV; ++j) mv[j] = x - mi[j];
                } else {
                    const int e0 = g.vptr_x[v], e1 = g.vptr_x[v + 1];
                    float S = 0.0f;
                    if (k > 0) {
                        for (int e = e0; e < e1; ++e) S = S + msg[e];
                        const float lam0 = om * L + gv * Pv;
                        Pv = lam0 + S;
                        P[v] = Pv;
                        if (k == T) continue;
                    }
                    const float lam = om * L + gv * Pv;
                    const float x = S + lam;
                    if (k > 0)
                        for (int e = e0; e < e1; ++e) msg[e] = x - msg[e];
                    else
                        for (int e = e0; e < e1; ++e) msg[e] = x - 0.0f;
                }
            }
        }
        __syncthreads();
        // ---- the decision weighed in the previous step: its weight is complete now, P still holds it ----
        if (pending) {
            const int total = wacc[cwl];
            const int w = total - wprev;
            wprev = total;
            if (found <= 1 || w < best_w) {
                best_w = w;
                best_r = pend_r;
                best_k = pend_k;
                for (int v = lane; v < n; v += a.tpc) a.hard_out[row + v] = (uint8_t)(P[v] < 0.0f);
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
        // ---- checks: parity of the decisions (k > 0), then the min-sum update (k < T) ----
        if (!done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned sy = !a.synd ? 0u : synd_in_reg ? ((synd_bits >> i) & 1u) : (a.synd[(size_t)b * m + c] & 1u);
                if constexpr (REGULAR) {
                    const uint4 pk = reinterpret_cast<const uint4*>(g.cslot16)[c];
                    const unsigned w[4] = {pk.x, pk.y, pk.z, pk.w};
                    unsigned off[DC];
#pragma unroll
                    for (int j = 0; j < DC; ++j) off[j] = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
                    if (k > 0) {
                        unsigned par = sy;
#pragma unroll
                        for (int j = 0; j < DC; ++j) par ^= (unsigned)(P[(off[j] >> 2) / DV] < 0.0f);  // slot v * DV + j belongs to bit v
                        if (par) stamp[cwl] = step;
                    }
                    if (k < T) cn_minsum_regular<DC>(msg, off, DC, sy, a.factor);
                } else if constexpr (DC > 0) {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {  // before the slot list is loaded: the two index lists are never live together
                        int vn[DC];
#pragma unroll
                        for (int j = 0; j < DC; ++j) vn[j] = (j < deg) ? g.cvn[c0 + j] : 0;
                        unsigned par = sy;
#pragma unroll
                        for (int j = 0; j < DC; ++j) par ^= (unsigned)((j < deg) && (P[vn[j]] < 0.0f));
                        if (par) stamp[cwl] = step;
                    }
                    if (k < T) {
                        unsigned off[DC];
#pragma unroll
                        for (int j = 0; j < DC; ++j) off[j] = (j < deg) ? 4u * (unsigned)g.cslot[c0 + j] : 0u;
                        cn_minsum_regular<DC>(msg, off, deg, sy, a.factor);
                    }
                } else {
                    const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
                    if (k > 0) {
                        unsigned par = sy;
                        for (int j = 0; j < deg; ++j) par ^= (unsigned)(P[g.cvn[c0 + j]] < 0.0f);
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
                    for (int v = lane; v < n; v += a.tpc)
                        if (P[v] < 0.0f) part += (int)__builtin_rintf(1024.0f * relay_prior(a, row, v));
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
int launch(const fgnn_graph* g, const RelayArgs& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    return fgnn_launch(relay_kernel<DV, DC>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
}

// the min-sum part of fgnn_bp2_decode's dispatch rule, restated
int dispatch(const fgnn_graph* g, const RelayArgs& a, const LaunchGeom& L, size_t lds_bytes, hipStream_t st)
{
    const bool regular = g->d.cslot16 && !g->force_generic;
    if (regular && g->d.dvx == 3 && g->d.dc == 6) return launch<3, 6>(g, a, L, lds_bytes, st);
    if (regular && g->d.dvx == 4 && g->d.dc == 8) return launch<4, 8>(g, a, L, lds_bytes, st);
    const int md = g->d.max_cdeg_x;
    if (md <= 8) return launch<0, 8>(g, a, L, lds_bytes, st);
    if (md <= 16) return launch<0, 16>(g, a, L, lds_bytes, st);
    return launch<0, 0>(g, a, L, lds_bytes, st);
}

}  // namespace

extern "C" int fgnn_relay_decode(const fgnn_graph* g, float normalization_factor, int pre_iter, int num_legs, int leg_iter,
                                 int stop_nconv, const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd,
                                 int B, uint8_t* hard_out, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (pre_iter < 1 || num_legs < 1 || leg_iter < 1 || stop_nconv < 1)
        return fgnn_fail(FGNN_ERR_ARG, "pre_iter, num_legs, leg_iter and stop_nconv must be >= 1");
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!gamma) return fgnn_fail(FGNN_ERR_ARG, "gamma is NULL");
    if (!hard_out || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    FGNN_DEVICE_GUARD(g->device);
    LaunchGeom L = fgnn_geom(g, B);
    RelayArgs a;
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
    a.synd = synd;
    a.hard_out = hard_out;
    a.stats = stats;
    // per codeword: E_x messages and n posteriors, each rounded up to 4 floats; per workgroup: stamp and wacc per codeword, ndone
    a.p_off = (g->d.E_x + 3) & ~3;
    a.lds_per_cw = a.p_off + ((g->d.n + 3) & ~3);
    const size_t lds_bytes = (size_t)a.lds_per_cw * sizeof(float) * (size_t)L.cpb + (((size_t)2 * L.cpb + 1 + 3) & ~(size_t)3) * sizeof(int);
    if (lds_bytes > FGNN_LDS_BUDGET) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident kernel");
    return dispatch(g, a, L, lds_bytes, static_cast<hipStream_t>(stream));
}
