// fgnn_stpost.hip — the glue between space-time BP4 (fgnn_stbp4.hip) and the binary solvers (fgnn_lsd.hip, fgnn_osd.hip): one side
// of an unsolved window as the binary problem H_st [e ; u] = d, and a solution of it put back into the decoder's outputs.  The
// contracts are stated at fgnn_st_window_problem and fgnn_st_window_apply in include/fgnn.h.
//
// One side of a window of R rounds of a code with n qubits and m = m_side checks, as the solvers see it:
//   row     t m + c        check (c,t)
//   column  t n + v        data bit (v,t), t = 0 .. R-1
//   column  R n + t m + c  time bit (c,t)
// The rows [b,t,c] of synd and gam and the rows [b,t,v] of the decoder's outputs are already in that order, so both kernels are flat
// copies over R m and R n elements with one transform each: the syndrome difference, and the binary LLR of a qubit's three totals
// (vn_llr_z / vn_llr_x of fgnn_vn.h on VnMath, the routines fgnn_lsd's marg path runs).
//
// One workgroup of 256 threads per listed window; window index[i] is read in place and its problem written to row i, so only the
// listed windows move.  Every element is written by one thread, with plain loads and stores: no atomics, nothing depends on the
// launch geometry.
#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_vn.h"

namespace {

constexpr int STPOST_T = 256;

struct StProblemArgs {
    int side, R, n, m;
    const uint8_t* synd;  // [B,R,m] or null
    const uint8_t* prev;  // [B,m] or null
    const float* marg;    // [B,R,3,n]
    const float* gam;     // [B,R,m]
    const int* index;     // [nact] or null: windows 0 .. nact-1
    uint8_t* d_out;       // [nact,R m]
    float* llr_out;       // [nact,R (n + m)]
};

__global__ void __launch_bounds__(STPOST_T) st_problem_kernel(StProblemArgs a)
{
    FG_LOG_TAB_SETUP();
    const int tid = threadIdx.x, R = a.R, n = a.n, m = a.m, NQ = R * n, NC = R * m;
    const size_t i = blockIdx.x, b = a.index ? (size_t)a.index[i] : i;
    uint8_t* d = a.d_out + i * NC;
    float* llr = a.llr_out + i * ((size_t)NQ + NC);
    const uint8_t* s = a.synd ? a.synd + b * NC : nullptr;
    const uint8_t* pv = a.prev ? a.prev + b * m : nullptr;
    // d_{c,0} = s_{c,0} ^ prev_c, d_{c,t} = s_{c,t} ^ s_{c,t-1}: in the flat order the bit before is m places back
    for (int j = tid; j < NC; j += STPOST_T) {
        const unsigned cur = s ? (s[j] & 1u) : 0u;
        unsigned before;
        if (j >= m) before = s ? (s[j - m] & 1u) : 0u;
        else before = pv ? (pv[j] & 1u) : 0u;
        d[j] = (uint8_t)(cur ^ before);
    }
    const float* mg = a.marg + b * 3 * NQ;
    for (int q = tid, v = tid, t = 0; q < NQ; q += STPOST_T, v += STPOST_T) {
        while (v >= n) { v -= n; ++t; }
        const float* mt = mg + (size_t)t * 3 * n;
        const float X = mt[v], Y = mt[n + v], Z = mt[2 * (size_t)n + v];
        llr[q] = a.side == 0 ? vn_llr_z<VnMath>(X, Y, Z) : vn_llr_x<VnMath>(X, Y, Z);
    }
    const float* gm = a.gam + b * NC;
    for (int j = tid; j < NC; j += STPOST_T) llr[NQ + j] = gm[j];
}

struct StApplyArgs {
    int R, n, m;
    const uint8_t* e;  // [nact,R (n + m)]
    const int* index;  // [nact] or null: windows 0 .. nact-1
    uint8_t* hat;      // [B,R,n]
    uint8_t* u_hat;    // [B,R,m]
};

__global__ void __launch_bounds__(STPOST_T) st_apply_kernel(StApplyArgs a)
{
    const int tid = threadIdx.x, NQ = a.R * a.n, NC = a.R * a.m;
    const size_t i = blockIdx.x, b = a.index ? (size_t)a.index[i] : i;
    const uint8_t* e = a.e + i * ((size_t)NQ + NC);
    uint8_t* hat = a.hat + b * NQ;
    uint8_t* uh = a.u_hat + b * NC;
    for (int q = tid; q < NQ; q += STPOST_T) hat[q] = e[q];
    for (int j = tid; j < NC; j += STPOST_T) uh[j] = e[NQ + j];
}

// the checks the two entry points share; *m = the checks of the side
int stpost_check(const fgnn_graph* g, int side, int rounds, int nact, int* m)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (side < 0 || side > 1) return fgnn_fail(FGNN_ERR_ARG, "side must be 0 or 1");
    if (rounds < 1) return fgnn_fail(FGNN_ERR_ARG, "rounds must be >= 1");
    if (nact < 0) return fgnn_fail(FGNN_ERR_ARG, "nact must be >= 0");
    *m = side ? g->d.m_z : g->d.m_x;
    if ((long long)rounds * ((long long)g->d.n + *m) > INT32_MAX)
        return fgnn_fail(FGNN_ERR_ARG, "window too large: rounds * (n + m_side) must fit 31 bits");
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_st_window_problem(const fgnn_graph* g, int side, int rounds, const uint8_t* synd, const uint8_t* prev, const float* marg,
                                      const float* gam, const int32_t* index, int nact, uint8_t* d_out, float* llr_out, void* stream)
{
    int m = 0;
    if (int err = stpost_check(g, side, rounds, nact, &m)) return err;
    if (nact == 0) return FGNN_OK;  // an empty list needs no buffers
    if (!marg || !gam || !d_out || !llr_out) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    FGNN_DEVICE_GUARD(g->device);
    const StProblemArgs a{side, rounds, g->d.n, m, synd, prev, marg, gam, index, d_out, llr_out};
    return fgnn_launch(st_problem_kernel, dim3(nact), dim3(STPOST_T), 0, static_cast<hipStream_t>(stream), a);
}

extern "C" int fgnn_st_window_apply(const fgnn_graph* g, int side, int rounds, const uint8_t* e, const int32_t* index, int nact, uint8_t* hat,
                                    uint8_t* u_hat, void* stream)
{
    int m = 0;
    if (int err = stpost_check(g, side, rounds, nact, &m)) return err;
    if (nact == 0) return FGNN_OK;
    if (!e || !hat || !u_hat) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    FGNN_DEVICE_GUARD(g->device);
    const StApplyArgs a{rounds, g->d.n, m, e, index, hat, u_hat};
    return fgnn_launch(st_apply_kernel, dim3(nact), dim3(STPOST_T), 0, static_cast<hipStream_t>(stream), a);
}
