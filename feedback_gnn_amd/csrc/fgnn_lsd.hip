// fgnn_lsd.hip — localized statistics decoding (LSD-0 with synchronous growth) of BP failures: the contract of fgnn_lsd in
// include/fgnn.h (Hillmann, Berent, Quintavalle, Eisert, Wille, Roffe 2024; BpLsdDecoder of ldpc v2).
//
// One workgroup of 256 threads owns one listed sample; all of its state is in LDS (lsd_lds below).  A round is
//   1. validity    every non-pivot check with t[c] = 1 marks its cluster invalid (atomicOr on cflag[label]);
//   2. select      every check of an invalid live cluster takes the least key over its bits outside inB and atomicMin's it into
//                  minkey[label]; a root without a bit is marked dead, the others append their key to sel (atomicAdd on a counter);
//   3. sort        bitonic over sel padded to the next power of two (duplicates stay adjacent and are skipped);
//   4. append      wave 0 alone walks sel in order — the serial spine, fgnn_lsd.h on one wave: x a lane per word in registers, the
//                  union of the clusters on lane 0 as a union-find whose roots are the least check index of their set;
//   5. relabel     every check reads its root into scratch, and after a barrier lab[c] = that root.
// Races: the only concurrent writes to one address are integer atomics (atomicOr / atomicMin / atomicAdd) whose results do not depend
// on arrival order (OR, minimum, and a counter whose slots are sorted afterwards).  Phases are separated by __syncthreads; inside
// phase 4 every LDS word is touched by one lane only (fgnn_lsd.h), so wave 0 needs no barrier of its own while waves 1-3 wait.
#include "fgnn_internal.h"
#include "fgnn_lsd.h"
#include "fgnn_math.h"
#include "fgnn_vn.h"

namespace {

constexpr int LSD_T = 256;
constexpr int LSD_MAX_WPL = 4;  // words of x per lane: m <= 32 * 64 * 4 = 8192 checks

struct LsdArgs {
    int side, B, m, W, NB, NPS, cap, max_rounds;  // W = ceil(m/32), NB = ceil(n/32), NPS = power of two >= m, cap = max_pivots > 0
    const float* marg;
    const float* llr_bin;
    const uint8_t* synd;
    const int* index;
    uint8_t* e_hat;
    int32_t* stats;
};

enum { CTL_P = 0, CTL_ROUNDS, CTL_COLS, CTL_CAPPED, CTL_GROW, CTL_CNT, CTL_BAD, CTL_WORDS = 8 };

// LDS of one workgroup: minkey [m] u64, sel [NPS] u64, L [cap][W], ukey [n], lab [m], cflag [m], piv [cap], col [cap], t [W],
// isPivot [W], inB [NB], ctl [8]
__host__ __device__ inline size_t lsd_lds_bytes(int n, int m, int cap)
{
    const size_t W = (size_t)(m + 31) / 32, NB = (size_t)(n + 31) / 32;
    size_t NPS = 1;
    while (NPS < (size_t)m) NPS <<= 1;
    return 8 * ((size_t)m + NPS) + 4 * ((size_t)cap * W + (size_t)n + 2 * (size_t)m + 2 * (size_t)cap + 2 * W + NB + CTL_WORDS);
}

struct LsdLds {
    unsigned long long* minkey;
    unsigned long long* sel;
    unsigned* L;
    unsigned* ukey;
    int* lab;
    int* cflag;  // at a cluster's label: bit 0 = invalid in this round, bit 1 = dead
    int* piv;
    int* col;
    unsigned* t;
    unsigned* isPivot;
    unsigned* inB;
    int* ctl;
};

__device__ inline LsdLds lsd_lds(unsigned char* smem, int n, const LsdArgs& a)
{
    LsdLds s;
    s.minkey = reinterpret_cast<unsigned long long*>(smem);
    s.sel = s.minkey + a.m;
    s.L = reinterpret_cast<unsigned*>(s.sel + a.NPS);
    s.ukey = s.L + (size_t)a.cap * a.W;
    s.lab = reinterpret_cast<int*>(s.ukey + n);
    s.cflag = s.lab + a.m;
    s.piv = s.cflag + a.m;
    s.col = s.piv + a.cap;
    s.t = reinterpret_cast<unsigned*>(s.col + a.cap);
    s.isPivot = s.t + a.W;
    s.inB = s.isPivot + a.W;
    s.ctl = reinterpret_cast<int*>(s.inB + a.NB);
    return s;
}

// one wave as the lane group of fgnn_lsd.h: the sources are wave-uniform, so the fetches are v_readlane
struct LsdWave {
    static constexpr int LANES = 64;
    static __device__ __forceinline__ int lane() { return (int)(threadIdx.x & 63); }
    static __device__ __forceinline__ unsigned fetch(unsigned v, int src) { return (unsigned)__builtin_amdgcn_readlane((int)v, src); }
    static __device__ __forceinline__ int min_all(int v)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int other = __shfl_xor(v, o);
            v = other < v ? other : v;
        }
        return v;
    }
};

__device__ __forceinline__ int lsd_find(const int* lab, int c)
{
    while (lab[c] != c) c = lab[c];
    return c;
}

template <int WPL>
__global__ void __launch_bounds__(LSD_T) lsd_kernel(GraphDev g, LsdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, T = LSD_T, lane = tid & 63, wave = tid >> 6;
    const int n = g.n, m = a.m, W = a.W;
    const int b = a.index ? a.index[blockIdx.x] : (int)blockIdx.x;
    const LsdLds s = lsd_lds(smem, n, a);
    const int coff = a.side ? g.m_x : 0;
    const int* vptr = a.side ? g.vptr_z : g.vptr_x;  // column v of this side: the checks g.vchk[vptr[v] .. vptr[v + 1])
    const uint8_t* sy = a.synd + (size_t)b * m;
    uint8_t* eo = a.e_hat + (size_t)b * n;

    // start: keys, t = s, every defect a cluster of its own, e = 0
    for (int v = tid; v < n; v += T) {
        float r;
        if (a.llr_bin) r = a.llr_bin[(size_t)b * n + v];
        else {
            const float* mg = a.marg + (size_t)b * 3 * n;
            const float X = mg[v], Y = mg[n + v], Z = mg[2 * n + v];
            r = a.side == 0 ? vn_llr_z<VnMath>(X, Y, Z) : vn_llr_x<VnMath>(X, Y, Z);
        }
        r = r + 0.0f;  // -0 -> +0, as fgnn_osd0
        s.ukey[v] = lsd_sortable(fg_f2u(r));
        eo[v] = 0;
    }
    for (int w = tid; w < W; w += T) {
        unsigned bits = 0u;
        for (int i = 0; i < 32 && w * 32 + i < m; ++i) bits |= (unsigned)(sy[w * 32 + i] & 1) << i;
        s.t[w] = bits;
        s.isPivot[w] = 0u;
    }
    for (int w = tid; w < a.NB; w += T) s.inB[w] = 0u;
    for (int c = tid; c < m; c += T) {
        s.lab[c] = (sy[c] & 1) ? c : -1;
        s.cflag[c] = 0;
    }
    if (tid < CTL_WORDS) s.ctl[tid] = 0;
    __syncthreads();

    for (;;) {
        // 1. validity
        for (int c = tid; c < m; c += T) {
            s.cflag[c] &= 2;
            s.minkey[c] = ~0ull;
        }
        if (tid == 0) {
            s.ctl[CTL_GROW] = 0;
            s.ctl[CTL_CNT] = 0;
        }
        __syncthreads();
        for (int c = tid; c < m; c += T) {
            const int l = s.lab[c];
            if (l >= 0 && ((s.t[c >> 5] & ~s.isPivot[c >> 5]) >> (c & 31)) & 1u) atomicOr(&s.cflag[l], 1);
        }
        __syncthreads();
        for (int c = tid; c < m; c += T)
            if (s.lab[c] == c && s.cflag[c] == 1) atomicOr(&s.ctl[CTL_GROW], 1);
        __syncthreads();
        const int rounds = s.ctl[CTL_ROUNDS];
        if (!s.ctl[CTL_GROW] || s.ctl[CTL_CAPPED] || (a.max_rounds && rounds >= a.max_rounds)) break;
        // 2. select
        for (int c = tid; c < m; c += T) {
            const int l = s.lab[c];
            if (l < 0 || s.cflag[l] != 1) continue;
            unsigned long long best = ~0ull;
            for (int jx = g.cptr[coff + c]; jx < g.cptr[coff + c + 1]; ++jx) {
                const int v = g.cvn[jx];
                if (!((s.inB[v >> 5] >> (v & 31)) & 1u)) {
                    const unsigned long long k = ((unsigned long long)s.ukey[v] << 32) | (unsigned)v;
                    best = k < best ? k : best;
                }
            }
            if (best != ~0ull) atomicMin(&s.minkey[l], best);
        }
        __syncthreads();
        for (int c = tid; c < m; c += T)
            if (s.lab[c] == c && s.cflag[c] == 1) {
                const unsigned long long k = s.minkey[c];
                if (k == ~0ull) s.cflag[c] = 3;  // dead: a whole component whose syndrome is not in the image of H
                else s.sel[atomicAdd(&s.ctl[CTL_CNT], 1)] = k;
            }
        __syncthreads();
        // 3. sort sel[0 .. cnt) ascending
        const int cnt = s.ctl[CTL_CNT];
        int NP = 1;
        while (NP < cnt) NP <<= 1;
        for (int i = cnt + tid; i < NP; i += T) s.sel[i] = ~0ull;
        __syncthreads();
        for (int k2 = 2; k2 <= NP; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                for (int i = tid; i < NP; i += T) {
                    const int ixj = i ^ j2;
                    if (ixj > i) {
                        const unsigned long long x = s.sel[i], y = s.sel[ixj];
                        const bool up = (i & k2) == 0;
                        if ((x > y) == up) { s.sel[i] = y; s.sel[ixj] = x; }
                    }
                }
                __syncthreads();
            }
        // 4. append, one wave
        if (wave == 0) {
            int P = s.ctl[CTL_P], cols = s.ctl[CTL_COLS], capped = 0;
            unsigned long long last = ~0ull;
            for (int i = 0; i < cnt && !capped; ++i) {
                const unsigned long long key = s.sel[i];
                if (key == last) continue;
                last = key;
                const int v = (int)(unsigned)key;
                const int* chk = g.vchk + vptr[v];
                const int deg = vptr[v + 1] - vptr[v];
                if (lane == 0) {
                    s.inB[v >> 5] |= 1u << (v & 31);
                    int root = 0x7fffffff;
                    for (int e = 0; e < deg; ++e) {
                        const int c = chk[e];
                        const int r = s.lab[c] < 0 ? c : lsd_find(s.lab, c);
                        root = r < root ? r : root;
                    }
                    s.lab[root] = root;  // a root already, or a check that joins: a root before anything points at it
                    for (int e = 0; e < deg; ++e) {
                        const int c = chk[e];
                        if (s.lab[c] < 0) s.lab[c] = root;
                        else s.lab[lsd_find(s.lab, c)] = root;
                    }
                }
                ++cols;
                unsigned x[WPL];
                lsd_column<WPL, LsdWave>(x, chk, deg);
                lsd_reduce<WPL, LsdWave>(x, s.piv, s.L, P, W);
                const int p = lsd_pivot<WPL, LsdWave>(x, s.isPivot, W);
                if (p == LSD_NO_PIVOT) continue;
                if (P == a.cap) {
                    capped = 1;
                    break;
                }
                lsd_store_pivot<WPL, LsdWave>(x, p, v, P, s.piv, s.col, s.L, s.isPivot, s.t, W);
                ++P;
            }
            if (lane == 0) {
                s.ctl[CTL_P] = P;
                s.ctl[CTL_COLS] = cols;
                s.ctl[CTL_CAPPED] = capped;
                s.ctl[CTL_ROUNDS] = rounds + 1;
            }
        }
        __syncthreads();
        // 5. relabel: lab[c] = the root of c (the least check index of its cluster); the roots go through scratch so that no
        //    thread walks parents another one is rewriting
        int* root_of = reinterpret_cast<int*>(s.minkey);
        for (int c = tid; c < m; c += T) root_of[c] = s.lab[c] < 0 ? -1 : lsd_find(s.lab, c);
        __syncthreads();
        for (int c = tid; c < m; c += T) s.lab[c] = root_of[c];
        __syncthreads();
    }

    // found = no non-pivot check with t[c] = 1; e[col[k]] = t[piv[k]]
    for (int w = tid; w < W; w += T)
        if (s.t[w] & ~s.isPivot[w]) atomicOr(&s.ctl[CTL_BAD], 1);
    const int P = s.ctl[CTL_P];
    for (int k = tid; k < P; k += T) lsd_readout(k, s.piv, s.col, s.t, eo);
    __syncthreads();
    if (tid == 0 && a.stats) {
        int32_t* st = a.stats + (size_t)b * 4;
        st[0] = s.ctl[CTL_BAD] ? 0 : 1;
        st[1] = s.ctl[CTL_ROUNDS];
        st[2] = s.ctl[CTL_COLS];
        st[3] = P;
    }
}

// the largest pivot count whose LDS fits the budget for this side (may be <= 0: the fixed part alone does not fit), capped by m and n
int lsd_cap(const fgnn_graph* g, int side)
{
    const int n = g->d.n, m = side ? g->d.m_z : g->d.m_x;
    const size_t fixed = lsd_lds_bytes(n, m, 0), per = lsd_lds_bytes(n, m, 1) - fixed;
    if (fixed > FGNN_LDS_BUDGET) return 0;
    const size_t fit = (FGNN_LDS_BUDGET - fixed) / per;
    const size_t lim = (size_t)(m < n ? m : n);
    return (int)(fit < lim ? fit : lim);
}

int lsd_check_graph(const fgnn_graph* g, int side)
{
    if (!g || side < 0 || side > 1) return fgnn_fail(FGNN_ERR_ARG, "bad LSD arguments");
    const int m = side ? g->d.m_z : g->d.m_x;
    if (m > 32 * 64 * LSD_MAX_WPL) return fgnn_fail(FGNN_ERR_ARG, "LSD kernel supports m <= 8192 checks per side");
    if (lsd_cap(g, side) < 1) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident LSD kernel");
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_lsd_max_pivots(const fgnn_graph* g, int side, int* cap)
{
    if (!cap) return fgnn_fail(FGNN_ERR_ARG, "bad LSD arguments");
    const int rc = lsd_check_graph(g, side);
    if (rc != FGNN_OK) return rc;
    *cap = lsd_cap(g, side);
    return FGNN_OK;
}

extern "C" int fgnn_lsd(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
                        const int32_t* index, int nact, int max_pivots, int max_rounds, uint8_t* e_hat, int32_t* stats, void* stream)
{
    const int rc = lsd_check_graph(g, side);
    if (rc != FGNN_OK) return rc;
    if ((marg == nullptr) == (llr_bin == nullptr)) return fgnn_fail(FGNN_ERR_ARG, "exactly one of marg and llr_bin must be given");
    if (!synd || !e_hat || B < 0 || (index && nact < 0)) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    if (max_pivots < 0 || max_rounds < 0) return fgnn_fail(FGNN_ERR_ARG, "max_pivots and max_rounds must be >= 0");
    const int cap = lsd_cap(g, side);
    if (max_pivots > cap)
        return fgnn_fail(FGNN_ERR_ARG, "max_pivots too large: the largest count that fits is " + std::to_string(cap));
    const int count = index ? nact : B;
    if (count <= 0) return FGNN_OK;
    LsdArgs a{};
    a.side = side;
    a.B = B;
    a.m = side ? g->d.m_z : g->d.m_x;
    a.W = (a.m + 31) / 32;
    a.NB = (g->d.n + 31) / 32;
    a.NPS = 1;
    while (a.NPS < a.m) a.NPS <<= 1;
    a.cap = max_pivots ? max_pivots : cap;
    a.max_rounds = max_rounds;
    a.marg = marg;
    a.llr_bin = llr_bin;
    a.synd = synd;
    a.index = index;
    a.e_hat = e_hat;
    a.stats = stats;
    const size_t lds = lsd_lds_bytes(g->d.n, a.m, a.cap);
    FGNN_DEVICE_GUARD(g->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const int wpl = (a.W + 63) / 64;
    if (wpl <= 1) return fgnn_launch(lsd_kernel<1>, dim3(count), dim3(LSD_T), lds, st, g->d, a);
    if (wpl == 2) return fgnn_launch(lsd_kernel<2>, dim3(count), dim3(LSD_T), lds, st, g->d, a);
    return fgnn_launch(lsd_kernel<LSD_MAX_WPL>, dim3(count), dim3(LSD_T), lds, st, g->d, a);
}
