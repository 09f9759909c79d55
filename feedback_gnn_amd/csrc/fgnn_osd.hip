// fgnn_osd.hip — order-0 ordered-statistics post-processing of BP failures.
//
// Replaces OSD0_Decoder.call / find_mrb of /root/reference sionna/fec/ldpc/bp_osd.py:14-77 as driven by
// BP4_OSD_Model.call_osd (:138-157): solve H_basis e = s on the most reliable independent columns, where H_basis is the
// full-rank row subset hx[pivot_hx] (or hz[pivot_hz]) and the column order is ascending binary reliability.
//
// The reference materialises a dense int32 [bs, rank, n+1] tensor (1.5 MB per sample) and runs `rank` XLA loop steps
// over it (3.8 s for 649 samples on an RTX 4090, examples/OSD.ipynb cell 6).  Here one workgroup owns one failed
// sample: the augmented matrix is bit-packed in LDS (429 x 28 words = 48 KB for [[882,24]]), columns are permuted by
// scattering the sparse rows through the inverse sort permutation, and each elimination step is one pivot search
// (ffs over the row's words) plus word-wide XORs of the rows that hold the pivot column.
// Bit-identical to oracle/fgnn_oracle.c: og_osd0 (stable sort: ties keep qubit order).
#include "fgnn_internal.h"
#include "fgnn_math.h"
#include "fgnn_vn.h"

namespace {

struct OsdArgs {
    int side, rank, B, nact, W, WS, NP;  // W words per row, WS padded row stride (odd), NP sort size (power of two)
    const int* pivot_rows;               // [rank] check ids (side-local) forming the row basis
    const float* marg;                   // [B,3,n] or null
    const float* llr_bin;                // [B,n] or null
    const uint8_t* synd;                 // [B,m_side]
    const int* index;                    // [nact] or null
    uint8_t* e_hat;                      // [B,n]
    int32_t* chosen;                     // [B] or null: winning candidate index (osd_search_kernel only)
    int method, order;                   // FGNN_OSD_* and the requested order (osd_search_kernel only)
};

// bytes of the OsdLds buffers (the search kernel's scratch follows, 8-aligned)
__host__ __device__ inline size_t osd_lds_bytes(int n, int rank, int WS, int NP)
{
    return sizeof(unsigned long long) * (size_t)NP + sizeof(unsigned) * (size_t)rank * WS + sizeof(int) * (size_t)(2 * n + rank);
}
constexpr size_t OSD_SEARCH_SCRATCH = 4 * sizeof(unsigned long long) + 8;  // per-wave best keys, |T|

// LDS of one OSD workgroup, carved from the dynamic allocation (osd_lds_bytes on the host counts the same buffers)
struct OsdLds {
    unsigned long long* keys;  // [NP]
    unsigned* mat;             // [rank][WS]
    int* order;                // [n]
    int* inv;                  // [n]
    int* piv;                  // [rank]
};

__device__ inline OsdLds osd_lds(unsigned char* smem, const GraphDev& g, const OsdArgs& a)
{
    OsdLds L;
    L.keys = reinterpret_cast<unsigned long long*>(smem);
    L.mat = reinterpret_cast<unsigned*>(L.keys + a.NP);
    L.order = reinterpret_cast<int*>(L.mat + (size_t)a.rank * a.WS);
    L.inv = L.order + g.n;
    L.piv = L.inv + g.n;
    return L;
}

// Steps 1-4 of OSD for sample b: sorted reliabilities (keys), order/inv permutation, e_hat[b] zeroed, and the reduced augmented
// matrix with pivot column piv[row] of every row.  Shared by osd0_kernel and osd_search_kernel.
__device__ __forceinline__ void osd_eliminate(const GraphDev& g, const OsdArgs& a, int b, const OsdLds& L)
{
    const int tid = threadIdx.x, T = 256;
    const int n = g.n, rank = a.rank, W = a.W, WS = a.WS;
    unsigned long long* keys = L.keys;
    unsigned* mat = L.mat;
    int* order = L.order;
    int* inv = L.inv;
    int* piv = L.piv;

    // 1. reliabilities -> sortable 64-bit keys (value, qubit): ascending, ties by qubit index (stable)
    for (int v = tid; v < a.NP; v += T) {
        unsigned long long k = ~0ull;
        if (v < n) {
            float r;
            if (a.llr_bin) r = a.llr_bin[(size_t)b * n + v];
            else {
                const float* mg = a.marg + (size_t)b * 3 * n;
                const float X = mg[v], Y = mg[n + v], Z = mg[2 * n + v];
                r = a.side == 0 ? vn_llr_z<VnMath>(X, Y, Z) : vn_llr_x<VnMath>(X, Y, Z);  // bp_osd.py:125-131
            }
            r = r + 0.0f;  // -0 -> +0: the oracle compares with '<', for which the two zeros tie
            unsigned u = fg_f2u(r);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
            k = ((unsigned long long)u << 32) | (unsigned)v;
        }
        keys[v] = k;
    }
    __syncthreads();
    // 2. bitonic sort
    for (int k2 = 2; k2 <= a.NP; k2 <<= 1)
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = tid; i < a.NP; i += T) {
                const int ixj = i ^ j2;
                if (ixj > i) {
                    const unsigned long long x = keys[i], y = keys[ixj];
                    const bool up = (i & k2) == 0;
                    if ((x > y) == up) { keys[i] = y; keys[ixj] = x; }
                }
            }
            __syncthreads();
        }
    for (int j = tid; j < n; j += T) {
        const int v = (int)(unsigned)keys[j];
        order[j] = v;
        inv[v] = j;
    }
    for (int i = tid; i < rank * WS; i += T) mat[i] = 0u;
    uint8_t* eo = a.e_hat + (size_t)b * n;
    for (int v = tid; v < n; v += T) eo[v] = 0;
    __syncthreads();
    // 3. permuted, augmented, bit-packed matrix: thread r owns row r
    const int coff = a.side ? g.m_x : 0;
    const int ms = a.side ? g.m_z : g.m_x;
    for (int r = tid; r < rank; r += T) {
        const int c = a.pivot_rows[r];
        unsigned* row = mat + (size_t)r * WS;
        for (int jx = g.cptr[coff + c]; jx < g.cptr[coff + c + 1]; ++jx) {
            const int j = inv[g.cvn[jx]];
            row[j >> 5] |= 1u << (j & 31);
        }
        if (a.synd[(size_t)b * ms + c] & 1) row[n >> 5] |= 1u << (n & 31);
    }
    __syncthreads();
    // 4. row-by-row Gauss-Jordan (find_mrb, bp_osd.py:14-47)
    for (int r = 0; r < rank; ++r) {
        const unsigned* prow = mat + (size_t)r * WS;
        if (tid < 64) {
            int pos = 0x7fffffff;
            if (tid < W) {
                const unsigned w = prow[tid];
                if (w) pos = tid * 32 + (__ffs((int)w) - 1);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int other = __shfl_xor(pos, o);
                pos = other < pos ? other : pos;
            }
            if (tid == 0) piv[r] = pos > n ? 0 : pos;  // all-zero row: tf.argmax returns 0
        }
        __syncthreads();
        const int p = piv[r];
        const int pw = p >> 5;
        const unsigned pm = 1u << (p & 31);
        for (int i = tid; i < rank; i += T)
            if (i != r) {
                unsigned* ri = mat + (size_t)i * WS;
                if (ri[pw] & pm)
                    for (int w = pw; w < W; ++w) ri[w] ^= prow[w];
            }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) osd0_kernel(GraphDev g, OsdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, T = 256;
    const int n = g.n, rank = a.rank, WS = a.WS;
    const int b = a.index ? a.index[blockIdx.x] : (int)blockIdx.x;
    const OsdLds L = osd_lds(smem, g, a);
    osd_eliminate(g, a, b, L);
    const unsigned* mat = L.mat;
    const int* order = L.order;
    const int* piv = L.piv;
    uint8_t* eo = a.e_hat + (size_t)b * n;
    // 5. e_hat[order[pivot_r]] = transformed syndrome bit of row r (bp_osd.py:44-45, :68-69), for the rows whose pivot bit is set: a
    //    zero row of a rank-deficient basis (pivot 0) writes nothing, as in og_osd0 and osd_search_kernel step 5
    for (int r = tid; r < rank; r += T) {
        const int p = piv[r];
        if (p < n) {
            const unsigned* row = mat + (size_t)r * WS;
            if ((row[p >> 5] >> (p & 31)) & 1u) eo[order[p]] = (uint8_t)((row[n >> 5] >> (n & 31)) & 1u);
        }
    }
}

// float -> uint32 whose unsigned order is the float order (the sort key of step 1), and back
__device__ __forceinline__ unsigned osd_sortable(float f)
{
    const unsigned u = fg_f2u(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float osd_unsortable(unsigned s) { return fg_u2f((s & 0x80000000u) ? (s & 0x7fffffffu) : ~s); }

// Candidate c of the list (fgnn.h, fgnn_osd) as a mask over the search columns T[0..lam) plus at most one further column T[xc]
// (xc = -1: none).  osd_e: bit i of c sets T[i].  osd_cs: 0, then T[0..k) one at a time, then the pairs {T[i], T[j]}, i < j < lam.
__device__ __forceinline__ void osd_candidate(int method, int c, int k, int lam, unsigned long long& cbits, int& xc)
{
    cbits = 0ull;
    xc = -1;
    if (method == FGNN_OSD_E) {
        cbits = (unsigned long long)c;
    } else if (c >= 1 && c <= k) {
        if (c - 1 < lam) cbits = 1ull << (c - 1);
        else xc = c - 1;
    } else if (c > k) {
        int q = c - k - 1, i = 0;
        while (q >= lam - 1 - i) {
            q -= lam - 1 - i;
            ++i;
        }
        cbits = (1ull << i) | (1ull << (i + 1 + q));
    }
}

// OSD-E / OSD-CS: the elimination of osd_eliminate, then every candidate of the list scored by its soft weight (the fixed-order tree
// sum of fgnn.h), the cheapest (lowest index on ties) written to e_hat[b].  NPL = max(NP, 64) / 64 sorted positions per lane: lane l
// of every wave holds positions l + 64 m (m < NPL) in registers — reliability, pivot row / non-pivot index, the bit of candidate 0
// and the row's bits on the search columns — so a candidate costs one masked parity per position, NPL - 1 lane-local adds per
// tree level h >= 64 and six cross-lane adds.  The four waves take candidates round-robin.
template <int NPL>
__global__ void __launch_bounds__(256) osd_search_kernel(GraphDev g, OsdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, T = 256, lane = tid & 63, wave = tid >> 6;
    const int n = g.n, rank = a.rank, WS = a.WS;
    const int b = a.index ? a.index[blockIdx.x] : (int)blockIdx.x;
    const OsdLds L = osd_lds(smem, g, a);
    unsigned long long* wave_best = reinterpret_cast<unsigned long long*>(smem + ((osd_lds_bytes(n, rank, WS, a.NP) + 7) & ~(size_t)7));  // [4]
    int* tcount = reinterpret_cast<int*>(wave_best + 4);                                                               // [1]
    osd_eliminate(g, a, b, L);
    const unsigned* mat = L.mat;
    const int* piv = L.piv;
    // after the sort, keys[p] = (sortable(r_sorted[p]) << 32) | order[p]; the low words are free and take the list T
    unsigned* kw = reinterpret_cast<unsigned*>(L.keys);  // kw[2p] = T[p] (p < k), kw[2p + 1] = sortable(r_sorted[p])
    int* pos = L.inv;                                    // pos[p] = pivot row of sorted position p, or -(j + 1) for p = T[j]
    // 5. pivot positions S: a row is a pivot row iff its pivot bit is set (a zero row of a rank-deficient basis is not)
    for (int p = tid; p < n; p += T) pos[p] = -1;
    __syncthreads();
    for (int r = tid; r < rank; r += T) {
        const int p = piv[r];
        if (p < n && ((mat[(size_t)r * WS + (p >> 5)] >> (p & 31)) & 1u)) pos[p] = r;
    }
    __syncthreads();
    // 6. T = the non-pivot positions in ascending order (one wave, ballot compaction)
    if (wave == 0) {
        int cnt = 0;
        for (int base = 0; base < n; base += 64) {
            const int p = base + lane;
            const bool isT = p < n && pos[p] < 0;
            const unsigned long long ball = __ballot(isT);
            if (isT) {
                const int j = cnt + __popcll(ball & ((1ull << lane) - 1ull));
                kw[2 * j] = (unsigned)p;
                pos[p] = -(j + 1);
            }
            cnt += __popcll(ball);
        }
        if (lane == 0) *tcount = cnt;
    }
    __syncthreads();
    const int k = *tcount;
    const int lam = a.order < k ? a.order : k;
    const int ncand = a.order == 0 ? 1 : a.method == FGNN_OSD_E ? (1 << lam) : 1 + k + lam * (lam - 1) / 2;
    // 7. per-lane registers for positions p = lane + 64 m
    float rv[NPL];
    int info[NPL];
    unsigned long long msk[NPL];
    unsigned e0 = 0u;
#pragma unroll
    for (int m = 0; m < NPL; ++m) {
        const int p = lane + 64 * m;
        rv[m] = 0.0f;
        info[m] = -(n + 1);  // padding: matches no column
        msk[m] = 0ull;
        if (p < n) {
            rv[m] = osd_unsortable(kw[2 * p + 1]);
            const int ip = pos[p];
            info[m] = ip;
            if (ip >= 0) {
                const unsigned* row = mat + (size_t)ip * WS;
                e0 |= ((row[n >> 5] >> (n & 31)) & 1u) << m;
                unsigned long long mm = 0ull;
                for (int j = 0; j < lam; ++j) {
                    const int t = (int)kw[2 * j];
                    mm |= (unsigned long long)((row[t >> 5] >> (t & 31)) & 1u) << j;
                }
                msk[m] = mm;
            } else if (-ip - 1 < lam) {
                msk[m] = 1ull << (-ip - 1);
            }
        }
    }
    // 8. the search: lane 0 of each wave keeps the wave's least (sortable(cost) << 32 | c)
    unsigned long long best = ~0ull;
    for (int c = wave; c < ncand; c += 4) {
        unsigned long long cbits;
        int xc;
        osd_candidate(a.method, c, k, lam, cbits, xc);
        const int xt = xc >= 0 ? (int)kw[2 * xc] : 0;
        float x[NPL];
#pragma unroll
        for (int m = 0; m < NPL; ++m) {
            unsigned bit = ((e0 >> m) & 1u) ^ ((unsigned)__popcll(msk[m] & cbits) & 1u);
            if (xc >= 0) {
                if (info[m] >= 0) bit ^= (mat[(size_t)info[m] * WS + (xt >> 5)] >> (xt & 31)) & 1u;
                else bit ^= info[m] == -(xc + 1) ? 1u : 0u;
            }
            x[m] = bit ? rv[m] : 0.0f;
        }
#pragma unroll
        for (int h = NPL / 2; h >= 1; h >>= 1)
#pragma unroll
            for (int m = 0; m < h; ++m) x[m] = x[m] + x[m + h];
        float s = x[0];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) s = s + __shfl_xor(s, h);
        const unsigned long long key = ((unsigned long long)osd_sortable(s) << 32) | (unsigned)c;
        best = key < best ? key : best;
    }
    if (lane == 0) wave_best[wave] = best;
    __syncthreads();
    unsigned long long w = wave_best[0];
    for (int i = 1; i < 4; ++i) w = wave_best[i] < w ? wave_best[i] : w;
    const int cw = (int)(unsigned)w;
    // 9. e_hat[b][order[p]] = bit p of the winner's solution
    unsigned long long cbits;
    int xc;
    osd_candidate(a.method, cw, k, lam, cbits, xc);
    const int xt = xc >= 0 ? (int)kw[2 * xc] : 0;
    uint8_t* eo = a.e_hat + (size_t)b * n;
    for (int p = tid; p < n; p += T) {
        const int ip = pos[p];
        unsigned bit;
        if (ip >= 0) {
            const unsigned* row = mat + (size_t)ip * WS;
            bit = (row[n >> 5] >> (n & 31)) & 1u;
            for (unsigned long long cb = cbits; cb; cb &= cb - 1ull) {
                const int t = (int)kw[2 * (__ffsll((long long)cb) - 1)];
                bit ^= (row[t >> 5] >> (t & 31)) & 1u;
            }
            if (xc >= 0) bit ^= (row[xt >> 5] >> (xt & 31)) & 1u;
        } else {
            const int j = -ip - 1;
            bit = (j < 64 && ((cbits >> j) & 1ull)) || j == xc ? 1u : 0u;
        }
        eo[L.order[p]] = (uint8_t)bit;
    }
    if (tid == 0 && a.chosen) a.chosen[b] = cw;
}

// ---- OSD beyond LDS: the same steps on a caller-owned global workspace (fgnn_osd_ws) ----------------------------------------------
// One persistent workgroup per slot walks the sample list (t = blockIdx.x, += gridDim.x).  Slot blockIdx.x holds the augmented matrix
// bit-packed WORD-MAJOR, mat[w * RS + row] (RS = rank rounded up to 64): in the thread-per-row XOR sweep word w of 64 consecutive rows is
// one contiguous 256-byte access per wave, and so is column t's word across the rows.  The sort keys (NP * 8 bytes) and the copy of the
// current pivot row (W words) stay in LDS; the tables order / inv / piv / msk live in LDS when they fit next to them, else in the slot
// (generic pointers: the kernel does not care which).
constexpr int OSDW_T = 1024, OSDW_NW = OSDW_T / 64;
constexpr int OSDW_MAX_N = 16384;

struct OsdWsArgs {
    int side, rank, B, W, RS, NP, LV;  // LV = log2(max(NP, 64) / 64): positions per lane of the search tree = 2^LV
    const int* pivot_rows;
    const float* marg;
    const float* llr_bin;
    const uint8_t* synd;
    const int* index;
    int count;
    uint8_t* e_hat;
    int32_t* chosen;
    int method, order;
    unsigned char* ws;        // slot s at ws + s * slot_bytes
    size_t slot_bytes;
    int tables_in_lds;        // 1: order / inv / piv / msk after the keys in LDS; 0: after the matrix in the slot
};

// bytes of the tables (order [n], inv [n], piv [rank], then msk [n] u64 when the method searches), 8-aligned
__host__ __device__ inline size_t osdw_table_bytes(int n, int rank, bool search)
{
    const size_t b = (sizeof(int) * (size_t)(2 * n + rank) + 7) & ~(size_t)7;
    return search ? b + sizeof(unsigned long long) * (size_t)n : b;
}
// LDS: keys [NP] u64, the pivot row [W] u32 (8-aligned), wave_best [NW] u64, wave_pos [NW] int + |T|, then the tables if they fit
__host__ __device__ inline size_t osdw_lds_fixed(int NP, int W)
{
    return sizeof(unsigned long long) * (size_t)NP + (((size_t)W * sizeof(unsigned) + 7) & ~(size_t)7) +
           sizeof(unsigned long long) * OSDW_NW + sizeof(int) * (OSDW_NW + 2);
}
__host__ __device__ inline size_t osdw_mat_bytes(int W, int RS) { return sizeof(unsigned) * (size_t)W * RS; }

__global__ void __launch_bounds__(OSDW_T) osd_ws_kernel(GraphDev g, OsdWsArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, T = OSDW_T, lane = tid & 63, wave = tid >> 6;
    const int n = g.n, rank = a.rank, W = a.W, RS = a.RS;
    const bool search = a.method != FGNN_OSD_0;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    unsigned* prow = reinterpret_cast<unsigned*>(keys + a.NP);
    unsigned long long* wave_best = reinterpret_cast<unsigned long long*>(smem + sizeof(unsigned long long) * (size_t)a.NP +
                                                                          ((W * sizeof(unsigned) + 7) & ~(size_t)7));
    int* wave_pos = reinterpret_cast<int*>(wave_best + OSDW_NW);
    int* tcount = wave_pos + OSDW_NW;
    unsigned* mat = reinterpret_cast<unsigned*>(a.ws + a.slot_bytes * blockIdx.x);
    unsigned char* tab = a.tables_in_lds ? smem + osdw_lds_fixed(a.NP, W) : a.ws + a.slot_bytes * blockIdx.x + osdw_mat_bytes(W, RS);
    int* order = reinterpret_cast<int*>(tab);
    int* inv = order + n;
    int* piv = inv + n;
    unsigned long long* msk = reinterpret_cast<unsigned long long*>(tab + osdw_table_bytes(n, rank, false));
    const int coff = a.side ? g.m_x : 0;
    const int ms = a.side ? g.m_z : g.m_x;
    const int nw = n >> 5;
    const unsigned nb = 1u << (n & 31);

    for (int t = blockIdx.x; t < a.count; t += gridDim.x) {
        const int b = a.index ? a.index[t] : t;
        // 1. reliabilities -> sortable keys (value, qubit), as osd_eliminate
        for (int v = tid; v < a.NP; v += T) {
            unsigned long long k = ~0ull;
            if (v < n) {
                float r;
                if (a.llr_bin) r = a.llr_bin[(size_t)b * n + v];
                else {
                    const float* mg = a.marg + (size_t)b * 3 * n;
                    const float X = mg[v], Y = mg[n + v], Z = mg[2 * n + v];
                    r = a.side == 0 ? vn_llr_z<VnMath>(X, Y, Z) : vn_llr_x<VnMath>(X, Y, Z);  // bp_osd.py:125-131
                }
                r = r + 0.0f;  // -0 -> +0
                k = ((unsigned long long)osd_sortable(r) << 32) | (unsigned)v;
            }
            keys[v] = k;
        }
        __syncthreads();
        // 2. bitonic sort (ascending; distinct keys, so the result is the stable order)
        for (int k2 = 2; k2 <= a.NP; k2 <<= 1)
            for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
                for (int i = tid; i < a.NP; i += T) {
                    const int ixj = i ^ j2;
                    if (ixj > i) {
                        const unsigned long long x = keys[i], y = keys[ixj];
                        const bool up = (i & k2) == 0;
                        if ((x > y) == up) { keys[i] = y; keys[ixj] = x; }
                    }
                }
                __syncthreads();
            }
        for (int j = tid; j < n; j += T) {
            const int v = (int)(unsigned)keys[j];
            order[j] = v;
            inv[v] = j;
        }
        for (size_t i = tid; i < (size_t)W * RS; i += T) mat[i] = 0u;
        uint8_t* eo = a.e_hat + (size_t)b * n;
        for (int v = tid; v < n; v += T) eo[v] = 0;
        __syncthreads();
        // 3. permuted, augmented, bit-packed rows: thread r owns row r
        for (int r = tid; r < rank; r += T) {
            const int c = a.pivot_rows[r];
            for (int jx = g.cptr[coff + c]; jx < g.cptr[coff + c + 1]; ++jx) {
                const int j = inv[g.cvn[jx]];
                mat[(size_t)(j >> 5) * RS + r] |= 1u << (j & 31);
            }
            if (a.synd[(size_t)b * ms + c] & 1) mat[(size_t)nw * RS + r] |= nb;
        }
        __syncthreads();
        // 4. row-by-row Gauss-Jordan: copy row r to LDS while the workgroup finds its first set bit, then every other row that holds
        //    the pivot column XORs the copy into its words pw..W-1
        for (int r = 0; r < rank; ++r) {
            int pos = 0x7fffffff;
            for (int w = tid; w < W; w += T) {
                const unsigned x = mat[(size_t)w * RS + r];
                prow[w] = x;
                if (x && pos == 0x7fffffff) pos = w * 32 + (__ffs((int)x) - 1);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const int other = __shfl_xor(pos, o);
                pos = other < pos ? other : pos;
            }
            if (lane == 0) wave_pos[wave] = pos;
            __syncthreads();
            pos = wave_pos[0];
            for (int i = 1; i < OSDW_NW; ++i) pos = wave_pos[i] < pos ? wave_pos[i] : pos;
            const int p = pos > n ? 0 : pos;  // all-zero row: tf.argmax returns 0
            if (tid == 0) piv[r] = p;
            if (pos <= n) {  // a zero row XORs nothing into anyone
                const int pw = p >> 5;
                const unsigned pm = 1u << (p & 31);
                for (int i = tid; i < rank; i += T)
                    if (i != r && (mat[(size_t)pw * RS + i] & pm)) {
                        unsigned* ri = mat + i;
#pragma unroll 4
                        for (int w = pw; w < W; ++w) ri[(size_t)w * RS] ^= prow[w];
                    }
            }
            __syncthreads();
        }
        if (!search) {
            // 5. OSD-0 output (osd0_kernel step 5): rows whose pivot bit is set
            for (int r = tid; r < rank; r += T) {
                const int p = piv[r];
                if (p < n && ((mat[(size_t)(p >> 5) * RS + r] >> (p & 31)) & 1u))
                    eo[order[p]] = (uint8_t)((mat[(size_t)nw * RS + r] & nb) ? 1 : 0);
            }
            if (tid == 0 && a.chosen) a.chosen[b] = 0;
            __syncthreads();
            continue;
        }
        // 5. pivot positions (osd_search_kernel step 5): pos[p] = 2 * row + (transformed syndrome bit of row) for a real pivot row
        unsigned* kw = reinterpret_cast<unsigned*>(keys);  // kw[2p] = T[p] (p < k), kw[2p + 1] = sortable(r_sorted[p])
        int* pos = inv;
        for (int p = tid; p < n; p += T) pos[p] = -1;
        __syncthreads();
        for (int r = tid; r < rank; r += T) {
            const int p = piv[r];
            if (p < n && ((mat[(size_t)(p >> 5) * RS + r] >> (p & 31)) & 1u))
                pos[p] = 2 * r + ((mat[(size_t)nw * RS + r] & nb) ? 1 : 0);
        }
        __syncthreads();
        // 6. T = the non-pivot positions in ascending order (one wave, ballot compaction)
        if (wave == 0) {
            int cnt = 0;
            for (int base = 0; base < n; base += 64) {
                const int p = base + lane;
                const bool isT = p < n && pos[p] < 0;
                const unsigned long long ball = __ballot(isT);
                if (isT) {
                    const int j = cnt + __popcll(ball & ((1ull << lane) - 1ull));
                    kw[2 * j] = (unsigned)p;
                    pos[p] = -(j + 1);
                }
                cnt += __popcll(ball);
            }
            if (lane == 0) *tcount = cnt;
        }
        __syncthreads();
        const int k = *tcount;
        const int lam = a.order < k ? a.order : k;
        const int ncand = a.order == 0 ? 1 : a.method == FGNN_OSD_E ? (1 << lam) : 1 + k + lam * (lam - 1) / 2;
        // 7. msk[p] = the bits of position p's solution that candidate bits over T[0..lam) flip: row bits on T[j] for a pivot row,
        //    bit j for p = T[j]
        for (int p = tid; p < n; p += T) {
            const int ip = pos[p];
            unsigned long long mm = 0ull;
            if (ip >= 0) {
                const int row = ip >> 1;
                for (int j = 0; j < lam; ++j) {
                    const int tc = (int)kw[2 * j];
                    mm |= (unsigned long long)((mat[(size_t)(tc >> 5) * RS + row] >> (tc & 31)) & 1u) << j;
                }
            } else if (-ip - 1 < lam) {
                mm = 1ull << (-ip - 1);
            }
            msk[p] = mm;
        }
        __syncthreads();
        // 8. the search.  The cost tree of fgnn.h over NP = 64 * 2^LV positions: its top LV levels pair positions of the same lane
        //    (p = lane + 64 m, pairs m, m + h), the last six pair lanes.  A lane's part is the halving tree over m, i.e. the pairwise
        //    (adjacent) tree over m in bit-reversed order: streamed with one pending partial sum per level, nothing indexed at run time.
        unsigned long long best = ~0ull;
        for (int c = wave; c < ncand; c += OSDW_NW) {
            unsigned long long cbits;
            int xc;
            osd_candidate(a.method, c, k, lam, cbits, xc);
            const int xt = xc >= 0 ? (int)kw[2 * xc] : 0;
            const unsigned* xcol = mat + (size_t)(xt >> 5) * RS;
            const int xs = xt & 31;
            float part[9];
#pragma unroll
            for (int l = 0; l < 9; ++l) part[l] = 0.0f;
            float v = 0.0f;
            const int npl = 1 << a.LV;
            for (int j = 0; j < npl; ++j) {
                const int m = a.LV ? (int)(__brev((unsigned)j) >> (32 - a.LV)) : 0;
                const int p = lane + 64 * m;
                v = 0.0f;
                if (p < n) {
                    const int ip = pos[p];
                    unsigned bit = (unsigned)__popcll(msk[p] & cbits) & 1u;
                    if (ip >= 0) {
                        bit ^= (unsigned)ip & 1u;
                        if (xc >= 0) bit ^= (xcol[ip >> 1] >> xs) & 1u;
                    } else if (ip == -(xc + 1)) {
                        bit ^= 1u;
                    }
                    if (bit) v = osd_unsortable(kw[2 * p + 1]);
                }
                bool open = true;
#pragma unroll
                for (int l = 0; l < 9; ++l)
                    if (open) {
                        if ((j >> l) & 1) v = part[l] + v;
                        else {
                            part[l] = v;
                            open = false;
                        }
                    }
            }
            float s = v;  // after j = npl - 1 every level has merged: the lane's total
#pragma unroll
            for (int h = 32; h >= 1; h >>= 1) s = s + __shfl_xor(s, h);
            const unsigned long long key = ((unsigned long long)osd_sortable(s) << 32) | (unsigned)c;
            best = key < best ? key : best;
        }
        if (lane == 0) wave_best[wave] = best;
        __syncthreads();
        unsigned long long wb = wave_best[0];
        for (int i = 1; i < OSDW_NW; ++i) wb = wave_best[i] < wb ? wave_best[i] : wb;
        const int cw = (int)(unsigned)wb;
        // 9. e_hat[b][order[p]] = bit p of the winner's solution
        unsigned long long cbits;
        int xc;
        osd_candidate(a.method, cw, k, lam, cbits, xc);
        const int xt = xc >= 0 ? (int)kw[2 * xc] : 0;
        for (int p = tid; p < n; p += T) {
            const int ip = pos[p];
            unsigned bit;
            if (ip >= 0) {
                const int row = ip >> 1;
                bit = (unsigned)ip & 1u;
                for (unsigned long long cb = cbits; cb; cb &= cb - 1ull) {
                    const int tc = (int)kw[2 * (__ffsll((long long)cb) - 1)];
                    bit ^= (mat[(size_t)(tc >> 5) * RS + row] >> (tc & 31)) & 1u;
                }
                if (xc >= 0) bit ^= (mat[(size_t)(xt >> 5) * RS + row] >> (xt & 31)) & 1u;
            } else {
                const int j = -ip - 1;
                bit = (j < 64 && ((cbits >> j) & 1ull)) || j == xc ? 1u : 0u;
            }
            eo[order[p]] = (uint8_t)bit;
        }
        if (tid == 0 && a.chosen) a.chosen[b] = cw;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) compact_u8_kernel(const uint8_t* __restrict__ mask, uint8_t bit, int B, int* __restrict__ index,
                                                         int* __restrict__ count)
{
    __shared__ int base;
    __shared__ int wsum[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = (i < B) && (mask[i] & bit);
    const unsigned long long ball = __ballot(on);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) wsum[wave] = __popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        base = tot ? atomicAdd(count, tot) : 0;
    }
    __syncthreads();
    if (on) {
        int off = base + __popcll(ball & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) off += wsum[w];
        index[off] = i;
    }
}

}  // namespace

extern "C" int fgnn_graph_set_basis(fgnn_graph* g, int side, int rank, const int32_t* pivot_rows)
{
    if (!g || side < 0 || side > 1 || rank <= 0 || !pivot_rows) return fgnn_fail(FGNN_ERR_ARG, "bad basis arguments");
    const int ms = side ? g->d.m_z : g->d.m_x;
    for (int r = 0; r < rank; ++r)
        if (pivot_rows[r] < 0 || pivot_rows[r] >= ms) return fgnn_fail(FGNN_ERR_ARG, "pivot row out of range");
    FGNN_DEVICE_GUARD(g->device);
    if (g->basis_dev[side]) (void)hipFree(g->basis_dev[side]);
    g->basis_dev[side] = nullptr;
    FGNN_HIP_CHECK(hipMalloc(&g->basis_dev[side], sizeof(int) * (size_t)rank));
    FGNN_HIP_CHECK(hipMemcpy(g->basis_dev[side], pivot_rows, sizeof(int) * (size_t)rank, hipMemcpyHostToDevice));
    g->basis_rank[side] = rank;
    return FGNN_OK;
}

// the method / order limits of fgnn_osd and fgnn_osd_ws
static int osd_check_method(int method, int order)
{
    if (method != FGNN_OSD_0 && method != FGNN_OSD_E && method != FGNN_OSD_CS) return fgnn_fail(FGNN_ERR_ARG, "unknown OSD method");
    if (order < 0) return fgnn_fail(FGNN_ERR_ARG, "OSD order must be >= 0");
    if (method == FGNN_OSD_E && order > 16) return fgnn_fail(FGNN_ERR_ARG, "osd_e supports order <= 16");
    if (method == FGNN_OSD_CS && order > 64) return fgnn_fail(FGNN_ERR_ARG, "osd_cs supports order <= 64");
    return FGNN_OK;
}

// The shape limits of the LDS-resident kernels (osd0_kernel; osd_search_kernel with scratch = OSD_SEARCH_SCRATCH): null if they take
// n columns and `rank` basis rows — with the row words W, stride WS, sort size NP and LDS bytes — else the message of the refusal.
// osd_prepare and fgnn_osd_resident both ask here.
static const char* osd_lds_refusal(int n, int rank, size_t scratch, int& W, int& WS, int& NP, size_t& lds)
{
    W = (n + 1 + 31) / 32;
    if (W > 64) return "OSD kernel supports n <= 2047";
    WS = W | 1;  // odd stride: row-per-thread accesses hit distinct LDS banks
    NP = 1;
    while (NP < n) NP <<= 1;
    lds = osd_lds_bytes(n, rank, WS, NP);
    if (scratch) lds = ((lds + 7) & ~(size_t)7) + scratch;
    if (lds > FGNN_LDS_BUDGET) return "code too large for the LDS-resident OSD kernel";
    return nullptr;
}

// The argument checks and launch parameters shared by fgnn_osd0 and fgnn_osd.  count = samples to process (0: nothing to launch);
// lds = the OSD-0 layout, plus `scratch` bytes after it rounded up to 8 when scratch > 0.
static int osd_prepare(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
                       const int32_t* index, int nact, uint8_t* e_hat, size_t scratch, OsdArgs& a, size_t& lds, int& count)
{
    count = 0;
    if (!g || side < 0 || side > 1) return fgnn_fail(FGNN_ERR_ARG, "bad OSD arguments");
    if (!g->basis_dev[side]) return fgnn_fail(FGNN_ERR_STATE, "row basis not installed (fgnn_graph_set_basis)");
    if ((!marg && !llr_bin) || !synd || !e_hat || B < 0) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    const int cnt = index ? nact : B;
    if (cnt <= 0) return FGNN_OK;
    a = OsdArgs{};
    a.side = side;
    a.rank = g->basis_rank[side];
    a.B = B;
    a.nact = nact;
    const char* refusal = osd_lds_refusal(g->d.n, a.rank, scratch, a.W, a.WS, a.NP, lds);
    if (refusal) return fgnn_fail(FGNN_ERR_ARG, refusal);
    a.pivot_rows = static_cast<const int*>(g->basis_dev[side]);
    a.marg = marg;
    a.llr_bin = llr_bin;
    a.synd = synd;
    a.index = index;
    a.e_hat = e_hat;
    count = cnt;
    return FGNN_OK;
}

extern "C" int fgnn_osd0(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
                         const int32_t* index, int nact, uint8_t* e_hat, void* stream)
{
    OsdArgs a;
    size_t lds;
    int count;
    const int rc = osd_prepare(g, side, marg, llr_bin, synd, B, index, nact, e_hat, 0, a, lds, count);
    if (rc != FGNN_OK || count == 0) return rc;
    FGNN_DEVICE_GUARD(g->device);
    return fgnn_launch(osd0_kernel, dim3(count), dim3(256), lds, static_cast<hipStream_t>(stream), g->d, a);
}

extern "C" int fgnn_osd(const fgnn_graph* g, int side, int method, int order, const float* marg, const float* llr_bin, const uint8_t* synd,
                        int B, const int32_t* index, int nact, uint8_t* e_hat, int32_t* chosen, void* stream)
{
    const int mc = osd_check_method(method, order);
    if (mc != FGNN_OK) return mc;
    OsdArgs a;
    size_t lds;
    int count;
    const int rc = osd_prepare(g, side, marg, llr_bin, synd, B, index, nact, e_hat, OSD_SEARCH_SCRATCH, a, lds, count);
    if (rc != FGNN_OK || count == 0) return rc;
    a.chosen = chosen;
    a.method = method;
    a.order = method == FGNN_OSD_0 ? 0 : order;
    FGNN_DEVICE_GUARD(g->device);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    switch ((a.NP > 64 ? a.NP : 64) / 64) {
    case 1: return fgnn_launch(osd_search_kernel<1>, dim3(count), dim3(256), lds, st, g->d, a);
    case 2: return fgnn_launch(osd_search_kernel<2>, dim3(count), dim3(256), lds, st, g->d, a);
    case 4: return fgnn_launch(osd_search_kernel<4>, dim3(count), dim3(256), lds, st, g->d, a);
    case 8: return fgnn_launch(osd_search_kernel<8>, dim3(count), dim3(256), lds, st, g->d, a);
    case 16: return fgnn_launch(osd_search_kernel<16>, dim3(count), dim3(256), lds, st, g->d, a);
    default: return fgnn_launch(osd_search_kernel<32>, dim3(count), dim3(256), lds, st, g->d, a);
    }
}

extern "C" int fgnn_osd_resident(const fgnn_graph* g, int side, int method, int* fits)
{
    if (method != FGNN_OSD_0 && method != FGNN_OSD_E && method != FGNN_OSD_CS) return fgnn_fail(FGNN_ERR_ARG, "unknown OSD method");
    if (!g || side < 0 || side > 1 || !fits) return fgnn_fail(FGNN_ERR_ARG, "bad OSD arguments");
    if (!g->basis_dev[side]) return fgnn_fail(FGNN_ERR_STATE, "row basis not installed (fgnn_graph_set_basis)");
    int W, WS, NP;
    size_t lds;
    *fits = osd_lds_refusal(g->d.n, g->basis_rank[side], method == FGNN_OSD_0 ? 0 : OSD_SEARCH_SCRATCH, W, WS, NP, lds) ? 0 : 1;
    return FGNN_OK;
}

// Shape of the workspace kernel for side `side`: words per row W, padded row count RS, sort size NP, tree depth LV; bytes of one slot
// and the LDS of one workgroup, the tables placed in LDS when they fit.
struct OsdWsShape {
    int W, RS, NP, LV, tables_in_lds;
    size_t slot_bytes, lds;
};

static int osd_ws_shape(const fgnn_graph* g, int side, int method, OsdWsShape& sh)
{
    if (!g || side < 0 || side > 1) return fgnn_fail(FGNN_ERR_ARG, "bad OSD arguments");
    if (!g->basis_dev[side]) return fgnn_fail(FGNN_ERR_STATE, "row basis not installed (fgnn_graph_set_basis)");
    const int n = g->d.n, rank = g->basis_rank[side];
    if (n > OSDW_MAX_N) return fgnn_fail(FGNN_ERR_ARG, "OSD workspace kernel supports n <= 16384");
    sh.W = (n + 1 + 31) / 32;
    sh.RS = (rank + 63) & ~63;
    sh.NP = 1;
    while (sh.NP < n) sh.NP <<= 1;
    sh.LV = 0;
    while ((64 << sh.LV) < sh.NP) ++sh.LV;
    const size_t tables = osdw_table_bytes(n, rank, method != FGNN_OSD_0);
    const size_t fixed = osdw_lds_fixed(sh.NP, sh.W);
    sh.tables_in_lds = fixed + tables <= FGNN_LDS_BUDGET;
    sh.lds = sh.tables_in_lds ? fixed + tables : fixed;
    sh.slot_bytes = (osdw_mat_bytes(sh.W, sh.RS) + tables + 255) & ~(size_t)255;
    return FGNN_OK;
}

extern "C" int fgnn_osd_workspace_bytes(const fgnn_graph* g, int side, int method, int order, int slots, size_t* bytes)
{
    const int rc = osd_check_method(method, order);
    if (rc != FGNN_OK) return rc;
    if (!bytes || slots < 1) return fgnn_fail(FGNN_ERR_ARG, "bad OSD workspace arguments");
    OsdWsShape sh;
    const int rs = osd_ws_shape(g, side, method, sh);
    if (rs != FGNN_OK) return rs;
    *bytes = sh.slot_bytes * (size_t)slots;
    return FGNN_OK;
}

extern "C" int fgnn_osd_ws(const fgnn_graph* g, int side, int method, int order, const float* marg, const float* llr_bin,
                           const uint8_t* synd, int B, const int32_t* index, int nact, uint8_t* e_hat, int32_t* chosen, void* workspace,
                           size_t workspace_bytes, void* stream)
{
    int rc = osd_check_method(method, order);
    if (rc != FGNN_OK) return rc;
    if (!workspace) return fgnn_fail(FGNN_ERR_ARG, "OSD workspace is NULL");
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return fgnn_fail(FGNN_ERR_ARG, "OSD workspace must be 8-byte aligned");
    OsdWsShape sh;
    rc = osd_ws_shape(g, side, method, sh);
    if (rc != FGNN_OK) return rc;
    if ((!marg && !llr_bin) || !synd || !e_hat || B < 0 || (index && nact < 0)) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    if (workspace_bytes < sh.slot_bytes)
        return fgnn_fail(FGNN_ERR_ARG, "OSD workspace too small: one slot needs " + std::to_string(sh.slot_bytes) + " bytes");
    const int count = index ? nact : B;
    if (count <= 0) return FGNN_OK;
    const size_t slots = workspace_bytes / sh.slot_bytes;
    OsdWsArgs a{};
    a.side = side;
    a.rank = g->basis_rank[side];
    a.B = B;
    a.W = sh.W;
    a.RS = sh.RS;
    a.NP = sh.NP;
    a.LV = sh.LV;
    a.pivot_rows = static_cast<const int*>(g->basis_dev[side]);
    a.marg = marg;
    a.llr_bin = llr_bin;
    a.synd = synd;
    a.index = index;
    a.count = count;
    a.e_hat = e_hat;
    a.chosen = chosen;
    a.method = method;
    a.order = method == FGNN_OSD_0 ? 0 : order;
    a.ws = static_cast<unsigned char*>(workspace);
    a.slot_bytes = sh.slot_bytes;
    a.tables_in_lds = sh.tables_in_lds;
    const int grid = (size_t)count < slots ? count : (int)slots;
    FGNN_DEVICE_GUARD(g->device);
    return fgnn_launch(osd_ws_kernel, dim3(grid), dim3(OSDW_T), sh.lds, static_cast<hipStream_t>(stream), g->d, a);
}

// index[0..count) = ids of the samples with (mask[b] & bit) != 0; *count must be zeroed by the caller (device int).
extern "C" int fgnn_compact(const uint8_t* mask, int bit, int B, int32_t* index, int32_t* count, void* stream)
{
    if (!count || B < 0 || bit <= 0 || bit > 255) return fgnn_fail(FGNN_ERR_ARG, "bad compact arguments");
    if (B == 0) return FGNN_OK;
    if (!mask || !index) return fgnn_fail(FGNN_ERR_ARG, "bad compact arguments");
    return fgnn_launch(compact_u8_kernel, dim3((B + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), mask, (uint8_t)bit, B,
                       index, count);
}
