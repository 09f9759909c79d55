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

namespace {

struct OsdArgs {
    int side, rank, B, nact, W, WS, NP;  // W words per row, WS padded row stride (odd), NP sort size (power of two)
    const int* pivot_rows;               // [rank] check ids (side-local) forming the row basis
    const float* marg;                   // [B,3,n] or null
    const float* llr_bin;                // [B,n] or null
    const uint8_t* synd;                 // [B,m_side]
    const int* index;                    // [nact] or null
    uint8_t* e_hat;                      // [B,n]
};

__global__ void __launch_bounds__(256) osd0_kernel(GraphDev g, OsdArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ unsigned char smem[];
    const int tid = threadIdx.x, T = 256;
    const int n = g.n, rank = a.rank, W = a.W, WS = a.WS;
    const int b = a.index ? a.index[blockIdx.x] : (int)blockIdx.x;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);     // [NP]
    unsigned* mat = reinterpret_cast<unsigned*>(keys + a.NP);                   // [rank][WS]
    int* order = reinterpret_cast<int*>(mat + (size_t)rank * WS);               // [n]
    int* inv = order + n;                                                       // [n]
    int* piv = inv + n;                                                         // [rank]

    // 1. reliabilities -> sortable 64-bit keys (value, qubit): ascending, ties by qubit index (stable)
    for (int v = tid; v < a.NP; v += T) {
        unsigned long long k = ~0ull;
        if (v < n) {
            float r;
            if (a.llr_bin) r = a.llr_bin[(size_t)b * n + v];
            else {
                const float* mg = a.marg + (size_t)b * 3 * n;
                const float X = mg[v], Y = mg[n + v], Z = mg[2 * n + v];
                r = a.side == 0 ? fg_softplus(-X) - fg_lse2(-Z, -Y) : fg_softplus(-Z) - fg_lse2(-X, -Y);  // bp_osd.py:125-131
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
    // 5. e_hat[order[pivot_r]] = transformed syndrome bit of row r (bp_osd.py:44-45, :68-69)
    for (int r = tid; r < rank; r += T) {
        const int p = piv[r];
        if (p < n) eo[order[p]] = (uint8_t)((mat[(size_t)r * WS + (n >> 5)] >> (n & 31)) & 1u);
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

extern "C" int fgnn_osd0(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
                         const int32_t* index, int nact, uint8_t* e_hat, void* stream)
{
    if (!g || side < 0 || side > 1) return fgnn_fail(FGNN_ERR_ARG, "bad OSD arguments");
    if (!g->basis_dev[side]) return fgnn_fail(FGNN_ERR_STATE, "row basis not installed (fgnn_graph_set_basis)");
    if ((!marg && !llr_bin) || !synd || !e_hat || B < 0) return fgnn_fail(FGNN_ERR_ARG, "required buffer is NULL");
    const int count = index ? nact : B;
    if (count <= 0) return FGNN_OK;
    FGNN_DEVICE_GUARD(g->device);
    OsdArgs a;
    a.side = side;
    a.rank = g->basis_rank[side];
    a.B = B;
    a.nact = nact;
    a.W = (g->d.n + 1 + 31) / 32;
    if (a.W > 64) return fgnn_fail(FGNN_ERR_ARG, "OSD kernel supports n <= 2047");
    a.WS = a.W | 1;  // odd stride: row-per-thread accesses hit distinct LDS banks
    a.NP = 1;
    while (a.NP < g->d.n) a.NP <<= 1;
    a.pivot_rows = static_cast<const int*>(g->basis_dev[side]);
    a.marg = marg;
    a.llr_bin = llr_bin;
    a.synd = synd;
    a.index = index;
    a.e_hat = e_hat;
    const size_t lds = sizeof(unsigned long long) * (size_t)a.NP + sizeof(unsigned) * (size_t)a.rank * a.WS +
                       sizeof(int) * (size_t)(2 * g->d.n + a.rank);
    if (lds > FGNN_LDS_BUDGET) return fgnn_fail(FGNN_ERR_ARG, "code too large for the LDS-resident OSD kernel");
    return fgnn_launch(osd0_kernel, dim3(count), dim3(256), lds, static_cast<hipStream_t>(stream), g->d, a);
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
