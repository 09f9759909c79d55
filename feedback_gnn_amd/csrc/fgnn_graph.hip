// fgnn_graph.hip — builds the device-resident Tanner-graph tables of a CSS code.
// Replaces the edge bookkeeping of QLDPCBPDecoder.__init__ (/root/reference
// sionna/fec/ldpc/decoding_q.py:53-94: scipy.sparse.find + argsort + ragged row splits) and of
// Feedback_GNN.create_edges (feedback_gnn.py:87-108) by one CSC + one CSR view per parity-check matrix.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <optional>

#include "fgnn_internal.h"

static thread_local std::string g_err;
void fgnn_set_error(const std::string& s) { g_err = s; }
int fgnn_fail(int code, const std::string& s)
{
    g_err = s;
    return code;
}
extern "C" const char* fgnn_last_error(void) { return g_err.c_str(); }
// 1: rounds 1-2.  2: round 3 — fgnn_bp4_decode_trace, fgnn_gnnbp4_weights_create_general / _workspace_bytes, options 4 and 5 (both
// default on: the operation sequence of the GNN message layers and of the BP4 qubit update changed), empty batches take NULL buffers.
extern "C" int fgnn_version(void) { return 2; }

namespace {

template <typename T>
int upload(fgnn_graph* g, const std::vector<T>& h, const T** dst)
{
    if (g->host_only) {  // fgnn_check_rows: the tables are built and kept on the host, no device is touched
        *dst = nullptr;
        return FGNN_OK;
    }
    void* p = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    FGNN_HIP_CHECK(hipMalloc(&p, bytes));
    g->allocs.push_back(p);
    if (!h.empty()) FGNN_HIP_CHECK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = static_cast<const T*>(p);
    return FGNN_OK;
}

// COO -> CSR with ascending columns inside each row
void coo_to_csr(int rows, int nnz, const int32_t* r, const int32_t* c, std::vector<int>& ptr, std::vector<int>& col)
{
    std::vector<int> order(nnz);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return r[a] != r[b] ? r[a] < r[b] : c[a] < c[b]; });
    ptr.assign(rows + 1, 0);
    col.resize(nnz);
    for (int i = 0; i < nnz; ++i) {
        ptr[r[order[i]] + 1]++;
        col[i] = c[order[i]];
    }
    for (int i = 0; i < rows; ++i) ptr[i + 1] += ptr[i];
}

int uniform_degree(const std::vector<int>& ptr)
{
    if (ptr.size() < 2) return 0;
    int d = ptr[1] - ptr[0];
    for (size_t i = 1; i + 1 < ptr.size(); ++i)
        if (ptr[i + 1] - ptr[i] != d) return 0;
    return d;
}

void default_launch(fgnn_graph* g)
{
    // One thread per node-slot; a codeword gets ceil(nodes / npt) threads with npt chosen so that a
    // workgroup stays <= 512 threads where possible (several workgroups per CU hide each other's
    // barriers).  Small codes pack several codewords into one workgroup.
    const int nodes = std::max(g->d.n, g->d.m);
    int tpc = nodes;
    int cpb = 1;
    if (nodes >= 256) {
        // 4 waves = one per SIMD; ~7 workgroups of [[882,24]] fit a CU's LDS and cover each other's barriers
        // (measured on MI355X: 256 beats 448/512/1024 by 6-20 %; wave counts that are not a multiple of 4
        // load the SIMDs unevenly)
        tpc = 256;
    } else if (tpc >= 64) {
        tpc = (tpc + 63) / 64 * 64;
    } else {
        int p2 = 1;
        while (p2 < tpc) p2 <<= 1;
        tpc = p2;
        cpb = 256 / tpc;
    }
    g->tpc = tpc;
    g->cpb = cpb;
}

}  // namespace

LaunchGeom fgnn_geom(const fgnn_graph* g, int B)
{
    LaunchGeom L;
    L.tpc = g->tpc;
    L.cpb = g->cpb;
    // fewer codewords than CUs (a compacted feedback round at low p): the launch is pure latency, so a codeword gets a thread per
    // node instead of one per four — same arithmetic, the kernels index by threads-per-codeword
    if (!g->user_launch && g->cpb == 1 && B <= 256) {
        const int nodes = std::max(g->d.n, g->d.m);
        L.tpc = std::min(1024, std::max(g->tpc, (nodes + 63) / 64 * 64));
    }
    L.threads = L.tpc * L.cpb;
    L.blocks = (B + g->cpb - 1) / g->cpb;
    return L;
}

// fgnn_graph_create; host_only: build every table on the host and upload none (fgnn_check_rows)
static int graph_build(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                       const int32_t* chk_z, const int32_t* var_z, int device, bool host_only, fgnn_graph** out)
{
    if (!out) return fgnn_fail(FGNN_ERR_ARG, "out is NULL");
    if (n <= 0 || m_x <= 0 || m_z <= 0 || nnz_x <= 0 || nnz_z <= 0)
        return fgnn_fail(FGNN_ERR_ARG, "n, m_x, m_z and the edge counts must be positive");
    const int32_t* chk[2] = {chk_x, chk_z};
    const int32_t* var[2] = {var_x, var_z};
    const int nnz[2] = {nnz_x, nnz_z};
    const int m[2] = {m_x, m_z};
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < nnz[s]; ++i)
            if (chk[s][i] < 0 || chk[s][i] >= m[s] || var[s][i] < 0 || var[s][i] >= n)
                return fgnn_fail(FGNN_ERR_ARG, "edge index out of range");
    std::optional<fgnn_device_guard> dev_guard;
    if (!host_only) {
        dev_guard.emplace(device);
        if (dev_guard->err != hipSuccess)
            return fgnn_fail(FGNN_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dev_guard->err));
    }
    fgnn_graph* g = new fgnn_graph();
    g->host_only = host_only;
    std::memset(&g->d, 0, sizeof(g->d));
    std::memset(g->row_alloc, 0, sizeof(g->row_alloc));
    g->device = device;
    g->user_launch = false;
    GraphDev& d = g->d;
    d.n = n;
    d.m_x = m_x;
    d.m_z = m_z;
    d.m = m_x + m_z;
    d.E_x = nnz_x;
    d.E_z = nnz_z;
    d.E = nnz_x + nnz_z;

    std::vector<int> vptr[2], vchk_side[2];
    for (int s = 0; s < 2; ++s) {
        coo_to_csr(n, nnz[s], var[s], chk[s], vptr[s], vchk_side[s]);  // rows = qubits
        for (int v = 0; v < n; ++v)
            for (int e = vptr[s][v]; e + 1 < vptr[s][v + 1]; ++e)
                if (vchk_side[s][e] == vchk_side[s][e + 1]) {
                    delete g;
                    return fgnn_fail(FGNN_ERR_ARG, "duplicate edge");
                }
        g->h_chk[s] = std::vector<int32_t>(vchk_side[s].begin(), vchk_side[s].end());
        g->h_var[s].resize(nnz[s]);
        for (int v = 0; v < n; ++v)
            for (int e = vptr[s][v]; e < vptr[s][v + 1]; ++e) g->h_var[s][e] = v;
    }
    // combined VN-major check ids and slot offsets
    std::vector<int> vptr_x = vptr[0], vptr_z = vptr[1], vchk(d.E);
    for (auto& x : vptr_z) x += d.E_x;
    std::copy(vchk_side[0].begin(), vchk_side[0].end(), vchk.begin());
    std::copy(vchk_side[1].begin(), vchk_side[1].end(), vchk.begin() + d.E_x);
    // combined CN-major view
    std::vector<int> cptr(d.m + 1, 0), cslot(d.E), cvn(d.E);
    {
        std::vector<int> deg(d.m, 0);
        for (int s = 0; s < 2; ++s)
            for (int i = 0; i < nnz[s]; ++i) deg[(s ? m_x : 0) + chk[s][i]]++;
        for (int c = 0; c < d.m; ++c) cptr[c + 1] = cptr[c] + deg[c];
        std::vector<int> fill(d.m, 0);
        // walking qubits in ascending order fills every check's list in ascending qubit order
        for (int s = 0; s < 2; ++s)
            for (int v = 0; v < n; ++v)
                for (int e = vptr[s][v]; e < vptr[s][v + 1]; ++e) {
                    int c = (s ? m_x : 0) + vchk_side[s][e];
                    int pos = cptr[c] + fill[c]++;
                    cslot[pos] = e + (s ? d.E_x : 0);
                    cvn[pos] = v;
                }
    }
    d.dvx = uniform_degree(vptr[0]);
    d.dvz = uniform_degree(vptr[1]);
    d.dc = uniform_degree(cptr);
    d.max_vdeg = 0;
    for (int v = 0; v < n; ++v)
        d.max_vdeg = std::max(d.max_vdeg, (vptr[0][v + 1] - vptr[0][v]) + (vptr[1][v + 1] - vptr[1][v]));
    d.max_cdeg = d.max_cdeg_x = 0;
    for (int c = 0; c < d.m; ++c) {
        d.max_cdeg = std::max(d.max_cdeg, cptr[c + 1] - cptr[c]);
        if (c < m_x) d.max_cdeg_x = std::max(d.max_cdeg_x, cptr[c + 1] - cptr[c]);
    }
    int rc;
    if (d.dvx > 0 && d.dvz > 0 && d.dc > 0 && d.dc <= 8 && (long long)d.E * 4 < 65536) {
        // BYTE offsets of the slots (slot * 4): a check's LDS addresses are then one mask / shift away from the packed row
        std::vector<uint16_t> pk((size_t)d.m * 8, 0);
        for (int c = 0; c < d.m; ++c)
            for (int j = 0; j < d.dc; ++j) pk[(size_t)c * 8 + j] = (uint16_t)(4 * cslot[cptr[c] + j]);
        if ((rc = upload(g, pk, &d.cslot16))) {
            fgnn_graph_destroy(g);
            return rc;
        }
        // the same offsets as 32-bit values, one row of 8 per check: what an LDS instruction takes as its address operand when the
        // message area starts at the base of the dynamic LDS (the base is the instruction's immediate offset) — no unpack in the loop
        std::vector<uint32_t> wide((size_t)d.m * 8, 0);
        for (size_t i = 0; i < wide.size(); ++i) wide[i] = pk[i];
        g->h_cslot32 = wide;
        if ((rc = upload(g, wide, &d.cslot32))) {
            fgnn_graph_destroy(g);
            return rc;
        }
    }
    if (d.dc > 0 && d.dc <= 8 && n < 65536) {
        // a check's qubits as one 16-byte row: the byte kernels and the fused flag test read it with one load
        std::vector<uint16_t> qv((size_t)d.m * 8, 0);
        for (int c = 0; c < d.m; ++c)
            for (int j = 0; j < d.dc; ++j) qv[(size_t)c * 8 + j] = (uint16_t)cvn[cptr[c] + j];
        g->h_cvn16 = qv;
        if ((rc = upload(g, qv, &d.cvn16))) {
            fgnn_graph_destroy(g);
            return rc;
        }
    }
    if ((rc = upload(g, vptr_x, &d.vptr_x)) || (rc = upload(g, vptr_z, &d.vptr_z)) || (rc = upload(g, vchk, &d.vchk)) ||
        (rc = upload(g, cptr, &d.cptr)) || (rc = upload(g, cslot, &d.cslot)) || (rc = upload(g, cvn, &d.cvn))) {
        fgnn_graph_destroy(g);
        return rc;
    }
    default_launch(g);
    *out = g;
    return FGNN_OK;
}

extern "C" int fgnn_graph_create(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x,
                                 int nnz_z, const int32_t* chk_z, const int32_t* var_z, int device, fgnn_graph** out)
{
    return graph_build(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, device, false, out);
}

extern "C" void fgnn_graph_destroy(fgnn_graph* g)
{
    if (!g) return;
    if (g->host_only) {
        delete g;
        return;
    }
    fgnn_device_guard _dg(g->device);
    for (hipEvent_t e : g->prof_ev) (void)hipEventDestroy(e);
    for (void* p : g->basis_dev)
        if (p) (void)hipFree(p);
    for (void* p : g->layer_alloc)
        if (p) (void)hipFree(p);
    for (void* p : g->bit_layer_alloc)
        if (p) (void)hipFree(p);
    for (void* p : g->qubit_layer_alloc)
        if (p) (void)hipFree(p);
    for (void* p : g->si_alloc)
        if (p) (void)hipFree(p);
    for (void* p : g->allocs) (void)hipFree(p);
    for (auto& r : g->row_alloc)
        for (void* p : r)
            if (p) (void)hipFree(p);
    delete g;
}

extern "C" int fgnn_graph_set_rows(fgnn_graph* g, int which, int rows, int nnz, const int32_t* row, const int32_t* col)
{
    if (!g || which < 0 || which > 5 || rows < 0 || nnz < 0) return fgnn_fail(FGNN_ERR_ARG, "bad row-set arguments");
    for (int i = 0; i < nnz; ++i)
        if (row[i] < 0 || row[i] >= rows || col[i] < 0 || col[i] >= g->d.n)
            return fgnn_fail(FGNN_ERR_ARG, "row-set index out of range");
    FGNN_DEVICE_GUARD(g->device);
    std::vector<int> ptr, c;
    coo_to_csr(rows, nnz, row, col, ptr, c);
    for (void*& p : g->row_alloc[which])
        if (p) {
            (void)hipFree(p);
            p = nullptr;
        }
    void *dp = nullptr, *dc = nullptr;
    FGNN_HIP_CHECK(hipMalloc(&dp, ptr.size() * sizeof(int)));
    g->row_alloc[which][0] = dp;
    FGNN_HIP_CHECK(hipMalloc(&dc, std::max<size_t>(c.size(), 1) * sizeof(int)));
    g->row_alloc[which][1] = dc;
    FGNN_HIP_CHECK(hipMemcpy(dp, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    if (!c.empty()) FGNN_HIP_CHECK(hipMemcpy(dc, c.data(), c.size() * sizeof(int), hipMemcpyHostToDevice));
    g->d.rows[which] = rows;
    g->d.rptr[which] = static_cast<const int*>(dp);
    g->d.rcol[which] = static_cast<const int*>(dc);
    if (which < 2) {  // column-major copy for the backward pass
        const int n = g->d.n;
        std::vector<int> tp(n + 1, 0), tr(std::max<size_t>(c.size(), 1), 0);
        for (int x : c) tp[x + 1]++;
        for (int v = 0; v < n; ++v) tp[v + 1] += tp[v];
        std::vector<int> fill(tp.begin(), tp.end() - 1);
        for (int r = 0; r < rows; ++r)
            for (int p = ptr[r]; p < ptr[r + 1]; ++p) tr[fill[c[p]]++] = r;
        void *tpd = nullptr, *trd = nullptr;
        FGNN_HIP_CHECK(hipMalloc(&tpd, tp.size() * sizeof(int)));
        g->row_alloc[which][2] = tpd;
        FGNN_HIP_CHECK(hipMalloc(&trd, tr.size() * sizeof(int)));
        g->row_alloc[which][3] = trd;
        FGNN_HIP_CHECK(hipMemcpy(tpd, tp.data(), tp.size() * sizeof(int), hipMemcpyHostToDevice));
        FGNN_HIP_CHECK(hipMemcpy(trd, tr.data(), tr.size() * sizeof(int), hipMemcpyHostToDevice));
        g->d.tptr[which] = static_cast<const int*>(tpd);
        g->d.trow[which] = static_cast<const int*>(trd);
    }
    return FGNN_OK;
}

extern "C" int fgnn_graph_set_launch(fgnn_graph* g, int threads_per_codeword, int codewords_per_block)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (threads_per_codeword <= 0 && codewords_per_block <= 0) {
        default_launch(g);
        g->user_launch = false;
        return FGNN_OK;
    }
    int tpc = threads_per_codeword > 0 ? threads_per_codeword : g->tpc;
    int cpb = codewords_per_block > 0 ? codewords_per_block : 1;
    if (tpc * cpb > 1024 || (tpc * cpb) % 64 != 0)
        return fgnn_fail(FGNN_ERR_ARG, "threads_per_codeword*codewords_per_block must be a multiple of 64 and <= 1024");
    g->tpc = tpc;
    g->cpb = cpb;
    g->user_launch = true;
    return FGNN_OK;
}

extern "C" int fgnn_graph_set_option(fgnn_graph* g, int option, int value)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    switch (option) {
    case FGNN_OPT_SATURATION_SHORTCUT: g->shortcut = value != 0; return FGNN_OK;
    case FGNN_OPT_FIXED_POINT_EXIT: g->early_exit = value != 0; return FGNN_OK;
    case FGNN_OPT_HW_TRANSCENDENTALS: g->hw_transcendentals = value != 0; return FGNN_OK;
    case FGNN_OPT_GNN_FACTORED: g->gnn_factored = value != 0; return FGNN_OK;
    case FGNN_OPT_BP4_SHARED_LSE: g->bp4_shared_lse = value != 0; return FGNN_OK;
    case FGNN_OPT_GNN_STREAM:
        if (value < 0 || value > 2) return fgnn_fail(FGNN_ERR_ARG, "FGNN_OPT_GNN_STREAM takes 0, 1 or 2");
        g->gnn_stream = value;
        return FGNN_OK;
    default: return fgnn_fail(FGNN_ERR_ARG, "unknown option");
    }
}

// testing hook: force the runtime-degree kernel on regular graphs (both paths must give the same bits)
extern "C" int fgnn_graph_force_generic(fgnn_graph* g, int on)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    g->force_generic = on != 0;
    return FGNN_OK;
}

extern "C" int fgnn_graph_info(const fgnn_graph* g, int32_t info[16])
{
    if (!g || !info) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    std::memset(info, 0, 16 * sizeof(int32_t));
    info[0] = g->d.n;
    info[1] = g->d.m_x;
    info[2] = g->d.m_z;
    info[3] = g->d.E_x;
    info[4] = g->d.E_z;
    info[5] = g->tpc;
    info[6] = g->cpb;
    info[7] = (int)((size_t)g->cpb * (size_t)(g->d.E + 3 * g->d.n) * sizeof(float));
    info[8] = (g->d.dvx > 0 && g->d.dvz > 0 && g->d.dc > 0) ? 1 : 0;
    info[9] = g->device;
    info[10] = g->d.dvx;
    info[11] = g->d.dvz;
    info[12] = g->d.dc;
    return FGNN_OK;
}

extern "C" int fgnn_graph_edges(const fgnn_graph* g, int side, int32_t* chk, int32_t* var)
{
    if (!g || side < 0 || side > 1 || !chk || !var) return fgnn_fail(FGNN_ERR_ARG, "bad arguments");
    std::copy(g->h_chk[side].begin(), g->h_chk[side].end(), chk);
    std::copy(g->h_var[side].begin(), g->h_var[side].end(), var);
    return FGNN_OK;
}

extern "C" int fgnn_check_rows(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                               const int32_t* chk_z, const int32_t* var_z, int32_t have[2], uint32_t* cslot32, uint16_t* cvn16)
{
    if (!have) return fgnn_fail(FGNN_ERR_ARG, "have is NULL");
    fgnn_graph* g = nullptr;
    const int rc = graph_build(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, 0, true, &g);
    if (rc) return rc;
    have[0] = !g->h_cslot32.empty();
    have[1] = !g->h_cvn16.empty();
    if (cslot32) std::copy(g->h_cslot32.begin(), g->h_cslot32.end(), cslot32);
    if (cvn16) std::copy(g->h_cvn16.begin(), g->h_cvn16.end(), cvn16);
    fgnn_graph_destroy(g);
    return FGNN_OK;
}

// ---- layers of the serial schedule (fgnn_bp4_decode_layered) ------------------------------------------------------------------
namespace {

// the qubits of every check, hx checks 0..m_x-1 then hz checks m_x..m_x+m_z-1, in the order of the edge lists
int check_qubits(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z, const int32_t* chk_z,
                 const int32_t* var_z, std::vector<int>& ptr, std::vector<int>& vn)
{
    if (n <= 0 || m_x <= 0 || m_z <= 0 || nnz_x < 0 || nnz_z < 0) return fgnn_fail(FGNN_ERR_ARG, "n, m_x and m_z must be positive");
    if ((nnz_x && (!chk_x || !var_x)) || (nnz_z && (!chk_z || !var_z))) return fgnn_fail(FGNN_ERR_ARG, "edge list is NULL");
    const int32_t* chk[2] = {chk_x, chk_z};
    const int32_t* var[2] = {var_x, var_z};
    const int nnz[2] = {nnz_x, nnz_z}, mm[2] = {m_x, m_z}, base[2] = {0, m_x};
    const int m = m_x + m_z;
    ptr.assign(m + 1, 0);
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < nnz[s]; ++i) {
            if (chk[s][i] < 0 || chk[s][i] >= mm[s] || var[s][i] < 0 || var[s][i] >= n)
                return fgnn_fail(FGNN_ERR_ARG, "edge index out of range");
            ptr[base[s] + chk[s][i] + 1]++;
        }
    for (int c = 0; c < m; ++c) ptr[c + 1] += ptr[c];
    vn.resize(ptr[m]);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < nnz[s]; ++i) vn[fill[base[s] + chk[s][i]]++] = var[s][i];
    return FGNN_OK;
}

std::string check_name(int c, int m_x)
{
    return c < m_x ? "hx check " + std::to_string(c) : "hz check " + std::to_string(c - m_x) + " (number " + std::to_string(c) + ")";
}

void greedy_layers(int n, int m, const std::vector<int>& ptr, const std::vector<int>& vn, int32_t* layer_of, int32_t* num_layers)
{
    std::vector<std::vector<int>> at(n);  // the layers that hold a check of qubit v
    std::vector<int> seen;                // seen[l] == c + 1: layer l holds a check that shares a qubit with check c
    int L = 0;
    for (int c = 0; c < m; ++c) {
        for (int p = ptr[c]; p < ptr[c + 1]; ++p)
            for (int l : at[vn[p]]) seen[l] = c + 1;
        int l = 0;
        while (l < L && seen[l] == c + 1) ++l;
        if (l == L) {
            ++L;
            seen.push_back(0);
        }
        layer_of[c] = l;
        for (int p = ptr[c]; p < ptr[c + 1]; ++p) at[vn[p]].push_back(l);
    }
    *num_layers = L;
}

// bits: the layering of side 0 alone (fgnn_validate_bit_layers) — its checks are "check c" and what two of them share is a bit
int validate_layers(int n, int m_x, int m, const std::vector<int>& ptr, const std::vector<int>& vn, int num_layers, const int32_t* layer_of,
                    bool bits = false)
{
    const auto name = [&](int c) { return bits ? "check " + std::to_string(c) : check_name(c, m_x); };
    if (!layer_of) return fgnn_fail(FGNN_ERR_ARG, "layer_of is NULL");
    if (num_layers < 1) return fgnn_fail(FGNN_ERR_ARG, "num_layers = " + std::to_string(num_layers) + " must be >= 1");
    std::vector<int> count(num_layers, 0);
    for (int c = 0; c < m; ++c) {
        if (layer_of[c] < 0 || layer_of[c] >= num_layers)
            return fgnn_fail(FGNN_ERR_ARG, name(c) + " has layer " + std::to_string(layer_of[c]) + ", outside [0, " +
                                               std::to_string(num_layers) + ")");
        count[layer_of[c]]++;
    }
    for (int l = 0; l < num_layers; ++l)
        if (!count[l]) return fgnn_fail(FGNN_ERR_ARG, "layer " + std::to_string(l) + " is empty");
    // per qubit: the checks at it; stamp[l] = the last qubit with a check in layer l, owner[l] = that check: two in one layer collide
    std::vector<int> owner(num_layers, -1), stamp(num_layers, -1);
    std::vector<std::vector<int>> at(n);
    for (int c = 0; c < m; ++c)
        for (int p = ptr[c]; p < ptr[c + 1]; ++p) at[vn[p]].push_back(c);
    for (int v = 0; v < n; ++v)
        for (int c : at[v]) {
            const int l = layer_of[c];
            if (stamp[l] == v && owner[l] != c)
                return fgnn_fail(FGNN_ERR_ARG, name(owner[l]) + " and " + name(c) + " of layer " + std::to_string(l) +
                                                   (bits ? " share bit " : " share qubit ") + std::to_string(v));
            stamp[l] = v;
            owner[l] = c;
        }
    return FGNN_OK;
}

void free_layers(const fgnn_graph* g)
{
    for (void*& p : g->layer_alloc)
        if (p) {
            (void)hipFree(p);  // waits for the launches that read it
            p = nullptr;
        }
    g->num_layers = 0;
    g->h_layer_of.clear();
}

int install_layers(const fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    const GraphDev& d = g->d;
    std::vector<int> ptr, vn;
    int rc = check_qubits(d.n, d.m_x, d.m_z, d.E_x, g->h_chk[0].data(), g->h_var[0].data(), d.E_z, g->h_chk[1].data(),
                          g->h_var[1].data(), ptr, vn);
    if (rc) return rc;
    std::vector<int32_t> lay(d.m);
    if (!layer_of) {
        greedy_layers(d.n, d.m, ptr, vn, lay.data(), &num_layers);
    } else {
        if ((rc = validate_layers(d.n, d.m_x, d.m, ptr, vn, num_layers, layer_of))) return rc;
        std::copy(layer_of, layer_of + d.m, lay.begin());
    }
    // the device tables, from the graph's own check-major view: a check's edges in ascending qubit order, slot = VN-major message slot
    std::vector<int> cptr(d.m + 1, 0), cslot(d.E), cvn(d.E);
    {
        std::vector<int> vptr[2];
        for (int s = 0; s < 2; ++s) {
            vptr[s].assign(d.n + 1, 0);
            for (int v : g->h_var[s]) vptr[s][v + 1]++;
            for (int v = 0; v < d.n; ++v) vptr[s][v + 1] += vptr[s][v];
        }
        for (int s = 0; s < 2; ++s)
            for (int c : g->h_chk[s]) cptr[(s ? d.m_x : 0) + c + 1]++;
        for (int c = 0; c < d.m; ++c) cptr[c + 1] += cptr[c];
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int s = 0; s < 2; ++s)
            for (int e = 0; e < (s ? d.E_z : d.E_x); ++e) {  // the canonical lists are sorted by (qubit, check): slot e of the side
                const int pos = fill[(s ? d.m_x : 0) + g->h_chk[s][e]]++;
                cslot[pos] = e + (s ? d.E_x : 0);
                cvn[pos] = g->h_var[s][e];
            }
    }
    std::vector<int> lcptr(num_layers + 1, 0), lchk(d.m), leptr(num_layers + 1, 0), ledge((size_t)2 * d.E);
    for (int c = 0; c < d.m; ++c) lcptr[lay[c] + 1]++;
    for (int l = 0; l < num_layers; ++l) lcptr[l + 1] += lcptr[l];
    {
        std::vector<int> fill(lcptr.begin(), lcptr.end() - 1);
        for (int c = 0; c < d.m; ++c) lchk[fill[lay[c]]++] = c;
    }
    int ne = 0;
    for (int l = 0; l < num_layers; ++l) {
        for (int i = lcptr[l]; i < lcptr[l + 1]; ++i)
            for (int p = cptr[lchk[i]]; p < cptr[lchk[i] + 1]; ++p, ++ne) {
                ledge[2 * (size_t)ne] = cslot[p];
                ledge[2 * (size_t)ne + 1] = cvn[p];
            }
        leptr[l + 1] = ne;
    }
    fgnn_device_guard dg(g->device);
    if (dg.err != hipSuccess) return fgnn_fail(FGNN_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
    free_layers(g);
    const std::vector<int>* tabs[4] = {&lcptr, &lchk, &leptr, &ledge};
    for (int i = 0; i < 4; ++i) {
        const size_t bytes = std::max<size_t>(tabs[i]->size(), 2) * sizeof(int);
        hipError_t e = hipMalloc(&g->layer_alloc[i], bytes);
        if (e == hipSuccess && !tabs[i]->empty())
            e = hipMemcpy(g->layer_alloc[i], tabs[i]->data(), tabs[i]->size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            free_layers(g);
            return fgnn_fail(FGNN_ERR_HIP, std::string("uploading the layer tables: ") + hipGetErrorString(e));
        }
    }
    g->num_layers = num_layers;
    g->h_layer_of = lay;
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_greedy_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                  const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers)
{
    if (!layer_of || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "layer_of or num_layers is NULL");
    std::vector<int> ptr, vn;
    const int rc = check_qubits(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, ptr, vn);
    if (rc) return rc;
    greedy_layers(n, m_x + m_z, ptr, vn, layer_of, num_layers);
    return FGNN_OK;
}

extern "C" int fgnn_validate_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                    const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of)
{
    std::vector<int> ptr, vn;
    const int rc = check_qubits(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, ptr, vn);
    if (rc) return rc;
    return validate_layers(n, m_x, m_x + m_z, ptr, vn, num_layers, layer_of);
}

extern "C" int fgnn_graph_set_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_layers(g, num_layers, layer_of);
}

extern "C" int fgnn_graph_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    if (!g || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    *num_layers = g->num_layers;
    if (layer_of) std::copy(g->h_layer_of.begin(), g->h_layer_of.end(), layer_of);
    return FGNN_OK;
}

int fgnn_graph_ensure_layers(const fgnn_graph* g)
{
    if (g->num_layers > 0) return FGNN_OK;
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_layers(g, 0, nullptr);
}

// ---- layers of side 0 alone, for the binary serial schedule (fgnn_bp2_decode_layered) ----------------------------------------------
namespace {

// the bits of every check of one matrix, in the order of the edge list
int check_bits(int n, int m, int nnz, const int32_t* chk, const int32_t* var, std::vector<int>& ptr, std::vector<int>& vn)
{
    if (n <= 0 || m <= 0 || nnz < 0) return fgnn_fail(FGNN_ERR_ARG, "n and m must be positive");
    if (nnz && (!chk || !var)) return fgnn_fail(FGNN_ERR_ARG, "edge list is NULL");
    ptr.assign(m + 1, 0);
    for (int i = 0; i < nnz; ++i) {
        if (chk[i] < 0 || chk[i] >= m || var[i] < 0 || var[i] >= n) return fgnn_fail(FGNN_ERR_ARG, "edge index out of range");
        ptr[chk[i] + 1]++;
    }
    for (int c = 0; c < m; ++c) ptr[c + 1] += ptr[c];
    vn.resize(ptr[m]);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int i = 0; i < nnz; ++i) vn[fill[chk[i]]++] = var[i];
    return FGNN_OK;
}

// validates (a refused layering leaves the installed one in place), then replaces the two device tables
int install_bit_layers(const fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    const GraphDev& d = g->d;
    std::vector<int> ptr, vn;
    int rc = check_bits(d.n, d.m_x, d.E_x, g->h_chk[0].data(), g->h_var[0].data(), ptr, vn);
    if (rc) return rc;
    std::vector<int32_t> lay(d.m_x);
    if (!layer_of) {
        greedy_layers(d.n, d.m_x, ptr, vn, lay.data(), &num_layers);
    } else {
        if ((rc = validate_layers(d.n, d.m_x, d.m_x, ptr, vn, num_layers, layer_of, true))) return rc;
        std::copy(layer_of, layer_of + d.m_x, lay.begin());
    }
    std::vector<int> lcptr(num_layers + 1, 0), lchk(d.m_x);
    for (int c = 0; c < d.m_x; ++c) lcptr[lay[c] + 1]++;
    for (int l = 0; l < num_layers; ++l) lcptr[l + 1] += lcptr[l];
    std::vector<int> fill(lcptr.begin(), lcptr.end() - 1);
    for (int c = 0; c < d.m_x; ++c) lchk[fill[lay[c]]++] = c;
    fgnn_device_guard dg(g->device);
    if (dg.err != hipSuccess) return fgnn_fail(FGNN_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
    const auto drop = [&] {
        for (void*& p : g->bit_layer_alloc)
            if (p) {
                (void)hipFree(p);  // waits for the launches that read it
                p = nullptr;
            }
        g->num_bit_layers = 0;
        g->h_bit_layer_of.clear();
    };
    drop();
    const std::vector<int>* tabs[2] = {&lcptr, &lchk};
    for (int i = 0; i < 2; ++i) {
        hipError_t e = hipMalloc(&g->bit_layer_alloc[i], tabs[i]->size() * sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(g->bit_layer_alloc[i], tabs[i]->data(), tabs[i]->size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            drop();
            return fgnn_fail(FGNN_ERR_HIP, std::string("uploading the bit-layer tables: ") + hipGetErrorString(e));
        }
    }
    g->num_bit_layers = num_layers;
    g->h_bit_layer_of = lay;
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_greedy_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int32_t* layer_of, int32_t* num_layers)
{
    if (!layer_of || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "layer_of or num_layers is NULL");
    std::vector<int> ptr, vn;
    const int rc = check_bits(n, m, nnz, chk, var, ptr, vn);
    if (rc) return rc;
    greedy_layers(n, m, ptr, vn, layer_of, num_layers);
    return FGNN_OK;
}

extern "C" int fgnn_validate_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int num_layers, const int32_t* layer_of)
{
    std::vector<int> ptr, vn;
    const int rc = check_bits(n, m, nnz, chk, var, ptr, vn);
    if (rc) return rc;
    return validate_layers(n, m, m, ptr, vn, num_layers, layer_of, true);
}

extern "C" int fgnn_graph_set_bit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_bit_layers(g, num_layers, layer_of);
}

extern "C" int fgnn_graph_bit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    if (!g || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    *num_layers = g->num_bit_layers;
    if (layer_of) std::copy(g->h_bit_layer_of.begin(), g->h_bit_layer_of.end(), layer_of);
    return FGNN_OK;
}

int fgnn_graph_ensure_bit_layers(const fgnn_graph* g)
{
    if (g->num_bit_layers > 0) return FGNN_OK;
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_bit_layers(g, 0, nullptr);
}

// ---- layers of the qubits, for the schedule that is serial along qubits (fgnn_mbp4_decode_serial) -------------------------------------
namespace {

// the checks of every qubit (combined numbers, hx checks first), ascending, from the qubits of every check
void qubit_checks(int n, int m, const std::vector<int>& cptr, const std::vector<int>& cvn, std::vector<int>& vptr, std::vector<int>& vchk)
{
    vptr.assign(n + 1, 0);
    for (int v : cvn) vptr[v + 1]++;
    for (int v = 0; v < n; ++v) vptr[v + 1] += vptr[v];
    vchk.resize(cvn.size());
    std::vector<int> fill(vptr.begin(), vptr.end() - 1);
    for (int c = 0; c < m; ++c)
        for (int p = cptr[c]; p < cptr[c + 1]; ++p) vchk[fill[cvn[p]]++] = c;
}

// checks ascending, a check's qubits ascending: the first qubit that meets an earlier one of its check in its own layer is refused
int validate_qubit_layers(int n, int m_x, int m, const std::vector<int>& cptr, const std::vector<int>& cvn, int num_layers,
                          const int32_t* layer_of)
{
    if (!layer_of) return fgnn_fail(FGNN_ERR_ARG, "layer_of is NULL");
    if (num_layers < 1) return fgnn_fail(FGNN_ERR_ARG, "num_layers = " + std::to_string(num_layers) + " must be >= 1");
    std::vector<int> count(num_layers, 0);
    for (int v = 0; v < n; ++v) {
        if (layer_of[v] < 0 || layer_of[v] >= num_layers)
            return fgnn_fail(FGNN_ERR_ARG, "qubit " + std::to_string(v) + " has layer " + std::to_string(layer_of[v]) + ", outside [0, " +
                                               std::to_string(num_layers) + ")");
        count[layer_of[v]]++;
    }
    for (int l = 0; l < num_layers; ++l)
        if (!count[l]) return fgnn_fail(FGNN_ERR_ARG, "layer " + std::to_string(l) + " is empty");
    // stamp[l] = the last check with a qubit in layer l, owner[l] = that qubit: two of one check in one layer collide
    std::vector<int> owner(num_layers, -1), stamp(num_layers, -1), row;
    for (int c = 0; c < m; ++c) {
        row.assign(cvn.begin() + cptr[c], cvn.begin() + cptr[c + 1]);
        std::sort(row.begin(), row.end());
        for (int v : row) {
            const int l = layer_of[v];
            if (stamp[l] == c && owner[l] != v)
                return fgnn_fail(FGNN_ERR_ARG, "qubit " + std::to_string(owner[l]) + " and qubit " + std::to_string(v) + " of layer " +
                                                   std::to_string(l) + " share " + check_name(c, m_x));
            stamp[l] = c;
            owner[l] = v;
        }
    }
    return FGNN_OK;
}

void free_qubit_layers(const fgnn_graph* g)
{
    for (void*& p : g->qubit_layer_alloc)
        if (p) {
            (void)hipFree(p);  // waits for the launches that read it
            p = nullptr;
        }
    g->num_qubit_layers = 0;
    g->h_qubit_layer_of.clear();
}

// validates (a refused layering leaves the installed one in place), then replaces the five device tables
int install_qubit_layers(const fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    const GraphDev& d = g->d;
    std::vector<int> cptr, cvn;
    int rc = check_qubits(d.n, d.m_x, d.m_z, d.E_x, g->h_chk[0].data(), g->h_var[0].data(), d.E_z, g->h_chk[1].data(),
                          g->h_var[1].data(), cptr, cvn);
    if (rc) return rc;
    std::vector<int32_t> lay(d.n);
    if (!layer_of) {
        std::vector<int> vptr, vchk;
        qubit_checks(d.n, d.m, cptr, cvn, vptr, vchk);
        greedy_layers(d.m, d.n, vptr, vchk, lay.data(), &num_layers);  // the check layering with the two kinds of node exchanged
    } else {
        if ((rc = validate_qubit_layers(d.n, d.m_x, d.m, cptr, cvn, num_layers, layer_of))) return rc;
        std::copy(layer_of, layer_of + d.n, lay.begin());
    }
    // the canonical edge lists are sorted by (qubit, check): slot e of a side is its e-th edge, and a check's row of the graph's
    // check-major view (cslot) lists its edges by ascending qubit, which is the order check_qubits leaves them in
    std::vector<int> cj((size_t)2 * d.E);
    {
        std::vector<int> fill(cptr.begin(), cptr.end() - 1);
        for (int s = 0; s < 2; ++s)
            for (int e = 0; e < (s ? d.E_z : d.E_x); ++e) {
                const int c = (s ? d.m_x : 0) + g->h_chk[s][e];
                const size_t slot = (size_t)e + (s ? d.E_x : 0);
                cj[2 * slot] = c;
                cj[2 * slot + 1] = fill[c]++ - cptr[c];
            }
    }
    std::vector<int> vpx(d.n + 1, 0), vpz(d.n + 1, 0);
    for (int v : g->h_var[0]) vpx[v + 1]++;
    for (int v : g->h_var[1]) vpz[v + 1]++;
    for (int v = 0; v < d.n; ++v) {
        vpx[v + 1] += vpx[v];
        vpz[v + 1] += vpz[v];
    }
    std::vector<int> qptr(num_layers + 1, 0), qub(d.n), eptr(num_layers + 1, 0), eslot(d.E);
    for (int v = 0; v < d.n; ++v) qptr[lay[v] + 1]++;
    for (int l = 0; l < num_layers; ++l) qptr[l + 1] += qptr[l];
    {
        std::vector<int> fill(qptr.begin(), qptr.end() - 1);
        for (int v = 0; v < d.n; ++v) qub[fill[lay[v]]++] = v;
    }
    int ne = 0;
    for (int l = 0; l < num_layers; ++l) {
        for (int i = qptr[l]; i < qptr[l + 1]; ++i) {
            const int v = qub[i];
            for (int e = vpx[v]; e < vpx[v + 1]; ++e) eslot[ne++] = e;
            for (int e = vpz[v]; e < vpz[v + 1]; ++e) eslot[ne++] = d.E_x + e;
        }
        eptr[l + 1] = ne;
    }
    fgnn_device_guard dg(g->device);
    if (dg.err != hipSuccess) return fgnn_fail(FGNN_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
    free_qubit_layers(g);
    const std::vector<int>* tabs[5] = {&qptr, &qub, &eptr, &eslot, &cj};
    for (int i = 0; i < 5; ++i) {
        const size_t bytes = std::max<size_t>(tabs[i]->size(), 2) * sizeof(int);
        hipError_t e = hipMalloc(&g->qubit_layer_alloc[i], bytes);
        if (e == hipSuccess && !tabs[i]->empty())
            e = hipMemcpy(g->qubit_layer_alloc[i], tabs[i]->data(), tabs[i]->size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            free_qubit_layers(g);
            return fgnn_fail(FGNN_ERR_HIP, std::string("uploading the qubit-layer tables: ") + hipGetErrorString(e));
        }
    }
    g->num_qubit_layers = num_layers;
    g->h_qubit_layer_of = lay;
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_greedy_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                        const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers)
{
    if (!layer_of || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "layer_of or num_layers is NULL");
    std::vector<int> cptr, cvn, vptr, vchk;
    const int rc = check_qubits(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, cptr, cvn);
    if (rc) return rc;
    qubit_checks(n, m_x + m_z, cptr, cvn, vptr, vchk);
    greedy_layers(m_x + m_z, n, vptr, vchk, layer_of, num_layers);
    return FGNN_OK;
}

extern "C" int fgnn_validate_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                          const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of)
{
    std::vector<int> cptr, cvn;
    const int rc = check_qubits(n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, cptr, cvn);
    if (rc) return rc;
    return validate_qubit_layers(n, m_x, m_x + m_z, cptr, cvn, num_layers, layer_of);
}

extern "C" int fgnn_graph_set_qubit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_qubit_layers(g, num_layers, layer_of);
}

extern "C" int fgnn_graph_qubit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    if (!g || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    *num_layers = g->num_qubit_layers;
    if (layer_of) std::copy(g->h_qubit_layer_of.begin(), g->h_qubit_layer_of.end(), layer_of);
    return FGNN_OK;
}

int fgnn_graph_ensure_qubit_layers(const fgnn_graph* g)
{
    if (g->num_qubit_layers > 0) return FGNN_OK;
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    return install_qubit_layers(g, 0, nullptr);
}

// Per-launch timing of the BP4 kernel: HIP events recorded on the launch stream immediately before and
// after each bp4 launch (inside fgnn_bp4_decode and inside fgnn_sandwich_decode), read back afterwards.
extern "C" int fgnn_profile_enable(fgnn_graph* g, int max_launches)
{
    if (!g || max_launches < 0) return fgnn_fail(FGNN_ERR_ARG, "bad profile arguments");
    FGNN_DEVICE_GUARD(g->device);
    for (hipEvent_t e : g->prof_ev) (void)hipEventDestroy(e);
    g->prof_ev.clear();
    g->prof_n = 0;
    g->prof_on = max_launches > 0;
    g->prof_iters.assign(max_launches, 0);
    g->prof_batch.assign(max_launches, 0);
    for (int i = 0; i < 2 * max_launches; ++i) {
        hipEvent_t e;
        FGNN_HIP_CHECK(hipEventCreate(&e));
        g->prof_ev.push_back(e);
    }
    return FGNN_OK;
}

// ms[i], iters[i], batch[i] for the launches recorded since the last read (host arrays of length cap);
// waits for the last recorded event; resets the recorder.
extern "C" int fgnn_profile_read(fgnn_graph* g, float* ms, int32_t* iters, int32_t* batch, int cap, int32_t* count)
{
    if (!g || !ms || !iters || !batch || !count) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    FGNN_DEVICE_GUARD(g->device);
    int n = g->prof_n < cap ? g->prof_n : cap;
    if (g->prof_n > 0) FGNN_HIP_CHECK(hipEventSynchronize(g->prof_ev[2 * g->prof_n - 1]));
    for (int i = 0; i < n; ++i) {
        FGNN_HIP_CHECK(hipEventElapsedTime(&ms[i], g->prof_ev[2 * i], g->prof_ev[2 * i + 1]));
        iters[i] = g->prof_iters[i];
        batch[i] = g->prof_batch[i];
    }
    *count = n;
    g->prof_n = 0;
    return FGNN_OK;
}
