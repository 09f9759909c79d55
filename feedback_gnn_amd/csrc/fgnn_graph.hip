// fgnn_graph.hip — builds the device-resident Tanner-graph tables of a CSS code.
// Replaces the edge bookkeeping of QLDPCBPDecoder.__init__ (/root/reference
// sionna/fec/ldpc/decoding_q.py:53-94: scipy.sparse.find + argsort + ragged row splits) and of
// Feedback_GNN.create_edges (feedback_gnn.py:87-108) by one CSC + one CSR view per parity-check matrix.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <optional>

#include "fgnn_internal.h"
#include "fgnn_layers.h"

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
    g->h_vptr[0] = std::move(vptr_x);  // the layerings are built from these views (install_layers)
    g->h_vptr[1] = std::move(vptr_z);
    g->h_cptr = std::move(cptr);
    g->h_cslot = std::move(cslot);
    g->h_cvn = std::move(cvn);
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
    for (fgnn_layering* rec : {&g->check_layers, &g->bit_layers, &g->qubit_layers}) rec->free();
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

// ---- the layerings of the serial schedules: checks (fgnn_bp4_decode_layered), bits = hx alone (fgnn_bp2_decode_layered,
// fgnn_relay_decode_layered) and qubits (fgnn_mbp4_decode_serial); the algorithms are in fgnn_layers.h --------------------------------
namespace {

// a caller's edge lists check-major: the qubits of every check, hx checks 0..m_x-1 then hz checks m_x..m_x+m_z-1, in the order of the
// lists; one_sided: one matrix alone (m_z = nnz_z = 0), whose nodes are bits
int check_qubits(bool one_sided, int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                 const int32_t* chk_z, const int32_t* var_z, std::vector<int>& ptr, std::vector<int>& vn)
{
    if (n <= 0 || m_x <= 0 || (!one_sided && m_z <= 0) || nnz_x < 0 || nnz_z < 0)
        return fgnn_fail(FGNN_ERR_ARG, one_sided ? "n and m must be positive" : "n, m_x and m_z must be positive");
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

// fgnn_greedy_layers / _bit_layers / _qubit_layers: no graph, no device
int greedy_of_lists(fgnn_layer_kind kind, int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                    const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers)
{
    if (!layer_of || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "layer_of or num_layers is NULL");
    std::vector<int> cptr, cvn;
    if (int rc = check_qubits(kind == LAYER_BITS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, cptr, cvn)) return rc;
    fgnn_layers::greedy(kind, n, m_x + m_z, cptr, cvn, layer_of, num_layers);
    return FGNN_OK;
}

// fgnn_validate_layers / _bit_layers / _qubit_layers: no graph, no device
int validate_of_lists(fgnn_layer_kind kind, int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                      const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of)
{
    std::vector<int> cptr, cvn;
    if (int rc = check_qubits(kind == LAYER_BITS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, cptr, cvn)) return rc;
    const std::string refused = fgnn_layers::validate(kind, n, m_x, m_x + m_z, cptr, cvn, num_layers, layer_of);
    return refused.empty() ? FGNN_OK : fgnn_fail(FGNN_ERR_ARG, refused);
}

fgnn_layering& layering(const fgnn_graph* g, fgnn_layer_kind kind)
{
    return kind == LAYER_CHECKS ? g->check_layers : kind == LAYER_BITS ? g->bit_layers : g->qubit_layers;
}

// The greedy layering (layer_of NULL) or the caller's, validated — a refused one leaves the installed layering in place —, then the
// kind's tables replace the installed ones on the device.  Everything comes from the host views graph_build kept.
int install_layers(const fgnn_graph* g, fgnn_layer_kind kind, int num_layers, const int32_t* layer_of)
{
    namespace FL = fgnn_layers;
    static const char* const tables_of[] = {"layer", "bit-layer", "qubit-layer"};
    if (g->host_only) return fgnn_fail(FGNN_ERR_STATE, "a host-only graph carries no device tables");
    const GraphDev& d = g->d;
    const int m = kind == LAYER_BITS ? d.m_x : d.m, items = FL::item_count(kind, d.n, m);
    std::vector<int32_t> lay(items);
    if (!layer_of) {
        FL::greedy(kind, d.n, m, g->h_cptr, g->h_cvn, lay.data(), &num_layers);
    } else {
        const std::string refused = FL::validate(kind, d.n, d.m_x, m, g->h_cptr, g->h_cvn, num_layers, layer_of);
        if (!refused.empty()) return fgnn_fail(FGNN_ERR_ARG, refused);
        lay.assign(layer_of, layer_of + items);
    }
    std::vector<std::vector<int>> tabs(kind == LAYER_CHECKS ? 4 : kind == LAYER_BITS ? 2 : 5);  // in the order of the LAY_* slots
    FL::bucket_by_layer(items, num_layers, lay.data(), tabs[0], tabs[1]);
    if (kind == LAYER_CHECKS)
        FL::check_layer_tables(tabs[LAY_CPTR], tabs[LAY_CHK], g->h_cptr, g->h_cslot, g->h_cvn, tabs[LAY_EPTR], tabs[LAY_EDGE]);
    if (kind == LAYER_QUBITS)
        FL::qubit_layer_tables(tabs[LAY_QPTR], tabs[LAY_QUB], g->h_vptr[0], g->h_vptr[1], g->h_cptr, g->h_cslot, tabs[LAY_QEPTR],
                               tabs[LAY_SLOT], tabs[LAY_SLOT_CJ]);
    fgnn_device_guard dg(g->device);
    if (dg.err != hipSuccess) return fgnn_fail(FGNN_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(dg.err));
    fgnn_layering& rec = layering(g, kind);
    rec.free();
    for (const std::vector<int>& t : tabs) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<size_t>(t.size(), 2) * sizeof(int));
        if (e == hipSuccess) {
            rec.dev.push_back(p);
            if (!t.empty()) e = hipMemcpy(p, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {
            rec.free();
            return fgnn_fail(FGNN_ERR_HIP, std::string("uploading the ") + tables_of[kind] + " tables: " + hipGetErrorString(e));
        }
    }
    rec.num = num_layers;
    rec.layer_of = lay;
    return FGNN_OK;
}

int set_layers(fgnn_graph* g, fgnn_layer_kind kind, int num_layers, const int32_t* layer_of)
{
    return g ? install_layers(g, kind, num_layers, layer_of) : fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
}

int get_layers(const fgnn_graph* g, fgnn_layer_kind kind, int32_t* num_layers, int32_t* layer_of)
{
    if (!g || !num_layers) return fgnn_fail(FGNN_ERR_ARG, "NULL argument");
    const fgnn_layering& rec = layering(g, kind);
    *num_layers = rec.num;
    if (layer_of) std::copy(rec.layer_of.begin(), rec.layer_of.end(), layer_of);
    return FGNN_OK;
}

int ensure_layers(const fgnn_graph* g, fgnn_layer_kind kind)
{
    return layering(g, kind).num > 0 ? FGNN_OK : install_layers(g, kind, 0, nullptr);
}

}  // namespace

extern "C" int fgnn_greedy_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                  const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers)
{
    return greedy_of_lists(LAYER_CHECKS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, layer_of, num_layers);
}

extern "C" int fgnn_validate_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                    const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of)
{
    return validate_of_lists(LAYER_CHECKS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, num_layers, layer_of);
}

extern "C" int fgnn_greedy_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int32_t* layer_of, int32_t* num_layers)
{
    return greedy_of_lists(LAYER_BITS, n, m, 0, nnz, chk, var, 0, nullptr, nullptr, layer_of, num_layers);
}

extern "C" int fgnn_validate_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int num_layers, const int32_t* layer_of)
{
    return validate_of_lists(LAYER_BITS, n, m, 0, nnz, chk, var, 0, nullptr, nullptr, num_layers, layer_of);
}

extern "C" int fgnn_greedy_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                        const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers)
{
    return greedy_of_lists(LAYER_QUBITS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, layer_of, num_layers);
}

extern "C" int fgnn_validate_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                                          const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of)
{
    return validate_of_lists(LAYER_QUBITS, n, m_x, m_z, nnz_x, chk_x, var_x, nnz_z, chk_z, var_z, num_layers, layer_of);
}

extern "C" int fgnn_graph_set_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    return set_layers(g, LAYER_CHECKS, num_layers, layer_of);
}
extern "C" int fgnn_graph_set_bit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    return set_layers(g, LAYER_BITS, num_layers, layer_of);
}
extern "C" int fgnn_graph_set_qubit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of)
{
    return set_layers(g, LAYER_QUBITS, num_layers, layer_of);
}

extern "C" int fgnn_graph_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    return get_layers(g, LAYER_CHECKS, num_layers, layer_of);
}
extern "C" int fgnn_graph_bit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    return get_layers(g, LAYER_BITS, num_layers, layer_of);
}
extern "C" int fgnn_graph_qubit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of)
{
    return get_layers(g, LAYER_QUBITS, num_layers, layer_of);
}

int fgnn_graph_ensure_layers(const fgnn_graph* g) { return ensure_layers(g, LAYER_CHECKS); }
int fgnn_graph_ensure_bit_layers(const fgnn_graph* g) { return ensure_layers(g, LAYER_BITS); }
int fgnn_graph_ensure_qubit_layers(const fgnn_graph* g) { return ensure_layers(g, LAYER_QUBITS); }

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
