// fgnn_mbp4_serial.hip — MBP4 / AMBP4 (fgnn_mbp4.hip) in Kuo and Lai's serial schedule, LDS-resident: the qubits are visited one
// layer after the other, and a qubit sees the messages the qubits of the layers before it have just sent.  The algorithm is stated to
// the float operation at fgnn_mbp4_decode_serial in include/fgnn.h.  The kernel stands on the frame of the step-loop decoders
// (fgnn_step.h: codeword rows, staged syndrome bits of the stop test, the parity of the decisions, the output write) and on the attempt
// schedule of fgnn_attempts.h (AttemptCtl, the tab / stamp / ndone words of AttemptLds); the qubit rules are those of fgnn_vn.h, the
// check rule is the single-output form of fgnn_cn1.h.
//
// A layer holds qubits that share no check, on hx or on hz (fgnn_graph_set_qubit_layers validates it).  So inside a layer
//   - mu_e of an edge e = (c, v) reads the nu of c's edges, of which only e belongs to a qubit of the layer, and writes slot e of mu;
//   - the qubit v reads its own mu slots and writes its own nu slots and its decision byte.
// Two thread mappings give the same bits (FGNN_MBP4_SERIAL_MAP):
//   0  a thread per edge of the layer for mu, barrier, a thread per qubit of the layer for the totals, the decision and nu, barrier;
//   1  a thread per qubit of the layer for all three, one barrier.
// DESIGN.md section 4, "Serial schedule of AMBP4", has the time of both.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats:
//   nu   [E_x + E_z]  v->c messages, bp4_kernel's slot layout
//   mu   [E_x + E_z]  c->v messages, same layout
//   dec  [n] bytes    decisions d_v = x_v | z_v << 1 of the last visit of every qubit
// and per workgroup tab[128], stamp[cpb] and ndone (AttemptLds, fgnn_step.h).  [[882,24]]: 2 x 5292 floats + 896 bytes = 43 232 bytes
// per codeword.
//
// A workgroup step is one iteration of every unfinished codeword of the workgroup:
//   layers   l = 0 .. num_layers - 1, as above
//   checks   parity of the decisions against the syndrome bit (stamp)
//   barrier
//   control  solved / out of attempts: outputs, done;  k = T: the next attempt, a restarting one from mu = 0 and the first nu
//   barrier
// Barriers.  The loop bounds and the conditions around the barriers are launch arguments or the same LDS word (ndone, last written
// before the barrier in front of its read): every thread of the workgroup reaches every barrier.  Finished and padded codewords and
// threads beyond a layer's edges or qubits skip the work, never a barrier.  The kernel body holds no atomic; the one atomic of a launch
// is the integer count of finished codewords inside the shared step_finish (fgnn_step.h), which only ends the workgroup's loop.  No
// result depends on the order in which threads arrive or on the launch geometry.
//
// Registers.  The LDS above admits 3 workgroups of [[882,24]] on a CU (3 x 43 760 bytes fit 160 KiB, 4 do not): with the 512 threads
// per codeword of the default launch 24 waves, 6 per SIMD.  The kernels are compiled for FGNN_MBP4_SERIAL_WAVES waves per SIMD; DESIGN.md lists what each
// instantiation takes.  Runtime degrees only: there is no (3,3,6) instantiation.
#include "fgnn_step.h"
#include "fgnn_cn1.h"

#ifndef FGNN_MBP4_SERIAL_WAVES
#define FGNN_MBP4_SERIAL_WAVES 6  // waves per SIMD the register allocation aims at: what the LDS of [[882,24]] admits
#endif
#ifndef FGNN_MBP4_SERIAL_MAP
#define FGNN_MBP4_SERIAL_MAP 0  // 0: a thread per edge, then a thread per qubit; 1: a thread per qubit
#endif
#ifndef FGNN_MBP4_SERIAL_TPC
#define FGNN_MBP4_SERIAL_TPC 512  // threads per codeword of a large code without fgnn_graph_set_launch: see fgnn_mbp4_decode_serial below
#endif

namespace {

struct MsArgs : AttemptArgs {
    int num_layers, m_off;   // m_off: mu of a codeword, in floats from its nu
    const int* lay_qptr;     // [num_layers+1] first entry of layer l in lay_qub
    const int* lay_qub;      // [n] qubits by layer, ascending inside a layer
    const int* lay_eptr;     // [num_layers+1] first entry of layer l in lay_slot
    const int* lay_slot;     // [E] slots of the edges of a layer's qubits
    const int2* slot_cj;     // [E] (combined check c, place j in c's row) of slot e
};

// mu_e: what check c of slot e sends along it now
template <int CN_TYPE>
__device__ __forceinline__ float serial_mu(const GraphDev& g, const MsArgs& a, const StepRows& rows, const float* nu, const int e, const float fac)
{
    const int2 cj = a.slot_cj[e];
    const int c0 = g.cptr[cj.x];
    return cn_output<CN_TYPE, PhiBp4>(nu, g.cslot + c0, g.cptr[cj.x + 1] - c0, cj.y, rows.synd_of(g, cj.x), fac);
}

// the qubit's totals from its mu, its decision, its nu with the own weight ow
__device__ __forceinline__ void serial_qubit(const GraphDev& g, const StepRows& rows, float* nu, const float* mu, uint8_t* dec, const int v,
                                             const float llr_const, const float ow)
{
    const int x0 = g.vptr_x[v], x1 = g.vptr_x[v + 1], z0 = g.vptr_z[v], z1 = g.vptr_z[v + 1];
    float lx, ly, lz, Sz, Sx, X, Y, Z;
    rows.llrs(g.n, v, llr_const, lx, ly, lz);
    vn_sums(mu, z0, z1, x0, x1, Sz, Sx);
    vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
    dec[v] = (uint8_t)vn_decide(X, Y, Z);
    const float numx = VnMath::softplus(-X);
    const float numz = VnMath::softplus(-Z);
    for (int e = x0; e < x1; ++e) nu[e] = vn_edge_own<VnMath>(numx, Z, Y, mu[e], ow);
    for (int e = z0; e < z1; ++e) nu[e] = vn_edge_own<VnMath>(numz, X, Y, mu[e], ow);
}

// a codeword's start, and a restarting attempt's: mu = 0 and the nu that follows from it (own * 0 = 0 whatever the own weight), each
// qubit's slots by the qubit's thread
__device__ __forceinline__ void serial_start(const GraphDev& g, const MsArgs& a, const StepRows& rows, float* nu, float* mu, const int lane)
{
    for (int v = lane; v < g.n; v += a.tpc) {
        const int x0 = g.vptr_x[v], x1 = g.vptr_x[v + 1], z0 = g.vptr_z[v], z1 = g.vptr_z[v + 1];
        for (int e = x0; e < x1; ++e) mu[e] = 0.0f;
        for (int e = z0; e < z1; ++e) mu[e] = 0.0f;
        float lx, ly, lz, Sz, Sx, X, Y, Z;
        rows.llrs(g.n, v, a.llr_const, lx, ly, lz);
        vn_sums(mu, z0, z1, x0, x1, Sz, Sx);
        vn_totals(Sz, Sx, lx, ly, lz, X, Y, Z);
        const float numx = VnMath::softplus(-X);
        const float numz = VnMath::softplus(-Z);
        for (int e = x0; e < x1; ++e) nu[e] = vn_edge_own<VnMath>(numx, Z, Y, 0.0f, 1.0f);
        for (int e = z0; e < z1; ++e) nu[e] = vn_edge_own<VnMath>(numz, X, Y, 0.0f, 1.0f);
    }
}

template <int CN_TYPE>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_MBP4_SERIAL_WAVES))) mbp4_serial_kernel(GraphDev g, MsArgs a)
{
    FG_LOG_TAB_SETUP();
    extern __shared__ float lds[];
    const StepCw cw(a);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepRows rows(g, a, cw);
    float* nu = lds + (size_t)cwl * a.lds_per_cw;
    float* mu = nu + a.m_off;
    uint8_t* dec = reinterpret_cast<uint8_t*>(nu + a.d_off);
    const int n = g.n, m = g.m;
    const AttemptLds w = attempt_stage(lds, a);
    if (cw.active) {
        for (int v = lane; v < n; v += a.tpc) dec[v] = 0;
        serial_start(g, a, rows, nu, mu, lane);
    }
    const StepSynd synd(g, rows, cw, a.tpc);
    __syncthreads();

    AttemptCtl ctl(cw.active);
    for (int step = 1; step <= a.max_steps; ++step) {
        const float fac = w.tab[ctl.r], ow = w.tab[ATTEMPT_MAX + ctl.r];
        // ---- the layers: mu of the layer's edges from the current nu, then the layer's qubits ----
        for (int l = 0; l < a.num_layers; ++l) {
            if constexpr (FGNN_MBP4_SERIAL_MAP == 0) {
                if (!ctl.done) {
                    const int e1 = a.lay_eptr[l + 1];
                    for (int i = a.lay_eptr[l] + lane; i < e1; i += a.tpc) {
                        const int e = a.lay_slot[i];
                        mu[e] = serial_mu<CN_TYPE>(g, a, rows, nu, e, fac);
                    }
                }
                __syncthreads();
                if (!ctl.done) {
                    const int q1 = a.lay_qptr[l + 1];
                    for (int i = a.lay_qptr[l] + lane; i < q1; i += a.tpc) serial_qubit(g, rows, nu, mu, dec, a.lay_qub[i], a.llr_const, ow);
                }
            } else {
                if (!ctl.done) {
                    const int q1 = a.lay_qptr[l + 1];
                    for (int i = a.lay_qptr[l] + lane; i < q1; i += a.tpc) {
                        const int v = a.lay_qub[i];
                        const int x0 = g.vptr_x[v], x1 = g.vptr_x[v + 1], z0 = g.vptr_z[v], z1 = g.vptr_z[v + 1];
                        for (int e = x0; e < x1; ++e) mu[e] = serial_mu<CN_TYPE>(g, a, rows, nu, e, fac);
                        for (int e = z0; e < z1; ++e) mu[e] = serial_mu<CN_TYPE>(g, a, rows, nu, e, fac);
                        serial_qubit(g, rows, nu, mu, dec, v, a.llr_const, ow);
                    }
                }
            }
            __syncthreads();
        }
        // ---- checks of both graphs: parity of the decisions against the syndrome bit ----
        if (!ctl.done) {
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const int c0 = g.cptr[c];
                if (parity_csr(g, dec, c0, g.cptr[c + 1] - c0, c < g.m_x, synd.at(g, rows, i, c)) != 0u) w.stamp[cwl] = step;
            }
        }
        __syncthreads();
        // ---- per codeword: solution found, attempt over, decoder finished ----
        if (!ctl.done) {
            const int T = ctl.T(a.sched);
            ctl.more();
            const bool sat = w.stamp[cwl] != step;
            if (sat || ctl.last(a.sched, T)) {
                step_write_decisions(a, dec, rows.bb, n, lane);
                if (lane == 0) step_finish(a, (size_t)cw.b, sat, ctl.r, ctl.its, ctl.k, w.ndone);
                ctl.done = true;
            } else if (ctl.k == T) {
                ctl.again();
                if (a.sched.restart) serial_start(g, a, rows, nu, mu, lane);
            }
        }
        __syncthreads();
        if (*w.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
    }
}

}  // namespace

extern "C" int fgnn_mbp4_decode_serial(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own,
                                       int pre_iter, int attempt_iter, int restart, const float* llr_ch, float llr_const,
                                       const uint8_t* synd_x, const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats,
                                       void* stream)
{
    if (int err = step_check_args(g, cn_type, B)) return err;
    if (int err = attempt_check_sched(num_attempts, pre_iter, attempt_iter, restart)) return err;
    if (int err = attempt_check_tables(num_attempts, factor, own)) return err;
    if (B == 0) return FGNN_OK;  // an empty batch needs no buffers
    if (!x_hat || !z_hat || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    LaunchGeom L = fgnn_geom(g, B);
    // Threads per codeword.  The LDS of a codeword keeps a CU at 3 workgroups of [[882,24]] whatever their size, and the edge phase
    // waits on the row and syndrome reads of its checks: more waves per workgroup hide them, although a layer has only 378 edges (14
    // greedy layers of 63 qubits).  tools/bench_mbp4_serial.py's sweep on [[882,24]] at 16 384 codewords (profiles/mbp4_serial_bench.json:
    // 64 / 128 / 192 / 256 / 384 / 512 / 1024 threads take 158 / 93 / 71 / 68 / 66 / 64 / 113 ms for 32 min-sum iterations) has its
    // minimum at 512, so without fgnn_graph_set_launch a codeword of a code that fgnn_geom gives 256 threads or more (one workgroup
    // per codeword; up to 1024 threads in a small batch) gets FGNN_MBP4_SERIAL_TPC; small batches and other codes have not been swept
    if (!g->user_launch && L.cpb == 1 && L.tpc >= 256) {
        L.tpc = FGNN_MBP4_SERIAL_TPC;
        L.threads = L.tpc;
    }
    MsArgs a;
    attempt_args_fill(a, L, B, num_attempts, factor, own, pre_iter, attempt_iter, restart, llr_ch, llr_const, synd_x, synd_z, x_hat, z_hat,
                      stats);
    // per codeword: E messages each way and n decision bytes; per workgroup: the two 64-float tables, a stamp per codeword and ndone
    const size_t m_off = lds_round4(g->d.E);
    size_t lds_bytes;
    if (int err = step_lds_bytes(a, "serial MBP4", 2 * m_off + lds_bytes_as_floats(g->d.n), 2 * ATTEMPT_MAX, L.cpb + 1, &lds_bytes)) return err;
    if (int err = fgnn_graph_ensure_qubit_layers(g)) return err;
    FGNN_DEVICE_GUARD(g->device);
    a.m_off = (int)m_off;
    a.d_off = (int)(2 * m_off);
    a.num_layers = g->qubit_layers.num;
    a.lay_qptr = g->qubit_layers.table<int>(LAY_QPTR);
    a.lay_qub = g->qubit_layers.table<int>(LAY_QUB);
    a.lay_eptr = g->qubit_layers.table<int>(LAY_QEPTR);
    a.lay_slot = g->qubit_layers.table<int>(LAY_SLOT);
    a.slot_cj = g->qubit_layers.table<int2>(LAY_SLOT_CJ);
    const hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid(L.blocks), block(L.threads);
    switch (cn_type) {
    case FGNN_CN_BOXPLUS_PHI: return fgnn_launch(mbp4_serial_kernel<FGNN_CN_BOXPLUS_PHI>, grid, block, lds_bytes, st, g->d, a);
    case FGNN_CN_MINSUM: return fgnn_launch(mbp4_serial_kernel<FGNN_CN_MINSUM>, grid, block, lds_bytes, st, g->d, a);
    default: return fgnn_launch(mbp4_serial_kernel<FGNN_CN_BOXPLUS>, grid, block, lds_bytes, st, g->d, a);
    }
}
