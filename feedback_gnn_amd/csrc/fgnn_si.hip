// fgnn_si.hip — binary min-sum BP with stabilizer inactivation (BP-SI) on one Tanner graph, LDS-resident: plain BP runs; where it
// fails, the stabilizer generators are ranked by the reliability of their bits, and one after the other the least reliable ones are
// inactivated: their bits are erased, BP runs again on the rest, and the erased bits are filled in from a linear system of a few unknowns.
//
// du Crest, Mhalla, Savin, "Stabilizer inactivation for message-passing decoding of quantum LDPC codes" (2022), in the form
// include/fgnn.h states at fgnn_si_decode.  The parity-check matrix is side 0 (hx) of an fgnn_graph; the groups to inactivate are the
// rows of side 1 (hz), read from the graph's check-major tables (cptr / cvn from row m_x on).  Nothing else of side 1 is used.
//
// The step is that of the binary leg decoders in fgnn_step.h (StepCw, BitRows, StepSynd, BitSlots; bit_check for the check phase, with
// its own action on an odd check, bit_sample for the sample's rows, BitArgs on the host), which relay_kernel (fgnn_relay.hip) and
// gdg_kernel (fgnn_gdg.hip) run too; its own is the bit phase, relay_kernel's with the memory term taken out and the inactive marks put
// in, the groups and the solve.  The control is that of fgnn_legs.h with an attempt as a leg: 1 + min(max_groups, non-empty groups)
// legs, stop at the first solution.  A decision has no weight here, so nothing is weighed
// or settled: what an attempt's end writes it writes in the control section of that step, from P, which still holds the tested decision.
// An attempt ends at its last test (k = T) or, from attempt 1 on, at the first test that leaves every non-adjacent check satisfied;
// LegCtl::test is told so by T = k.
//
// The solve.  H[adjacent, I] depends on the group alone, so the host eliminates it once per group (si_ensure below: Gauss-Jordan over
// the columns in ascending order with the row operations tracked) and uploads per group j
//   adj[aptr[j] ..)    its adjacent hx checks, 64 at the most
//   xmask, per bit     x_i = parity(r & xmask_i); 0 for a column that depends on the earlier ones
//   cons[kptr[j] ..)   solvable iff parity(r & cons_t) = 0 for every t (the rows the elimination left empty)
// r is one 64-bit word per codeword: an adjacent check of odd parity ORs its bit in (integer atomic in LDS), bit = its place in adj.
// The words alternate by step parity: the one of step s is read in the control section of s and zeroed in that of s + 1.
//
// The pick is gdg_kernel's (fgnn_gdg.hip): a 64-bit atomicMin in LDS over key_j = bits(score_j) << 32 | j, an integer minimum of a
// total order whatever the arrival order.  The scores are formed once, from the P of plain BP's last test, and kept; the a-th pick is
// the minimum over the keys above the (a-1)-th pick's key.  An attempt may end at any test, so its successor is picked ahead: the keys
// for attempt a + 1 are posted in step k = 0 of attempt a (for attempt 1: in plain BP's last step, after the barrier that completes P)
// and read where next_leg() is called.  Two key words alternate by attempt parity; the one just read is reset one attempt later.
//
// Marks.  inact[v] is written and read by the thread that owns bit v only.  adjpos[c] = 1 + (place of c in adj) or 0 is cleared in
// the control section that ends an attempt and set, for the next group, after the first barrier of the next step (k = 0, whose check
// phase tests nothing and does not read it).  Every step has the same two barriers for every codeword.
//
// LDS of one codeword, in floats, each area rounded up to 4 floats (si_lds_bytes in tests/test_gpu_si.py mirrors it):
//   msg    [E_x]        c->v / v->c messages of hx, sorted by (bit, check): bp2_kernel's layout
//   P      [n]          posteriors of the last test; 0 on an inactive bit, which decides 0
//   score  [m_z]        float bits of the group scores; all ones for a group without a bit
//   inact  [n] bytes, adjpos [m_x] bytes
// and per workgroup
//   key[2], res[2] per codeword (64-bit), then stamp[cpb], wacc[cpb] (unused), ndone: the words of the leg control (leg_stage)
// hx of [[882,24]] with its hz as groups: 2648 + 884 + 444 + 224 + 112 floats = 17 248 bytes per codeword.
#include "fgnn_step.h"

#ifndef FGNN_SI_WAVES
#define FGNN_SI_WAVES 6  // waves per SIMD the register allocation aims at (relay_kernel's target)
#endif
// next to relay_kernel's state a thread holds the group, its 64-bit key and the addresses of the marks and tables: at six waves (80
// VGPRs) the instantiations with eight slots per check spill 2 to 3 VGPRs to scratch, and the predicated update for degrees up to 16,
// which holds 16 magnitudes and signs, spills 14 at relay_kernel's five; each runs at one wave per SIMD fewer, spill-free
#define FGNN_SI_WAVES_OF(DC) ((DC) >= 16 ? FGNN_SI_WAVES - 2 : (DC) >= 8 ? FGNN_SI_WAVES - 1 : FGNN_SI_WAVES)

namespace {

typedef unsigned long long u64;

struct SiTabs {
    const int* aptr;    // [m_z+1]
    const int* adj;     // adjacent hx checks of every group
    const int* kptr;    // [m_z+1]
    const u64* cons;    // consistency masks of every group
    const u64* xmask;   // [E_z] one mask per hz edge, in the order of g.cvn from g.cptr[m_x] on
};

struct SiArgs : BitArgs {   // B = the nact listed samples
    int s_off, i_off, a_off, max_steps;
    LegSched legs;          // an attempt is a leg: num_iter, 1 + attempts, si_iter, 1
    float factor, llr_const;
    const float* llr_ch;    // [.,n] logits or null
    const uint8_t* synd;    // [.,m_x] or null (all-zero syndrome)
    const int32_t* index;   // [nact] samples or null (sample i is i)
    uint8_t* hard_out;      // [.,n]
    int32_t* stats;         // [.,4]
    SiTabs t;
};

constexpr unsigned SI_NO_SCORE = 0xFFFFFFFFu;  // a group without a bit: never posted

// DV/DC > 0: (DV,DC)-regular hx with the packed slot rows of g.cslot16; DV = 0, DC > 0: runtime degrees up to DC, predicated; DV = DC = 0: the loop.
template <int DV, int DC>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(FGNN_SI_WAVES_OF(DC)))) si_kernel(GraphDev g, SiArgs a)
{
    FG_LOG_TAB_SETUP();  // cn_update names the phi policy: the table every kernel of that family installs
    extern __shared__ float lds[];
    const StepCw cw(a.B, a.tpc, a.cpb);
    const int cwl = cw.cwl, lane = cw.lane;
    const StepCw in = bit_sample(cw, a.index, cw.b);  // the rows, input and output, are the sample's
    const BitRows rows(g, a.llr_ch, a.llr_const, a.synd, in);
    float* msg = lds + (size_t)cwl * a.lds_per_cw;
    float* P = msg + a.p_off;
    unsigned* score = reinterpret_cast<unsigned*>(msg + a.s_off);
    uint8_t* inact = reinterpret_cast<uint8_t*>(msg + a.i_off);
    uint8_t* adjpos = reinterpret_cast<uint8_t*>(msg + a.a_off);
    u64* key = reinterpret_cast<u64*>(lds + (size_t)a.cpb * a.lds_per_cw) + 4 * cwl;  // 16-byte aligned
    u64* res = key + 2;
    const int n = g.n, m = g.m_x;

    const LegLds ws = leg_stage(lds + 8 * a.cpb, a.cpb, a.lds_per_cw);  // behind the 4 cpb 64-bit words
    if (cw.active) {
        for (int v = lane; v < n; v += a.tpc) {
            P[v] = rows.prior(v);
            inact[v] = 0;
        }
        for (int c = lane; c < m; c += a.tpc) adjpos[c] = 0;
        if (lane == 0) {
            key[0] = key[1] = ~0ull;
            res[0] = res[1] = 0ull;
        }
    }
    const StepSynd synd(g, rows, in, a.tpc, m, a.synd != nullptr);
    __syncthreads();

    LegCtl ctl(cw.active);
    int grp = -1;   // the inactivated group of this attempt
    u64 cur = 0;    // its key
    for (int step = 1; step <= a.max_steps; ++step) {
        const int T = ctl.T(a.legs), r = ctl.r, k = ctl.k;
        // ---- bits: posterior after k check updates, messages to the checks; an inactive bit decides 0 and sends +0 ----
        if (!ctl.done) {
            for (int v = lane; v < n; v += a.tpc) {
                const bool ina = r > 0 && inact[v];
                const float L = rows.prior(v);
                // the bit's c->v messages: zeros before the first check update of an attempt, whatever the last one left in the slots
                BitSlots<DV> q(g, msg, v);
                float S = 0.0f;
                if (k > 0) {
                    S = q.fetch();
                    P[v] = ina ? 0.0f : L + S;
                    if (k == T) continue;
                } else {
                    q.zeros();
                }
                if (ina) {
                    q.zeros();
                    q.store_zeros(0.0f);
                    continue;
                }
                const float x = S + L;
                if (k > 0) q.store(x);
                else q.store_zeros(x);
            }
        }
        __syncthreads();
        if (*ws.ndone == cw.nact) break;  // the same word for every thread, last written before the barrier above
        if (!ctl.done) {
            // ---- groups: the next pick is posted ahead.  Plain BP's last test (P is complete): the scores, and every key; step 0 of
            // attempt r: the adjacent marks of its group, and the keys above its own ----
            if (r == 0 ? (k == T && a.legs.num_legs > 1) : k == 0) {
                if (r > 0) {
                    const int a0 = a.t.aptr[grp], a1 = a.t.aptr[grp + 1];
                    for (int t = a0 + lane; t < a1; t += a.tpc) adjpos[a.t.adj[t]] = (uint8_t)(1 + t - a0);
                }
                if (r + 1 < a.legs.num_legs)
                    for (int j = lane; j < g.m_z; j += a.tpc) {
                        unsigned sb;
                        if (r == 0) {
                            const int c0 = g.cptr[m + j], c1 = g.cptr[m + j + 1];
                            float s = 0.0f;
                            for (int e = c0; e < c1; ++e) s = s + __builtin_fabsf(P[g.cvn[e]]);
                            sb = c1 > c0 ? fg_f2u(s) : SI_NO_SCORE;
                            score[j] = sb;
                        } else {
                            sb = score[j];
                        }
                        const u64 kj = ((u64)sb << 32) | (u64)(unsigned)j;
                        if (sb != SI_NO_SCORE && (r == 0 || kj > cur)) atomicMin(&key[(r + 1) & 1], kj);
                    }
            }
            // ---- checks: parity of the decisions (k > 0), then the min-sum update (k < T).  Odd parity marks the step on a
            // non-adjacent check and sets the check's bit of the residual word on an adjacent one ----
            const auto odd = [&](const unsigned ap) {
                if (ap) atomicOr(&res[step & 1], 1ull << (ap - 1u));
                else ws.stamp[cwl] = step;
            };
            int i = 0;
            for (int c = lane; c < m; c += a.tpc, ++i) {
                const unsigned ap = r > 0 ? adjpos[c] : 0u;
                bit_check<DV, DC>(g, msg, P, c, synd.at(g, rows, i, c), k > 0, k < T, a.factor, [&] { odd(ap); });
            }
        }
        __syncthreads();
        // ---- per codeword: the solve, solution found, attempt over (the pick), codeword finished (fgnn_legs.h) ----
        if (!ctl.done) {
            if (lane == 0) res[(step + 1) & 1] = 0ull;  // read a step ago, set a step from now
            if (k == 0) {
                ctl.more();
            } else {
                const bool quiet = ws.stamp[cwl] != step;  // every non-adjacent check is satisfied
                const u64 rr = res[step & 1];
                bool solved = quiet;
                if (quiet && r > 0)
                    for (int t = a.t.kptr[grp]; t < a.t.kptr[grp + 1]; ++t)
                        if (__popcll(rr & a.t.cons[t]) & 1) solved = false;
                const LegTest t = ctl.test(a.legs, quiet ? k : T, solved);
                if (t.leg_end) {
                    // a solution, or plain BP's last decision, which a codeword that nothing rescues keeps
                    if (solved || r == 0) {
                        for (int v = lane; v < n; v += a.tpc) a.hard_out[rows.at(v)] = (uint8_t)(P[v] < 0.0f);
                        if (r > 0)
                            for (int e = g.cptr[m + grp]; e < g.cptr[m + grp + 1]; ++e) {
                                const int v = g.cvn[e];
                                if (v % a.tpc == lane) a.hard_out[rows.at(v)] = (uint8_t)(__popcll(rr & a.t.xmask[e - g.E_x]) & 1);
                            }
                    }
                    if (t.fin) {
                        if (lane == 0) {
                            int32_t* st = a.stats + (size_t)in.b * 4;
                            st[0] = solved ? 1 : 0;
                            st[1] = r;  // without a solution: the last attempt, that is the attempts made
                            st[2] = solved ? k : 0;
                            st[3] = (solved && r > 0) ? grp : -1;
                            atomicAdd(ws.ndone, 1);
                        }
                        ctl.finish();
                    } else {
                        // the marks of this attempt's group go, the group posted for the next one comes: a bit's owner writes its mark
                        const u64 win = key[(r + 1) & 1];
                        if (r > 0) {
                            for (int e = g.cptr[m + grp]; e < g.cptr[m + grp + 1]; ++e) {
                                const int v = g.cvn[e];
                                if (v % a.tpc == lane) inact[v] = 0;
                            }
                            for (int t2 = a.t.aptr[grp] + lane; t2 < a.t.aptr[grp + 1]; t2 += a.tpc) adjpos[a.t.adj[t2]] = 0;
                        }
                        grp = (int)(unsigned)(win & 0xFFFFFFFFull);
                        cur = win;
                        for (int e = g.cptr[m + grp]; e < g.cptr[m + grp + 1]; ++e) {
                            const int v = g.cvn[e];
                            if (v % a.tpc == lane) inact[v] = 1;
                        }
                        // the other word: read an attempt ago, posted to in the next step
                        if (lane == 0) key[r & 1] = ~0ull;
                        ctl.next_leg();
                    }
                } else {
                    ctl.more();
                }
            }
        }
    }
}

template <typename T>
int si_upload(const fgnn_graph* g, int slot, const std::vector<T>& h)
{
    const size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    hipError_t e = hipMalloc(&g->si_alloc[slot], bytes);
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(g->si_alloc[slot], h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        for (void*& p : g->si_alloc) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
        return fgnn_fail(FGNN_ERR_HIP, std::string("uploading the inactivation tables: ") + hipGetErrorString(e));
    }
    return FGNN_OK;
}

// The solve tables of a graph that has none yet (fgnn_si_decode takes a const handle: the tables are mutable members, as the greedy
// layerings are).  Per group: Gauss-Jordan on M = H[adjacent, I] with the columns in ascending order and T, the product of the row
// operations, next to it (T M = the reduced matrix, T starts as the identity: one 64-bit row per adjacent check).  A column without a
// pivot among the rows not yet used depends on the earlier ones: x = 0.  A pivot column c with pivot row p has x_c = (T r)_p once the
// dependent columns are 0; a row that never became a pivot is empty in the end, and r is consistent iff (T r) is 0 there.
int si_ensure(const fgnn_graph* g)
{
    if (g->si_state > 0) return FGNN_OK;
    if (g->si_state < 0) return fgnn_fail(FGNN_ERR_ARG, g->si_error);
    const GraphDev& d = g->d;
    std::vector<int> vp(d.n + 1, 0);  // hx by bit: the checks of bit v are h_chk[0][vp[v] .. vp[v+1])
    for (int v : g->h_var[0]) vp[v + 1]++;
    for (int v = 0; v < d.n; ++v) vp[v + 1] += vp[v];
    std::vector<std::vector<int>> bits(d.m_z);  // the edges are sorted by (bit, check): a group's bits arrive ascending
    for (int e = 0; e < d.E_z; ++e) bits[g->h_chk[1][e]].push_back(g->h_var[1][e]);
    std::vector<int> aptr(d.m_z + 1, 0), kptr(d.m_z + 1, 0), adj;
    std::vector<u64> cons, xmask;
    int groups = 0;
    const auto refuse = [&](const std::string& s) {
        g->si_state = -1;
        g->si_error = s;
        return fgnn_fail(FGNN_ERR_ARG, s);
    };
    for (int j = 0; j < d.m_z; ++j) {
        const std::vector<int>& I = bits[j];
        groups += !I.empty();
        if ((int)I.size() > FGNN_SI_MAX_GROUP_BITS)
            return refuse("group " + std::to_string(j) + " (row " + std::to_string(j) + " of side 1) has " + std::to_string(I.size()) +
                          " bits: stabilizer inactivation takes groups of up to " + std::to_string((int)FGNN_SI_MAX_GROUP_BITS));
        std::vector<int> A;
        for (int v : I) A.insert(A.end(), g->h_chk[0].begin() + vp[v], g->h_chk[0].begin() + vp[v + 1]);
        std::sort(A.begin(), A.end());
        A.erase(std::unique(A.begin(), A.end()), A.end());
        if ((int)A.size() > FGNN_SI_MAX_ADJACENT)
            return refuse("group " + std::to_string(j) + " (row " + std::to_string(j) + " of side 1) has " + std::to_string(A.size()) +
                          " adjacent checks: the solve tables of stabilizer inactivation hold " + std::to_string((int)FGNN_SI_MAX_ADJACENT));
        const int na = (int)A.size(), ni = (int)I.size();
        std::vector<uint32_t> M(na, 0u);
        std::vector<u64> Tm(na);
        std::vector<char> used(na, 0);
        for (int i = 0; i < na; ++i) Tm[i] = 1ull << i;
        for (int c = 0; c < ni; ++c)
            for (int e = vp[I[c]]; e < vp[I[c] + 1]; ++e)
                M[std::lower_bound(A.begin(), A.end(), g->h_chk[0][e]) - A.begin()] |= 1u << c;
        std::vector<int> piv(ni, -1);
        for (int c = 0; c < ni; ++c) {
            int p = -1;
            for (int i = 0; i < na && p < 0; ++i)
                if (!used[i] && ((M[i] >> c) & 1u)) p = i;
            if (p < 0) continue;
            used[p] = 1;
            piv[c] = p;
            for (int i = 0; i < na; ++i)
                if (i != p && ((M[i] >> c) & 1u)) {
                    M[i] ^= M[p];
                    Tm[i] ^= Tm[p];
                }
        }
        for (int c = 0; c < ni; ++c) xmask.push_back(piv[c] >= 0 ? Tm[piv[c]] : 0ull);  // a T row is final after the last column only
        for (int i = 0; i < na; ++i)
            if (!used[i]) cons.push_back(Tm[i]);
        adj.insert(adj.end(), A.begin(), A.end());
        aptr[j + 1] = (int)adj.size();
        kptr[j + 1] = (int)cons.size();
    }
    int rc;
    if ((rc = si_upload(g, 0, aptr)) || (rc = si_upload(g, 1, adj)) || (rc = si_upload(g, 2, kptr)) || (rc = si_upload(g, 3, cons)) ||
        (rc = si_upload(g, 4, xmask)))
        return rc;
    g->si_groups = groups;
    g->si_state = 1;
    return FGNN_OK;
}

}  // namespace

extern "C" int fgnn_si_decode(const fgnn_graph* g, float normalization_factor, int num_iter, int si_iter, int max_groups,
                              const float* llr_ch, float llr_const, const uint8_t* synd, int B, const int32_t* index, int nact,
                              uint8_t* hard_out, int32_t* stats, void* stream)
{
    if (!g) return fgnn_fail(FGNN_ERR_ARG, "graph is NULL");
    if (g->host_only) return fgnn_fail(FGNN_ERR_ARG, "a host-only graph cannot decode");
    if (B < 0) return fgnn_fail(FGNN_ERR_ARG, "B must be >= 0");
    if (num_iter < 1 || si_iter < 1) return fgnn_fail(FGNN_ERR_ARG, "num_iter and si_iter must be >= 1");
    if (max_groups < 0) return fgnn_fail(FGNN_ERR_ARG, "max_groups must be >= 0");
    if (int err = bit_check_list(index, B, nact)) return err;  // as fgnn_gdg_decode: no list = all B samples
    if (B == 0 || nact == 0) return FGNN_OK;  // nothing to decode needs no buffers
    if (!hard_out || !stats) return fgnn_fail(FGNN_ERR_ARG, "no output buffer");
    const LaunchGeom L = fgnn_geom(g, nact);
    SiArgs a;
    // per codeword: E_x messages, n posteriors, m_z scores, n inactive and m_x adjacent bytes; per workgroup: four 64-bit words per codeword
    size_t lds_bytes;
    if (int err = bit_lds_bytes(a, g, L, "BP-SI", {{4 * (size_t)g->d.m_z, &a.s_off}, {(size_t)g->d.n, &a.i_off}, {(size_t)g->d.m_x, &a.a_off}},
                                4, &lds_bytes))
        return err;
    FGNN_DEVICE_GUARD(g->device);
    if (int err = si_ensure(g)) return err;
    const int attempts = std::min(max_groups, g->si_groups);
    bit_args_fill(a, nact, {num_iter, attempts + 1, si_iter, 1}, normalization_factor, llr_ch, llr_const, synd);
    a.index = index;
    a.hard_out = hard_out;
    a.stats = stats;
    a.t.aptr = static_cast<const int*>(g->si_alloc[0]);
    a.t.adj = static_cast<const int*>(g->si_alloc[1]);
    a.t.kptr = static_cast<const int*>(g->si_alloc[2]);
    a.t.cons = static_cast<const u64*>(g->si_alloc[3]);
    a.t.xmask = static_cast<const u64*>(g->si_alloc[4]);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return bit_dispatch(g, FGNN_CN_MINSUM, true, [&](auto, auto dv, auto dc) {
        return fgnn_launch(si_kernel<decltype(dv)::value, decltype(dc)::value>, dim3(L.blocks), dim3(L.threads), lds_bytes, st, g->d, a);
    });
}
