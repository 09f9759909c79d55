/* fgnn.h — C ABI of the MI355X-native BP4 + feedback-GNN decoder (libfgnn_hip.so).
 *
 * The reference (gongaa/Feedback-GNN, a Sionna/TensorFlow fork) has no FFI: its boundary is the
 * Keras-Layer call contract.  This header is the C boundary placed directly beneath the Python
 * classes that keep the reference's names (feedback_gnn_amd/decoding_q.py, feedback_gnn.py).
 * Each entry point cites the reference code it replaces (paths relative to /root/reference).
 *
 * Conventions
 *   - plain C types only; every data pointer is a DEVICE pointer (HIP) unless marked "host";
 *   - the caller owns all buffers; the library owns only the immutable tables inside fgnn_graph /
 *     fgnn_weights; no allocation, no synchronisation on the hot path: all work is enqueued on
 *     `stream` (a hipStream_t passed as void*);
 *   - every per-codeword array is codeword-major ("batch first"), contiguous:
 *       llr      float32 [B,3,n]   planes (x,y,z): L_E = log(P(I)/P(E)), positive = no error
 *       synd_x   uint8   [B,m_x]   hx * noise_z mod 2          synd_z uint8 [B,m_z]  hz * noise_x mod 2
 *       x_hat    uint8   [B,n]     z_hat uint8 [B,n]
 *       messages float32 [B,E]     canonical edge order = sorted by (qubit, check)
 *   - return value 0 = OK, negative = error; text via fgnn_last_error().
 */
#ifndef FGNN_H
#define FGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fgnn_graph fgnn_graph;     /* Tanner graphs + row sets of one CSS code, on one device */
typedef struct fgnn_weights fgnn_weights; /* one feedback GNN's 3 923 parameters, on one device */
typedef struct fgnn_gnnbp4_weights fgnn_gnnbp4_weights; /* parameters of one GNN_BP4 decoder, on one device */

enum { FGNN_CN_BOXPLUS = 0, FGNN_CN_BOXPLUS_PHI = 1, FGNN_CN_MINSUM = 2 }; /* decoding_q.py:97-107 */
enum { FGNN_ROWS_X_LOGIT = 0, FGNN_ROWS_Z_LOGIT = 1, FGNN_ROWS_HX_PERP = 2, FGNN_ROWS_HZ_PERP = 3, FGNN_ROWS_LX = 4, FGNN_ROWS_LZ = 5 };

enum {
    FGNN_OK = 0,
    FGNN_ERR_ARG = -1,     /* shape / value rejected (the Python shim raises ValueError) */
    FGNN_ERR_HIP = -2,     /* a HIP runtime call failed */
    FGNN_ERR_STATE = -3,   /* e.g. row set missing */
    FGNN_ERR_NOMEM = -4
};

const char* fgnn_last_error(void);
int fgnn_version(void); /* 2 = this header (round 3: trace entry point, general GNN_BP4, options 4 and 5 default on) */

/* QLDPCBPDecoder.__init__ edge tables, decoding_q.py:53-94: built here from COO lists of hx and hz
 * (host pointers, any order).  `device` = HIP device ordinal. */
int fgnn_graph_create(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                      const int32_t* chk_z, const int32_t* var_z, int device, fgnn_graph** out);
void fgnn_graph_destroy(fgnn_graph* g);

/* Extra binary row sets as COO (host pointers):
 *   FGNN_ROWS_X_LOGIT / Z_LOGIT : pcm_x_perp / pcm_z_perp of decoding_q.py:33-37,93-94
 *                                 (hz / hx when stage_one or stage_two, else hx_perp / hz_perp);
 *   FGNN_ROWS_HX_PERP / HZ_PERP : code.hx_perp / code.hz_perp for the residual check,
 *                                 feedback_gnn.py:352-353;
 *   FGNN_ROWS_LX / LZ           : code.lx / code.lz, the logical rows appended to the soft syndromes of
 *                                 GNN_BP4.cal_logit, gnn.py:305-313. */
int fgnn_graph_set_rows(fgnn_graph* g, int which, int rows, int nnz, const int32_t* row, const int32_t* col);

/* Launch geometry of the LDS-resident kernels: threads per codeword and codewords per workgroup.
 * 0 = keep the built-in heuristic.  (No reference equivalent: XLA picks its own launch shapes.) */
int fgnn_graph_set_launch(fgnn_graph* g, int threads_per_codeword, int codewords_per_block);
/* Options.  FGNN_OPT_SATURATION_SHORTCUT (default 1): the BP4 kernels (compile-time and runtime degrees) skip the exp/log evaluation
 * of a wave whose 64 nodes are all saturated (|v->c| >= 16.635532 at a check; totals beyond the softplus threshold
 * and 20 apart at a qubit), writing the values those evaluations produce bit for bit (phi(clip max) = 0,
 * phi(clip min), log(1) = 0); and a decode from zero messages and one constant channel LLR (the first decoder of a sandwich) on a
 * degree-regular graph starts from the closed form of its first iteration (every qubit sends the same value, a check's outputs
 * differ by the syndrome sign alone: the same float operations, evaluated once per thread).  Results are identical with 0 and 1; 0 evaluates every transcendental like the
 * reference's fixed dataflow (decoding_q.py:732-767) and is what bench.py's headline number uses.
 * FGNN_OPT_FIXED_POINT_EXIT (default 1, effective only with the shortcut on, boxplus-phi, one codeword per workgroup,
 * at most 32 edges per qubit):
 * when two consecutive check-node phases were all-saturated and no c->v sign changed in between, the messages are at a
 * bit-exact fixed point of the (deterministic) iteration map, every remaining iteration is the identity, and the
 * workgroup leaves the loop.  Results are identical with 0 and 1.
 * FGNN_OPT_HW_TRANSCENDENTALS (default 0; opt-in, NOT bit-exact, never used by a parity test or by bench.py's headline):
 * boxplus-phi decodes evaluate exp / log on the hardware's v_exp_f32 / v_log_f32 units instead of the shared float32 routines
 * of fgnn_math.h, in the fixed dataflow (the two exact options above are proofs about fgnn_math.h and are ignored while this is
 * set).  Same TensorFlow op structure (softplus thresholds, max-shifted log-sum-exp, _phi clip; _phi's two clip points pinned to
 * 0 and 16.635532, the values the reference's saturation known answer fixes), ~1 ulp per elementary function, but bits that no
 * CPU oracle reproduces: on non-converged samples decisions may differ from the default path's (chaotic
 * transients).  bench.py reports its rate and its measured agreement with the exact kernel under `extras`.
 * FGNN_OPT_GNN_FACTORED and FGNN_OPT_BP4_SHARED_LSE (both default 0 since round 6; OPT-IN re-associations of the reference's own formulas, same
 * real-number functions, NOT the reference's float32 operation sequence).  The library's default evaluates the reference's formulas term
 * by term — one 40 -> 20 Dense per edge (feedback_gnn.py:175-184), one reduce_logsumexp per edge (decoding_q.py:254-273) — and that is what
 * bench.py's `value`, smoke() and every default parity test run.
 * FGNN_OPT_GNN_FACTORED = 1: the feedback GNN's message MLP and mean (feedback_gnn.py:175-184) in the factored association:
 * [g, X, Y, Z] W1 + b1 = g W1[0,:] + ([X, Y, Z] W1[1:4,:] + b1) with the bracket formed once per qubit and side, and
 * mean_e(h_e W2 + b2) = (sum_e h_e) W2 / deg + b2 with ONE 40 -> 20 Dense per qubit and side instead of one per edge.  float32 results
 * differ from the literal association's by rounding only (measured <= 5e-7 on GNN outputs of magnitude 0.2 .. 2.7).  Applies to the kernels
 * of the shipped architecture (fgnn_weights_create); the runtime-shaped kernel (fgnn_weights_create_general, any reduce_op) always runs the
 * literal order.
 * FGNN_OPT_BP4_SHARED_LSE = 1: the variable-node update (decoding_q.py:254-273) evaluates, on every hx edge e of a qubit,
 * reduce_logsumexp([-(Z - mu_e), -(Y - mu_e)]) = max(.,.) + log(1 + exp(-|(Z - mu_e) - (Y - mu_e)|)), and the last term's argument is
 * Z - Y for all of the qubit's edges: with the option on it is formed once per qubit and side from the unshifted totals (the per-edge
 * max term stays as it is) — 4 instead of 8 exp/log pairs per qubit and iteration.  A v->c message moves by the rounding of two
 * subtractions, and BP's transient amplifies that like any other float32 rounding.
 * What a caller who turns both on gets, against the default, per sample through the whole sandwich (these are MEASURED RATES, not
 * guarantees; bench.py prints the same comparison for its timed batch under extras.reassociated_forms.forms_agreement):
 *     north-star bar = decisions identical and LLRs within 1e-4.  [[882,24]] (64, G, 16), p = 0.01, 65 536 samples per window: 0 samples
 *     with a different decision in most windows, but NOT in all: the driver's round-5 batch (global samples 327 680 - 393 215) has one
 *     SOLVED sample at 1.03e-4, and 8.4 M samples hold 3 differing decisions and 40 solved samples beyond 1e-4 (up to 101)
 *     (profiles/r4_forms_agreement_8M.json); p = 0.02: 40 / 8.4 M decisions differ; p = 0.03: 2 of 65 536; 0.05: 74 (0.11 %); 0.06: 344;
 *     0.08: 2 746 (4.2 %); 0.10: 9 611 (14.7 %) end on a different — equally valid or equally failed — estimate.
 *     [[1270,28]] (64, G, 64): p = 0.01: 6 / 8.4 M; 0.03: 4 of 65 536; 0.05: 126; 0.06: 426; 0.08: 4 539; 0.10: 15 177 (23 %).
 *     BASELINE configs[0] as the reference constructs it ('boxplus', 0.625, p = 0.05, 256 samples): 0 decisions differ but 250 of the 256
 *     solved samples are beyond 1e-4 (max 0.575): the 'boxplus' rule does not saturate its messages, so rounding differences persist.
 *     Published workloads (batch 5 000 / 50 000): n1270_3r (p = 0.07) 144 of 5 000 decisions differ; osd_bp4_minsum (p = 0.09) 1 497 of 50 000.
 * So the re-associated forms are the reference's decoder only STATISTICALLY: BP4-64 decodes the same number of samples (24 M compared
 * at p = 0.06 .. 0.10 on both codes: differences within 1.8 sigma, both signs, profiles/r3j_bp4_shared_lse_ab.txt), paired block-error
 * counts on 40 M samples agree (profiles/r3v_bp4_lse_forms_mcnemar.json) and the 77 published rows of the nine sandwich curves land on
 * the same z-scores (max |z| 1.89, profiles/r3k_published_curves_bp4_shared_lse.json).  They buy ~1.15x on the sandwich step.  The oracle
 * restates both forms (og_graph_set_gnn_order, og_graph_set_vn_shared_lse); the kernels equal it bit for bit in either.
 * FGNN_OPT_GNN_STREAM (default 1): which kernel runs the feedback GNN (either association) on a graph with 3, 4 or 5 checks per qubit and
 * side — the streaming VALU kernel (one lane per qubit, weights as scalar operands; the literal association's 40 -> 20 Dense per edge as
 * v_pk_fma_f32 on scalar weight pairs) or the MFMA-tile kernel ((3,3) only; other degrees: the runtime-degree kernel).  0: never the
 * streaming kernel; 1: wherever it is the faster one (from 4 096 codewords per launch on; smaller launches are latency-bound and
 * quicker on the MFMA tiles); 2: always.  The same float operations in the same
 * order: results are bit-identical; the option exists for A/B timing and tests.  No effect on irregular graphs.
 * Value 2 ALSO moves fgnn_gnnbp4_decode on a (3,3,6)-regular graph from its MFMA-tile kernel to its streaming packed-FMA kernel — the
 * tested second implementation of the same float operations, bit-identical and SLOWER (180 ms against 134 ms per 16 384 x 10
 * iterations of [[1270,28]], profiles/r4_gnnbp4_stream_ab.txt); values 0 and 1 leave GNN_BP4 on the MFMA tiles.  A caller who wants
 * "always" for the feedback GNN and times GNN_BP4 on the same graph handle should set the option back to 1 around GNN_BP4 calls. */
enum { FGNN_OPT_SATURATION_SHORTCUT = 1, FGNN_OPT_FIXED_POINT_EXIT = 2, FGNN_OPT_HW_TRANSCENDENTALS = 3, FGNN_OPT_GNN_FACTORED = 4,
       FGNN_OPT_BP4_SHARED_LSE = 5, FGNN_OPT_GNN_STREAM = 6 };
int fgnn_graph_set_option(fgnn_graph* g, int option, int value);
/* Testing hook: on != 0 forces the runtime-degree (CSR) kernel even on a degree-regular graph. */
int fgnn_graph_force_generic(fgnn_graph* g, int on);
/* info[0..9] = n, m_x, m_z, E_x, E_z, threads_per_codeword, codewords_per_block, lds_bytes_per_block,
 *              regular(0/1), device */
int fgnn_graph_info(const fgnn_graph* g, int32_t info[16]);
/* canonical (qubit, check)-sorted edge lists, host output: chk[E_s], var[E_s] for side 0 (hx) / 1 (hz) */
int fgnn_graph_edges(const fgnn_graph* g, int side, int32_t* chk, int32_t* var);
/* The per-check row tables fgnn_graph_create builds and uploads for a check-regular graph (check degree <= 8), formed on the HOST from the
 * same edge lists by the same code — no device is touched, so a test can hold them to the parity-check matrices without a GPU:
 * cslot32[m][8] = byte offsets (4 * slot) of a check's message slots (also needs degree-regular qubits and 4 E < 65536), cvn16[m][8] = its
 * qubits (needs n < 65536), both in ascending qubit order and zero padded; hx checks first, then hz.  have[0], have[1] = whether a graph of
 * these edges carries each table (a table it does not carry is not written; either output pointer may be NULL). */
int fgnn_check_rows(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z, const int32_t* chk_z,
                    const int32_t* var_z, int32_t have[2], uint32_t* cslot32, uint16_t* cvn16);

/* Per-launch timing of the BP4 and feedback-GNN kernels (no reference equivalent; sim_ber only has wall-clock per point,
 * misc.py:639,696): HIP events are recorded on the launch stream right before and after every BP4 / feedback-GNN launch,
 * standalone or inside fgnn_sandwich_decode, up to max_launches (0 disables).  fgnn_profile_read waits for the
 * last one and returns ms / tag / B per launch in host arrays of length cap; tag = num_iter of a BP4 launch,
 * -1 for a feedback-GNN launch, -2 for a GNN_BP4 launch (fgnn_gnnbp4_decode). */
int fgnn_profile_enable(fgnn_graph* g, int max_launches);
int fgnn_profile_read(fgnn_graph* g, float* ms, int32_t* iters, int32_t* batch, int cap, int32_t* count);

/* QLDPCBPDecoder.call, decoding_q.py:661-797 (flooding BP4, num_iter iterations, then marginals,
 * hard decision :783-790 and soft syndrome cal_logit :455-471).
 *   llr_ch       [B,3,n] or NULL: all three channel LLRs = llr_const (feedback_gnn.py:311-313)
 *   msg_init_*   [B,E_x]/[B,E_z] or NULL (= zeros, :726-727)        msg_out_* optional
 *   llr_out      [B,3,n] marginals (llrx, llry, llrz of :777)       x_hat,z_hat [B,n]
 *   x_logit      [B,rows(X_LOGIT)]  z_logit [B,rows(Z_LOGIT)]  (either may be NULL)
 */
int fgnn_bp4_decode(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                    float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, const float* msg_init_x,
                    const float* msg_init_z, float* llr_out, uint8_t* x_hat, uint8_t* z_hat, float* x_logit,
                    float* z_logit, float* msg_out_x, float* msg_out_z, void* stream);

/* The `trainable` / `stage_two` return mode of QLDPCBPDecoder.call (decoding_q.py:730, 743-746, 779-781, 794-795) in ONE launch:
 * the soft syndromes cal_logit (:455-471) of the marginals after 0, 1, ..., num_iter iterations,
 *   x_logit_trace [num_iter+1, B, rows(X_LOGIT)],  z_logit_trace [num_iter+1, B, rows(Z_LOGIT)]
 * (the reference's llr_hat[2k] / llr_hat[2k+1], transposed), plus the usual marginals and decisions of the last iteration.
 * tape_x [num_iter+1, B, E_x] / tape_z [num_iter+1, B, E_z] (both or neither): the c->v messages before iteration k (slot num_iter:
 * after the last) — the tape fgnn_bp4_backward reads.  Fixed dataflow on the shared float32 routines; every value equals what
 * num_iter + 1 chained fgnn_bp4_decode calls (0, 1, 1, ... iterations through msg_init / msg_out) produce, bit for bit. */
int fgnn_bp4_decode_trace(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                          float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, const float* msg_init_x,
                          const float* msg_init_z, float* llr_out, uint8_t* x_hat, uint8_t* z_hat, float* x_logit_trace,
                          float* z_logit_trace, float* tape_x, float* tape_z, void* stream);

/* load_weights, gnn.py:774-791: 12 host arrays in the reference's file order
 * [W_out(40,3), b_out(3), Wx1(4,40), bx1(40), Wx2(40,20), bx2(20), Wz1, bz1, Wz2, bz2, We(43,40), be(40)]. */
int fgnn_weights_create(const float* const host_arrays[12], int device, fgnn_weights** out);
void fgnn_weights_destroy(fgnn_weights* w);

/* Feedback_GNN with other hyper-parameters than the shipped weights' (constructor feedback_gnn.py:21-28, build :110-128):
 * num_msg_dims D <= 32, num_hidden_units H <= 96, num_mlp_layers L in 1..4, reduce_op (:139-148), the activation of the
 * hidden layers, use_bias.  host_arrays = Layer.get_weights() order: _llr_inv_embed [(L>1 ? H : 2D+3), 3] (+ bias),
 * vn_msg_mlp_x: L Dense layers 4 -> H -> ... -> D, vn_msg_mlp_z: likewise, vn_embed_mlp: L-1 Dense layers 2D+3 -> H -> ... -> H;
 * every kernel [in, out] row-major, a bias array after each kernel iff use_bias.  num_arrays must equal
 * (3L) * (1 + use_bias).  The handle is accepted wherever fgnn_weights is (fgnn_feedback_gnn, fgnn_sandwich_decode); it runs
 * a runtime-shaped VALU kernel (the MFMA kernel is specialised for D=20, H=40, L=2, mean, tanh, bias). */
typedef struct {
    int num_msg_dims, num_hidden_units, num_mlp_layers;
    int reduce_op;   /* FGNN_REDUCE_* */
    int activation;  /* FGNN_ACT_* */
    int use_bias;
} fgnn_gnn_config;
enum { FGNN_REDUCE_SUM = 0, FGNN_REDUCE_MEAN = 1, FGNN_REDUCE_MAX = 2, FGNN_REDUCE_MIN = 3 };
enum { FGNN_ACT_LINEAR = 0, FGNN_ACT_TANH = 1, FGNN_ACT_RELU = 2, FGNN_ACT_SIGMOID = 3 };
int fgnn_weights_create_general(const fgnn_gnn_config* cfg, const float* const* host_arrays, int num_arrays, int device,
                                fgnn_weights** out);

/* Feedback_GNN.call, feedback_gnn.py:161-188 (reduce_op="mean", activation="tanh", 2-layer MLPs):
 *   llr [B,3,n] = h_vn planes (llrx, llry, llrz);  logit_hx [B,m_x], logit_hz [B,m_z] soft syndromes
 *   of the hx / hz rows;  out [B,3,n] = new channel LLRs for the next BP run. */
int fgnn_feedback_gnn(const fgnn_graph* g, const fgnn_weights* w, const float* llr, const float* logit_hx,
                      const float* logit_hz, const uint8_t* synd_x, const uint8_t* synd_z, int B, float* out,
                      void* stream);

/* Pauli.call (non-wt branch), sionna/channel/pauli.py:98-108 with px=pz=2p/3, py=p/3
 * (feedback_gnn.py:298): Philox4x32-10 stream keyed by (seed, first_sample + b). */
int fgnn_pauli_noise(uint64_t seed, float p, uint64_t first_sample, int B, int n, uint8_t* noise_x, uint8_t* noise_z,
                     void* stream);
/* Pauli.call (non-wt branch) for ANY triple, sionna/channel/pauli.py:98-108: noise_x = u < px, noise_z = (u >= px - py) & (u < (px + pz) - py)
 * in float32, u the same Philox uniform as fgnn_pauli_noise (which is this call with px = pz = 2p/3, py = p/3 formed in float32).  Like
 * the reference it validates nothing but NaNs: X, Y, Z are disjoint events of probability px - py, py, pz - py when
 * 0 <= py <= min(px, pz) and px + pz - py <= 1. */
int fgnn_pauli_noise_xyz(uint64_t seed, float px, float py, float pz, uint64_t first_sample, int B, int n, uint8_t* noise_x,
                         uint8_t* noise_z, void* stream);
/* fgnn_pauli_noise with the stream position read on the DEVICE: sample b is keyed by (*first_sample_dev + offset + b).  For Monte-Carlo loops
 * captured in a hipGraph (the reference's `while` loop of misc.py:636-738 with no host in it): the graph owns an 8-byte device counter,
 * every noise launch of the captured loop reads it, and the graph's last node advances it, so each replay draws the next samples. */
int fgnn_pauli_noise_dev(uint64_t seed, float p, const uint64_t* first_sample_dev, uint64_t offset, int B, int n, uint8_t* noise_x,
                         uint8_t* noise_z, void* stream);
/* Pauli.call with wt=True, pauli.py:80-97 (training-set harvesting, Generate_dataset.ipynb): exactly `wt` qubits per sample
 * carry an error, X / Y / Z with probability 1/3 each; positions by a Philox-driven partial Fisher-Yates shuffle. */
int fgnn_pauli_noise_wt(uint64_t seed, int wt, uint64_t first_sample, int B, int n, uint8_t* noise_x, uint8_t* noise_z, void* stream);
/* syndrome_x = hx noise_z, syndrome_z = hz noise_x (mod 2), feedback_gnn.py:305-309. */
int fgnn_syndrome(const fgnn_graph* g, const uint8_t* noise_x, const uint8_t* noise_z, int B, uint8_t* synd_x,
                  uint8_t* synd_z, void* stream);
/* errors[b] &= (syndrome of (x_hat,z_hat) != (synd_z, synd_x)), feedback_gnn.py:324-330. */
int fgnn_flag_update(const fgnn_graph* g, const uint8_t* x_hat, const uint8_t* z_hat, const uint8_t* synd_x,
                     const uint8_t* synd_z, int B, uint8_t* errors, void* stream);
/* x_hat[b], z_hat[b] <- x_upd[b], z_upd[b] where errors[b], feedback_gnn.py:339-340. */
int fgnn_merge(const uint8_t* errors, const uint8_t* x_upd, const uint8_t* z_upd, int B, int n, uint8_t* x_hat,
               uint8_t* z_hat, void* stream);
/* Residual check, feedback_gnn.py:343-361: s_hat [B,m_z+m_x] = [hz xd ; hx zd], ls_hat
 * [B,rows(hx_perp)+rows(hz_perp)] (either may be NULL), flags[b] bit0 = any(s_hat), bit1 = any(ls_hat)
 * (= what count_block_errors sees, sionna/utils/metrics.py:221-223 via misc.py:649-651). */
int fgnn_residual(const fgnn_graph* g, const uint8_t* noise_x, const uint8_t* noise_z, const uint8_t* x_hat,
                  const uint8_t* z_hat, int B, uint8_t* s_hat, uint8_t* ls_hat, uint8_t* flags, void* stream);
/* Same with the two row sets chosen by the caller: ls_hat = [rows_x . xd ; rows_z . zd], e.g. (FGNN_ROWS_LZ, FGNN_ROWS_LX) for
 * BP4_OSD_Model.call, bp_osd.py:184-188. */
int fgnn_residual_rows(const fgnn_graph* g, int rows_x, int rows_z, const uint8_t* noise_x, const uint8_t* noise_z,
                       const uint8_t* x_hat, const uint8_t* z_hat, int B, uint8_t* s_hat, uint8_t* ls_hat, uint8_t* flags, void* stream);
/* Bit-packed decisions for the multi-GPU gather (no reference equivalent: the reference runs one process per GPU id and
 * never collects decisions, n882.py:9,15-21): packed[b] = the 2n bits [x_hat[b,:] | z_hat[b,:]], most significant bit first
 * (numpy.packbits order), ceil(2n/8) bytes per codeword; fgnn_unpack_decisions is the inverse.  Runs on the current device. */
int fgnn_pack_decisions(const uint8_t* x_hat, const uint8_t* z_hat, int B, int n, uint8_t* packed, void* stream);
int fgnn_unpack_decisions(const uint8_t* packed, int B, int n, uint8_t* x_hat, uint8_t* z_hat, void* stream);
/* counts[0] += #flagged, counts[1] += #block errors, counts[2] += B (device uint64[3]), misc.py:649-669. */
int fgnn_count_flags(const uint8_t* flags, int B, uint64_t* counts, void* stream);
/* The same for num_batches consecutive batches of `batch` samples whose flags lie back to back in flags[num_batches * batch] (the
 * batches were decoded as one launch): ring[3 j .. 3 j + 2] = the cumulative counters after batch j, counts = ring of the last batch —
 * what num_batches calls of fgnn_count_flags would have produced one after the other, so the stopping rule of sim_ber
 * (misc.py:700-738) can be applied batch by batch afterwards.  scratch: device uint32[2 * num_batches].  Current device. */
int fgnn_count_flags_batches(const uint8_t* flags, int num_batches, int batch, uint64_t* counts, uint64_t* ring, uint32_t* scratch,
                             void* stream);

/* Sandwich_BP_GNN_Evaluation_Model.call, feedback_gnn.py:293-361, from the syndromes on:
 * decoder 0, then for i = 1..num_layers-1: flag update, GNN i-1, decoder i, masked merge.
 * iters/factors/cn_types: host arrays [num_layers]; weights: host array of num_layers-1 handles.
 * Needs the logit row sets to be (hz, hx) ("stage_one").  compact != 0 runs the GNN/BP rounds only on
 * the samples still in `errors` (same x_hat/z_hat, fewer FLOPs; llr_final then holds the last marginals
 * computed for each sample).  rounds[b] (optional) = rounds in which sample b was still in `errors`. */
size_t fgnn_sandwich_workspace_bytes(const fgnn_graph* g, int B);
int fgnn_sandwich_decode(const fgnn_graph* g, int num_layers, const int32_t* iters, const float* factors,
                         const int32_t* cn_types, const fgnn_weights* const* weights, float llr_const,
                         const uint8_t* synd_x, const uint8_t* synd_z, int B, int compact, uint8_t* x_hat,
                         uint8_t* z_hat, float* llr_final, uint8_t* rounds, void* workspace, size_t ws_bytes,
                         void* stream);

/* Binary syndrome BP — LDPCBPDecoder.call with is_syndrome=True, sionna/fec/ldpc/decoding.py:874-1048 (SURVEY.md §8f
 * rank 1).  The parity-check matrix is side 0 (hx) of the graph.  llr_ch [B,n] are LOGITS as in the reference (clipped
 * to +-20, sign flipped on entry and exit, :918-920,:940,:1031) or NULL (= llr_const everywhere); synd [B,m_x] or NULL
 * (all-zero syndrome = ordinary decoding).  soft_out [B,n] = output logits, hard_out [B,n] = (0 < logit) (:1033-1034). */
int fgnn_bp2_decode(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                    float llr_const, const uint8_t* synd, int B, float* soft_out, uint8_t* hard_out, void* stream);
/* Relay-BP (Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories", 2025): a chain of
 * num_legs min-sum BP runs ("legs") on side 0 (hx) with per-bit memory strengths gamma [num_legs,n] (device float32, shared by the
 * batch); every leg starts from the posteriors the previous one ended with, and the lowest-weight solution met is kept.  llr_ch /
 * llr_const / synd as fgnn_bp2_decode.  All arithmetic is float32 in the order written; sums run over a bit's slots in ascending
 * order from 0.0f.  Per codeword:
 *     L_v = -1 * clamp(llr_v, -20, 20);  q_v = (int32) rint(1024 * L_v);  P_v = L_v;  found = 0
 *     for r in 0 .. num_legs-1:   T = pre_iter if r == 0 else leg_iter;  mu_e = 0 on every edge;  gam_v = gamma[r, v]
 *         for k in 0 .. T:                                   (k = finished check updates of this leg)
 *             S_v = sum of mu_e over the bit's edges
 *             if k > 0:  P_v = Lam_v + S_v;  d_v = (P_v < 0)
 *                        if H d == s:  w = sum_v d_v q_v;  found += 1;  if found == 1 or w < best_w: best = (d, w, r, k);  end this leg
 *                        if k == T: end this leg
 *             Lam_v = (1.0f - gam_v) * L_v + gam_v * P_v     (two products, then one add)
 *             x = S_v + Lam_v;  nu_e = x - mu_e on the bit's edges;  mu = min-sum check update of nu (clip +-20, * normalization_factor)
 *         if found == stop_nconv: stop
 * hard_out [B,n] = the best d if found > 0, else the d of the last test made (last leg, k = T); stats [B,4] (int32) = found, the
 * weight w of the output d, the leg and the k of the output d.  pre_iter, num_legs, leg_iter, stop_nconv >= 1.  The messages and
 * posteriors of a codeword stay in LDS for the whole launch; a graph they do not fit is refused (FGNN_ERR_ARG). */
int fgnn_relay_decode(const fgnn_graph* g, float normalization_factor, int pre_iter, int num_legs, int leg_iter, int stop_nconv,
                      const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd, int B, uint8_t* hard_out,
                      int32_t* stats, void* stream);
/* Relay-BP4: Relay-BP's memory term applied to each of a qubit's three LLRs of the quaternary decoder — a chain of num_legs min-sum BP4
 * runs ("legs") on both Tanner graphs with per-qubit memory strengths gamma [num_legs,n] (device float32, shared by the batch); every
 * leg starts from the marginals the previous one ended with, and the lowest-weight solution met is kept.  No paper states this form.
 * llr_ch [B,3,n] (X, Y, Z) or NULL (= llr_const for all three), synd_x [B,m_x] / synd_z [B,m_z] as fgnn_bp4_decode (NULL = all-zero).
 * All arithmetic is float32 in the order written; sums run over a qubit's slots in ascending order from 0.0f, exactly as
 * fgnn_bp4_decode.  Per codeword, with lam^W_v the channel LLRs (W = X, Y, Z):
 *     q^W_v = (int32) rint(1024 * clamp(lam^W_v, -20, 20)),  q^I_v = 0;   M^W_v = lam^W_v;   found = 0
 *     for r in 0 .. num_legs-1:   T = pre_iter if r == 0 else leg_iter;  all c->v messages = 0;  gam_v = gamma[r,v]
 *         for k in 0 .. T:                                   (k = finished check updates of this leg)
 *             Sx_v, Sz_v = sums of the hx / hz messages at qubit v
 *             if k > 0:  M^X = Sz + Lam^X;  M^Z = Sx + Lam^Z;  M^Y = (Sz + Sx) + Lam^Y        (BP4's marginals, on the Lam of the previous step)
 *                        d_v = argmin(0, M^X, M^Z, M^Y), first minimum wins (BP4's rule);  x_v = d_v & 1;  z_v = d_v >> 1
 *                        if hz.x == synd_z and hx.z == synd_x:  w = sum_v q^{d_v}_v  (d = 1: X, 2: Z, 3: Y);  found += 1;
 *                             if found == 1 or w < best_w: best = (x, z, w, r, k);   end this leg
 *                        if k == T: end this leg
 *             Lam^W_v = (1.0f - gam_v) * lam^W_v + gam_v * M^W_v   for W = X, Y, Z      (two products, then one add)
 *             qubit update of BP4 with Lam in place of the channel LLRs, literal form (one log-sum-exp per edge; option 5 is ignored)
 *             min-sum check update on both graphs (clip +-20, * normalization_factor)
 *         if found == stop_nconv: stop
 * x_hat, z_hat [B,n] = the best pair if found > 0, else the pair of the last test made (last leg, k = T); stats [B,4] (int32) = found,
 * the weight of the output pair, its leg, its k.  pre_iter, num_legs, leg_iter, stop_nconv >= 1.  cn_type must be FGNN_CN_MINSUM
 * (anything else: FGNN_ERR_ARG).  With gamma = 0, Lam = 1 * lam + 0 * M = lam bit for bit: one leg is then min-sum fgnn_bp4_decode
 * that stops at its first solution.  The messages, marginals and decisions of a codeword stay in LDS for the whole launch; a graph
 * they do not fit is refused (FGNN_ERR_ARG), there is no global-memory variant. */
int fgnn_relay4_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int num_legs, int leg_iter,
                       int stop_nconv, const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                       const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream);
/* BP4 with guided decimation (BP4-GD; Yao, Abu Laban, Haeger, Amat, Pfister, "Belief propagation decoding of quantum LDPC codes with
 * guided decimation", 2023, quaternary variant): when BP4 has run its iterations without a solution, the most reliable undecided qubit
 * is fixed to its current decision and BP4 goes on from the messages it has.  llr_ch [B,3,n] (X, Y, Z) or NULL (= llr_const for all
 * three), synd_x [B,m_x] / synd_z [B,m_z] as fgnn_bp4_decode (NULL = all-zero); all three cn_types.  All arithmetic is float32 in the
 * order written; sums run over a qubit's slots in ascending order from 0.0f, exactly as fgnn_bp4_decode.  Per codeword, with
 * D = decim_llr and R = min(max_rounds, n):
 *     fix_v = free for all v;  mu = 0 on every edge;  its = 0
 *     lamhat_v = channel LLRs (lam^X, lam^Y, lam^Z) of v while free; once fixed to d:
 *                d = I: (+D, +D, +D)   d = X: (-D, +0, +0)   d = Z: (+0, +0, -D)   d = Y: (+0, -D, +0)        (order X, Y, Z)
 *     for r in 0 .. R:                                   (r = number of qubits fixed so far)
 *         T = pre_iter if r == 0 else round_iter
 *         for k in 1 .. T:
 *             BP4 qubit update, literal form (one log-sum-exp per edge; options 1, 2, 3, 5 ignored), with lamhat in place of the channel LLRs
 *             check update cn_type on both graphs, * normalization_factor;   its += 1
 *             Sx, Sz = sums of the new hx / hz messages;  M^X = Sz + lamhat^X;  M^Z = Sx + lamhat^Z;  M^Y = (Sz + Sx) + lamhat^Y
 *             d_v = argmin(0, M^X, M^Z, M^Y), first minimum wins (BP4's rule);  x_v = d_v & 1;  z_v = d_v >> 1
 *             if hz.x == synd_z and hx.z == synd_x:  found = 1;  stop
 *         if r == R: stop                                (found = 0; the output is the pair of this last test)
 *         c = (0, M^X, M^Z, M^Y);  margin_v = min(c_j, j != d_v) - c_{d_v}        (>= +0; one float32 subtraction)
 *         v* = the free qubit of largest margin, lowest index on ties;  fix v* to d_{v*}.  The messages are kept.
 * x_hat, z_hat [B,n] = the pair of the last test made; stats [B,4] (int32) = found, qubits fixed, its, the k of the last test.
 * pre_iter, round_iter >= 1, max_rounds >= 0, decim_llr > 0 (anything else: FGNN_ERR_ARG); B = 0 returns FGNN_OK and needs no
 * buffers.  With max_rounds = 0 this is fgnn_bp4_decode stopped at its first solution.  The margin stands in for the paper's "largest
 * posterior probability": it is the log-ratio of the decided Pauli to the runner-up, orders the qubits by how clear their decision is,
 * needs no transcendental and does not underflow on saturated marginals, where the probabilities themselves all round to 1.  The
 * messages, decisions and fix marks of a codeword stay in LDS for the whole launch; a graph they do not fit is refused (FGNN_ERR_ARG),
 * there is no global-memory variant. */
int fgnn_bp4gd_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int round_iter, int max_rounds,
                      float decim_llr, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B,
                      uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream);
/* BP-GDG: binary min-sum BP with guided decimation guessing over a path tree (GDG; Gong, Cammerer, Renes, "Toward low-latency iterative
 * decoding of QLDPC codes under circuit-level noise", 2024; with depth = 0 and FGNN_GDG_MOST the binary BPGD of Yao et al. 2023).  BP
 * runs, a free bit is fixed ("decimated"), BP goes on from the messages it has; for the first `depth` fixes both values are tried, which
 * makes P = 2^depth paths per sample, each path then continues greedily, and the lowest-weight solution among the paths is the output.
 * One simplification against the paper: the bits are ranked by the posterior of the last test, not by a history of posteriors.
 * The decoder works on side 0 (hx).  llr_ch [B,n] logits or NULL (= llr_const everywhere) and synd [B,m_x] or NULL (all-zero) exactly
 * as fgnn_relay_decode, the +-20 clip and the sign flip included.  index (device int32 [nact]) selects the samples as in fgnn_osd0 /
 * fgnn_lsd, NULL = all B (nact is then ignored); with a list 0 <= nact <= B and the ids must be distinct; samples that are not
 * selected are left untouched in every output.  Min-sum is the only check rule.  All arithmetic is float32 in the order written; a
 * bit's slot sums run in ascending order from 0.0f.  With D = decim_llr and R = min(max_rounds, n):
 *     L_v = -1 * clamp(llr_v, -20, 20);  q_v = (int32) rint(1024 * L_v)
 * Per selected sample and per path p in 0 .. P-1, independently of every other path:
 *     fix_v = free for all v;  mu = 0 on every edge;  its = 0;  found = 0
 *     Lhat_v = L_v while free;  +D once fixed to 0;  -D once fixed to 1
 *     for r in 0 .. R:                                  (r = bits fixed so far)
 *         T = pre_iter if r == 0 else round_iter
 *         for k in 1 .. T:
 *             S_v = sum of mu over the bit's edges;  x = S_v + Lhat_v;  nu_e = x - mu_e
 *             mu = min-sum check update of nu (clip +-20, * normalization_factor), as fgnn_relay_decode;  its += 1
 *             P_v = Lhat_v + (sum of the new mu);  d_v = (P_v < 0)
 *             if H d == s:  found = 1;  w = sum_v d_v q_v;  stop this path
 *         if r == R: stop this path                     (found = 0; d of this last test is the path's output)
 *         least = (r < depth) or (tail_pick == FGNN_GDG_LEAST)
 *         v* = the free bit of smallest |P_v| if least, else of largest |P_v|; lowest index on ties
 *         val = (P_v* < 0);  if r < depth: val ^= (p >> r) & 1
 *         fix v* to val.  The messages are kept.
 * Per sample, after its paths: the output is the d of the path with found = 1 that has the smallest w, compared as signed int32, ties
 * to the lowest p; if no path found a solution, the d of path 0.  hard_out [B,n] = that d; stats [B,4] (int32) = the number of paths
 * that found a solution, the w of the output (0 when none found), the path of the output, the bits fixed on that path.  path_stats
 * [nact,P,4] (int32) or NULL = per listed sample and path (found, w or 0, bits fixed, its).
 * pre_iter, round_iter >= 1, max_rounds >= 0, 0 <= depth <= FGNN_GDG_MAX_DEPTH, tail_pick FGNN_GDG_MOST or FGNN_GDG_LEAST,
 * decim_llr > 0: anything else returns FGNN_ERR_ARG before any write.  workspace: caller-owned device memory (4-byte aligned) of
 * fgnn_gdg_workspace_bytes(g, depth, nact) bytes (nact = B without a list): nact * P * (16 + n), the four result words and the decision
 * row of every path; a smaller ws_bytes returns FGNN_ERR_ARG and the message names the required size.  B = 0 or nact = 0 returns
 * FGNN_OK and needs no buffers.  Nothing is allocated; both kernels (the paths, then the selection) run on `stream`.
 * Identities: depth = 0 and max_rounds = 0 is fgnn_relay_decode with gamma = 0, one leg and stop_nconv = 1 (hard_out, found, and on a
 * solution its weight and k = its, bit for bit); path p at depth d is a depth-0 run in which the first d picks are forced to p's bits.
 * The pick is an integer extremum of a total order ((float bits of |P_v|) << 32 with the index below) and w is an integer: nothing
 * depends on arrival order or launch geometry.  A path is a virtual codeword of its own: its messages, posteriors and fix marks stay in
 * LDS for the whole launch; a graph whose per-path state does not fit is refused (FGNN_ERR_ARG), there is no global-memory variant. */
enum { FGNN_GDG_MOST = 0, FGNN_GDG_LEAST = 1 };
enum { FGNN_GDG_MAX_DEPTH = 6 };
int fgnn_gdg_workspace_bytes(const fgnn_graph* g, int depth, int nact, size_t* bytes);
int fgnn_gdg_decode(const fgnn_graph* g, float normalization_factor, int pre_iter, int round_iter, int max_rounds, int depth,
                    int tail_pick, float decim_llr, const float* llr_ch, float llr_const, const uint8_t* synd, int B,
                    const int32_t* index, int nact, uint8_t* hard_out, int32_t* stats, int32_t* path_stats, void* workspace,
                    size_t ws_bytes, void* stream);
/* BP-SI: binary min-sum BP with stabilizer inactivation (du Crest, Mhalla, Savin, "Stabilizer inactivation for message-passing decoding
 * of quantum LDPC codes", 2022).  BP on a degenerate code stalls between errors that differ by a stabilizer; so the least reliable
 * stabilizer generator is taken, its few bits are erased ("inactivated"), BP runs again on the rest, and the erased bits are filled in
 * from a small linear system.  No big matrix is inverted.
 * H is side 0 (hx) of the graph, m_x checks by n bits.  The GROUPS are the rows of side 1 (hz): group j is the set of bits of hz row j.
 * Nothing else of side 1 is used, and hx.hz^T = 0 is not required.  llr_ch [B,n] logits or NULL (= llr_const everywhere) and synd
 * [B,m_x] or NULL (all-zero) exactly as fgnn_bp2_decode / fgnn_relay_decode, the +-20 clip and the sign flip included.  index (device
 * int32 [nact]) selects the samples as in fgnn_gdg_decode, NULL = all B (nact is then ignored); with a list 0 <= nact <= B and the ids
 * must be distinct; the rows of the samples that are not listed are left untouched in every output.  All arithmetic is float32 in the
 * order written; a bit's sum runs over its slots ascending from 0.0f; the check update is the min-sum rule of fgnn_relay_decode (clip
 * +-20 inside the rule, then * normalization_factor).  Per codeword:
 *     L_v = -1 * clamp(llr_v, -20, 20)
 *     attempt 0 (plain BP):  mu = 0;  for k = 0 .. num_iter:
 *         S_v = sum of mu over v's edges
 *         if k > 0:  P_v = L_v + S_v;  d_v = (P_v < 0)
 *                    if H d == s:  found = 1, output d, stats = (1, 0, k, -1), done
 *                    if k == num_iter: leave
 *         nu_e = (S_v + L_v) - mu_e;  mu = minsum(nu) * normalization_factor
 *     write d (the decision of k = num_iter) to hard_out: a sample nothing rescues keeps plain BP's output
 *     score_j = ((0.0f + |P_v0|) + |P_v1|) + ... over group j's bits ascending, P of that last test; groups without a bit are left out
 *     key_j = (bits(score_j) << 32) | j                 (score >= +0: the float bits order as unsigned integers)
 *     for a = 1 .. min(max_groups, number of non-empty groups):
 *         j = the group with the a-th smallest key;  I = its bits;  a check is "adjacent" if it holds a bit of I
 *         mu = 0;  for k = 0 .. si_iter:
 *             S_v as above;  if k > 0:  for v not in I: P_v = L_v + S_v, d_v = (P_v < 0);  d_v = 0 on I
 *                 if every non-adjacent check has parity(d) == s_c:
 *                     this ends attempt a whether or not the solve below succeeds
 *                     r_c = s_c ^ parity(d over c) on the adjacent checks
 *                     solve H[adjacent, I] x = r
 *                     solvable: e = d with x on I;  found = 1, output e, stats = (1, a, k, j), done
 *                     else: go to the next group
 *                 if k == si_iter: next group
 *             nu_e = (S_v + L_v) - mu_e for v not in I;  nu_e = +0.0f on every edge of a bit of I (erased in every iteration)
 *             mu = minsum(nu) * normalization_factor
 *     found = 0:  stats = (0, attempts made, 0, -1)
 * The solve is unique by definition: take the bits of I in ascending order as columns; a column that depends on the earlier ones gets
 * x = 0, the others are then determined.  With found = 1, H e == s holds exactly.  hard_out [B,n] (uint8), stats [B,4] (int32) =
 * found, the attempt a of the output, its k, its group j (-1 for attempt 0).
 * num_iter, si_iter >= 1, max_groups >= 0; NULL graph or outputs, bad counts, a graph whose state does not fit in LDS (the message
 * gives the bytes needed and the limit), a group with more than FGNN_SI_MAX_GROUP_BITS bits or with more than FGNN_SI_MAX_ADJACENT
 * adjacent checks (the message names the first such group; with max_groups = 0 too): FGNN_ERR_ARG before anything is launched or
 * written.  B = 0 or nact = 0 returns FGNN_OK and needs no buffers.
 * H[adjacent, I] depends on the group alone: on the first call the host eliminates it once per group and uploads, per group, the
 * adjacent checks, one 64-bit mask over them per bit of I (x_i = parity(r & mask_i), 0 for a dependent column) and one per
 * consistency row (solvable iff every parity(r & mask) is 0); the tables stay with the graph.  The kernel gathers r as one 64-bit
 * word, which is what limits a group to 64 adjacent checks.
 * Identities: attempt 0 is fgnn_relay_decode with one leg, gamma = 0 and stop_nconv = 1, bit for bit (hard_out, found, and on a
 * solution k).  The pick is an integer minimum of a total order: nothing depends on arrival order or launch geometry.  Messages,
 * posteriors, the m_z scores, the inactive marks and the adjacent checks' residual bits of a codeword stay in LDS for the whole launch;
 * there is no global-memory variant. */
enum { FGNN_SI_MAX_GROUP_BITS = 32, FGNN_SI_MAX_ADJACENT = 64 };
int fgnn_si_decode(const fgnn_graph* g, float normalization_factor, int num_iter, int si_iter, int max_groups, const float* llr_ch,
                   float llr_const, const uint8_t* synd, int B, const int32_t* index, int nact, uint8_t* hard_out, int32_t* stats,
                   void* stream);
/* BP4 with prior feedback: when BP4 has run its iterations without a solution, the unsatisfied checks of its last estimate choose
 * qubits whose channel LLRs are changed, and BP4 runs again: the hand-written rules the learned feedback of the GNN replaces.
 *   FGNN_FB_PERTURB    random perturbation (Poulin, Chung, "On the iterative decoding of sparse quantum codes", 2008)
 *   FGNN_FB_ENHANCED   enhanced feedback (Wang, Sanders, Poulin, "Enhanced feedback iterative decoding of sparse quantum codes", 2012)
 * llr_ch [B,3,n] (X, Y, Z) or NULL (= llr_const for all three), synd_x [B,m_x] / synd_z [B,m_z] (NULL = all-zero) and all three
 * cn_types as fgnn_bp4gd_decode.  All arithmetic is float32 in the order written; sums run over a qubit's slots in ascending order from
 * 0.0f, exactly as fgnn_bp4_decode.  Checks are numbered 0..m_x-1 (hx) and m_x..m_x+m_z-1 (hz), as for the layers.  Per codeword b, with
 * i = first_sample + b, lam the channel LLRs (never changed), F = strength and A = max_attempts:
 *     lamhat = lam;  mu = 0 on every edge;  its = 0
 *     for a in 0 .. A:                                   (a = number of feedback steps made so far)
 *         T = pre_iter if a == 0 else attempt_iter
 *         if restart and a > 0: mu = 0 on every edge
 *         for k in 1 .. T:
 *             BP4 qubit update, literal form (one log-sum-exp per edge; options 1, 2, 3, 5 ignored), with lamhat in place of the channel LLRs
 *             check update cn_type on both graphs, * normalization_factor;   its += 1
 *             Sx, Sz = sums of the new hx / hz messages;  M^X = Sz + lamhat^X;  M^Z = Sx + lamhat^Z;  M^Y = (Sz + Sx) + lamhat^Y
 *             d_v = argmin(0, M^X, M^Z, M^Y), first minimum wins (BP4's rule);  x_v = d_v & 1;  z_v = d_v >> 1
 *             if hz.x == synd_z and hx.z == synd_x:  found = 1;  stop
 *         if a == A: stop                                (found = 0; the output is the pair of this last test)
 *         U = the checks (both sides) whose parity in this last test (k = T) differs from their syndrome bit
 *         lamhat = lam, then the rule below with attempt number a + 1        (feedback never accumulates: always from lam)
 * Random draws: w(idx, att, s) = fg_philox4x32_10(lo32(i), hi32(i), idx, (att << 8) | s, lo32(seed), hi32(seed)) (fgnn_rng.h), floats
 * unit(x) = fg_u32_to_unit(x).  Streams 0-2 of fgnn_rng.h keep the fourth counter word below 256, so the channel noise of the same
 * seed is never reused.
 *   FGNN_FB_PERTURB: for every qubit v on at least one check of U, with w = w(v, a+1, 3):
 *         lamhat^X_v = lam^X_v - F * unit(w[0]);  lamhat^Y_v = lam^Y_v - F * unit(w[1]);  lamhat^Z_v = lam^Z_v - F * unit(w[2])
 *     each one product, then one subtraction, not contracted.  This is Poulin-Chung's p_W -> (1 + delta) p_W on the qubits of the
 *     frustrated checks, written in the LLR domain (lam^W = log(p_I / p_W): raising p_W by a random factor lowers lam^W by a random
 *     amount), so that no transcendental enters the definition.
 *   FGNN_FB_ENHANCED: every c in U has the key (uint64) w(c, a+1, 4)[0] << 32 | (0xFFFFFFFF - c); c* is the check of largest key;
 *     v* is the j-th qubit of c* in ascending qubit order, j = fg_fy_pick(unit(w(c*, a+1, 4)[1]), deg(c*)).  With s the syndrome bit of
 *     c* and t = s ? -F : +F, an hx check changes lamhat^Z_{v*} = lam^Z + t and lamhat^Y_{v*} = lam^Y + t, an hz check lamhat^X_{v*}
 *     and lamhat^Y_{v*} the same way.  The measured bit says that the error anticommutes with the check on an odd (s = 1) or even (s = 0)
 *     number of its qubits and the estimate says the opposite: the two Paulis that anticommute with the check are made likelier, or
 *     less likely, at one of its qubits.  A check without qubits changes nothing.
 *   All other qubits keep lam.
 * x_hat, z_hat [B,n] = the pair of the last test made; stats [B,4] (int32) = found, the a of that test, its, the k of that test.
 * rule 0 or 1, pre_iter and attempt_iter >= 1, 0 <= max_attempts <= 65535, strength finite and >= 0, restart 0 or 1 (anything else:
 * FGNN_ERR_ARG); B = 0 returns FGNN_OK and needs no buffers.  With max_attempts = 0 the result is that of fgnn_bp4gd_decode with
 * max_rounds = 0, bit for bit (stats column 1 is 0).  The original enhanced-feedback paper restarts BP from zero messages
 * (restart = 1); restart = 0 keeps them.  The messages, decisions and marks of a codeword stay in LDS for the whole launch, in the byte
 * count of fgnn_bp4gd_decode; a graph they do not fit is refused (FGNN_ERR_ARG), there is no global-memory variant. */
enum { FGNN_FB_PERTURB = 0, FGNN_FB_ENHANCED = 1 };
int fgnn_bp4fb_decode(const fgnn_graph* g, int rule, int cn_type, float normalization_factor, int pre_iter, int attempt_iter,
                      int max_attempts, float strength, int restart, uint64_t seed, uint64_t first_sample, const float* llr_ch,
                      float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat,
                      int32_t* stats, void* stream);
/* Augmented BP4 (Rigby, Olivier, Jarvis, "Modified belief propagation decoders for quantum low-density parity-check codes", Phys. Rev.
 * A 100, 012330, 2019): when BP4 has run its iterations without a solution, a random fraction of the check rows is written into the
 * matrix a second time and BP4 runs again, with fresh draws until an estimate reproduces both syndromes.  llr_ch [B,3,n] (X, Y, Z) or
 * NULL (= llr_const for all three), synd_x [B,m_x] / synd_z [B,m_z] (NULL = all-zero), all three cn_types and stats as
 * fgnn_bp4fb_decode.  All arithmetic is float32 in the order written.  Checks are numbered 0..m_x-1 (hx) and m_x..m_x+m_z-1 (hz).  Per
 * codeword b, with i = first_sample + b, lam the channel LLRs (never changed) and A = max_attempts:
 *     dup_c = 0 for every check;  mu = 0 on every edge;  its = 0
 *     for a in 0 .. A:                                   (a = number of draws made so far)
 *         T = pre_iter if a == 0 else attempt_iter
 *         if a > 0: dup_c = unit(w(c, a, 5)[0]) < density  for every check c      (float32 compare; w and unit as at fgnn_bp4fb_decode)
 *         if restart and a > 0: mu = 0 on every edge
 *         for k in 1 .. T:
 *             Sz = 0.0f;  for the qubit's hz slots in ascending order: Sz = Sz + mu_e;  if dup of that slot's check: Sz = Sz + mu_e
 *                                                                                          (a second, separate add)
 *             Sx likewise over the hx slots;  X = Sz + lam^X;  Z = Sx + lam^Z;  Y = (Sz + Sx) + lam^Y
 *             BP4 qubit update, literal form (one log-sum-exp per edge; options 1, 2, 3, 5 ignored), on these totals: the edge's own
 *             message is taken out ONCE
 *             check update cn_type on both graphs, * normalization_factor;   its += 1
 *             marginals M^X, M^Z, M^Y from the new messages with the same duplicated sums
 *             d_v = argmin(0, M^X, M^Z, M^Y), first minimum wins (BP4's rule);  x_v = d_v & 1;  z_v = d_v >> 1
 *             if hz.x == synd_z and hx.z == synd_x:  found = 1;  stop
 *         if a == A: stop                                (found = 0; the output is the pair of this last test)
 * x_hat, z_hat [B,n] = the pair of the last test made; stats [B,4] (int32) = found, the a of that test, its, the k of that test.
 * pre_iter and attempt_iter >= 1, 0 <= max_attempts <= 65535, density finite and in [0, 1], restart 0 or 1 (anything else:
 * FGNN_ERR_ARG); B = 0 returns FGNN_OK and needs no buffers.
 *   With max_attempts = 0 the result is that of fgnn_bp4gd_decode with max_rounds = 0, bit for bit: no mark is ever set, and S + mu is
 * the only add.
 *   With restart = 1, attempt a >= 1 is plain BP4 from zero messages on the code with every row of {c : dup_c} inserted once more
 * directly after itself, its syndrome bit repeated: in flooding BP from zero messages a copy sees the inputs of its original in the same
 * order, so its messages equal the original's bit for bit, and a qubit's ascending sum meets the two equal messages one after the other.
 * With restart = 0 the messages of the attempt before are kept and the copies start from their originals' messages.
 *   Rigby et al. draw a subset of fixed size.  The per-row Bernoulli draw here marks the same expected fraction of the rows, needs no
 * shuffle and depends on no order: a check's mark is a function of (seed, i, a, c) alone, so every thread that needs it re-derives it.
 * Stream 5 is apart from the channel noise (streams 0-2) and the feedback rules (3, 4) of the same seed.
 *   The messages, decisions and marks of a codeword stay in LDS for the whole launch: a mark byte per qubit on (3,3,6)-regular graphs
 * under min-sum (the per-codeword byte count of fgnn_bp4gd_decode), a mark byte per edge otherwise; a graph they do not fit is refused
 * (FGNN_ERR_ARG), there is no global-memory variant. */
int fgnn_bp4aug_decode(const fgnn_graph* g, int cn_type, float normalization_factor, int pre_iter, int attempt_iter, int max_attempts,
                       float density, int restart, uint64_t seed, uint64_t first_sample, const float* llr_ch, float llr_const,
                       const uint8_t* synd_x, const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream);
/* BP4 with message-strength control (MBP4 / AMBP4; Kuo, Lai, "Exploiting degeneracy in belief propagation decoding of quantum codes",
 * npj Quantum Information, 2022), flooding schedule: a qubit's belief is formed from its incoming check messages scaled by 1 / alpha,
 * while the message it sends back to a check has that check's own contribution removed at full strength (the inhibition term); the
 * adaptive form tries a list of alphas and keeps the first whose estimate reproduces both syndromes.  This entry point holds no
 * formula for alpha: every check output of attempt a is multiplied by factor[a], and a qubit takes the edge's own message out of the
 * totals multiplied by own[a].  Kuo-Lai's MBP4 with strength alpha_a on a check rule normalised by `base` is own[a] = alpha_a,
 * factor[a] = base / alpha_a.  factor and own are HOST arrays of num_attempts floats, shared by the batch.  llr_ch [B,3,n] (X, Y, Z)
 * or NULL (= llr_const for all three), synd_x [B,m_x] / synd_z [B,m_z] (NULL = all-zero) and all three cn_types as fgnn_bp4fb_decode.
 * All arithmetic is float32 in the order written; sums run over a qubit's slots in ascending order from 0.0f, exactly as
 * fgnn_bp4_decode.  Per codeword, with lam the channel LLRs (never changed):
 *     mu = 0 on every edge;  its = 0
 *     for a in 0 .. num_attempts-1:
 *         T = pre_iter if a == 0 else attempt_iter
 *         if restart and a > 0: mu = 0 on every edge
 *         for k in 1 .. T:
 *             Sz, Sx = sums of the hz / hx messages at qubit v;  X = Sz + lam^X;  Z = Sx + lam^Z;  Y = (Sz + Sx) + lam^Y      (BP4's totals)
 *             own_e = own[a] * mu_e                                                   (one product, not contracted into what follows)
 *             nu_e = softplus(-X) - lse2(-(Z - own_e), -(Y - own_e)) on an hx edge,
 *                    softplus(-Z) - lse2(-(X - own_e), -(Y - own_e)) on an hz edge    (literal form, one log-sum-exp per edge; options
 *                                                                                      1, 2, 3, 5 ignored)
 *             mu = check update cn_type of nu on both graphs, * factor[a];   its += 1
 *             Sx, Sz = sums of the new hx / hz messages;  M^X = Sz + lam^X;  M^Z = Sx + lam^Z;  M^Y = (Sz + Sx) + lam^Y
 *             d_v = argmin(0, M^X, M^Z, M^Y), first minimum wins (BP4's rule);  x_v = d_v & 1;  z_v = d_v >> 1
 *             if hz.x == synd_z and hx.z == synd_x:  found = 1;  stop
 * x_hat, z_hat [B,n] = the pair of the last test made; stats [B,4] (int32) = found, the a of that test, its, the k of that test.
 * 1 <= num_attempts <= 64, pre_iter and attempt_iter >= 1, restart 0 or 1, every factor[a] finite and > 0, every own[a] finite and
 * >= 0 (anything else: FGNN_ERR_ARG); B = 0 returns FGNN_OK and needs no buffers.  With own[a] = 1.0f the product is mu_e bit for bit:
 * num_attempts = 1 and own[0] = 1.0f give the result of fgnn_bp4fb_decode with max_attempts = 0 and normalization_factor = factor[0],
 * bit for bit (stats column 1 is 0).  The messages and decisions of a codeword stay in LDS for the whole launch, next to the two
 * 64-float tables of factor and own; a graph they do not fit is refused (FGNN_ERR_ARG), there is no global-memory variant. */
int fgnn_mbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                     int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z,
                     int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream);
/* Layers of the qubits, for the schedule that is serial along qubits (fgnn_mbp4_decode_serial).  layer_of[n] with values in
 * [0, num_layers), no layer empty, no two qubits of a layer sharing a check, on hx or on hz.  Arguments as fgnn_greedy_layers /
 * fgnn_validate_layers: chk / var [nnz] are the edges of the two matrices; all pointers are host pointers; fgnn_greedy_qubit_layers and
 * fgnn_validate_qubit_layers touch no device.  layer_of[v] = v with num_layers = n is always valid: the literal order 1 .. N of Kuo
 * and Lai.
 * fgnn_greedy_qubit_layers: qubits in ascending number, each into the lowest-numbered layer that holds no qubit sharing a check with it.
 * fgnn_validate_qubit_layers: FGNN_OK, or FGNN_ERR_ARG with a message naming the qubit whose layer is out of range ("qubit 3 has layer
 * 9, outside [0, 4)"), the empty layer ("layer 2 is empty"), or the two qubits of one layer and the check they share ("qubit 0 and
 * qubit 5 of layer 1 share hx check 7", "... share hz check 2 (number 9)"): checks are scanned in ascending combined number (hx rows
 * first), a check's qubits in ascending number, and the first qubit that meets an earlier one of its check in its own layer is named.
 * fgnn_graph_set_qubit_layers: layer_of = NULL installs the greedy layering (num_layers is ignored); a caller's layering is validated as
 * above and uploaded as a list of qubits per layer, ascending inside a layer; a refused layering leaves the installed one in place.
 * fgnn_graph_qubit_layers: the installed layering (*num_layers = 0 and layer_of untouched when there is none; layer_of may be NULL).
 * This layering is kept next to those of fgnn_graph_set_layers and fgnn_graph_set_bit_layers and is independent of them: installing
 * one never changes another, and none changes any flooding decoder. */
int fgnn_greedy_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                             const int32_t* chk_z, const int32_t* var_z, int32_t* layer_of, int32_t* num_layers);
int fgnn_validate_qubit_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                               const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of);
int fgnn_graph_set_qubit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of);
int fgnn_graph_qubit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of);
/* fgnn_mbp4_decode in Kuo and Lai's serial schedule: the qubits are visited one layer after the other, and a qubit sees the messages
 * the qubits of the layers before it have just sent.  Arguments, argument checks, outputs, the four stats columns and the B = 0 case
 * are those of fgnn_mbp4_decode; a graph without a qubit layering gets the greedy one (fgnn_graph_set_qubit_layers(g, 0, NULL)).  All
 * arithmetic is float32 in the order written, and every routine (totals, the edge rule with own[a], the check rules, the decision) is
 * the one of fgnn_mbp4_decode.  A codeword keeps two arrays in fgnn_bp4_decode's slot layout, nu (v->c) and mu (c->v):
 *     mu = 0 on every edge;  nu = the qubit rule of fgnn_mbp4_decode on mu = 0 (all qubits);  its = 0
 *     for a in 0 .. num_attempts-1:
 *         T = pre_iter if a == 0 else attempt_iter
 *         if restart and a > 0: mu = 0 and nu re-formed from it as above
 *         for k in 1 .. T:
 *             for l in 0 .. num_layers-1, for every qubit v of layer l (in any order: they share no check):
 *                 for every edge e = (c, v):  mu_e = output e of check update cn_type on the CURRENT nu of c's edges with c's
 *                                             syndrome bit, * factor[a]      (the bits the check update of fgnn_mbp4_decode writes to slot e)
 *                 Sz, Sx, X, Y, Z from v's mu as fgnn_mbp4_decode forms them
 *                 d_v = BP4's decision from (X, Z, Y);  x_v = d_v & 1;  z_v = d_v >> 1
 *                 nu_e = the edge rule of fgnn_mbp4_decode with own_e = own[a] * mu_e, for every edge e of v
 *             its += 1
 *             if hz.x == synd_z and hx.z == synd_x:  found = 1;  stop
 * With mu = 0 the product own[a] * mu_e is 0 for every own[a], so the first nu does not depend on the attempt.  On a graph for which
 * one layer is valid (no two qubits share a check) this is fgnn_mbp4_decode bit for bit whenever num_attempts = 1, restart = 1 or all
 * own[a] are equal; with restart = 0 and different weights the first check update of attempt a > 0 reads the nu formed with own[a-1]
 * here and with own[a] there.  No result depends on the launch geometry or on the order of the qubits inside a layer.
 *   nu, mu and a decision byte per qubit stay in LDS for the whole launch (2 E floats and n bytes per codeword, next to the two
 * 64-float tables of factor and own); a graph they do not fit is refused (FGNN_ERR_ARG) with the bytes needed and the limit, there is
 * no global-memory variant.  Runtime degrees only: there is no (3,3,6) instantiation. */
int fgnn_mbp4_decode_serial(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                            int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x,
                            const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, int32_t* stats, void* stream);
/* Soft-syndrome BP4: data and syndrome errors decoded together (Kuo, Chern, Lai, "Decoding of quantum data-syndrome codes via belief
 * propagation", 2021; Raveendran et al., "Soft syndrome decoding of quantum LDPC codes for joint correction of data and syndrome
 * errors", 2022; Berent et al., "Analog information decoding of bosonic quantum LDPC codes", 2023), flooding schedule, with the attempt
 * list of fgnn_mbp4_decode kept.  Check c carries a log-likelihood ratio gamma_c that says how far its measured bit s_c can be trusted:
 * the bit's error u_c is a degree-one variable on that check, and the decoder returns u_hat, its estimate of which syndrome bits were
 * wrong, next to the data error.  In real numbers this is hard-syndrome BP4 on the data-syndrome code [H | I]; here the extra
 * variable is one more constant input of the check rule.  One attempt with own = 1 is plain soft-syndrome flooding BP4; a descending
 * alpha list (own[a] = alpha_a, factor[a] = base / alpha_a) is Kuo, Chern and Lai's MBP4 on the data-syndrome code.
 * synd_llr_x [B,m_x] / synd_llr_z [B,m_z] hold gamma per check; NULL means the scalar gamma_x / gamma_z for every check of that side.
 * Everything not mentioned here is fgnn_mbp4_decode to the float operation: message layout, the literal qubit update with own[a],
 * factor[a], pre_iter / attempt_iter / restart, iteration counting, the four stats columns and B = 0.  Two things differ.
 * 1. Soft check rule.  A check has d edges with inputs nu_1 .. nu_d in ascending qubit order, syndrome bit s and syndrome LLR gamma.
 *    The rule of that cn_type is evaluated on the d + 1 inputs (nu_1, .., nu_d, gamma), in that order, with the same float operations.
 *    Outputs 1 .. d, times factor[a], are the new c->v messages.  Output d + 1, times factor[a], is w_c; it is stored nowhere in the
 *    message array.  Per rule, including the orders that matter for bits:
 *      boxplus-phi: a_gamma = phi(|gamma|);  T = ((a_1 + ..) + a_d) + a_gamma;  the sign of gamma enters neg like any input's sign;
 *                   w_c = with_sign(phi(T - a_gamma), neg ^ (gamma < 0)) * factor.
 *      minsum:      gamma is clipped to +-20 like the rest;  minv, min2 and nsum run over all d + 1 values in order;  w_c takes min_e
 *                   or minv by the same d == 0 test.
 *      boxplus:     t_gamma = tanh(gamma / 2), with 0 -> 1e-12;  P = (..(t_1 * t_2) .. * t_d) * t_gamma, then the syndrome sign;
 *                   w_c = (2 * atanh(clip(rcp(t_gamma) * P))) * factor, with the same small-magnitude flush and clip.
 *    Then, for every check and rule:  Gamma_c = gamma_c + w_c (one add);  u_hat_c = Gamma_c < 0.
 *    gamma = +inf is a legal value and means a perfect measurement: no rule forms a NaN from it, and u_hat_c is then 0.  Negative values
 *    are legal and mean what the rule makes of them.  NaN is unspecified.
 * 2. Joint test.  It runs after check update k, on the decisions BP4's rule forms from the new messages.  A sample is solved iff, for
 *    every hx row c, parity(z_hat over c) ^ s_c ^ u_hat_c == 0, and for every hz row c, parity(x_hat over c) ^ s_c ^ u_hat_c == 0, with
 *    u_hat that of check update k.
 * x_hat, z_hat [B,n] and u_x_hat [B,m_x], u_z_hat [B,m_z] = those of the last test made; stats [B,4] as fgnn_mbp4_decode.  A scalar
 * gamma_x or gamma_z that is NaN is FGNN_ERR_ARG; argument checks otherwise as fgnn_mbp4_decode.  With min-sum and gamma = +inf on every
 * check of degree >= 2 the clipped extra input is 20, which no clipped edge exceeds, and Gamma = +inf: x_hat, z_hat and stats are those
 * of fgnn_mbp4_decode bit for bit, and u_hat is zero.  The messages, decisions and one u_hat byte per check of a codeword stay in LDS for
 * the whole launch, next to the two 64-float tables; a graph they do not fit is refused (FGNN_ERR_ARG), there is no global-memory
 * variant. */
int fgnn_dsbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                      int attempt_iter, int restart, const float* llr_ch, float llr_const, const uint8_t* synd_x, const uint8_t* synd_z,
                      const float* synd_llr_x /* [B,m_x] or NULL */, float gamma_x, const float* synd_llr_z /* [B,m_z] or NULL */,
                      float gamma_z, int B, uint8_t* x_hat, uint8_t* z_hat, uint8_t* u_x_hat /* [B,m_x] */, uint8_t* u_z_hat /* [B,m_z] */,
                      int32_t* stats /* [B,4] */, void* stream);
/* Space-time BP4: a window of `rounds` = R >= 1 repeated, noisy syndrome measurements decoded in one launch (the phenomenological
 * noise model of fault-tolerant memory experiments), flooding schedule, with the attempt list of fgnn_mbp4_decode kept.  Before
 * measurement t a fresh data error e_t occurs, and measurement t reports s_t = H (e_0 ^ .. ^ e_t) ^ u_t with u_t its own flips.  The
 * differences of consecutive syndromes satisfy d_t = s_t ^ s_{t-1} = H e_t ^ u_t ^ u_{t-1}: R copies of the code's two Tanner graphs,
 * coupled only by binary "time" variables u_{c,t} of degree two, between check c of round t and check c of round t + 1.  The time
 * variable of the last round has degree one, which is exactly the extra input of fgnn_dsbp4_decode.
 * Inputs.  synd_x [B,R,m_x] / synd_z [B,R,m_z]: the raw measured syndromes (NULL = all zero).  prev_x [B,m_x] / prev_z [B,m_z]: the
 * syndrome a sliding window starts from (NULL = zero).  The differences are formed inside: d_{c,0} = s_{c,0} ^ prev_c and d_{c,t} =
 * s_{c,t} ^ s_{c,t-1}.  llr_ch [B,3,n] or llr_const: one prior per qubit, the same in every round.  Syndrome LLRs per side: gamma_x /
 * gamma_z for rounds 0 .. R-2 and gamma_last_x / gamma_last_z for round R-1 (+inf: the final perfect read-out; a window that is not
 * the last one passes gamma here too); synd_llr_x [B,R,m_x] / synd_llr_z [B,R,m_z], where not NULL, replace both scalars of their side.
 * Everything not mentioned here is fgnn_dsbp4_decode and fgnn_mbp4_decode to the float operation: the message layout of every round,
 * the literal qubit update with own[a], factor[a], pre_iter / attempt_iter / restart, iteration counting, the four stats columns,
 * B = 0 and the argument checks.
 * Variables.  Qubit (v,t) is a quaternary variable on the checks of round t only, with BP4's qubit rule unchanged.  Time variable
 * (c,t), t = 0 .. R-1, is binary with prior gamma_{c,t}; for t < R-1 it sits on check (c,t) and check (c,t+1), for t = R-1 on check
 * (c,t) only.  u_{c,-1} is known to be 0 and is no variable.
 * Check rule.  Check (c,t) with d edges (inputs nu_1 .. nu_d in ascending qubit order) and syndrome bit d_{c,t} evaluates the rule of
 * cn_type on the inputs (nu_1, .., nu_d, b) for t = 0 and (nu_1, .., nu_d, a, b) for t >= 1, in that order, with the same float
 * operations; a is the message from time variable (c,t-1), b the message from time variable (c,t).  Every extra input is treated as
 * fgnn_dsbp4_decode treats its one extra input:
 *   boxplus-phi: phi of the magnitude is added to T after the edges, in order (T = (((a_1 + ..) + a_d) + phi|a|) + phi|b|), and the
 *                sign enters neg;  the output for an extra input x is with_sign(phi(T - phi|x|), neg ^ (x < 0)) * factor.
 *   minsum:      the same +-20 clip;  minv, min2 and nsum run over all inputs in order;  an extra input's output takes min_e or minv by
 *                the same d == 0 test.
 *   boxplus:     tanh(x / 2) with 0 -> 1e-12 is multiplied in after the edges, in order, then the syndrome sign;  the output is
 *                (2 * atanh(clip(rcp(t_x) * P))) * factor, with the same small-magnitude flush and clip.
 * Outputs 1 .. d, times factor[a], are the new c->v messages.  The outputs for the extra inputs, times factor[a], are w_up_{c,t}
 * (towards time variable (c,t-1), only for t >= 1) and w_dn_{c,t} (towards time variable (c,t)).
 * Time variable rule, evaluated in the qubit phase together with the qubits, on the outputs of the check update before it:
 *     Gamma_{c,t} = (gamma_{c,t} + w_dn_{c,t}) + w_up_{c,t+1}  for t < R-1;   Gamma_{c,t} = gamma_{c,t} + w_dn_{c,t}  for t = R-1
 *     u_hat_{c,t} = Gamma_{c,t} < 0
 *     to check (c,t+1):  a = gamma_{c,t} + w_dn_{c,t}
 *     to check (c,t):    b = gamma_{c,t} + w_up_{c,t+1}  for t < R-1;   b = gamma_{c,t} itself, with no add, for t = R-1
 * own[a] acts on qubits only: a time variable's messages are the plain extrinsic sums above.  Before the first check update, and at
 * a restarting attempt, every w is 0 (the adds are still made).
 * Joint test, after check update k, on the decisions and the u_hat formed from the new messages.  A window is solved iff for every
 * round t, for every hx row c, parity(z_hat_t over c) ^ d_{c,t} ^ u_hat_{c,t} ^ u_hat_{c,t-1} == 0, and for every hz row c,
 * parity(x_hat_t over c) ^ d_{c,t} ^ u_hat_{c,t} ^ u_hat_{c,t-1} == 0, with u_hat_{c,-1} = 0.
 * Outputs of the last test made: x_hat, z_hat [B,R,n] = the error estimated for each round (not cumulative), u_x_hat [B,R,m_x],
 * u_z_hat [B,R,m_z], stats [B,4] as fgnn_mbp4_decode (per window).  rounds < 1 or a NaN scalar gamma is FGNN_ERR_ARG; +inf and
 * negative values are legal, as in fgnn_dsbp4_decode.  With rounds = 1, prev = NULL and gamma_last = gamma every output equals
 * fgnn_dsbp4_decode's bit for bit.  The messages, a and b slots, decisions and u_hat bytes of a whole window stay in LDS for the whole
 * launch, next to the two 64-float tables: per window 4 (R round4(E_x + E_z) + round4(R m) + round4((R-1) m)) bytes of floats plus
 * R n and R m bytes, each byte area rounded up to 16 bytes.  A window that does not fit is refused (FGNN_ERR_ARG) with a message that
 * names the bytes needed and the largest number of rounds that fits; there is no global-memory variant.  The launch is planned for
 * the window (R n qubits, R m checks); fgnn_graph_set_launch is honoured, with "codeword" read as "window", and no result depends on
 * the geometry. */
int fgnn_stbp4_decode(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                      int attempt_iter, int restart, int rounds, const float* llr_ch, float llr_const,
                      const uint8_t* synd_x /* [B,R,m_x] or NULL */, const uint8_t* synd_z /* [B,R,m_z] or NULL */,
                      const uint8_t* prev_x /* [B,m_x] or NULL */, const uint8_t* prev_z /* [B,m_z] or NULL */,
                      const float* synd_llr_x /* [B,R,m_x] or NULL */, float gamma_x, float gamma_last_x,
                      const float* synd_llr_z /* [B,R,m_z] or NULL */, float gamma_z, float gamma_last_z, int B,
                      uint8_t* x_hat /* [B,R,n] */, uint8_t* z_hat /* [B,R,n] */, uint8_t* u_x_hat /* [B,R,m_x] */,
                      uint8_t* u_z_hat /* [B,R,m_z] */, int32_t* stats /* [B,4] */, void* stream);
/* fgnn_stbp4_decode with the soft values of the last test, for a post-processor of the unsolved windows.  The arguments are those of
 * fgnn_stbp4_decode followed by marg [B,R,3,n], gam_x [B,R,m_x] and gam_z [B,R,m_z] (device float32).
 * Hard outputs: x_hat, z_hat, u_x_hat, u_z_hat and stats equal fgnn_stbp4_decode's bit for bit, for every input.
 * Unsolved window (stats[b,0] == 0): marg[b,t,0..2,v] = the totals X, Y, Z (Y = (Sz + Sx) + ly, X = Sz + lx, Z = Sx + lz, the sums
 * over the qubit's hz and hx messages each ascending from 0, as fgnn_mbp4_decode forms them) of qubit (v,t) in the last test, the
 * values its decision was taken from; gam_*[b,t,c] = Gamma_{c,t} of that test as defined above, (gamma + w_dn) + w_up for t < R-1 and
 * gamma + w_dn for t = R-1, the value u_hat_{c,t} was taken from.  Same float operations in the same order as the decoder's own: an
 * unsolved window ends at the last test of its last attempt, after which no message is sent and no check is updated, so the LDS
 * still holds the c->v messages, w_dn and w_up of that test and the values are formed again from them.  +inf is a legal Gamma.
 * Solved window (stats[b,0] == 1): every element of its rows of marg, gam_x and gam_z is +0.0f (a window solved before the end of an
 * attempt has had its messages overwritten by the next update, so no marginals are defined for it).  No element of any output is
 * left unwritten.
 * Argument checks as fgnn_stbp4_decode, in its order; then a NULL marg, gam_x or gam_z is FGNN_ERR_ARG.  B = 0 needs no buffers.  The
 * soft outputs take no LDS: a window fits here iff it fits fgnn_stbp4_decode, and is refused with the same message. */
int fgnn_stbp4_decode_soft(const fgnn_graph* g, int cn_type, int num_attempts, const float* factor, const float* own, int pre_iter,
                           int attempt_iter, int restart, int rounds, const float* llr_ch, float llr_const,
                           const uint8_t* synd_x /* [B,R,m_x] or NULL */, const uint8_t* synd_z /* [B,R,m_z] or NULL */,
                           const uint8_t* prev_x /* [B,m_x] or NULL */, const uint8_t* prev_z /* [B,m_z] or NULL */,
                           const float* synd_llr_x /* [B,R,m_x] or NULL */, float gamma_x, float gamma_last_x,
                           const float* synd_llr_z /* [B,R,m_z] or NULL */, float gamma_z, float gamma_last_z, int B,
                           uint8_t* x_hat /* [B,R,n] */, uint8_t* z_hat /* [B,R,n] */, uint8_t* u_x_hat /* [B,R,m_x] */,
                           uint8_t* u_z_hat /* [B,R,m_z] */, int32_t* stats /* [B,4] */, float* marg /* [B,R,3,n] */,
                           float* gam_x /* [B,R,m_x] */, float* gam_z /* [B,R,m_z] */, void* stream);
/* One side of a window as a binary problem, and its solution put back.  For side 0 (hx: the Z components z_hat and the flips u_x) or
 * side 1 (hz: x_hat and u_z), with h = that side's matrix, m = m_side and R = rounds, a window is H_st [e ; u] = d over GF(2):
 *   row     t m + c          check (c,t):      (h e_t)_c ^ u_{c,t} ^ u_{c,t-1} = d_{c,t}   (u_{c,-1} = 0)
 *   column  t n + v          data bit (v,t),   t = 0 .. R-1
 *   column  R n + t m + c    time bit (c,t),   t = 0 .. R-1
 * R m rows and R (n + m) columns.  The time columns form a unit lower-bidiagonal block, so H_st has full row rank R m; R = 1 is [h | I].
 * A binary graph of H_st (side 0 of a graph created from it) is what fgnn_lsd, fgnn_osd0 and fgnn_osd_ws solve it on, with llr_bin.
 * Both calls run over the list index[0..nact) of windows (device int32, distinct entries; NULL = windows 0 .. nact-1), one workgroup
 * per listed window; row i of the compact arrays belongs to window index[i], and the window's own rows are read or written in place.
 * fgnn_st_window_problem: d_out[i, t m + c] = d_{c,t} exactly as fgnn_stbp4_decode forms it from synd [B,R,m] (NULL = all zero) and
 * prev [B,m] (NULL = zero): s_{c,0} ^ prev_c, s_{c,t} ^ s_{c,t-1}, on bit 0 of each byte.  llr_out[i, t n + v] = the binary LLR of
 * the totals (X, Y, Z) = marg[b,t,0..2,v] of fgnn_stbp4_decode_soft: softplus(-X) - lse2(-Z, -Y) for side 0, softplus(-Z) -
 * lse2(-X, -Y) for side 1, the reliabilities fgnn_osd0 and fgnn_lsd form from BP4 marginals, by the same routines.  llr_out[i, R n +
 * t m + c] = gam[b,t,c] unchanged (+inf is legal: that flip is the last column any solver takes).
 * fgnn_st_window_apply: for a solution e [nact, R (n + m)] (uint8) in that column order, hat[b,t,v] = e[i, t n + v] and
 * u_hat[b,t,c] = e[i, R n + t m + c] for b = index[i]: side 0 is handed z_hat and u_x_hat, side 1 x_hat and u_z_hat.  The rows of
 * windows that are not listed are not touched.
 * Plain loads and stores, every element written by one thread: no atomics, nothing depends on the launch geometry.  Refused with
 * FGNN_ERR_ARG before any launch: a NULL graph, side outside 0..1, rounds < 1, nact < 0, R (n + m) beyond 31 bits, and, for nact > 0,
 * a NULL marg, gam, d_out, llr_out, e, hat or u_hat.  nact = 0 needs no buffers. */
int fgnn_st_window_problem(const fgnn_graph* g, int side, int rounds, const uint8_t* synd /* [B,R,m_side] or NULL */,
                           const uint8_t* prev /* [B,m_side] or NULL */, const float* marg /* [B,R,3,n] */,
                           const float* gam /* [B,R,m_side] */, const int32_t* index, int nact, uint8_t* d_out /* [nact,R m_side] */,
                           float* llr_out /* [nact,R (n+m_side)] */, void* stream);
int fgnn_st_window_apply(const fgnn_graph* g, int side, int rounds, const uint8_t* e /* [nact,R (n+m_side)] */, const int32_t* index,
                         int nact, uint8_t* hat /* [B,R,n] */, uint8_t* u_hat /* [B,R,m_side] */, void* stream);
/* Layers of the serial (layered) check schedule.  Checks are numbered 0..m_x-1 for hx and m_x..m_x+m_z-1 for hz; a layering is
 * layer_of[m_x+m_z] with values in [0, num_layers) such that every layer is non-empty and no two checks of a layer share a qubit —
 * across hx and hz too, since a qubit's update reads the messages of both sides.  All pointers are host pointers; fgnn_greedy_layers and
 * fgnn_validate_layers touch no device.
 * fgnn_greedy_layers: checks in ascending number, each into the lowest-numbered layer that holds no check sharing a qubit with it.
 * fgnn_validate_layers: FGNN_OK, or FGNN_ERR_ARG with a message naming the check whose layer is out of range, the empty layer, or
 * the two checks of one layer and the qubit they share.
 * fgnn_graph_set_layers: layer_of = NULL installs the greedy layering (num_layers is ignored); a caller's layering is validated as
 * above and uploaded as a CSR list of checks per layer.  fgnn_graph_layers: the installed layering (*num_layers = 0 and layer_of
 * untouched when there is none; layer_of may be NULL). */
int fgnn_greedy_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z, const int32_t* chk_z,
                       const int32_t* var_z, int32_t* layer_of, int32_t* num_layers);
int fgnn_validate_layers(int n, int m_x, int m_z, int nnz_x, const int32_t* chk_x, const int32_t* var_x, int nnz_z,
                         const int32_t* chk_z, const int32_t* var_z, int num_layers, const int32_t* layer_of);
int fgnn_graph_set_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of);
int fgnn_graph_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of);
/* BP4 in the layered (serial) schedule: the checks are updated one layer at a time and every update sees the results of the layers
 * before it.  Arguments, buffers and outputs as fgnn_bp4_decode (llr_ch = NULL: llr_const; msg_init_* = NULL: zeros; msg_out_*, x_logit,
 * z_logit optional; all three cn_types), and a syndrome that is NULL is all-zero.  A graph without a layering gets the greedy one
 * (fgnn_graph_set_layers(g, 0, NULL)).  All arithmetic is float32 in the order written, on the shared float32 routines of fgnn_math.h:
 * options 1, 2, 3 and 5 are ignored.  Per codeword, with mu the c->v messages:
 *     mu = msg_init, or 0
 *     for it in 0 .. num_iter-1:
 *         for l in 0 .. num_layers-1:
 *             for every check c of layer l (any order: they share no qubit):
 *                 for every edge e = (c, v) of c:
 *                     Sz_v, Sx_v = sums of the CURRENT mu over v's hz / hx slots, each ascending from 0.0f
 *                     X = Sz + lam^X_v;  Z = Sx + lam^Z_v;  Y = (Sz + Sx) + lam^Y_v                    (BP4's totals)
 *                     nu_e = softplus(-X) - lse2(-(Z - mu_e), -(Y - mu_e)) on an hx edge,
 *                            softplus(-Z) - lse2(-(X - mu_e), -(Y - mu_e)) on an hz edge               (literal form, one per edge)
 *                 mu on c's edges = check update cn_type of (nu_e)_e with c's syndrome bit, * normalization_factor
 *     marginals, decisions, soft syndromes and msg_out from the final mu: exactly what fgnn_bp4_decode returns for num_iter = 0 and
 *     msg_init = mu.
 * So num_iter = 0 is fgnn_bp4_decode with num_iter = 0, two launches chained through msg_out -> msg_init equal one launch of the
 * summed iteration count, and a layering of ONE layer (possible only when no two checks share a qubit) is the flooding schedule.
 * One codeword's messages (fgnn_bp4_decode's slot layout) and 3n floats (the channel LLRs, then the epilogue's binary LLRs) stay in
 * LDS for the whole launch; a graph they do not fit is refused (FGNN_ERR_ARG), there is no global-memory variant.  Without
 * fgnn_graph_set_launch a codeword gets at most 256 threads (a layer holds a fraction of the checks).  B = 0: FGNN_OK. */
int fgnn_bp4_decode_layered(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                            float llr_const, const uint8_t* synd_x, const uint8_t* synd_z, int B, const float* msg_init_x,
                            const float* msg_init_z, float* llr_out, uint8_t* x_hat, uint8_t* z_hat, float* x_logit,
                            float* z_logit, float* msg_out_x, float* msg_out_z, void* stream);
/* Layers of side 0 (hx) alone, for the serial schedule of the binary decoder (fgnn_bp2_decode_layered).  The rules are those of
 * fgnn_greedy_layers / fgnn_validate_layers restricted to the hx checks: layer_of[m] (m = m_x) with values in [0, num_layers), no layer
 * empty, no two checks of a layer sharing a bit.  chk / var [nnz] are the edges of the one matrix; all pointers are host pointers;
 * fgnn_greedy_bit_layers and fgnn_validate_bit_layers touch no device.
 * fgnn_greedy_bit_layers: checks in ascending number, each into the lowest-numbered layer that holds no check sharing a bit with it.
 * fgnn_validate_bit_layers: FGNN_OK, or FGNN_ERR_ARG with a message naming the check whose layer is out of range ("check 3 has layer
 * 9, outside [0, 4)"), the empty layer ("layer 2 is empty"), or the two checks of one layer and the bit they share ("check 0 and check
 * 5 of layer 1 share bit 7").
 * fgnn_graph_set_bit_layers: layer_of = NULL installs the greedy layering (num_layers is ignored); a caller's layering is validated as
 * above and uploaded as a list of checks per layer, ascending inside a layer; a refused layering leaves the installed one in place.
 * fgnn_graph_bit_layers: the installed layering (*num_layers = 0 and layer_of untouched when there is none; layer_of may be NULL).
 * This layering is kept next to the one of fgnn_graph_set_layers and is independent of it: installing one never changes the other,
 * and neither changes any flooding decoder. */
int fgnn_greedy_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int32_t* layer_of, int32_t* num_layers);
int fgnn_validate_bit_layers(int n, int m, int nnz, const int32_t* chk, const int32_t* var, int num_layers, const int32_t* layer_of);
int fgnn_graph_set_bit_layers(fgnn_graph* g, int num_layers, const int32_t* layer_of);
int fgnn_graph_bit_layers(const fgnn_graph* g, int32_t* num_layers, int32_t* layer_of);
/* Binary syndrome BP in the layered (serial) schedule: the checks of side 0 (hx) are updated one layer at a time and every update sees
 * the results of the layers before it.  Inputs as fgnn_bp2_decode: llr_ch [B,n] logits or NULL (= llr_const), synd [B,m_x] or NULL
 * (all-zero), all three cn_types, soft_out / hard_out [B,n] (one of them may be NULL).  A graph without a bit layering gets the greedy
 * one (fgnn_graph_set_bit_layers(g, 0, NULL)).  All arithmetic is float32 in the order written.  Per codeword:
 *     L_v = -1 * clamp(llr_v, -20, 20);   P_v = L_v + 0.0f;   mu_e = 0 on every edge;   it_run = 0
 *     for it in 1 .. num_iter:
 *         for l in 0 .. num_layers-1:
 *             for every check c of layer l (any order: they share no bit):
 *                 nu_e  = P_v - mu_e                          on c's edges e = (c, v)
 *                 mu_e  = check update cn_type of (nu_e)_e with c's syndrome bit, * normalization_factor
 *                         (the rules of fgnn_bp2_decode unchanged: min-sum clips nu to +-20 inside the rule)
 *                 P_v   = nu_e + mu_e                         (the new mu_e)
 *         it_run = it
 *         if stop and H d == s with d_v = (P_v < 0): leave the loop
 *     soft_out_v = -1 * P_v;   hard_out_v = (0 < soft_out_v);   stats = (H hard_out == s, it_run)
 * So num_iter = 0 returns the bytes of fgnn_bp2_decode with num_iter = 0.  stats [B,2] (int32) or NULL is written whenever it is given,
 * with stop set or not; with stop = 0 the parity test runs once, after the last iteration.  stop is 0 or 1.
 * One codeword's E_x messages and n posteriors stay in LDS for the whole launch, each area rounded up to 4 floats; a launch with stop
 * or stats keeps one more word per codeword of the workgroup.  A graph that does not fit is refused (FGNN_ERR_ARG, the message gives
 * the bytes needed and the limit); there is no global-memory variant.  Without fgnn_graph_set_launch a codeword gets at most 128 threads
 * (one thread takes a check of the layer, and a layer holds a fraction of the checks).  B = 0: FGNN_OK. */
int fgnn_bp2_decode_layered(const fgnn_graph* g, int cn_type, int num_iter, float normalization_factor, const float* llr_ch,
                            float llr_const, const uint8_t* synd, int B, int stop, float* soft_out, uint8_t* hard_out,
                            int32_t* stats /* [B,2] or NULL */, void* stream);
/* Relay-BP whose legs run in the layered (serial) schedule: fgnn_relay_decode's chain of min-sum legs with per-bit memory strengths,
 * every iteration of a leg updating the hx checks one layer at a time on running posteriors as fgnn_bp2_decode_layered does.  The
 * arguments, hard_out [B,n], stats [B,4] and the refusals are those of fgnn_relay_decode.  It runs on the bit layering of the graph
 * (fgnn_graph_set_bit_layers; a graph without one gets the greedy one) and is min-sum only.  All arithmetic is float32 in the order
 * written; a bit's sum runs over its slots in ascending order from 0.0f.  Per codeword:
 *     L_v = -1 * clamp(llr_v, -20, 20);  q_v = (int32) rint(1024 * L_v);  P_v = L_v;  found = 0
 *     for r in 0 .. num_legs-1:   T = pre_iter if r == 0 else leg_iter;  mu_e = 0 on every edge;  gam_v = gamma[r, v]
 *         for k in 1 .. T:                                   (k = finished iterations of this leg)
 *             Lam_v = (1.0f - gam_v) * L_v + gam_v * P_v     (two products, then one add; P_v is what the previous iteration, or the previous leg, ended with)
 *             P_v = Lam_v + S_v,  S_v = sum of mu_e over the bit's edges      (re-summed once per iteration; at k = 1 S_v = 0.0f)
 *             for each layer in order, for each check c of the layer:
 *                 nu_e = P_v - mu_e on c's edges;  mu = min-sum update of nu (clip +-20, * normalization_factor);  P_v = nu_e + mu_e
 *             d_v = (P_v < 0)
 *             if H d == s:  w = sum_v d_v q_v;  found += 1;  if found == 1 or w < best_w: best = (d, w, r, k);  end this leg
 *         if found == stop_nconv: stop
 * hard_out = the best d if found > 0, else the d of the last test made (last leg, k = T);  stats = found, w of the output, its leg, its k.
 * The posterior is re-summed at the head of an iteration, not corrected by the change of Lam: no rounding drift builds up over
 * hundreds of iterations and no second per-bit array is kept.  The consequence: with gamma = 0 and one leg the decisions equal those of
 * fgnn_bp2_decode_layered (min-sum, stop = 1) bit for bit at pre_iter = 1 only, where P = L + 0.0f on both sides; from the second
 * iteration on the two associate the same sum differently (Lam + (mu_0 + mu_1 + ..) here, ((L + ..) - mu_e) + mu_e' there).
 * The messages and posteriors of a codeword stay in LDS for the whole launch, laid out as for fgnn_relay_decode; a graph they do not
 * fit is refused (FGNN_ERR_ARG), there is no global-memory variant.  Without fgnn_graph_set_launch a codeword gets at most 128 threads,
 * as in fgnn_bp2_decode_layered.  B = 0: FGNN_OK. */
int fgnn_relay_decode_layered(const fgnn_graph* g, float normalization_factor, int pre_iter, int num_legs, int leg_iter, int stop_nconv,
                              const float* gamma, const float* llr_ch, float llr_const, const uint8_t* synd, int B, uint8_t* hard_out,
                              int32_t* stats, void* stream);
/* BinarySymmetricChannel on the all-zero word, BP_BSC_Model.call feedback_gnn.py:213-214: noise = u < p (Philox stream). */
int fgnn_bsc_noise(uint64_t seed, float p, uint64_t first_sample, int B, int n, uint8_t* noise, void* stream);

/* OSD-0 post-processing of BP failures — OSD0_Decoder.call / find_mrb, sionna/fec/ldpc/bp_osd.py:14-77, as driven by
 * BP4_OSD_Model.call_osd (:138-157).  fgnn_graph_set_basis installs code.pivot_hx (side 0) or
 * code.pivot_hz (side 1) (host array): the rows hx[pivot_hx] form the full-rank matrix of :147-150.  fgnn_osd0 solves, for
 * every listed sample, H_basis e = syndrome on the most reliable independent columns and writes e_hat[b,:]:
 * side 0 -> z_hat from hx and osd_llrz, side 1 -> x_hat from hz and osd_llrx (:125-131), computed from the BP4 marginals
 * marg [B,3,n], or from llr_bin [B,n] if given (BP2_OSD_Model).  synd [B,m_side] is the FULL syndrome (reduced
 * internally, :144-145).  index (device int32[nact]) selects the samples to process, NULL = all B.
 * Ties in the reliability sort keep qubit order (tf.argsort leaves them unspecified).
 * The basis may be rank-deficient (find_mrb runs on any matrix): a row whose pivot bit is not set after the elimination (an all-zero
 * row, or one that is zero on H with syndrome bit 1 — an inconsistent syndrome) writes nothing.  H_basis e = syndrome holds whenever
 * the syndrome lies in the row space of H_basis. */
int fgnn_graph_set_basis(fgnn_graph* g, int side, int rank, const int32_t* pivot_rows);
int fgnn_osd0(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
              const int32_t* index, int nact, uint8_t* e_hat, void* stream);
/* Higher-order OSD (OSD-E, OSD-CS), the osd_method / osd_order choices of ldpc.bposd_decoder (examples/OSD.ipynb cell 5), on the same
 * row basis and inputs as fgnn_osd0.  The reliabilities r, the -0 -> +0 step, the stable ascending sort into positions 0..n-1 and the
 * Gauss-Jordan elimination (pivot of a row = its first set column) are those of fgnn_osd0.  S = the pivot positions, T = the other
 * positions in ascending order (T[0] = the least reliable non-pivot column), k = |T| = n - rank, lambda = min(order, k).
 * A candidate t is a bit vector over T; its solution e(t) equals t on T and, on the pivot of reduced row i, s'[i] XOR the parity of
 * row i over the set bits of t (s' = the transformed syndrome).  Candidate 0 (t = 0) is the OSD-0 solution.  Candidates, by index c:
 *   FGNN_OSD_0   c = 0 only (order is ignored);
 *   FGNN_OSD_E   c = 0 .. 2^lambda - 1, bit i of c sets T[i] (order <= 16);
 *   FGNN_OSD_CS  c = 0, then c = 1..k the weight-1 vectors T[c-1], then the pairs {T[i], T[j]}, 0 <= i < j < lambda, in
 *                lexicographic (i, j) order: 1 + k + lambda(lambda-1)/2 candidates (order <= 64);
 *   order 0 = OSD-0 for every method.
 * Cost = soft weight, bit-reproducibly: x[p] = r_sorted[p] where e(t) has bit p, +0.0f elsewhere, zero-padded to NP (the power of
 * two >= n); for h = NP/2, NP/4, ..., 1: x[i] = x[i] + x[i+h] for i < h (float32, round to nearest, no fma); cost = x[0].  The
 * winner minimises (sortable(cost) << 32) | c, with the order-preserving float -> uint32 map of the sort key: ties go to the lowest
 * index and the answer never costs more than OSD-0.  Inputs must be finite.  e_hat[b,:] = e(winner) mapped back to qubit order;
 * chosen (device int32[B]) may be NULL, else chosen[b] = the winner's index for every processed b (other entries untouched).
 * Same n <= 2047 limit and LDS check as fgnn_osd0 (the search adds 40 bytes).  The basis may be rank-deficient: S holds only the pivots
 * of the rows whose pivot bit is set (zero rows are ignored, as in fgnn_osd0), so k = n - rank(H_basis), and every candidate solves
 * H_basis e = syndrome whenever the syndrome lies in the row space. */
enum { FGNN_OSD_0 = 0, FGNN_OSD_E = 1, FGNN_OSD_CS = 2 };
int fgnn_osd(const fgnn_graph* g, int side, int method, int order, const float* marg, const float* llr_bin, const uint8_t* synd, int B,
             const int32_t* index, int nact, uint8_t* e_hat, int32_t* chosen, void* stream);
/* OSD for codes whose basis does not fit in LDS: the same inputs, candidate list, cost, tie rule and outputs as fgnn_osd (method
 * FGNN_OSD_0: the outputs of fgnn_osd0, plus chosen[b] = 0), bit for bit, at any shape with n <= 16384 (larger n: FGNN_ERR_ARG).
 * fgnn_osd_resident sets *fits = 1 iff the LDS-resident kernels accept this graph's side-`side` basis — fgnn_osd0 for FGNN_OSD_0,
 * fgnn_osd for FGNN_OSD_E / FGNN_OSD_CS (the same predicate those calls refuse by).  fgnn_osd_workspace_bytes = slots times the bytes
 * of one slot (the bit-packed augmented matrix rank x (n+1) plus the per-position tables; the order only needs to be valid).
 * fgnn_osd_ws runs on a caller-owned device workspace of workspace_bytes (8-byte aligned): it holds workspace_bytes / slot bytes slots,
 * and min(slots, samples) persistent workgroups each walk the sample list in one slot, so the workspace bounds the parallelism, not
 * the batch.  It does not allocate and does not synchronise.  Accepts every shape fgnn_osd0 / fgnn_osd accept too.  A bad method or
 * order, a NULL or misaligned workspace, a missing basis, a NULL buffer or a workspace smaller than one slot are refused before
 * anything is written or launched.  The workspace is scratch: nothing past workspace_bytes is touched. */
int fgnn_osd_resident(const fgnn_graph* g, int side, int method, int* fits);
int fgnn_osd_workspace_bytes(const fgnn_graph* g, int side, int method, int order, int slots, size_t* bytes);
int fgnn_osd_ws(const fgnn_graph* g, int side, int method, int order, const float* marg, const float* llr_bin, const uint8_t* synd,
                int B, const int32_t* index, int nact, uint8_t* e_hat, int32_t* chosen, void* workspace, size_t workspace_bytes,
                void* stream);
/* index[0..*count) = ids b with (mask[b] & bit) != 0 (tf.where(err), bp_osd.py:166-171); *count (device int32) must be
 * zero on entry; ids of one 256-sample block are ascending, blocks arrive in any order. */
int fgnn_compact(const uint8_t* mask, int bit, int B, int32_t* index, int32_t* count, void* stream);

/* Localized statistics decoding, LSD-0 with synchronous growth (Hillmann, Berent, Quintavalle, Eisert, Wille, Roffe 2024; BpLsdDecoder
 * of ldpc v2): cluster-based post-processing of BP failures.  It needs no row basis (fgnn_graph_set_basis is not used) and takes
 * dependent rows as they are.  One side of the graph is a binary matrix H of m checks by n bits (side 0 = hx, solves z_hat; side 1 =
 * hz, solves x_hat, as fgnn_osd0); every listed sample of that side is solved on its own.
 * Inputs: the full syndrome s [m] (synd [B,m_side]); the reliabilities r of fgnn_osd0 (from marg [B,3,n] or llr_bin [B,n], exactly
 * one of them, then r + 0.0f); key(v) = (sortable(r[v]) << 32) | v with fgnn_osd's order-preserving float -> uint32 map: the smallest
 * key is the most likely error, ties go to the lower bit index.
 * State: t = the reduced syndrome over the m checks, initially s; lab[c] = the cluster label of check c, -1 outside every cluster, else
 * the smallest check index of its cluster; inB[v] = bit v is in a cluster; isPivot[c] = check c is a pivot row; pivots k = 0 .. P-1,
 * each a check piv[k], a bit col[k] and an m-bit vector L[k].
 * Start: every check with s[c] = 1 is a cluster of its own (a zero syndrome: e = 0, found = 1, 0 rounds).  A cluster is invalid while
 * some non-pivot check of it has t[c] = 1.  Rounds run while an invalid cluster that is not dead exists, no cap has been hit, and
 * max_rounds is 0 or fewer than max_rounds rounds have run.  A round:
 *   1. select, on the state at the start of the round: every invalid live cluster picks the bit of smallest key among the bits not in
 *      inB that touch one of its checks; a cluster with no such bit is dead (a whole connected component whose syndrome is not in the
 *      image of H): it stays invalid and is never grown again.  S = the distinct bits selected.
 *   2. append the bits v of S in ascending key order, one after the other: set inB[v]; all checks of v join one cluster together with
 *      every cluster they belonged to (label = the smallest check index of the union); x = column v of H; for k = 0 .. P-1 in order:
 *      if x[piv[k]] is set, x ^= L[k] with its own piv[k] bit left out (x[piv[k]] stays set); if x is zero on every non-pivot check
 *      the column is dependent and nothing more happens; otherwise, if P == max_pivots the sample ends here (found = 0); otherwise
 *      p = the lowest non-pivot check set in x, piv[P] = p, col[P] = v, L[P] = x, p becomes a pivot, if t[p] is set t ^= x with bit p
 *      left out, and P += 1.
 * These are Gauss-Jordan row operations kept as a list: every pivot column is a unit vector, so e[col[k]] = t[piv[k]] and every other
 * bit is 0, without back-substitution.
 * Outputs, for every processed sample b (others untouched): e_hat[b,:] zeroed and then written (with found = 0: the read-out of the
 * pivots there are); stats[b] = (found, rounds, columns appended, pivots) (device int32 [B,4], may be NULL).  A round in which a
 * cluster dies counts as a round; the column that hits the pivot cap counts as a column; found = 1 iff no cluster is invalid at the
 * end.  With no caps H e_hat = s holds whenever s is the syndrome of some error.  Selection is an integer minimum per cluster and the
 * append is sequential in key order: nothing depends on arrival order or launch geometry.
 * All state lives in LDS.  fgnn_lsd_max_pivots: *cap = min(m_side, n, the largest pivot count whose LDS fits); a side with more than
 * 8192 checks, or one whose state does not fit with one pivot, is refused by both calls.  max_pivots = 0 means that cap; max_rounds =
 * 0 means no limit.  Refused with FGNN_ERR_ARG before anything is launched or written: a NULL graph, synd or e_hat; both or neither
 * of marg / llr_bin; max_pivots above the cap (the message names the largest count that fits); a negative max_pivots or max_rounds.
 * index / nact select the samples as in fgnn_osd0. */
int fgnn_lsd_max_pivots(const fgnn_graph* g, int side, int* cap);
int fgnn_lsd(const fgnn_graph* g, int side, const float* marg, const float* llr_bin, const uint8_t* synd, int B, const int32_t* index,
             int nact, int max_pivots, int max_rounds, uint8_t* e_hat, int32_t* stats, void* stream);

/* GNN_BP4 (the syndrome-only "full GNN" decoder), sionna/fec/ldpc/gnn.py:71-423 with UpdateCNEmbeddings (:426-610)
 * and UpdateVNEmbeddings (:612-751): num_mlp_layers=2, tanh, mean, use_bias, num_embed_dims=20, num_hidden_units=40.
 * Weights: 30 host arrays — cn_msg_x, cn_msg_z, cn_embed_x, cn_embed_z, vn_msg_x, vn_msg_z, vn_embed, each
 * {W1[in,40], b1[40], W2[40,20], b2[20]} with in = 40, 40, 41, 41, 40, 40, 60, then llr_inv {W[20,3], b[3]}.
 * Outputs: x_hat/z_hat [B,n] (make_hard_decision :359-367), llr_out [B,3,n] = last embed_to_llr (:283-289),
 * x_logit_all [num_iter,B,m_z+rows(lz)], z_logit_all [num_iter,B,m_x+rows(lx)] = llr_hat of :409 (may be NULL).
 * The reference's call raises as shipped (:408 unpacks 5 of cal_logit's 4 values); that line is repaired. */
int fgnn_gnnbp4_weights_create(const float* const host_arrays[30], int num_embed_dims, int num_hidden_units, int device,
                               fgnn_gnnbp4_weights** out);
void fgnn_gnnbp4_weights_destroy(fgnn_gnnbp4_weights* w);
size_t fgnn_gnnbp4_workspace_bytes(const fgnn_graph* g, int B);
/* GNN_BP4 with any other constructor setting the reference's classes accept (gnn.py:131-207; UpdateCNEmbeddings :494-610,
 * UpdateVNEmbeddings :640-751): num_embed_dims D <= 32, num_hidden_units H <= 96, num_mlp_layers L in 1..4, reduce_op (:556-568), the
 * activation of the hidden layers, use_bias, use_attributes with node_attribute_dims / msg_attribute_dims <= 16 (trainable per-node
 * and per-edge vectors concatenated to the MLP inputs, :584-599, :724-746).  num_msg_dims has no effect in the reference
 * (`units[-1] = num_embed_dims` rewrites the list the message MLPs share, :548, :690); clip_llr_to, input_embed and the syndrome_embed
 * layers are never used by call.  host_arrays: for each MLP in the order cn_msg_x, cn_msg_z, cn_embed_x, cn_embed_z, vn_msg_x,
 * vn_msg_z, vn_embed its L Dense layers {W[in,out] (, b[out])}, then _llr_inv_embed {W[D,3] (, b[3])}, then with attributes
 * cn_node_x [m_x,An], cn_node_z [m_z,An], cn_msg_x [E_x,Am], cn_msg_z [E_z,Am], vn_node [n,An], vn_msg_x [E_x,Am], vn_msg_z [E_z,Am]
 * with edge rows in the reference's order np.where(pcm) (check-major); MLP inputs [h_from | h_to | msg attr], [m | node attr | h_to |
 * logit], [m_x | m_z | node attr | h_to].  The handle is accepted by fgnn_gnnbp4_decode and runs a runtime-shaped VALU kernel in the
 * literal association (the MFMA kernel is specialised for D = 20, H = 40, L = 2, mean, tanh, bias, no attributes); the workspace
 * it needs is fgnn_gnnbp4_weights_workspace_bytes (which also serves handles of fgnn_gnnbp4_weights_create). */
typedef struct {
    int num_embed_dims, num_hidden_units, num_mlp_layers;
    int reduce_op;   /* FGNN_REDUCE_* */
    int activation;  /* FGNN_ACT_* */
    int use_bias, use_attributes, node_attribute_dims, msg_attribute_dims;
} fgnn_gnnbp4_config;
int fgnn_gnnbp4_weights_create_general(const fgnn_graph* g, const fgnn_gnnbp4_config* cfg, const float* const* host_arrays,
                                       int num_arrays, fgnn_gnnbp4_weights** out);
size_t fgnn_gnnbp4_weights_workspace_bytes(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int B);
int fgnn_gnnbp4_decode(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, const uint8_t* synd_x,
                       const uint8_t* synd_z, int B, uint8_t* x_hat, uint8_t* z_hat, float* llr_out, float* x_logit_all,
                       float* z_logit_all, void* workspace, size_t ws_bytes, void* stream);

/* ---- training: reverse pass of Second_Stage_GNN_BP_Model (feedback_gnn.py:423-463, train_n882.ipynb cell 7) -------------
 * The reference differentiates GNN -> 16 BP4 iterations (boxplus-phi, stage_two soft syndromes per iteration,
 * decoding_q.py:768-775) -> BCE with tf.GradientTape.  The two entry points below are that chain rule by hand.
 *
 * fgnn_bp4_backward: tape_x/tape_z [T+1,B,E_s] are the c->v messages before iteration k (k = T: after the last one), i.e.
 * the msg_out of T chained one-iteration fgnn_bp4_decode calls, slot 0 all zero.  grad_x_logit [T+1,B,rows0] /
 * grad_z_logit [T+1,B,rows1] are d loss / d (soft syndromes after k iterations) (either may be NULL); has_grad [T+1]
 * (device, u8) flags the k at which a gradient enters.  Output grad_llr_ch [B,3,n] = d loss / d llr_ch.  */
int fgnn_bp4_backward(const fgnn_graph* g, int num_iter, float normalization_factor, const float* llr_ch,
                      const uint8_t* synd_x, const uint8_t* synd_z, int B, const float* tape_x, const float* tape_z,
                      const float* grad_x_logit, const float* grad_z_logit, const uint8_t* has_grad, float* grad_llr_ch,
                      void* stream);

/* fgnn_feedback_gnn_backward: inputs as fgnn_feedback_gnn plus grad_out [B,3,n] = d loss / d (GNN output).  Leaves the
 * (activation, delta) pair of every Dense layer in device memory — node_in [B,n,44] (= [mean_x|mean_z|X,Y,Z|0]),
 * node_h2 / node_d2 [B,n,40], and per side s (0 = hx, 1 = hz) edge_feat[s] [B,E_s,4], edge_h1[s] / edge_d1[s] [B,E_s,40],
 * edge_dm[s] [B,E_s,20] — so that each weight gradient is one plain GEMM activation^T * delta and each bias gradient a
 * column sum (Keras order of get_weights(): Wout = node_h2^T G, We = node_in[:, :43]^T node_d2, W1_s = edge_feat^T edge_d1,
 * W2_s = edge_h1^T edge_dm). */
int fgnn_feedback_gnn_backward(const fgnn_graph* g, const fgnn_weights* w, const float* llr, const float* logit_hx,
                               const float* logit_hz, const uint8_t* synd_x, const uint8_t* synd_z, int B,
                               const float* grad_out, float* node_in, float* node_h2, float* node_d2,
                               float* const edge_feat[2], float* const edge_h1[2], float* const edge_d1[2],
                               float* const edge_dm[2], void* stream);
/* The same for weights made by fgnn_weights_create_general (any constructor setting of Feedback_GNN: the reference trains whatever
 * feedback_gnn.py:21-128 built, :423-463).  For Dense layer li in EXECUTION order — [0, L) vn_msg_mlp_x, [L, 2L) vn_msg_mlp_z,
 * [2L, 3L-1) vn_embed_mlp, 3L-1 _llr_inv_embed; L = num_mlp_layers, num_layers = 3L — the kernel leaves acts[li] [rows, K_li] = the
 * layer's input and deltas[li] [rows, J_li] = d loss / d (its pre-activation), rows = B*E_x / B*E_z (message MLPs, canonical edge
 * order) or B*n; the caller forms W_li grad = acts^T deltas and b_li grad = column sums.  max / min reduce: the gradient goes to the
 * edges attaining the extremum, shared equally among ties. */
int fgnn_feedback_gnn_backward_general(const fgnn_graph* g, const fgnn_weights* w, const float* llr, const float* logit_hx,
                                       const float* logit_hz, const uint8_t* synd_x, const uint8_t* synd_z, int B,
                                       const float* grad_out, float* const* acts, float* const* deltas, int num_layers, void* stream);

/* ---- training GNN_BP4 -------------------------------------------------------------------------------------------------
 * A forward pass that records a tape and the reverse pass through GNN_BP4.call, for weights made by
 * fgnn_gnnbp4_weights_create_general with reduce_op sum or mean and use_attributes = 0 (max / min and attributes: FGNN_ERR_ARG
 * naming the setting).  D = 20, H = 40, L = 2, tanh, mean, bias runs kernels with compile-time widths (unless
 * fgnn_graph_force_generic is on), every other setting runtime-shaped ones.
 *
 * fgnn_gnnbp4_forward_tape: x_logit_all / z_logit_all as fgnn_gnnbp4_decode writes them for the same handle, bit for bit, and
 * the tape [B][num_iter][(n + m) D + m] floats: per codeword and iteration h_vn [n][D] after the VN update, h_cn [m][D] that
 * update read, and the hx then hz logits [m] that feed the next CN update.  The embeddings live in the tape: no workspace.
 *
 * fgnn_gnnbp4_backward: grad_x_logit_all [num_iter,B,m_z+rows(lz)] / grad_z_logit_all [num_iter,B,m_x+rows(lx)] = d loss / d of
 * the arrays the forward returned (either may be NULL: that side contributes nothing).  grad_weights [grad_count] receives the
 * gradient of every Dense array, summed over the batch, in the order of host_arrays (7 MLPs x L layers {W (, b)}, then
 * _llr_inv_embed {W (, b)}); grad_count = fgnn_gnnbp4_grad_count.  workspace: fgnn_gnnbp4_backward_workspace_bytes, caller-owned
 * (per-node and per-edge gradient state and one partial gradient per workgroup).  No floating-point atomics: the same inputs
 * give the same bits.  A tape or workspace smaller than needed is refused with both byte counts in the message.
 * Conventions as fgnn_bp4_backward: constant sign products, clip_by_value's gradient inside phi, |x|' = sign(x). */
int fgnn_gnnbp4_grad_count(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int* count);
int fgnn_gnnbp4_tape_bytes(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, int B, size_t* bytes);
int fgnn_gnnbp4_backward_workspace_bytes(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int B, size_t* bytes);
int fgnn_gnnbp4_forward_tape(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, const uint8_t* synd_x,
                             const uint8_t* synd_z, int B, float* x_logit_all, float* z_logit_all, float* tape, size_t tape_bytes,
                             void* stream);
int fgnn_gnnbp4_backward(const fgnn_graph* g, const fgnn_gnnbp4_weights* w, int num_iter, const uint8_t* synd_x,
                         const uint8_t* synd_z, int B, const float* tape, size_t tape_bytes, const float* grad_x_logit_all,
                         const float* grad_z_logit_all, float* grad_weights, int grad_count, void* workspace, size_t ws_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FGNN_H */
