/*
 * cqlrec.h -- C ABI of libcqlrec.so, the MI355X (gfx950) CQL recommender hot path.
 *
 * The reference (monkey0head/RePlay_cql @ 2025-02-28 = replay-rec 0.10.0) has NO FFI layer and no CQL model
 * (SURVEY.md F1-F3): its plug-in boundary is the Python abstract class replay/models/base_rec.py:1202-1335
 * (Recommender.fit/predict) with the hooks _fit (:376-392) and _predict (:607-637).  The entry points below
 * are what a `replay/models/cql.py` behind that boundary binds with ctypes; each one cites
 * the reference code whose role it takes over.  Arithmetic follows SURVEY.md section 8.0 (S1-S7, P1-P4).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'd / a torch tensor's data_ptr()) unless marked [host].  The marker
 *     is load-bearing: the Python binding reads its ctypes table from this file (replay_cql_amd/_header.py), and a comment
 *     holding [host] inside a parameter's own text is what makes that parameter a typed host pointer there instead of a
 *     device pointer that takes a tensor.  A pointer to a cqlrec_* struct is a host pointer with or without it;
 *   - plain pointers and sizes only, no torch types; `stream` is a hipStream_t passed as void* (0 = null stream);
 *   - all calls are asynchronous on `stream`, allocate nothing, never synchronise: they may be captured in a hipGraph
 *     (after one warm-up call: kernels with > 64 KiB of dynamic LDS opt in on first use; tests/test_gpu_kernels.py
 *     ::test_entry_points_capture_in_a_hip_graph).  The step drivers take the step number by value -- sampling seed and
 *     Adam bias corrections are baked into their launches -- so a captured training step replays THAT step;
 *   - bf16 tensors are uint16_t bit patterns; matrices are row-major; W1/W2 are stored [out][in];
 *   - return value: CQLREC_OK, or a negative code with the message available from cqlrec_last_error();
 *   - the kernel-level entry points are re-entrant; the step driver (cqlrec_train_step*) keeps one set of internal
 *     side streams and events per DEVICE (indexed by the calling thread's current device): drive one training context
 *     per device from one host thread at a time (one process per GPU is the deployment model);
 *   - the training step contains no float atomics: the same calls on the same inputs give the same bits.
 */
#ifndef CQLREC_H
#define CQLREC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CQLREC_OK 0
#define CQLREC_ERR_INVALID (-1)
#define CQLREC_ERR_HIP (-2)
#define CQLREC_ABI_VERSION 2
#define CQLREC_SEG_ALIGN 64 /* every parameter segment starts on a multiple of 64 elements */

typedef void* cqlrec_stream;

int cqlrec_abi_version(void);
const char* cqlrec_last_error(void); /* [host] thread-local message of the last failing call */

/* ---------------------------------------------------------------------------------------------------------
 * Parameter layout (S3).  One flat buffer holds  E_in[(N+1) x d] | E_out[N x d] | b_out[N] | W1[d x d] | b1[d] |
 * W2[d x d] | b2[d]; theta (fp32), grads, Adam m/v, the target copy and both bf16 shadows share these offsets.
 * Replaces the nn.Module parameter containers of the torch analogues (replay/models/neuromf.py:37-211).
 * --------------------------------------------------------------------------------------------------------- */
typedef struct cqlrec_layout {
  int64_t n_items;
  int32_t d;
  int32_t reserved;
  int64_t off_E_in, off_E_out, off_b_out, off_W1, off_b1, off_W2, off_b2;
  int64_t total; /* elements, padded */
} cqlrec_layout;
int cqlrec_layout_make(int64_t n_items, int32_t d, cqlrec_layout* out /* [host] */);

/* ---------------------------------------------------------------------------------------------------------
 * a2/a8  Transition sampler: counter-based, bit-exact with oracle.sample_positions().  Takes the place of the
 * DataLoader iteration in TorchRecommender.train (replay/models/base_torch_rec.py:78-80).
 *   k1 = mix64(seed ^ step*0xD1B54A32D192ED03); p = mulhi64(mix64(k1 + slot0 + b), nnz); user = last u with
 *   offsets[u] <= p; t = p - offsets[u]; act = items[p]; rew = rewards[p]; done = (t == count(u)-1).
 * --------------------------------------------------------------------------------------------------------- */
int cqlrec_sample_transitions(const int64_t* offsets, const int32_t* items, const float* rewards, int64_t n_users,
                              uint64_t seed, uint64_t step, uint64_t slot0, int32_t batch, int32_t* users,
                              int32_t* tpos, int32_t* act, float* rew, float* done, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a3  Window gather + masked mean (S4 h0).  No reference counterpart (closest: nn.Embedding lookups,
 * replay/models/neuromf.py:72-73).  State i = the last min(end_i, L) items of users[i] before position
 * end_i = ends[i] + end_delta  (ends == NULL: end_i = row length, the predict-time state, S7).
 * Outputs (either may be NULL): h0 fp32 [n x d], h0_b bf16 [n x d], lens int32 [n].
 * --------------------------------------------------------------------------------------------------------- */
int cqlrec_gather_pool_fwd(const uint16_t* E_in_b, const int64_t* offsets, const int32_t* items,
                           const int32_t* users, const int32_t* ends, int32_t end_delta, int64_t n_states,
                           int32_t L, int32_t d, float* h0, uint16_t* h0_b, int32_t* lens, cqlrec_stream stream);
/* backward of the above: g_E_in[item] += dh0[i] / len_i for every item of window i.
 * cqlrec_gather_pool_bwd: direct fp32 atomic scatter (small inputs / reference form).
 * cqlrec_gather_pool_bwd_sorted: the production form -- (item, state) pairs are radix-sorted by item and summed
 * per run in registers, so a hot item costs one row-add per 64 contributions; rows touched by a single chunk are
 * written with plain stores.  g_E_in must be zero on entry for both.  ws: cqlrec_gather_pool_bwd_ws_bytes. */
int cqlrec_gather_pool_bwd(const float* dh0, const int64_t* offsets, const int32_t* items, const int32_t* users,
                           const int32_t* ends, int32_t end_delta, int64_t n_states, int32_t L, int32_t d,
                           float* g_E_in, cqlrec_stream stream);
int64_t cqlrec_gather_pool_bwd_ws_bytes(int64_t n_states, int32_t L, int32_t d);
/* the same, split at the point where the gradient is needed: _prepare (pairs + sort) depends only on the sampled
 * states, _apply (scale + segmented sum) on dh0.  The step driver runs _prepare on a side stream. */
int cqlrec_gather_pool_bwd_prepare(const int64_t* offsets, const int32_t* items, const int32_t* users,
                                   const int32_t* ends, int32_t end_delta, int64_t n_states, int32_t L, int32_t d,
                                   int64_t n_items, void* ws, int64_t ws_bytes, cqlrec_stream stream);
int cqlrec_gather_pool_bwd_apply(const float* dh0, int64_t n_states, int32_t L, int32_t d, int64_t n_items, void* ws,
                                 int64_t ws_bytes, float* g_E_in, cqlrec_stream stream);
int cqlrec_gather_pool_bwd_sorted(const float* dh0, const int64_t* offsets, const int32_t* items,
                                  const int32_t* users, const int32_t* ends, int32_t end_delta, int64_t n_states,
                                  int32_t L, int32_t d, int64_t n_items, void* ws, int64_t ws_bytes,
                                  float* g_E_in, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a4  One encoder layer  Y = act(X_b W_b^T + bias)  on bf16 MFMA, fp32 accumulate (closest reference code:
 * MLP.forward, replay/models/neuromf.py:133-145).  Y (fp32) and Y_b (bf16) may each be NULL.
 * --------------------------------------------------------------------------------------------------------- */
int cqlrec_linear_bf16(const uint16_t* X_b, const uint16_t* W_b, const float* bias, int64_t rows, int32_t d,
                       int32_t relu, float* Y, uint16_t* Y_b, cqlrec_stream stream);
/* Both layers of the state encoder in one launch:  Z_b = bf16(relu(X_b W1_b^T + b1)),  H_b = bf16(Z_b W2_b^T + b2) -- the
 * bits of two cqlrec_linear_bf16 calls (same products, same k-order, same roundings); Z_b is kept for the backward. */
int cqlrec_encoder_fwd(const uint16_t* X_b, const uint16_t* W1_b, const float* b1, const uint16_t* W2_b, const float* b2,
                       int64_t rows, int32_t d, uint16_t* Z_b, uint16_t* H_b, cqlrec_stream stream);
/* fp32 backward of the two-layer encoder on the bf16-valued forward operands.  ws: cqlrec_encoder_bwd_ws_bytes. */
int64_t cqlrec_encoder_bwd_ws_bytes(int64_t rows, int32_t d);
int cqlrec_encoder_bwd(const float* dH, const uint16_t* z_b, const uint16_t* h0_b, const uint16_t* W1_b,
                       const uint16_t* W2_b, int64_t rows, int32_t d, void* ws, int64_t ws_bytes, float* g_W1,
                       float* g_b1, float* g_W2, float* g_b2, float* dh0, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a5  Full-catalog Q-head, fused with its row reduction; the rows x N score matrix never reaches HBM.
 * Closest reference code: the catalog-wide Linear + log_softmax of MultVAE (replay/models/mult_vae.py:101,
 * :275-276).   Q[r][j] = <H_b[r], E_out_b[j]> + b_out[j].
 *   mode CQLREC_QHEAD_LSE    : out_val[r] = logsumexp_j Q[r][j]; out_nlse2[r] = -out_val[r]*log2(e) (may be NULL)
 *   mode CQLREC_QHEAD_ARGMAX : out_val[r] = max_j Q[r][j]; out_idx[r] = argmax (ties -> smallest j)
 * ws: cqlrec_qhead_ws_bytes(rows, n_items, d) bytes of scratch.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_QHEAD_LSE 1
#define CQLREC_QHEAD_ARGMAX 2
int64_t cqlrec_qhead_ws_bytes(int64_t rows, int64_t n_items, int32_t d);
int cqlrec_qhead_fwd(const uint16_t* H_b, int64_t rows, const uint16_t* E_out_b, const float* b_out,
                     int64_t n_items, int32_t d, int32_t mode, void* ws, int64_t ws_bytes, float* out_val,
                     int32_t* out_idx, float* out_nlse2, cqlrec_stream stream);

/* out[r] = <H_b[r], E_b[idx[r]]> + b[idx[r]]   (q_a, the target-net Q(s',a*), and _predict_pairs, a11:
 * replay/models/base_rec.py:784-823) */
int cqlrec_gather_dot(const uint16_t* H_b, const uint16_t* E_b, const float* b, const int32_t* idx, int64_t rows,
                      int32_t d, float* out, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a6  CQL + double-Q TD loss (S5) and its backward.  Reference analogue of the role: the _loss hooks +
 * loss.backward() (replay/models/base_torch_rec.py:35-37).
 *   y = rew + gamma (1-done) q_targ;  delta = q_a - y;  loss = inv_batch * sum_b [0.5 delta^2 + alpha (lse - q_a)]
 *   coef[b] = (delta - alpha) * inv_batch         (inv_batch = 1 / global batch)
 * loss_out: one float, written (deterministic tree reduction).
 * --------------------------------------------------------------------------------------------------------- */
int cqlrec_td_loss(const float* q_a, const float* lse, const float* q_targ, const float* rew, const float* done,
                   int32_t batch, float gamma, float alpha, float inv_batch, float* coef, float* y,
                   float* loss_out, cqlrec_stream stream);
/* dQ = scale * bf16(exp(Q - lse)) + coef * onehot(act)   (scale = alpha * inv_batch), never materialised:
 *   dH[b]        = scale * sum_j P_b[b][j] E_out_b[j] + coef[b] E_out_b[act[b]]
 *   g_E_out[j]   = scale * sum_b P_b[b][j] H_b[b]     + sum_{b: act[b]=j} coef[b] H_b[b]        (overwritten)
 *   g_b_out[j]   = scale * sum_b P[b][j]              + sum_{b: act[b]=j} coef[b]               (overwritten)
 * nlse2 = -lse*log2(e) from cqlrec_qhead_fwd.  ws: cqlrec_qhead_bwd_ws_bytes. */
int64_t cqlrec_qhead_bwd_ws_bytes(int64_t batch, int64_t n_items, int32_t d);
int cqlrec_qhead_bwd(const uint16_t* H_b, const float* nlse2, const float* coef, const int32_t* act,
                     int64_t batch, const uint16_t* E_out_b, const float* b_out, int64_t n_items, int32_t d,
                     float scale, void* ws, int64_t ws_bytes, float* dH, float* g_E_out, float* g_b_out,
                     cqlrec_stream stream);

/* the two halves of cqlrec_qhead_bwd, separately callable (a data-parallel caller all-reduces g_E_out/g_b_out
 * while the state-side half still runs) */
int cqlrec_qhead_bwd_items(const uint16_t* H_b, const float* nlse2, const float* coef, const int32_t* act,
                           int64_t batch, const uint16_t* E_out_b, const float* b_out, int64_t n_items, int32_t d,
                           float scale, void* ws, int64_t ws_bytes, float* g_E_out, float* g_b_out,
                           cqlrec_stream stream);
int cqlrec_qhead_bwd_states(const uint16_t* H_b, const float* nlse2, const float* coef, const int32_t* act,
                            int64_t batch, const uint16_t* E_out_b, const float* b_out, int64_t n_items, int32_t d,
                            float scale, void* ws, int64_t ws_bytes, float* dH, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a5+a10 fused ("flash" form), used by the training step: ONE pass over the catalogue yields per state the
 * logsumexp AND sum_j exp(S_j - m) E_out_b[j] relative to a running reference m (kept in `ws`, one slab per
 * catalogue slice), so the state-side backward needs no second catalogue pass.  Once the TD coefficients are
 * known, dh_finish combines the slabs:
 *     dH[b] = scale * sum_k slab_k[b] * exp(m_k[b] - lse[b]) + coef[b] * E_out_b[act[b]]
 * P is rounded to bf16 relative to the running reference instead of the final lse (same 2^-9 relative error per
 * probability, different rounding points): dH agrees with cqlrec_qhead_bwd_states to ~1e-3 normwise, lse to 1e-6.
 * Replaces, together with cqlrec_qhead_bwd_items, loss.backward() through the catalogue-wide Linear + log_softmax
 * (replay/models/mult_vae.py:101, :274-284; replay/models/base_torch_rec.py:37).
 * --------------------------------------------------------------------------------------------------------- */
int64_t cqlrec_qhead_fused_ws_bytes(int64_t rows, int64_t n_items, int32_t d);
int cqlrec_qhead_fwd_lse_dh(const uint16_t* H_b, int64_t rows, const uint16_t* E_out_b, const float* b_out,
                            int64_t n_items, int32_t d, void* ws, int64_t ws_bytes, float* out_lse,
                            float* out_nlse2 /* -lse*log2(e), may be NULL */, cqlrec_stream stream);
int cqlrec_qhead_dh_finish(const void* ws, int64_t rows, int64_t n_items, int32_t d, const float* lse,
                           const float* coef, const int32_t* act, const uint16_t* E_out_b, float scale, float* dH,
                           cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a7  Fused Adam + Polyak target + bf16 shadows over the flat buffer (S6).  Replaces optimizer.step()
 * (replay/models/base_torch_rec.py:38; torch.optim.Adam at replay/models/neuromf.py:351-355).
 *   m = b1 m + (1-b1) g;  v = b2 v + ((1-b2) g) g;  theta -= step_size * (m / (sqrt(v)/sqrt_bc2 + eps));
 *   target = (1-tau) target + tau theta;  theta_b = bf16(theta);  target_b = bf16(target);  g = 0 if zero_grads.
 * step_size = lr/(1-b1^t), sqrt_bc2 = sqrt(1-b2^t) are computed by the caller in double and passed as float.
 * --------------------------------------------------------------------------------------------------------- */
int cqlrec_adam_ema(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b,
                    uint16_t* target_b, int64_t n, float step_size, float sqrt_bc2, float beta1, float beta2,
                    float eps, float tau, int32_t zero_grads, cqlrec_stream stream);
/* dst_b = bf16(src) (shadow refresh after load / init) */
int cqlrec_cast_bf16(const float* src, uint16_t* dst_b, int64_t n, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a10  All-users top-K scoring (S7).  Takes the place of TorchRecommender._predict's per-user pandas UDF
 * (replay/models/base_torch_rec.py:120-149) + NeuroMF._predict_by_user's argsort (replay/models/neuromf.py:
 * 393-438) + _filter_seen / get_top_k_recs (replay/models/base_rec.py:417-464, replay/utils.py:112-127).
 *   H_b      [n_users x d]  bf16 state vectors (encoder output)
 *   E_b, b   candidate item table [n_cand x d] bf16 and bias [n_cand]
 *   item_ids [n_cand] global id of candidate row c (NULL: identity); must be ascending
 *   seen_off, seen_items: CSR of ascending global item ids to exclude; scored user u uses CSR row
 *            seen_rows[u] (seen_rows NULL: row u).  seen_off NULL: no filter.
 * Output, per user: the k best (score desc, item id asc) admissible items: out_idx/out_val [n_users x k]
 * (padding: -1 / -inf) and out_cnt [n_users] = number of valid entries.
 * --------------------------------------------------------------------------------------------------------- */
int64_t cqlrec_topk_ws_bytes(int64_t n_users, int64_t n_cand, int32_t d, int32_t k);
int cqlrec_score_topk(const uint16_t* H_b, int64_t n_users, const uint16_t* E_b, const float* b, int64_t n_cand,
                      int32_t d, const int32_t* item_ids, const int64_t* seen_off, const int32_t* seen_items,
                      const int32_t* seen_rows, int32_t k, void* ws, int64_t ws_bytes, int32_t* out_idx,
                      float* out_val, int32_t* out_cnt, cqlrec_stream stream);
/* The same in two phases, so that the part that depends on the seen lists only (their bitmap, built in `ws`: it is
 * what _filter_seen's anti-join becomes here) can run on another stream while the caller still encodes the state
 * vectors:  CQLREC_TOPK_SEEN (H_b, outputs ignored; may be NULL) ... CQLREC_TOPK_SCORE on the same ws, ordered
 * behind it by the caller.  CQLREC_TOPK_ALL = cqlrec_score_topk.  Shapes whose selection kernel filters on the
 * fly do nothing in the first phase. */
#define CQLREC_TOPK_ALL 0
#define CQLREC_TOPK_SEEN 1
#define CQLREC_TOPK_SCORE 2
#define CQLREC_TOPK_SEEN_BESIDE 3 /* = _SEEN, launched while a _SCORE phase of another workspace runs on another stream:
                                     the builder then uses what that kernel leaves free of a CU (small LDS tiles) */
int cqlrec_score_topk_phase(const uint16_t* H_b, int64_t n_users, const uint16_t* E_b, const float* b, int64_t n_cand,
                            int32_t d, const int32_t* item_ids, const int64_t* seen_off, const int32_t* seen_items,
                            const int32_t* seen_rows, int32_t k, void* ws, int64_t ws_bytes, int32_t* out_idx,
                            float* out_val, int32_t* out_cnt, int32_t phase, cqlrec_stream stream);

/* Debug / tests: which form of the seen filter the last SEEN (or ALL) phase on `ws` left for the on-chip-selection
 * kernel.  *out (host) = -1: this shape filters by bitmap only; 0: entry lists (256-byte slots per 128 users x 64 items
 * + an overflow area, built in the bitmap's space; the bitmap was not built); 1: the lists did not fit, bitmap.
 * Synchronises `stream`. */
int cqlrec_topk_seen_form(const void* ws, int64_t n_users, int64_t n_cand, int32_t d, int32_t k,
                          int32_t* out /* [host] */, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a11  Item-to-item nearest neighbours.  Takes the place of ItemVectorModel._get_nearest_items' cross join of the item
 * vectors with a per-pair UDF (replay/models/base_rec.py:955-1030; vector_dot, vector_euclidean_distance_similarity,
 * cosine_similarity at replay/utils.py:131, :677-685, :689-697) + the window top-k of _get_nearest_items_wrap
 * (base_rec.py:893-926).  The queries x candidates matrix is never written.
 *   E_b        [n_rows x d] bf16 item rows v_j (the E_out shadow); all arithmetic is fp32 on these values
 *   norms      [n_rows] n_j = dot(j, j), written by cqlrec_item_norms
 *   query_rows [n_query] distinct rows to find neighbours of;  cand_rows [n_cand] distinct rows to choose from
 *              (NULL: every row, n_cand = n_rows).  Both hold values in [0, n_rows).
 *   metric     CQLREC_SIM_DOT     dot(i,j)
 *              CQLREC_SIM_COSINE  dot / (sqrtf(n_i) * sqrtf(n_j));  a pair whose denominator is 0 is not admissible
 *              CQLREC_SIM_EUCLID  1 / (1 + sqrtf(max((n_i + n_j) - 2*dot, 0)))
 *              in exactly this operation order, sqrtf and / correctly rounded, nothing contracted into an FMA.
 * The pair (i, i) is never returned (base_rec.py:1015-1017); equal rows under different ids are.
 * Output, per query: the k best (value desc, neighbour row DESC -- base_rec.py:911-917; not the predict tie rule)
 * admissible candidates: out_idx/out_val [n_query x k] (padding: -1 / -inf) and out_cnt [n_query] = number of valid
 * entries.  k <= 512.  Exact: group-wise upper bounds from an MFMA pass steer which candidates are re-scored, every
 * returned value comes from the re-scoring.  No float atomics: the same call gives the same bits twice.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_SIM_DOT 0
#define CQLREC_SIM_COSINE 1
#define CQLREC_SIM_EUCLID 2
#define CQLREC_ITEM_KNN_MAX_K 512
int cqlrec_item_norms(const uint16_t* E_b, int64_t n_rows, int32_t d, float* norms, cqlrec_stream stream);
int64_t cqlrec_item_knn_ws_bytes(int64_t n_query, int64_t n_cand, int32_t d, int32_t k); /* [host]; 0: bad arguments */
int cqlrec_item_knn(const uint16_t* E_b, const float* norms, int64_t n_rows, int32_t d, const int32_t* query_rows,
                    int64_t n_query, const int32_t* cand_rows, int64_t n_cand, int32_t metric, int32_t k, void* ws,
                    int64_t ws_bytes, int32_t* out_idx, float* out_val, int32_t* out_cnt, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a12  Ranking of per-row candidate lists = predict_pairs(..., k=) (replay/models/base_rec.py:725-782; the use
 * sample_top_k_recs' docstring describes, replay/utils.py:717-727; TwoStagesScenario's candidate frames,
 * two_stages_scenario.py:478-483): the score of every (row, item) pair of a ragged CSR and, per selected row, the k
 * best admissible pairs.  Nothing of size nnz x d is built: a wave keeps its row's state vector in registers.
 *   H_b        [n_sel x d] bf16 state vectors;  rows [n_sel] the CSR row of H_b[i] (NULL: row i), distinct
 *   pair_off / pair_items   CSR of candidates: items of a row ascending, duplicates allowed, values in [0, n_items)
 *   seen_off / seen_items   CSR over the SAME rows, items ascending (NULL, NULL: no filter)
 * Score of a pair: bit for bit what cqlrec_gather_dot gives for (h, item) -- per lane eight sequential fmaf, the
 * butterfly sum over d/8 lanes, + b[item].  out_score (optional, [nnz], CSR order) receives the score of every pair of
 * a selected row, seen or not; pairs of rows that are not selected are not touched.
 * Selection (k > 0), per selected row: the k best pairs by (score desc, item id asc) -- the tie rule of
 * cqlrec_score_topk -- among those whose item is not in the row's seen list.  A candidate listed twice is two entries
 * (adjacent in the output).  out_idx / out_val [n_sel x k] (padding -1 / -inf), out_cnt [n_sel] = valid entries.
 * Scores are assumed finite.  k == 0: scores only (out_idx, out_val, out_cnt NULL, out_score required).
 * Lists of any length in one call: a row longer than max(4096, (summed length of such rows) / 8192) is cut into
 * pieces on the device and merged there; the workspace depends on k alone
 * (8192 * 8 k bytes + 192 KiB).  n_sel <= 2^26 per call (one 64-thread block per row).  Integer atomics hand out piece slots, no
 * float atomics: the same call gives the same bits twice.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_PAIRS_MAX_K 512
int64_t cqlrec_pairs_topk_ws_bytes(int64_t n_sel, int64_t nnz, int32_t d, int32_t k);   /* [host]; 0: bad arguments */
int cqlrec_pairs_topk(const uint16_t* H_b, const uint16_t* E_b, const float* b, int64_t n_items, int32_t d,
                      const int64_t* pair_off, const int32_t* pair_items, const int32_t* rows, int64_t n_sel,
                      const int64_t* seen_off, const int32_t* seen_items, int32_t k, void* ws, int64_t ws_bytes,
                      float* out_score, int32_t* out_idx, float* out_val, int32_t* out_cnt, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * a8  Whole training step = TorchRecommender._run_train_step (replay/models/base_torch_rec.py:32-39) without
 * the per-step host sync.  The step is split in two so that a data-parallel caller can all-reduce ctx.grads
 * (RCCL) between them; losses[] receives one float per step.
 * --------------------------------------------------------------------------------------------------------- */
typedef struct cqlrec_train_ctx {
  cqlrec_layout layout;
  /* training set (CSR by user, S2) */
  const int64_t* offsets;
  const int32_t* items;
  const float* rewards;
  int64_t n_users;
  /* model state, each `layout.total` elements */
  float* theta;
  float* grads;
  float* adam_m;
  float* adam_v;
  float* target;
  uint16_t* theta_b;
  uint16_t* target_b;
  /* hyper-parameters */
  int32_t batch;        /* transitions per step on this rank (multiple of 32) */
  int32_t window;       /* L */
  int32_t world;        /* data-parallel ranks (loss is a mean over batch*world) */
  int32_t rank;
  /* doubles: the Adam bias corrections 1 - beta^t are formed in double from the caller's values (as torch.optim.Adam
   * does with its Python floats); the kernels receive them rounded to float */
  double gamma, alpha, lr, beta1, beta2, eps, tau;
  uint64_t seed;
  /* scratch: cqlrec_train_ws_bytes(batch, n_items, d, window) bytes */
  void* ws;
  int64_t ws_bytes;
} cqlrec_train_ctx;
int64_t cqlrec_train_ws_bytes(int32_t batch, int64_t n_items, int32_t d, int32_t window);
/* sample + forward + loss + backward into ctx->grads (which must be zero on entry; step_update re-zeroes it).
 * loss_out: device float (may be NULL). */
int cqlrec_train_step_fwd_bwd(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, float* loss_out,
                              cqlrec_stream stream);
/* Adam + target + shadows (+ zero grads). `step` is the same 0-based counter. */
int cqlrec_train_step_update(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, cqlrec_stream stream);
/* Finer-grained phases for overlapping the gradient all-reduce with compute (fwd_bwd == forward; backward_items;
 * backward_rest.  update == update_range over [0, layout.total)):
 *   forward         sample, state vectors, encoder, Q-head LSE/argmax, TD target, loss
 *   backward_items  g_E_out, g_b_out                (elements [off_E_out, off_W1) of ctx->grads are final afterwards)
 *   backward_rest   dH, encoder gradients, g_E_in   (the remaining elements are final afterwards)
 *   update_range    Adam/Polyak/shadows/zero-grads over elements [lo, hi) (multiples of 4) */
/* What is still in flight when cqlrec_train_step_forward (or _forward_after / _forward_early_items) has returned AND
 * `stream` has drained: the sorts of the (item, state) and (action, transition) pairs that the backward needs run on a
 * library stream that only the backward joins.  They read ctx->offsets / ctx->items and write ctx->ws until a
 * cqlrec_train_step_backward_* call of that step has been issued and has completed, or until a device-wide
 * synchronize.  A caller that runs forwards only (a validation loop) must synchronize the DEVICE, not `stream`, before it
 * frees or rewrites the log or the workspace. */
int cqlrec_train_step_forward(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, float* loss_out,
                              cqlrec_stream stream);
/* The same with a dependency the caller still has in flight on ANOTHER stream: `items_ready` (a hipEvent_t, or NULL)
 * completes when the item-side parameters (E_out, b_out, their shadows and target copies) are up to date.  Sampling,
 * window gathers and both encoders -- they read only E_in / W1 / W2 -- are enqueued in front of the wait, only the
 * catalogue-wide kernels behind it.  A data-parallel caller uses it to start step t+1 while the all-reduce and Adam of
 * the item-side half of step t are still running on its side stream. */
int cqlrec_train_step_forward_after(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, float* loss_out,
                                    cqlrec_stream stream, void* items_ready /* hipEvent_t */);
/* forward_after that ALSO starts the long part of backward_items -- the dE_out kernel, which needs nothing from the
 * loss but the forward's logsumexp -- on `items_stream` as soon as the catalogue pass of branch A is done, i.e. under
 * the arg-max pass, the TD target and the loss (what cqlrec_train_steps does for a single rank).  The
 * cqlrec_train_step_backward_items call of the same step, which must then be made on `items_stream`, adds only the
 * parts that need the loss (one-hot rows, then the cut pieces: the order in which a gradient row is summed does not
 * change).  items_ready may be NULL.
 *
 * The record of an early launch.  A successful call with items_stream != NULL, != stream and the library's concurrency
 * on leaves a record (ctx->ws, ctx->grads, step, items_stream) with the current device; with items_stream NULL or equal
 * to `stream`, or with cqlrec_set_concurrency(0), the call IS cqlrec_train_step_forward_after and leaves none.  The host
 * address of the ctx struct is no part of it: a copy of the struct with the same ws / grads is the same context, another
 * context never sees the record.  cqlrec_train_step_backward_items(ctx, step, s) then
 *   - finds the record of (ws, grads, step) and s == items_stream: adds the one-hot rows and the cut pieces, and the
 *     record is gone;
 *   - finds it and s != items_stream: returns CQLREC_ERR_INVALID (the message names the item-side stream), launches
 *     nothing and keeps the record, so the call can be repeated on the right stream;
 *   - finds none: runs all of backward_items on s, the long kernel included.  That is the plain path and it is also
 *     correct behind an early launch whose record is gone, because the long kernel stores every row of g_E_out / g_b_out
 *     before anything is added to them.
 * A record is dropped, without being used, by every call that overwrites the step vectors of the same workspace and step
 * parity: cqlrec_train_step_forward, _forward_after, _fwd_bwd, cqlrec_train_steps and a newer _forward_early_items.
 * The library keeps four records per device (two contexts at both parities); a fifth pushes the oldest out, whose step
 * then takes the plain path.  An abandoned early launch (its backward_items never comes) still WRITES ctx->grads on
 * items_stream: order it in front of whatever zeroes or fills ctx->grads next. */
int cqlrec_train_step_forward_early_items(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, float* loss_out,
                                          cqlrec_stream stream, void* items_ready /* hipEvent_t */,
                                          cqlrec_stream items_stream);
int cqlrec_train_step_backward_items(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, cqlrec_stream stream);
int cqlrec_train_step_backward_rest(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, cqlrec_stream stream);
int cqlrec_train_step_update_range(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step, int64_t lo, int64_t hi,
                                   cqlrec_stream stream);
/* n_steps whole steps (steps step0 .. step0+n_steps-1) of a single-rank job (ctx->world == 1) in one call: the epoch
 * loop of TorchRecommender.train (replay/models/base_torch_rec.py:78-84) without a host round trip per batch.
 * Same dataflow and results as fwd_bwd + update per step, software-pipelined across the two halves of the model:
 * Adam on E_in + encoder runs under the (MFMA-bound) item-side backward, the next step's sample / window gathers /
 * encoder start while the item-side Adam is still running, and only the Q-head kernels wait for it.  Everything is
 * joined on `stream` before the call returns.  loss_out: n_steps device floats (may be NULL).
 * ctx->grads must be zero on entry and is zero again when a successful call has completed; during the call, and after
 * a failed one, its content is unspecified (steps that have a successor do not re-zero it).
 * Inside a call of more than one step, rows of E_in that no step reads are brought up to date late (their missed
 * optimizer steps are replayed, bit for bit, when a step needs the row, and at the latest by the last step of the call):
 * a successful call leaves theta, adam_m, adam_v, target and both shadows complete, but after an error return from the
 * middle of a call the E_in rows of those six buffers may be several steps behind -- reload the model, as after losing
 * the side streams in the middle of a call. */
int cqlrec_train_steps(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step0, int32_t n_steps, float* loss_out,
                       cqlrec_stream stream);

/* 1 (default; env CQL_CONCURRENCY=0 to disable): independent parts of a step (the sort for the gather backward, the
 * two forward branches, the item-side vs state-side Q-head backward) run on internal side streams, forked and joined
 * with events on `stream`.  0: strict program order on `stream` -- use it when timing individual kernels. */
int cqlrec_set_concurrency(int32_t on);

/* The step driver's internal side streams and events of the CURRENT device, chosen and created NOW instead of at the
 * first training step, plus CQLREC_AUX_STREAMS library-owned streams for the caller's own side work:
 * cqlrec_aux_stream(0) = the data-parallel loop's item-side stream (the stream cqlrec_train_steps uses for its
 * sample-ahead, which a phased caller never runs), cqlrec_aux_stream(1) = the predict pass's encoder stream; NULL before
 * cqlrec_runtime_init or for a bad index.
 * WHY (measured on MI355X / ROCm 7.2: tools/probes/pipe_probe.hip, tools/stream_order_probe3.py): a process's hardware
 * queues sit on the 4 compute pipes round-robin in the order in which its streams were first used, and while a grid
 * larger than the chip is being handed out on one queue, no kernel of another queue ON THE SAME PIPE is dispatched.  The
 * step runs four streams side by side; if two of them share a pipe -- which used to depend on what else the process had
 * created streams for, and when -- the step loses its concurrency (cfg3: 1.33 instead of 0.69 ms per step).  So the
 * library picks its streams by test: out of up to eight fresh candidates, three that block neither the DEFAULT stream (the
 * stream the caller is expected to train on) nor each other.  One-time cost: a few milliseconds, a device
 * synchronisation; CQL_PIPE_PROBE=0 skips the test.  cqlrec_runtime_probe_count: candidates examined (0: no test ran).
 * Idempotent; needs a visible GPU; replay_cql_amd calls it when a model is constructed.
 * No reference counterpart (the reference trains on one stream, replay/models/base_torch_rec.py:57-98). */
#define CQLREC_AUX_STREAMS 2
int cqlrec_runtime_init(void);
int cqlrec_runtime_probe_count(void);
cqlrec_stream cqlrec_aux_stream(int32_t index);

/* Debug/inspection of the intermediates of step `step` inside ctx->ws (device pointers; valid after that step's
 * fwd_bwd, until step+2 overwrites them: the per-step vectors are double-buffered by step parity). */
typedef struct cqlrec_train_views {
  int32_t *users, *tpos, *act, *a_star;
  float *rew, *done, *q_a, *lse, *q_targ, *y, *coef, *dH, *dh0, *h0_s;
  uint16_t *hb_s, *hb_sn, *hb_tn;
} cqlrec_train_views;
int cqlrec_train_views_get(const cqlrec_train_ctx* ctx /* [host] */, uint64_t step,
                           cqlrec_train_views* out /* [host] */);

/* ---------------------------------------------------------------------------------------------------------
 * f2  log -> CSR by user on the device: rows sorted by (user_idx, timestamp asc, item_idx asc), S2.  Takes the place of
 * `log.toPandas()` + DataLoader construction (replay/models/neuromf.py:332-339).  Inputs are the LOG_SCHEMA columns
 * (replay/constants.py:16-23) as device arrays; timestamp in any monotone int64 unit.  Bit-exact vs a host lexsort.
 * timestamp == NULL: rows ordered by (user_idx, item_idx asc) instead -- the per-user ascending `seen` lists that
 * cqlrec_score_topk filters with (the role of the anti-join in _filter_seen, replay/models/base_rec.py:417-464).
 * relevance == NULL (then rewards must be NULL too): no reward column is produced.
 * --------------------------------------------------------------------------------------------------------- */
int64_t cqlrec_build_csr_ws_bytes(int64_t n_rows);
int cqlrec_build_csr(const int32_t* user_idx, const int32_t* item_idx, const int64_t* timestamp,
                     const double* relevance, int64_t n_rows, int64_t n_users, void* ws, int64_t ws_bytes,
                     int64_t* offsets /* [n_users+1] */, int32_t* items, float* rewards, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f4  Quality metrics of a recommendation block on the device, so that optimize()-style loops
 * (replay/optuna_objective.py:80-111) need not ship U*k rows back through Spark.  Per-user formulas:
 * replay/metrics/{ndcg.py:50-59, hitrate.py:22-27, precision.py, recall.py, map.py, mrr.py}; user set and
 * "no recommendations -> empty prediction" as get_enriched_recommendations (replay/metrics/base_metric.py:102-140).
 *   rec_idx  [n_users x kmax] item ids, best first, unique per row, -1 padded
 *   rec_rows [n_users] row of the ground-truth CSR for each rec row (NULL: identity)
 *   gt_off / gt_items  ground-truth CSR, items ascending and unique per row
 *   ks       [host] n_ks ascending cut-offs (<= kmax, n_ks <= 8)
 * Output: sums[CQLREC_EVAL_METRICS][n_ks] = per-metric sums over the n_users rows (divide by the number of
 * ground-truth users); per_user[n_users][CQLREC_EVAL_METRICS][n_ks] optional.  Order: NDCG, HitRate, Precision,
 * Recall, MAP, MRR.  Double precision, deterministic reduction.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_EVAL_METRICS 6
int64_t cqlrec_eval_topk_ws_bytes(int64_t n_users, int32_t n_ks);
int cqlrec_eval_topk(const int32_t* rec_idx, int64_t n_users, int32_t kmax, const int32_t* rec_rows,
                     const int64_t* gt_off, const int32_t* gt_items, const int32_t* ks /* [host] */, int32_t n_ks,
                     void* ws, int64_t ws_bytes, double* per_user, double* sums, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f4, continued: the other metrics of replay/metrics, from any recommendation FRAME (a baseline, a loaded file,
 * another model's output), not only from a block this library produced.  fp64 throughout; deterministic sums
 * (per-block partials + one final pass); the only atomics are integer atomicMin / atomicAdd.
 *
 * cqlrec_recs_frame_to_block: the device columns (row, item_idx, relevance) of a frame -> rec_idx [n_users x kmax]
 * (-1 padded) as get_top_k_recs followed by sorter do it (replay/metrics/base_metric.py:121-134, :22-51): per user
 * order by relevance descending, keep the first kmax rows, drop later repeats of an item (dedup != 0), compact.
 * Ties in relevance: item_idx ascending (the reference leaves them to Spark); -0.0 == +0.0.  NaN is the caller's to
 * reject.  `row` is the row of the evaluated user set; a row outside 0..n_users-1 leaves (the right join of
 * base_metric.py:135).  Optional outputs: rec_val (relevance), rec_pos (row_number BEFORE the repeats are dropped,
 * 1-based: what coverage.py:90-103 ranks by), rec_w (`payload`, a per-row double, through the same permutation).
 * n_rows == 0 is legal: every list is empty (payload may then be NULL beside a rec_w).
 * --------------------------------------------------------------------------------------------------------- */
int64_t cqlrec_recs_frame_to_block_ws_bytes(int64_t n_rows, int64_t n_users);
int cqlrec_recs_frame_to_block(const int32_t* row, const int32_t* item_idx, const double* relevance,
                               const double* payload, int64_t n_rows, int64_t n_users, int32_t kmax, int32_t dedup,
                               void* ws, int64_t ws_bytes, int32_t* rec_idx, double* rec_val, int32_t* rec_pos,
                               double* rec_w, cqlrec_stream stream);

/* The left join of prev_policy_weights onto a frame's rows (replay/metrics/base_metric.py:535-542): `keys` ascending,
 * (user_idx << 32 | item_idx), or item_idx alone when user_idx == NULL; out[i] = vals of the FIRST equal key, 0.0 for
 * a miss (.na.fill(0.0)). */
int cqlrec_recs_join_prev(const uint64_t* keys, const double* vals, int64_t n_keys, const int32_t* user_idx,
                          const int32_t* item_idx, int64_t n_rows, double* out, cqlrec_stream stream);

/* NCIS weights, in place, on a block that frame_to_block made with dedup == 0, rec_val = relevance and rec_w = the
 * joined previous-policy relevance: the activation over each user's kept rows (_softmax_by_user: minus the user's
 * minimum, base_metric.py:429-449; _sigmoid, :451-458), _weigh_and_clip (:460-488: prev == 0 -> threshold, else
 * the ratio clipped to [1/threshold, threshold]), then sorter(extra_position=2) (:549-575): later repeats of an item
 * leave with their weight.  On return rec_idx is de-duplicated and rec_w holds the weights. */
#define CQLREC_NCIS_NONE 0
#define CQLREC_NCIS_SIGMOID 1
#define CQLREC_NCIS_SOFTMAX 2
int cqlrec_recs_ncis_weights(int32_t* rec_idx, double* rec_val, double* rec_w, int64_t n_users, int32_t kmax,
                             int32_t activation, double threshold, cqlrec_stream stream);

/* Per-user metrics beside cqlrec_eval_topk's six, same indexing contract (rec_rows, CSR with ascending unique
 * items, ks ascending within 1..kmax, n_ks <= 8).  Order: RocAuc (replay/metrics/rocauc.py:43-60, length =
 * min(k, len(pred))), Unexpectedness (unexpectedness.py:40-46; base_idx [n_users x kb]: row u is user u's base list),
 * Surprisal (surprisal.py:65-68; item_w [n_item_w] by item id, 1.0 beyond the table: :99-101), NCISPrecision
 * (ncis_precision.py:24-30; rec_w beside rec_idx).  A metric whose input is NULL (gt_off / gt_items, base_idx,
 * item_w, rec_w) comes out 0.  sums[CQLREC_EVAL_EXTRAS][n_ks]; per_user[n_users][CQLREC_EVAL_EXTRAS][n_ks] optional. */
#define CQLREC_EVAL_EXTRAS 4
int64_t cqlrec_eval_extras_ws_bytes(int64_t n_users, int32_t n_ks);
int cqlrec_eval_extras(const int32_t* rec_idx, int64_t n_users, int32_t kmax, const int32_t* rec_rows,
                       const int64_t* gt_off, const int32_t* gt_items, const int32_t* base_idx, int32_t kb,
                       const double* item_w, int64_t n_item_w, const double* rec_w, const int32_t* ks /* [host] */,
                       int32_t n_ks, void* ws, int64_t ws_bytes, double* per_user, double* sums, cqlrec_stream stream);

/* Distinct users per item of a log (countDistinct: replay/metrics/surprisal.py:57-63, replay/distributions.py:74-78):
 * the (user, item) pairs sorted as one 64-bit key, run heads counted.  cnt [n_items] by item id (ids >= n_items are
 * not counted); *n_distinct_users (device) = distinct users of the log. */
int64_t cqlrec_eval_item_user_counts_ws_bytes(int64_t n_rows);
int cqlrec_eval_item_user_counts(const int32_t* item_idx, const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                                 void* ws, int64_t ws_bytes, int32_t* cnt, int64_t* n_distinct_users,
                                 cqlrec_stream stream);
/* w[i] = log2(n_users / cnt[i]) / log2(n_users) (surprisal.py:57-63), 1.0 where cnt[i] == 0; n_users > 1. */
int cqlrec_eval_surprisal_weights(const int32_t* cnt, int64_t n_items, int64_t n_users, double* w, cqlrec_stream stream);

/* Coverage (replay/metrics/coverage.py:90-112): best [n_items] = min rec_pos per item (integer atomicMin over a table
 * set to INT_MAX), counts[q] (device int64) = items with best <= ks[q].  Items the log never saw count too (:84-88):
 * n_items covers every id of rec_idx. */
int cqlrec_eval_coverage(const int32_t* rec_idx, const int32_t* rec_pos, int64_t n_users, int32_t kmax, int64_t n_items,
                         const int32_t* ks /* [host] */, int32_t n_ks, int32_t* best, int64_t* counts,
                         cqlrec_stream stream);
/* cnt[i] = cells of rec_idx that hold item i: rec_count of item_distribution (replay/distributions.py:80-86) when the
 * block was cut at k with repeats dropped. */
int cqlrec_eval_item_hist(const int32_t* rec_idx, int64_t n_users, int32_t kmax, int64_t n_items, int32_t* cnt,
                          cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f5  Train/test splitters on the device: the window passes of replay/splitters/{user_log_splitter,log_splitter}.py
 * (row_number() over a user's history, the order statistics behind DateSplitter / NewUsersSplitter, the distinct + join
 * passes of base_splitter.py:73-107) as a ranking inside each user, a row predicate and a stable compaction.  Integer
 * work throughout; the only atomics are integer ones (atomicMin / atomicAdd / atomicOr), so the same input gives the
 * same bytes.  user_idx / item_idx are dense non-negative ids below n_users / n_items: the CALLER range-checks them,
 * the kernels index count arrays and bitmaps with them.  n_rows < 2^31; n_rows == 0 is legal where stated.
 *
 * Tie-break.  The reference's row_number().over(partitionBy(user).orderBy(ts.desc())) leaves rows of equal timestamp
 * to Spark.  Here: rank = 1-based row number inside the user ordered by (key DESCENDING, input row index DESCENDING)
 * -- of equal timestamps the later input row is the "more recent" one.
 *
 * Random draws (Spark's rand(seed) / randomSplit cannot be reproduced): for element x (an input row index or a user
 * id) h(x) = mix64(mix64(seed) ^ x), mix64 = the splitmix64 finaliser of the transition sampler above (add the golden
 * constant first); u(x) = ((h >> 11) + 0.5) * 2^-53 in double.  A shuffled ranking uses h(row), compared as an
 * unsigned number, in place of the key.
 * --------------------------------------------------------------------------------------------------------- */
/* rank [n_rows] (see above), count [n_users] rows per user, *n_present (may be NULL) = users with count > 0.
 * key: any int64 whose signed order is the order wanted (data.timestamp_key); shuffle != 0: key is ignored (may be
 * NULL) and h(row) under `seed` ranks the rows.  Two stable LSD radix sorts over a row permutation (key, then user)
 * and one pass that turns sorted position into rank, as cqlrec_build_csr does it.  n_rows == 0: count = 0. */
int64_t cqlrec_split_rank_ws_bytes(int64_t n_rows, int64_t n_users);
int cqlrec_split_rank(const int32_t* user_idx, const int64_t* key, int64_t n_rows, int64_t n_users, int32_t shuffle,
                      uint64_t seed, void* ws, int64_t ws_bytes, int32_t* rank, int32_t* count, int64_t* n_present,
                      cqlrec_stream stream);

/* *out = the m-th smallest (1-based, 1 <= m <= n) of key[n]: DateSplitter's float test_start (log_splitter.py:71-80). */
int64_t cqlrec_split_kth_key_ws_bytes(int64_t n);
int cqlrec_split_kth_key(const int64_t* key, int64_t n, int64_t m, void* ws, int64_t ws_bytes, int64_t* out,
                         cqlrec_stream stream);

/* NewUsersSplitter (log_splitter.py:238-264): user_start [n_users] = min key of the user's rows (INT64_MAX for a user
 * without rows), *threshold = the largest start key dt such that the number of users starting at or after dt is
 * >= total_users * test_size (total_users = users with a row; the comparison in double).  n_rows >= 1. */
int64_t cqlrec_split_new_users_ws_bytes(int64_t n_users);
int cqlrec_split_new_users(const int32_t* user_idx, const int64_t* key, int64_t n_rows, int64_t n_users,
                           double test_size, void* ws, int64_t ws_bytes, int64_t* user_start, int64_t* threshold,
                           cqlrec_stream stream);

/* user_test_size (user_log_splitter.py:142-180): test_user [n_users] = 1 for the n_pick users with the smallest h(user)
 * among those with count > 0, ties by user id ascending; 0 for the others.  0 <= n_pick. */
int64_t cqlrec_split_pick_users_ws_bytes(int64_t n_users);
int cqlrec_split_pick_users(const int32_t* count, int64_t n_users, uint64_t seed, int64_t n_pick, void* ws,
                            int64_t ws_bytes, uint8_t* test_user, cqlrec_stream stream);

/* Per-row train / test bytes.  Unless stated, is_train = !is_test.  test_user (NULL: every user) gates the two
 * per-user rules.
 *   QUANTITY     test_user[u] && rank <= n                                       (_split_quantity)
 *   PROPORTION   test_user[u] && (double)rank / (double)count[u] <= frac         (_split_proportion's `_frac`)
 *   DATE         key >= *threshold                                               (DateSplitter)
 *   RANDOM_ROW   u(row) >= frac     (frac = 1 - test_size, computed by the caller) (RandomSplitter)
 *   RANDOM_USER  u(user) >= frac                                                 (ColdUserRandomSplitter)
 *   NEW_USERS    is_train = key < *threshold; is_test = user_start[u] >= *threshold: a row may be in neither
 *   FOLD         rank % n == fold, n folds                                       (k_folds)
 * Arrays a rule does not read may be NULL. */
#define CQLREC_SPLIT_QUANTITY 0
#define CQLREC_SPLIT_PROPORTION 1
#define CQLREC_SPLIT_DATE 2
#define CQLREC_SPLIT_RANDOM_ROW 3
#define CQLREC_SPLIT_RANDOM_USER 4
#define CQLREC_SPLIT_NEW_USERS 5
#define CQLREC_SPLIT_FOLD 6
int cqlrec_split_classify(int32_t rule, const int32_t* user_idx, const int64_t* key, const int32_t* rank,
                          const int32_t* count, const uint8_t* test_user, const int64_t* user_start,
                          const int64_t* threshold, int64_t n_rows, int64_t n, int64_t fold, double frac, uint64_t seed,
                          uint8_t* is_train, uint8_t* is_test, cqlrec_stream stream);

/* _drop_cold_items_and_users + _filter_zero_relevance (base_splitter.py:59-107), in place on is_test: presence bitmaps
 * of the users and items among the train rows (atomicOr on 32-bit words); a test row stays if its item is present
 * (drop_cold_items), its user is present (drop_cold_users) and relevance > 0.0 (drop_zero_rel).  item_idx / relevance
 * may be NULL when their flag is 0. */
int64_t cqlrec_split_filter_test_ws_bytes(int64_t n_users, int64_t n_items);
int cqlrec_split_filter_test(const int32_t* user_idx, const int32_t* item_idx, const double* relevance,
                             const uint8_t* is_train, int64_t n_rows, int64_t n_users, int64_t n_items,
                             int32_t drop_cold_users, int32_t drop_cold_items, int32_t drop_zero_rel, void* ws,
                             int64_t ws_bytes, uint8_t* is_test, cqlrec_stream stream);

/* Stable compaction: train_rows / test_rows [n_rows each] receive the ascending indices of the rows whose byte is
 * non-zero, counts[0] / counts[1] (device) how many.  n_rows == 0: counts = 0. */
int64_t cqlrec_split_compact_ws_bytes(int64_t n_rows);
int cqlrec_split_compact(const uint8_t* is_train, const uint8_t* is_test, int64_t n_rows, void* ws, int64_t ws_bytes,
                         int64_t* train_rows, int64_t* test_rows, int64_t* counts, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f6  Log preparation on the device: the filters of replay/filters.py (k-core by minimum count, rating threshold,
 * first / last N events or days of a user, global day windows, a time period) and the Indexer of
 * replay/data_preparator.py (raw integer ids <-> dense indices).  The rules of f5 carry over: integer work throughout,
 * integer atomics only (atomicAdd / atomicMin / atomicMax / atomicOr), the same input gives the same bytes; group ids
 * (user_idx, item_idx, any group column) are dense non-negative ids below n_groups which the CALLER range-checks;
 * n_rows < 2^31; arguments are validated on the host before any HIP call.
 * --------------------------------------------------------------------------------------------------------- */
/* rank [n_rows] = 1-based row number inside the user ordered by (key DESCENDING, key2 DESCENDING, input row index
 * DESCENDING); count [n_users] = rows per user.  The ascending row number is count[u] + 1 - rank.  key: as in
 * cqlrec_split_rank.  key2: NULL, or non-negative values below n_key2 (the item of take_num_user_interactions).  Stable
 * LSD radix sorts over a reversed row permutation: key2, key, user.  n_rows == 0: count = 0. */
int64_t cqlrec_prepare_rank_ws_bytes(int64_t n_rows, int64_t n_users);
int cqlrec_prepare_rank(const int32_t* user_idx, const int64_t* key, const int32_t* key2, int64_t n_rows, int64_t n_users,
                        int64_t n_key2, void* ws, int64_t ws_bytes, int32_t* rank, int32_t* count, cqlrec_stream stream);

/* count [n_groups] = rows whose id is g (integer atomicAdd). */
int cqlrec_prepare_count(const int32_t* ids, int64_t n_rows, int64_t n_groups, int32_t* count, cqlrec_stream stream);

/* gmin / gmax [n_groups] = least / greatest key of the group's rows (INT64_MAX / INT64_MIN for a group without rows).
 * group == NULL: the whole column is one group (n_groups must be 1; block reductions, one pair of atomics per block). */
int cqlrec_prepare_minmax(const int32_t* group, const int64_t* key, int64_t n_rows, int64_t n_groups, int64_t* gmin,
                          int64_t* gmax, cqlrec_stream stream);

/* keep [n_rows]: one byte per row, 1 = the row stays.
 *   MIN_COUNT         count[group] >= n                                              (filter_by_min_count)
 *   MIN_VALUE         value >= x, IEEE: a NaN row goes                               (filter_out_low_ratings)
 *   NUM_INTERACTIONS  first ? count[group] + 1 - rank <= n : rank <= n               (take_num_user_interactions)
 *   DAYS_USER         first ? t < extreme[group] (+) span : t > extreme[group] (-) span   (take_num_days_of_user_hist;
 *                     extreme = the group's min when first, its max otherwise)
 *   DAYS_GLOBAL       the same with extreme[0]                                       (take_num_days_of_global_hist)
 *   PERIOD            lo <= key && (open_end || key < hi)                            (take_time_period)
 * The span of the DAYS rules: float_key == 0: n, in the key's unit, added / subtracted in int64 SATURATING at the int64
 * limits; float_key != 0: key and extreme are data.timestamp_key images of doubles, decoded back, the bound is ONE
 * double add / subtract of x and the comparison is made in double.  Arrays a rule does not read may be NULL. */
#define CQLREC_KEEP_MIN_COUNT 0
#define CQLREC_KEEP_MIN_VALUE 1
#define CQLREC_KEEP_NUM_INTERACTIONS 2
#define CQLREC_KEEP_DAYS_USER 3
#define CQLREC_KEEP_DAYS_GLOBAL 4
#define CQLREC_KEEP_PERIOD 5
int cqlrec_prepare_keep(int32_t rule, const int32_t* group, const int64_t* key, const double* value, const int32_t* rank,
                        const int32_t* count, const int64_t* extreme, int64_t n_rows, int64_t n, int32_t first,
                        int32_t float_key, int64_t lo, int64_t hi, int32_t open_end, double x, uint8_t* keep,
                        cqlrec_stream stream);

/* Stable compaction: rows [n_rows] receives the ascending indices of the rows whose byte is non-zero, *n_kept (device)
 * how many.  n_rows == 0: *n_kept = 0. */
int64_t cqlrec_prepare_compact_ws_bytes(int64_t n_rows);
int cqlrec_prepare_compact(const uint8_t* keep, int64_t n_rows, void* ws, int64_t ws_bytes, int64_t* rows,
                           int64_t* n_kept, cqlrec_stream stream);

/* Indexer.  distinct: out [n] receives the distinct values of ids[n] in ascending signed order, *n_out (device) how
 * many (radix sort + unique).  sort_labels: sorted [m] = labels ascending, sorted_idx [m] = the position each had in
 * labels (labels are distinct).  lookup: out[i] = the label index of ids[i] (binary search over sorted), or -1 and
 * *miss = 1 (device; 0 when every id was found).  gather: out[i] = labels[idx[i]]; an index outside [0, m) gives 0
 * and *bad = 1 (device). */
int64_t cqlrec_prepare_distinct_ws_bytes(int64_t n);
int cqlrec_prepare_distinct(const int64_t* ids, int64_t n, void* ws, int64_t ws_bytes, int64_t* out, int64_t* n_out,
                            cqlrec_stream stream);
int64_t cqlrec_prepare_sort_labels_ws_bytes(int64_t m);
int cqlrec_prepare_sort_labels(const int64_t* labels, int64_t m, void* ws, int64_t ws_bytes, int64_t* sorted,
                               int32_t* sorted_idx, cqlrec_stream stream);
int cqlrec_prepare_lookup(const int64_t* ids, int64_t n_rows, const int64_t* sorted, const int32_t* sorted_idx, int64_t m,
                          int32_t* out, int32_t* miss, cqlrec_stream stream);
int cqlrec_prepare_gather(const int64_t* idx, int64_t n_rows, const int64_t* labels, int64_t m, int64_t* out,
                          int32_t* bad, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f7  History-based features on the device (replay/history_based_fp.py): what LogStatFeaturesProcessor and
 * ConditionalPopularityProcessor compute with group-bys and joins is sorted segments, fixed-order fp64 sums, binary
 * searches and one fused gather here.  The rules of f5 / f6 carry over: integer atomics only, no floating-point
 * atomics, the same input gives the same bytes; ids are dense non-negative ids below n_groups which the CALLER
 * range-checks; n_rows < 2^31; arguments are validated on the host before any HIP call.
 *
 * A floating-point sum over a segment is formed in an order fixed by position: pieces of 1024 consecutive sorted rows
 * counted from the segment's first row, each summed by one wave (lane l takes rows l, l + 64, ..., then a butterfly
 * over the lanes), and the pieces of a group summed by one wave the same way.  Work per thread is bounded whatever
 * the group sizes are.
 * --------------------------------------------------------------------------------------------------------- */
/* day [n] = floor(key / unit) (floor division: keys before 1970 work), unit > 0. */
int cqlrec_features_day(const int64_t* key, int64_t n, int64_t unit, int64_t* day, cqlrec_stream stream);

/* perm [n_rows] = the rows ordered by (group, key, input row index) ascending; offsets [n_groups + 1] = the first
 * sorted position of every group (offsets[n_groups] = n_rows).  key == NULL: by (group, input row index).  Stable LSD
 * radix sorts: key, then group.  n_rows == 0: offsets = 0. */
int64_t cqlrec_features_segments_ws_bytes(int64_t n_rows, int64_t n_groups);
int cqlrec_features_segments(const int32_t* group, const int64_t* key, int64_t n_rows, int64_t n_groups, void* ws,
                             int64_t ws_bytes, int32_t* perm, int64_t* offsets, cqlrec_stream stream);

/* out [n_groups][CQLREC_FEATURES_STATS] = count, mean, sample std (n - 1; 0 for a group of one row), and the elements
 * of the group's rows at the 1-based ranks clamp(ceil(p * n), 1, n) for p = 0.05, 0.5, 0.95 -- quantiles when perm
 * orders every group by value ascending (cqlrec_features_segments with the order-preserving key of the value).  The
 * variance is two-pass: the mean first, then the squared deviations around it.  A group without rows gets zeros. */
#define CQLREC_FEATURES_STATS 6
int64_t cqlrec_features_segment_stats_ws_bytes(int64_t n_rows, int64_t n_groups);
int cqlrec_features_segment_stats(const int32_t* perm, const int64_t* offsets, const double* value, int64_t n_rows,
                                  int64_t n_groups, void* ws, int64_t ws_bytes, double* out, cqlrec_stream stream);

/* out [n_groups] = the mean over the group's rows of an expression of the row (0 for a group without rows), over any
 * ordering by group.  o = other[row] * tab_stride:
 *   GATHER          tab_a[o]
 *   ABNORMALITY     |value - tab_a[o]|
 *   ABNORMALITY_CR  (|value - tab_a[o]| * (1 - (tab_b[o] - min_std) / (max_std - min_std)))^2, min_std < max_std */
#define CQLREC_FEATURES_MEAN_GATHER 0
#define CQLREC_FEATURES_MEAN_ABNORMALITY 1
#define CQLREC_FEATURES_MEAN_ABNORMALITY_CR 2
int64_t cqlrec_features_segment_mean_ws_bytes(int64_t n_rows, int64_t n_groups);
int cqlrec_features_segment_mean(int32_t rule, const int32_t* perm, const int64_t* offsets, const double* value,
                                 const int32_t* other, const double* tab_a, const double* tab_b, int64_t tab_stride,
                                 double min_std, double max_std, int64_t n_rows, int64_t n_groups, void* ws,
                                 int64_t ws_bytes, double* out, cqlrec_stream stream);

/* out [n_groups] = the number of distinct keys among the group's rows, over an ordering by (group, key): the heads of
 * the runs are counted (integer atomicAdd). */
int cqlrec_features_segment_distinct(const int32_t* group, const int32_t* perm, const int64_t* offsets, const int64_t* key,
                                     int64_t n_rows, int64_t n_groups, int32_t* out, cqlrec_stream stream);

/* Conditional popularity.  The composite key of a row is entity * (n_cat + 1) + code[other], code [ids of the other
 * entity] in [0, n_cat] with n_cat = the null category.  keys [n_rows] receives the distinct keys ascending, pop
 * [n_rows] the rows with that key divided by entity_count[entity], *n_out (device) how many.  n_rows == 0: *n_out = 0. */
int64_t cqlrec_features_pair_counts_ws_bytes(int64_t n_rows);
int cqlrec_features_pair_counts(const int32_t* entity, const int32_t* other, const int32_t* code,
                                const int32_t* entity_count, int64_t n_rows, int64_t n_entity, int64_t n_cat, void* ws,
                                int64_t ws_bytes, int64_t* keys, double* pop, int64_t* entity_off, int64_t* n_out,
                                cqlrec_stream stream);

/* One fitted popularity table as the block kernel reads it (device pointers).  The category of a pair comes from
 * pair_code [n_pairs] when given, otherwise from code [n_code] indexed by the other entity's id (an id beyond it has
 * the null category).  A category outside [0, n_cat) -- null or unseen -- and a key that is not in keys [m] are `na`.  The search
 * for a key runs over the entity's own keys, keys[entity_off[e] .. entity_off[e + 1]): at most n_cat + 1 of them. */
typedef struct cqlrec_features_pop {
  const int32_t* code;
  const int32_t* pair_code;
  const int64_t* keys;
  const double* pop;
  const int64_t* entity_off;
  int64_t n_code, n_entity, n_cat, m;
  int32_t entity_is_item, reserved;
} cqlrec_features_pop;

/* block [n_pairs][n_cols], row-major float or double, written once by one launch.  colmap (HOST) [n_cols][3] =
 * (kind, a, b); a cold id -- outside the table, or with count 0 -- reads 0 from its table:
 *   COL_USER / COL_ITEM        column a of utab [n_users][fu] / itab [n_items][fi]
 *   COL_NA_USER / COL_NA_ITEM  1 for a cold id, else 0
 *   COL_DIFF_USER              user column a - item column b, after the zero fill;  COL_DIFF_ITEM: item a - user b
 *   COL_POP / COL_POP_NA       the popularity of table a (0 where na) / 1 where na, else 0 */
#define CQLREC_FEATURES_MAX_COLS 64
#define CQLREC_FEATURES_MAX_POP 8
#define CQLREC_FEATURES_F32 0
#define CQLREC_FEATURES_F64 1
#define CQLREC_FEATURES_COL_USER 0
#define CQLREC_FEATURES_COL_ITEM 1
#define CQLREC_FEATURES_COL_NA_USER 2
#define CQLREC_FEATURES_COL_NA_ITEM 3
#define CQLREC_FEATURES_COL_DIFF_USER 4
#define CQLREC_FEATURES_COL_DIFF_ITEM 5
#define CQLREC_FEATURES_COL_POP 6
#define CQLREC_FEATURES_COL_POP_NA 7
int cqlrec_features_block(const int64_t* user_idx, const int64_t* item_idx, int64_t n_pairs, const double* utab,
                          const int32_t* ucount, int64_t n_users, int32_t fu, const double* itab, const int32_t* icount,
                          int64_t n_items, int32_t fi, const int32_t* colmap /* [host] */, int32_t n_cols,
                          const cqlrec_features_pop* pops, int32_t n_pop, int32_t dtype, void* block,
                          cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f8  Neighbourhood models on the device (replay/models/knn.py, NeighbourRec of replay/models/base_rec.py): the row-wise
 * top-k of a sparse x sparse product, so that the n x n similarity matrix is never formed, and the small kernels around
 * it.  ItemKNN.fit (C = A^T A, the k best per row) and NeighbourRec.predict (R = B S, the k best unseen per row) are the
 * same operation with two epilogues.  The rules of f5 - f7 carry over: integer atomics only, no floating-point atomics,
 * the same input gives the same bytes; ids are dense non-negative ids which the CALLER range-checks; arguments are
 * validated on the host before any HIP call.  Both matrices are CSR: int64 offsets, int32 column ids, fp64 values.
 *
 * Shape: expand, sort, reduce, select.  Query rows are taken in chunks of consecutive rows whose expansion -- the
 * number of (L entry, R entry) combinations -- fits max_tuples (a larger row is a chunk of its own).  One thread per
 * tuple finds its L entry by binary search in the entry prefix and writes the key (local row, j) and the product; a
 * stable radix sort over the bits the key uses brings the terms of one (row, j) together in (L entry, R entry) order;
 * a sum of up to 32 terms is added left to right by one thread, a longer one by one wave (lane l takes the terms
 * l, l + 64, ... in that order, then a butterfly over the lanes): the order is fixed by the position inside the sum, so
 * the result does not depend on max_tuples, bit for bit.  The k best of a row come out of two more stable sorts (the
 * order-preserving image of the fp64 value, then the row).  No buffer of n_q x n_cols elements exists.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_NEIGHBOUR_FIT 0
#define CQLREC_NEIGHBOUR_PREDICT 1
#define CQLREC_NEIGHBOUR_MAX_K 1024
#define CQLREC_NEIGHBOUR_WEIGHT_NONE 0
#define CQLREC_NEIGHBOUR_WEIGHT_TF_IDF 1
#define CQLREC_NEIGHBOUR_WEIGHT_BM25 2

/* w [n_rows]: the weight of a log row (knn.py:76-154).  rel = relevance[row], or 1 when relevance is NULL.
 *   NONE    rel
 *   TF_IDF  rel * log1p(n_items / ucount[user])
 *   BM25    (rel * (k1 + 1) / (rel + k1 * (1 - b + b * (icount[item] / avgdl)))) * log1p((n_items - DF + 0.5) / (DF + 0.5)),
 *           DF = ucount[user], avgdl = n_rows / n_items (one fp64 division)
 * n_items is the number of DISTINCT items of the log; every expression is evaluated in fp64 exactly as written. */
int cqlrec_neighbour_weights(const int32_t* user_idx, const int32_t* item_idx, const double* relevance,
                             const int32_t* ucount, const int32_t* icount, int64_t n_rows, int64_t n_items,
                             int32_t weighting, double k1, double b, double* w, cqlrec_stream stream);

/* norm [n_groups] = sqrt(sum of w[row]^2 over the group's rows), over an ordering by group (cqlrec_features_segments);
 * one wave per group sums in an order fixed by position.  A group without rows gets 0. */
int cqlrec_neighbour_norms(const int32_t* perm, const int64_t* offsets, const double* w, int64_t n_rows, int64_t n_groups,
                           double* norm, cqlrec_stream stream);

/* The count pass.  entry_prefix [nnz_l + 1]: the exclusive int64 prefix of the R row lengths of the L entries, the total
 * at the end; row_prefix [n_q + 1] = entry_prefix[l_off[q]]; stats [2] (device) = the total expansion and the largest
 * expansion of one row.  l_col holds ids below n_mid, r_off has n_mid + 1 entries. */
int64_t cqlrec_neighbour_count_ws_bytes(int64_t nnz_l);
int cqlrec_neighbour_count(const int64_t* l_off, const int32_t* l_col, int64_t n_q, int64_t nnz_l, const int64_t* r_off,
                           int64_t n_mid, void* ws, int64_t ws_bytes, int64_t* entry_prefix, int64_t* row_prefix,
                           int64_t* stats, cqlrec_stream stream);

/* For every query row q: C[q][j] = sum of a * b over the L entries (m, a) of row q and the R entries (j, b) of row m,
 * then the k best j.  ids [n_q][k] (padded with -1), vals [n_q][k] (padded with 0), count [n_q].  A j that no
 * combination reaches is never a candidate; a reached j whose sum is 0 is one.
 *   FIT      drops j == q; value = C / (norm_q[q] * norm_j[j] + shrink); drops a pair whose denominator is 0;
 *            order: value descending, j DESCENDING (knn.py:214-217)
 *   PREDICT  value = C; drops j with mask[j] == 0 (mask: NULL or one byte per column); drops j found in the ascending
 *            list seen_col[seen_off[q] .. seen_off[q + 1]) (NULL: none); order: value descending, j ASCENDING
 * row_prefix_host: the row prefix of the count pass, copied to the HOST (the chunks are cut there).  The workspace
 * holds max(max_tuples, largest_row) tuples; 1 <= k <= CQLREC_NEIGHBOUR_MAX_K; the result does not depend on
 * max_tuples.  No synchronisation. */
int64_t cqlrec_neighbour_topk_ws_bytes(int64_t n_q, int64_t n_cols, int64_t max_tuples, int64_t largest_row, int32_t k);
int cqlrec_neighbour_topk(int32_t mode, const int64_t* l_off, const int32_t* l_col, const double* l_val, int64_t n_q,
                          int64_t nnz_l, const int64_t* r_off, const int32_t* r_col, const double* r_val, int64_t n_mid,
                          int64_t n_cols, const int64_t* entry_prefix, const int64_t* row_prefix_host, int64_t max_tuples,
                          int64_t largest_row, int32_t k, const double* norm_q, const double* norm_j, double shrink,
                          const uint8_t* mask, const int64_t* seen_off, const int32_t* seen_col, void* ws,
                          int64_t ws_bytes, int32_t* ids, double* vals, int32_t* count, cqlrec_stream stream);

/* score [n_pairs] = sum over the history rows i of pair_user (h_item[h_off[u] .. h_off[u + 1]), in that order) of
 * S[i -> pair_item], S a CSR whose rows are sorted by column ascending (binary search); present [n_pairs] = 1 when at
 * least one i contributes.  A user beyond n_users or a history item beyond n_s_rows contributes nothing. */
int cqlrec_neighbour_pair_scores(const int32_t* pair_user, const int32_t* pair_item, int64_t n_pairs, const int64_t* h_off,
                                 const int32_t* h_item, int64_t n_users, const int64_t* s_off, const int32_t* s_col,
                                 const double* s_val, int64_t n_s_rows, double* score, uint8_t* present,
                                 cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f9  Alternating least squares on the device (ALSWrap of replay/models/als.py; the solver is Spark ML's ALS at the
 * settings that wrapper uses; DESIGN.md section 3.10 is the normative text).  Factors are fp32 [n][rank], 1 <= rank <=
 * CQLREC_ALS_MAX_RANK; normal equations and the solve are fp64.  A side is a CSR over its destination rows in the order
 * of cqlrec_features_segments: int64 offsets, int32 source ids, fp64 ratings.  With (s, rho) the entries of a row:
 *   IMPLICIT  c = alpha |rho|;  A = G + sum c y_s y_s^T;  b = sum over rho > 0 of (1 + c) y_s;  n_expl = #{rho > 0}
 *   EXPLICIT  A = sum y_s y_s^T;  b = sum rho y_s;  n_expl = the number of entries;  no G
 * Sum order: the entries of a row are cut into pieces of CQLREC_ALS_PIECE consecutive entries; inside a piece the terms
 * are added left to right from +0.0 (element (i, j), j <= i: acc = fma(c y_i, y_j, acc); b_j: acc = fma(w, y_j, acc)),
 * the pieces are added in piece order, G is added last.  A row longer than a piece is always spread over one workgroup
 * per piece, with the partial matrices in the workspace; nothing depends on the grid, on the other rows of a call or on
 * the order of a row list.  Integer atomics only; the same input gives the same bytes.  A source id outside [0, n_src)
 * reads a zero row.  The rules of f5 - f8 carry over: arguments are validated on the host before any HIP call.
 *
 * rows [n_list]: the destination rows to work on (NULL: all of them, n_list = n_dst).  n_pieces: the number of pieces
 * of the listed rows that are longer than CQLREC_ALS_PIECE -- the sum of ceil(len / CQLREC_ALS_PIECE) over them --
 * which the caller knows from the offsets; it sizes the workspace and two of the three launches.  A long row beyond the
 * announced pieces is not computed: the half step counts it as failed, the normal equations return NaN and n_expl = -1.
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_ALS_PIECE 1024
#define CQLREC_ALS_GRAM_BLOCK 4096
#define CQLREC_ALS_MAX_RANK 128
#define CQLREC_ALS_MAX_K 512
#define CQLREC_ALS_EXPLICIT 0
#define CQLREC_ALS_IMPLICIT 1

/* G [rank][rank] = F^T F in fp64, F [n_rows][rank] fp32: blocks of CQLREC_ALS_GRAM_BLOCK consecutive rows are summed
 * left to right (acc = fma(y_i, y_j, acc)), then the blocks in block order.  n_rows == 0: zeros. */
int64_t cqlrec_als_gram_ws_bytes(int64_t n_rows, int32_t rank);
int cqlrec_als_gram(const float* F, int64_t n_rows, int32_t rank, void* ws, int64_t ws_bytes, double* G,
                    cqlrec_stream stream);

/* A [n_list][rank][rank] (symmetric, G included when given, the regulariser not), b [n_list][rank], n_expl [n_list], by
 * position in the list.  A row without entries gets A = G (or zeros), b = 0, n_expl = 0. */
int64_t cqlrec_als_normal_equations_ws_bytes(int64_t n_list, int64_t n_pieces, int32_t rank);
int cqlrec_als_normal_equations(const int64_t* offsets, const int32_t* src, const double* rating, int64_t n_dst,
                                const float* F, int64_t n_src, int32_t rank, const double* G, int32_t mode, double alpha,
                                const int32_t* rows, int64_t n_list, int64_t n_pieces, void* ws, int64_t ws_bytes, double* A,
                                double* b, int32_t* n_expl, cqlrec_stream stream);

/* The update of one side: for every listed row, X[row] = fp32 of the solution of (A + reg n_expl I) x = b by an fp64
 * Cholesky factorisation (L L^T, forward and back substitution) on chip, has_factor[row] = 1.  A row without entries
 * gets a zero row and has_factor = 0.  A pivot that is not positive leaves the row zero with has_factor = 0 and adds 1
 * to *n_failed (device int32, which the caller zeroes).  G: the Gram matrix of F (IMPLICIT; ignored for EXPLICIT). */
int64_t cqlrec_als_half_step_ws_bytes(int64_t n_list, int64_t n_pieces, int32_t rank);
int cqlrec_als_half_step(const int64_t* offsets, const int32_t* src, const double* rating, int64_t n_dst, const float* F,
                         int64_t n_src, int32_t rank, const double* G, int32_t mode, double alpha, double reg,
                         const int32_t* rows, int64_t n_list, int64_t n_pieces, void* ws, int64_t ws_bytes, float* X,
                         uint8_t* has_factor, int32_t* n_failed, cqlrec_stream stream);

/* score(u, i) = the fmaf chain s = fmaf(U[u][c], V[i][c], s) over c ascending from s = 0, in fp32: the one function of
 * both entry points below.
 * ids [n_q][k] (padded with -1), vals [n_q][k] (padded with -inf), count [n_q]: the k best items of users[q] by score
 * descending, then item id ascending, among the items with v_has != 0, mask != 0 (mask: NULL or one byte per item) and
 * not in the ascending list seen_col[seen_off[u] .. seen_off[u + 1]) (seen_off [n_users + 1], indexed by the user id;
 * NULL: none).  A user outside [0, n_users) or with u_has == 0 gets count 0.  1 <= k <= CQLREC_ALS_MAX_K.  V is 16-byte
 * aligned.  No scratch. */
int cqlrec_als_topk(const int32_t* users, int64_t n_q, const float* U, const uint8_t* u_has, int64_t n_users, const float* V,
                    const uint8_t* v_has, int64_t n_items, int32_t rank, const uint8_t* mask, const int64_t* seen_off,
                    const int32_t* seen_col, int32_t k, int32_t* ids, float* vals, int32_t* count, cqlrec_stream stream);

/* score [n_pairs] and valid [n_pairs] = 0 where either id is out of range or has no factor (the score is then 0) */
int cqlrec_als_pair_scores(const int32_t* pair_user, const int32_t* pair_item, int64_t n_pairs, const float* U,
                           const uint8_t* u_has, int64_t n_users, const float* V, const uint8_t* v_has, int64_t n_items,
                           int32_t rank, float* score, uint8_t* valid, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f10  Association rules on the device (AssociationRulesItemRec of replay/models/association_rules.py; DESIGN.md section
 * 3.13 is the normative text): the engine of f8 with a third epilogue.  The rules of f5 - f9 carry over: integer atomics
 * only, the same input gives the same bytes, arguments are validated on the host before any HIP call.  The count pass is
 * cqlrec_neighbour_count, the chunk loop is the one of cqlrec_neighbour_topk.
 * --------------------------------------------------------------------------------------------------------- */

/* keep [n_rows] = 1 at ONE row of every distinct (session, item[, relevance]) triple, 0 at the others.  perm [n_rows]: a
 * permutation of the rows that brings equal triples together (any order by (session, item, relevance value) does); one
 * thread per position compares its row with the row in front, so a long run of equal rows costs its length.  relevance:
 * NULL (every weight is 1) or fp64 without NaN; -0.0 and +0.0 are one value.  No scratch. */
int cqlrec_rules_distinct(const int32_t* session, const int32_t* item, const double* relevance, const int32_t* perm,
                          int64_t n_rows, uint8_t* keep, cqlrec_stream stream);

/* L = items x sessions and R = sessions x items, both CSR (int64 offsets, int32 columns, fp64 weights) over the distinct
 * rows that passed the item filter; entry_prefix / row_prefix_host / largest_row as cqlrec_neighbour_count gave them for
 * (L, R).  For every ordered pair a != b that shares a session:
 *   pair_count = the number of (row of a, row of b) combinations in one session; pair_relevance p = the sum of
 *   min(w_a, w_b) over them, in the order of f8's sums (up to 32 terms left to right, more by one wave)
 *   item_relevance [n_items] (output) = the sum of the weights of an item's rows, one wave per item; A = item_relevance[a],
 *   C = item_relevance[b], n = (double)num_sessions
 *   confidence = p / A;   lift = (n * confidence) / C;
 *   confidence_gain = (C - p == 0) ? +inf : (confidence * (n - A)) / (C - p)        -- each evaluated as written, in fp64
 * A pair with pair_count < min_pair_count, A == 0 or C == 0 is dropped.  Per a the k best by (lift descending, b
 * DESCENDING; -0.0 = +0.0): ids [n_items][k] (padded with -1), confidence / lift / confidence_gain [n_items][k] (padded
 * with 0), count [n_items].  The workspace is cqlrec_neighbour_topk's for n_q = n_cols = n_items; the result does not
 * depend on max_tuples.  No synchronisation. */
int64_t cqlrec_rules_topk_ws_bytes(int64_t n_items, int64_t max_tuples, int64_t largest_row, int32_t k);
int cqlrec_rules_topk(const int64_t* l_off, const int32_t* l_col, const double* l_val, int64_t n_items, int64_t nnz_l,
                      const int64_t* r_off, const int32_t* r_col, const double* r_val, int64_t n_sessions,
                      const int64_t* entry_prefix, const int64_t* row_prefix_host, int64_t max_tuples, int64_t largest_row,
                      int32_t k, int64_t num_sessions, int64_t min_pair_count, void* ws, int64_t ws_bytes, int32_t* ids,
                      double* confidence, double* lift, double* confidence_gain, int32_t* count, double* item_relevance,
                      cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f11  Dense fp64 linear algebra and ADMM SLIM on the device (ADMMSLIM of replay/models/admm_slim.py; DESIGN.md section
 * 3.14 is the normative text).  Every matrix is row-major fp64.  The rules of f5 - f10 carry over: integer atomics only,
 * no floating-point atomics, the same input gives the same bytes, arguments are validated on the host before any HIP
 * call.  Element-wise expressions are evaluated as written (no contraction).
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_DENSE_GRAM_PIECE 1024 /* entries of an item row that one workgroup of cqlrec_dense_gram sums */
#define CQLREC_DENSE_BLOCK 64        /* the edge of a diagonal block that is factorised and inverted on chip */

/* D = alpha op(A) op(B) + beta E on v_mfma_f64_16x16x4_f64; op(A) is m x k, op(B) is k x n, D and E are m x n; trans_x =
 * 0: the matrix as stored, 1: its transpose (A is then stored k x m, B n x k).  Any m, n, k >= 1; edge tiles are
 * predicated.  The sum over k of an element runs k ascending whatever the grid (no split over k); the element is
 * alpha * sum, plus beta * E when beta != 0 (E is not read when beta == 0 and may be NULL).  D may be E; D must not
 * overlap A or B.  No scratch. */
int cqlrec_dense_gemm_f64(const double* A, int64_t lda, int32_t trans_a, const double* B, int64_t ldb, int32_t trans_b,
                          const double* E, int64_t lde, double alpha, double beta, int64_t m, int64_t n, int64_t k, double* D,
                          int64_t ldd, cqlrec_stream stream);

/* G [n_items][n_items] = X^T X, X the users x items matrix of a log whose duplicated (user, item) rows are summed in row
 * order.  The two views of the log as cqlrec_features_segments orders them: items -> (user, value) by (item, user, row)
 * and users -> (item, value) by (user, item, row).  G_ij is summed users ascending; an item row of more than
 * CQLREC_DENSE_GRAM_PIECE entries is cut into pieces of that many entries which are summed apart and combined in piece
 * order.  n_pieces: the sum of ceil(len / CQLREC_DENSE_GRAM_PIECE) over the item rows longer than a piece, which the
 * caller knows from the offsets; a long row beyond the announced pieces comes out as NaN. */
int64_t cqlrec_dense_gram_ws_bytes(int64_t n_items, int64_t n_pieces);
int cqlrec_dense_gram(const int64_t* i_off, const int32_t* i_user, const double* i_val, const int64_t* u_off,
                      const int32_t* u_item, const double* u_val, int64_t n_items, int64_t n_users, int64_t n_pieces, void* ws,
                      int64_t ws_bytes, double* G, cqlrec_stream stream);

/* X [n][n] = (A + shift I)^-1 for a symmetric positive definite A + shift I, of which the lower triangle is read: a
 * blocked Cholesky factorisation whose diagonal blocks (CQLREC_DENSE_BLOCK) are factorised and inverted by one workgroup
 * on chip; panels, trailing updates and L^-T L^-1 go through the GEMM above.  *status (device int32): 0, or 1 + the index
 * of the first pivot that was not positive -- X is then finite garbage; nothing faults or loops.  X must not overlap A. */
int64_t cqlrec_dense_spd_inverse_ws_bytes(int64_t n);
int cqlrec_dense_spd_inverse(const double* A, int64_t lda, int64_t n, double shift, void* ws, int64_t ws_bytes, double* X,
                             int32_t* status, cqlrec_stream stream);

/* One ADMM iteration on W, P, C, Gamma [n][n] (C and Gamma are updated in place), with c = lambda_1 / rho:
 *   T = P + W (rho C - Gamma);  v_j = T_jj / W_jj;  B_ij = T_ij - W_ij v_j;  S = B + Gamma / rho;
 *   C' = max(S - c, 0) - max(-S - c, 0);  Gamma' = Gamma + rho (B - C')
 * sums [5] (device) = the sums of squares of B - C', C' - C, B, C', Gamma', per tile, then over the tiles in an order
 * fixed by the tile index.  B is never stored; the workspace holds rho C - Gamma, v and the tile sums.  rho > 0,
 * lambda_1 >= 0. */
int64_t cqlrec_admm_iteration_ws_bytes(int64_t n);
int cqlrec_admm_iteration(const double* W, const double* P, double* C, double* Gamma, int64_t n, double rho, double lambda_1,
                          void* ws, int64_t ws_bytes, double* sums, cqlrec_stream stream);

/* The non-zeros of C [n][n] as CSR, columns ascending.  Two calls: with col == val == NULL it counts and writes offsets
 * [n_rows + 1] (int64; the rows n .. n_rows - 1 are empty); the caller reads offsets[n], allocates col (int32) and val
 * (fp64) and calls again with them to have them written.  -0.0 is a zero. */
int cqlrec_admm_compact(const double* C, int64_t n, int64_t n_rows, int64_t* offsets, int32_t* col, double* val,
                        cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * f12  SLIM on the device (SLIM of replay/models/slim.py; DESIGN.md section 3.15 is the normative text).  The rules of
 * f5 - f11 carry over: integer atomics only, no floating-point atomics, the same input gives the same bytes, arguments
 * are validated on the host before any HIP call, expressions are evaluated as written (no contraction).
 * --------------------------------------------------------------------------------------------------------- */
#define CQLREC_SLIM_MAX_ITEMS 16384 /* the largest n of cqlrec_slim_fit: q of one column (8 n bytes) lives in the LDS */

/* Per target column j in [col_begin, col_end): the minimiser over w >= 0, w_j = 0 of
 *   1/(2 nu) |x_j - X w|^2 + lambda_ |w|_1 + beta/2 |w|^2,   nu = n_users,
 * by cyclic coordinate descent on G = X^T X [n][n] (symmetric, as cqlrec_dense_gram writes it; rows are read where the
 * text says columns).  From w = 0, q = G[:, j]; a sweep visits i = 0 .. n-1 ascending, i != j: d = G_ii + nu * beta; if
 * d <= 0 the coordinate stays 0; otherwise new = max(0, (q_i + G_ii * w_i) - nu * lambda_) / d, and where new != w_i:
 * q = q - (new - w_i) * G[i, :], w_i = new.  After every full sweep q is recomputed from w, element by element
 * ((G_ej - w_k1 G_k1,e) - w_k2 G_k2,e) - ... over the support k ascending, and the certificate is taken from it:
 *   g_i = ((-q_i) / nu + beta * w_i) + lambda_;  v_i = g_i where w_i > 0, min(g_i, 0) where w_i = 0;  v_j = 0.
 * The column is done when max |v_i| <= tol * lambda_ or after max_iter sweeps.  A column with G_jj = 0 is all zeros,
 * without a sweep (sweeps = 0, kkt = 0).
 * S [n][lds] (row-major): S[i, j] = w_i of column j; only the columns of the range are written, all n rows of them.
 * sweeps, kkt, updates [n], indexed by j: the number of sweeps, the last max |v_i|, the number of non-zero updates; only
 * the entries of the range are written.  A column's bytes do not depend on the range or on which workgroup ran it.
 * No synchronisation. */
int64_t cqlrec_slim_fit_ws_bytes(int64_t n); /* 0: n out of range (1 .. CQLREC_SLIM_MAX_ITEMS) */
int cqlrec_slim_fit(const double* G, int64_t ldg, int64_t n, int64_t n_users, double beta, double lambda_, double tol,
                    int32_t max_iter, int64_t col_begin, int64_t col_end, void* ws, int64_t ws_bytes, double* S, int64_t lds,
                    int32_t* sweeps, double* kkt, int64_t* updates, cqlrec_stream stream);

/* ---------------------------------------------------------------------------------------------------------
 * Measurement hooks (bench.py): when enabled, every launcher brackets its kernel with a pair of HIP events on
 * the stream it launches on; cqlrec_prof_read synchronises those events and returns, per phase, the summed
 * kernel time in ms and the number of launches, then resets the pool.  Not capturable in a hipGraph; off by
 * default.  The reference's only harness is time.time() around fit/predict
 * (experiments/02_models_comparison.ipynb:843-867).
 * --------------------------------------------------------------------------------------------------------- */
enum {
  CQLREC_PH_SAMPLE = 0, CQLREC_PH_GATHER_FWD, CQLREC_PH_ENCODER_FWD, CQLREC_PH_QHEAD_LSE, CQLREC_PH_QHEAD_ARGMAX,
  CQLREC_PH_QHEAD_BWD_DH, CQLREC_PH_QHEAD_BWD_DE, CQLREC_PH_QHEAD_SMALL, CQLREC_PH_ENCODER_BWD,
  CQLREC_PH_GATHER_BWD, CQLREC_PH_ADAM, CQLREC_PH_TOPK_TILEMAX, CQLREC_PH_TOPK_SELECT, CQLREC_PH_COUNT
};
int cqlrec_prof_enable(int32_t on);
/* Restrict the bracketing to the phases whose bit (1u << CQLREC_PH_*) is set; default: all.  Every event pair
 * costs two barrier packets on its stream, so a throughput measurement brackets only the kernel it reports on. */
int cqlrec_prof_select(uint32_t phase_mask);
int cqlrec_prof_read(double* ms_sum /* [host] CQLREC_PH_COUNT */, int64_t* launches /* [host] CQLREC_PH_COUNT */);

/* Schedule marks (tools/phase_timing.py): nine timing events at the joints of the middle step of a
 * cqlrec_train_steps call (n_steps >= 4) -- loss, dH done, item-side backward done, encoder+gather backward done,
 * Adam(E_in) done, Adam(E_out) done, next step's prologue done, its LSE done, its loss; then encoder dx done, window-
 * gather backward done, the next step's sample + pair sorts done -- cheap enough not to disturb
 * the overlap they measure.  marks_read synchronises and returns ms relative to the first mark (-1: not recorded). */
#define CQLREC_DEBUG_MARKS 12
int cqlrec_debug_marks_enable(int32_t on);
int cqlrec_debug_marks_read(float* ms_out /* [host] CQLREC_DEBUG_MARKS */);

#ifdef __cplusplus
}
#endif
#endif /* CQLREC_H */
