// Training-step driver (a8): enqueues the whole CQL step from C++, no host sync, no allocation.  Top to bottom: schedule
// marks, step workspace, `Step` (what every part of a step needs, built once per (ctx, step)), the parts, the phase entry
// points -- split so that a data-parallel caller can all-reduce ctx->grads (RCCL over xGMI) in between -- and
// cqlrec_train_steps, the pipelined single-rank loop.  The streams it all runs on come from step_streams.hip.
#include <math.h>
#include <stdlib.h>
#include <optional>
#include "adam_math.h"
#include "qhead_internal.h"
#include "step_streams.h"

#define CQL_TRY(expr)            \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ != CQLREC_OK) return rc__; \
  } while (0)
#define CQL_HIP_TRY(expr, what)                 \
  do {                                          \
    if ((expr) != hipSuccess) {                 \
      cql_set_error("%s: %s failed", what, #expr); \
      return CQLREC_ERR_HIP;                    \
    }                                           \
  } while (0)

// ---- schedule marks (tools/phase_timing.py): a handful of timing events at the joints of ONE step of a
// cqlrec_train_steps call -- cheap enough not to disturb the overlap they measure (unlike bracketing every kernel)
enum { MK_LOSS = 0, MK_DH, MK_DE, MK_CHAIN, MK_ADAM_IN, MK_ADAM_OUT, MK_PROLOGUE, MK_LSE, MK_NEXT_LOSS, MK_ENC_DX, MK_GATHER_BWD, MK_SORT_NEXT, MK_COUNT };
static hipEvent_t g_marks[MK_COUNT];
static int g_marks_on = 0;       // cqlrec_debug_marks_enable
static int g_mark_phase = 0;     // 1: backward of the marked step, 2: forward of the step after it
static void mark(int phase, int k, hipStream_t s) {
  if (g_marks_on && g_mark_phase == phase) (void)hipEventRecord(g_marks[k], s);
}
extern "C" int cqlrec_debug_marks_enable(int32_t on) {
  if (on && !g_marks[0])
    for (int i = 0; i < MK_COUNT; ++i)
      if (hipEventCreate(&g_marks[i]) != hipSuccess) return CQLREC_ERR_HIP;
  g_marks_on = on ? 1 : 0;
  return CQLREC_OK;
}
// ms of each mark relative to MK_LOSS (device must be idle: synchronises); order as the enum above
extern "C" int cqlrec_debug_marks_read(float* ms_out) {
  if (!g_marks[0] || !ms_out) return CQLREC_ERR_INVALID;
  for (int i = 0; i < MK_COUNT; ++i) {
    ms_out[i] = -1.f;
    if (hipEventSynchronize(g_marks[i]) != hipSuccess) continue;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_marks[MK_LOSS], g_marks[i]) == hipSuccess) ms_out[i] = ms;
  }
  return CQLREC_OK;
}

namespace {
// ---- the step workspace ----------------------------------------------------------------------------------------------------
struct Carve {
  char* base;
  int64_t off;
  explicit Carve(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(int64_t n) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += (n * (int64_t)sizeof(T) + 255) / 256 * 256;
    return p;
  }
  // two copies side by side, the step's own picked by its parity
  template <typename T>
  T* take_by_parity(int64_t n, uint64_t step) {
    T* even = take<T>(n);
    T* odd = take<T>(n);
    return (step & 1) ? odd : even;
  }
};

struct StepWs {
  int32_t *users, *tpos, *act, *a_star;
  float *rew, *done, *q_a, *lse, *nlse2, *nlse_nat, *q_targ, *y, *coef, *maxv, *loss, *term;
  float *h0_s, *dH, *dh0;
  uint16_t *h0b, *zb, *hb, *h0b_t, *zb_t, *hb_t;
  void *ws_q, *ws_q2, *ws_qb, *ws_qb2, *ws_enc, *ws_gb, *ws_oh;
  uint8_t* row_map;      // [n_items] which rows of g_E_in this step's window-gather backward writes (cqlrec_train_steps)
  uint8_t* read_map;     // [n_items] which rows of E_in this step's forward gathers (windows of s and of s')
  uint8_t* age;          // [n_items] steps each E_in row is behind inside a cqlrec_train_steps call (one copy, not by parity)
  int64_t ws_q_bytes, ws_qb_bytes, ws_qf_bytes, ws_enc_bytes, ws_gb_bytes, ws_oh_bytes;
  int64_t total;
};

// The per-step vectors and activations exist twice (parity = step & 1): cqlrec_train_steps starts the prologue of step
// t+1 (sample, gathers, encoder) while the item-side backward of step t still reads act / coef / nlse2 / hb of step t.
void carve_small(Carve& c, StepWs& w, int32_t B, int32_t d) {
  const int64_t Bd = (int64_t)B * d;      // (the sections in this order: tests/golden/train_ws_layout_known_answers.json)
  for (int32_t** p : {&w.users, &w.tpos, &w.act, &w.a_star}) *p = c.take<int32_t>(B);
  for (float** p : {&w.rew, &w.done, &w.q_a, &w.lse, &w.nlse2, &w.nlse_nat, &w.q_targ, &w.y, &w.coef, &w.maxv})
    *p = c.take<float>(B);
  w.loss = c.take<float>(64);
  w.term = c.take<float>(B);      // per-transition loss terms (cql_td_coef -> cql_td_loss_sum)
  for (float** p : {&w.h0_s, &w.dH, &w.dh0}) *p = c.take<float>(Bd);
  for (uint16_t** p : {&w.h0b, &w.zb, &w.hb}) *p = c.take<uint16_t>(2 * Bd);      // rows of s, then rows of s'
  for (uint16_t** p : {&w.h0b_t, &w.zb_t, &w.hb_t}) *p = c.take<uint16_t>(Bd);    // s' under the target network
}

StepWs carve_step(void* ws, int32_t B, int64_t N, int32_t d, int32_t L, uint64_t step) {
  StepWs w, other;
  Carve c(ws);
  carve_small(c, (step & 1) ? other : w, B, d);
  carve_small(c, (step & 1) ? w : other, B, d);
  w.ws_q_bytes = cqlrec_qhead_ws_bytes(B, N, d);
  w.ws_q = c.take<char>(w.ws_q_bytes);     // LSE partials (branch A)
  w.ws_q2 = c.take<char>(w.ws_q_bytes);    // ARGMAX partials (branch B runs concurrently)
  w.ws_qb_bytes = cqlrec_qhead_bwd_ws_bytes(B, N, d);
  w.ws_qf_bytes = w.ws_qb_bytes + w.ws_q_bytes;
  w.ws_qb = c.take<char>(w.ws_qf_bytes);    // fused forward of branch A: slabs of the soft part of dH + LSE partials
  w.ws_qb2 = c.take<char>(w.ws_qb_bytes);   // item-side backward: its own scratch, the two kernels run concurrently
  w.ws_enc_bytes = cqlrec_encoder_bwd_ws_bytes(B, d);
  w.ws_enc = c.take<char>(w.ws_enc_bytes);
  // sorted (item, state) pairs: by parity as well, the sort of step t+1 is issued while the gather backward of step t has
  // not run yet
  w.ws_gb_bytes = cqlrec_gather_pool_bwd_ws_bytes(B, L, d);
  w.ws_gb = c.take_by_parity<char>(w.ws_gb_bytes, step);
  w.ws_oh_bytes = cql_onehot_ws_bytes(B, d);
  w.ws_oh = c.take_by_parity<char>(w.ws_oh_bytes, step);   // sorted (action, transition) pairs of the one-hot scatter
  // by parity like the pairs it is built from: the map of step t+1 is made while the optimizer of step t has not read its
  // own yet; the read map of step t+1 is made while step t runs, too
  w.row_map = c.take_by_parity<uint8_t>(N, step);
  w.read_map = c.take_by_parity<uint8_t>(N, step);
  w.age = c.take<uint8_t>(N);
  w.total = c.off;
  return w;
}

int check_ctx(const cqlrec_train_ctx* c) {
  CQL_REQUIRE(c != nullptr, "train_step: ctx is NULL");
  CQL_REQUIRE(c->offsets && c->items && c->rewards, "train_step: CSR pointers are NULL");
  CQL_REQUIRE(c->theta && c->grads && c->adam_m && c->adam_v && c->target && c->theta_b && c->target_b,
              "train_step: model state pointers are NULL");
  CQL_REQUIRE(c->ws != nullptr, "train_step: workspace is NULL");
  CQL_REQUIRE(c->batch > 0 && c->window > 0 && c->world > 0 && c->rank >= 0 && c->rank < c->world,
              "train_step: batch=%d window=%d world=%d rank=%d", c->batch, c->window, c->world, c->rank);
  const int32_t d = c->layout.d;
  CQL_REQUIRE(cql_d_ok(d), "train_step: d=%d unsupported", d);
  CQL_REQUIRE(c->ws_bytes >= cqlrec_train_ws_bytes(c->batch, c->layout.n_items, d, c->window),
              "train_step: workspace too small");
  return CQLREC_OK;
}

// ---- one step of one context: what every part below works on, built once by the entry point --------------------------------
struct StepPtrs {
  const uint16_t *Ein_b, *Eout_b, *W1_b, *W2_b, *tEin_b, *tEout_b, *tW1_b, *tW2_b;
  const float *b_out, *b1, *b2, *tb_out, *tb1, *tb2;
};
StepPtrs step_ptrs(const cqlrec_train_ctx* c) {
  const cqlrec_layout& L = c->layout;
  StepPtrs p;
  p.Ein_b = c->theta_b + L.off_E_in;   p.Eout_b = c->theta_b + L.off_E_out;
  p.W1_b = c->theta_b + L.off_W1;      p.W2_b = c->theta_b + L.off_W2;
  p.b_out = c->theta + L.off_b_out;    p.b1 = c->theta + L.off_b1;   p.b2 = c->theta + L.off_b2;
  p.tEin_b = c->target_b + L.off_E_in; p.tEout_b = c->target_b + L.off_E_out;
  p.tW1_b = c->target_b + L.off_W1;    p.tW2_b = c->target_b + L.off_W2;
  p.tb_out = c->target + L.off_b_out;  p.tb1 = c->target + L.off_b1; p.tb2 = c->target + L.off_b2;
  return p;
}
struct Step {
  const cqlrec_train_ctx* c;      // (checked: check_ctx)
  uint64_t step;
  const cqlrec_layout& L;
  int32_t B, d, W;
  int64_t N;
  StepWs w;                       // this step's sections of c->ws
  StepPtrs p;
  float alpha_scale;              // alpha / (global batch), formed in double and rounded once (the oracle's np.float32(alpha / Bg))
  Step(const cqlrec_train_ctx* ctx, uint64_t t)
      : c(ctx), step(t), L(ctx->layout), B(ctx->batch), d(L.d), W(ctx->window), N(L.n_items),
        w(carve_step(ctx->ws, B, N, d, W, t)), p(step_ptrs(ctx)),
        alpha_scale((float)(ctx->alpha / ((double)ctx->batch * (double)ctx->world))) {}
  float* g_E_out() const { return c->grads + L.off_E_out; }
  float* g_b_out() const { return c->grads + L.off_b_out; }
  float inv_batch() const { return 1.0f / ((float)B * (float)c->world); }
};

// ---- forward ---------------------------------------------------------------------------------------------------------------
// transitions of this rank's slots of the global step (they depend on (seed, step) only)
int sample(const Step& st, hipStream_t s) {
  const cqlrec_train_ctx* c = st.c;
  const StepWs& w = st.w;
  return cqlrec_sample_transitions(c->offsets, c->items, c->rewards, c->n_users, c->seed, st.step,
                                   (uint64_t)c->rank * (uint64_t)st.B, st.B, w.users, w.tpos, w.act, w.rew, w.done, s);
}
// the sorted pairs the backward of the step needs, from its sampled batch alone: the (item, state) pairs of the window
// gather -- with_row_map: and the step's row map from them -- and the (action, transition) pairs of the one-hot scatter
int prepare_pairs(const Step& st, hipStream_t s, bool with_row_map) {
  const cqlrec_train_ctx* c = st.c;
  const StepWs& w = st.w;
  CQL_TRY(cqlrec_gather_pool_bwd_prepare(c->offsets, c->items, w.users, w.tpos, 0, st.B, st.W, st.d, st.N, w.ws_gb,
                                         w.ws_gb_bytes, s));
  if (with_row_map) CQL_TRY(cql_gather_pool_bwd_mark_rows(w.ws_gb, st.B, st.W, st.d, st.N, w.row_map, s));
  return cql_onehot_prepare(w.act, st.B, st.N, st.d, w.ws_oh, w.ws_oh_bytes, s);
}
// the step's sample and pairs ahead of its forward (cqlrec_train_steps, during the backward of the step before).
// `sampled_ev`: recorded behind the transitions.  `read_map_ev`: recorded behind the step's read map, which needs users /
// tpos only and so sits in front of the pair sorts.  The caller records ss.sorted[step & 1] behind the call.
int sample_ahead(const Step& st, hipStream_t s, hipEvent_t sampled_ev, hipEvent_t read_map_ev) {
  CQL_TRY(sample(st, s));
  CQL_HIP_TRY(hipEventRecord(sampled_ev, s), "train_steps");
  CQL_TRY(cql_mark_read_rows(st.c->offsets, st.c->items, st.w.users, st.w.tpos, st.B, st.W, st.N, st.w.read_map, s));
  CQL_HIP_TRY(hipEventRecord(read_map_ev, s), "train_steps");
  return prepare_pairs(st, s, true);
}

// the loss VALUE of the step from the terms its forward left (nothing in the step waits for it)
int loss_sum_impl(const Step& st, float* loss_out, hipStream_t on) {
  return cql_td_loss_sum(st.w.term, st.B, st.inv_batch(), loss_out ? loss_out : st.w.loss, on);
}
int backward_items_long_impl(const Step& st, hipStream_t s, CqlAdamFix* fix);

struct FwdOpts {
  // event after which the item-side parameters (E_out, b_out and their shadows) are up to date -- everything before the
  // Q-head kernels (sample, window gathers, encoder) reads only E_in / W1 / W2 and may start earlier
  hipEvent_t eout_ready = nullptr;
  // event after which this step's transitions are already in place (sample_ahead); the sorted pairs the backward needs
  // follow under ss.sorted[step & 1]
  hipEvent_t presampled = nullptr;
  // early_items (a stream) + early_fix: the long item-side kernel of THIS step is launched on that stream as soon as the
  // fused forward has produced -lse (it needs nothing from the loss), see backward_items_impl
  hipStream_t early_items = nullptr;
  CqlAdamFix* early_fix = nullptr;
  bool* loss_sum_deferred = nullptr;   // != NULL: the loss terms are left for the caller's loss_sum_impl (on a stream that has slack)
  bool want_row_map = false;   // the side-stream sort of a step that was not sampled ahead also fills the step's row map
};

// sample + forward + loss (+ the sorts for the backward, forked onto the item-side stream)
int forward_impl(const Step& st, float* loss_out, hipStream_t s, const FwdOpts& o) {
  const cqlrec_train_ctx* c = st.c;
  const StepWs& w = st.w;
  const StepPtrs& p = st.p;
  const int32_t B = st.B, d = st.d, W = st.W;
  const int64_t N = st.N, Bd = (int64_t)B * d;

  SideStream& ss = side_stream();
  if (o.presampled) {
    CQL_HIP_TRY(hipStreamWaitEvent(s, o.presampled, 0), "train_step_forward");
  } else {
    CQL_TRY(sample(st, s));
    if (ss.ok && (hipEventRecord(ss.forked, s) != hipSuccess || hipStreamWaitEvent(ss.st_items, ss.forked, 0) != hipSuccess))
      ss.ok = false;
    if (ss.ok) {
      CQL_TRY(prepare_pairs(st, ss.st_items, o.want_row_map));
      CQL_HIP_TRY(hipEventRecord(ss.sorted[st.step & 1], ss.st_items), "train_step_forward");
    } else {
      CQL_TRY(prepare_pairs(st, s, false));
    }
  }
  // The forward has two independent branches that meet at the TD target:
  //   A (this stream):    s  under theta  -> encoder -> logsumexp over the catalogue, Q(s, a)
  //   B (branch stream):  s' under theta  -> encoder -> argmax;  s' under the target net -> encoder -> Q_target(s', a*)
  // Run concurrently, the small gather / encoder / finalize launches of one branch fill the launch gaps of the other.
  const bool par = ss.ok && hipEventRecord(ss.fork2, s) == hipSuccess && hipStreamWaitEvent(ss.st_branch, ss.fork2, 0) == hipSuccess;
  hipStream_t sb = par ? ss.st_branch : s;
  // ---- branch A
  CQL_TRY(cqlrec_gather_pool_fwd(p.Ein_b, c->offsets, c->items, w.users, w.tpos, 0, B, W, d, w.h0_s, w.h0b, nullptr, s));
  CQL_TRY(cqlrec_encoder_fwd(w.h0b, p.W1_b, p.b1, p.W2_b, p.b2, B, d, w.zb, w.hb, s));
  mark(2, MK_PROLOGUE, s);
  CQL_TRY(cql_qhead_fwd_lse_dh_prepare(w.ws_qb, B, N, d, s));      // (a 4-byte memset: in front of the wait, not behind it)
  if (o.eout_ready) CQL_HIP_TRY(hipStreamWaitEvent(s, o.eout_ready, 0), "train_step_forward");
  // logsumexp AND the softmax-weighted sum of item rows (the soft part of dH) in ONE pass over the catalogue
  CQL_TRY(cql_qhead_fwd_lse_dh(w.hb, B, p.Eout_b, p.b_out, N, d, w.ws_qb, w.ws_qf_bytes, w.lse, w.nlse2, s, w.nlse_nat, 1));
  mark(2, MK_LSE, s);
  if (o.early_items) {
    CQL_HIP_TRY(hipEventRecord(ss.fwd_done, s), "train_step_forward");
    CQL_HIP_TRY(hipStreamWaitEvent(o.early_items, ss.fwd_done, 0), "train_step_forward");
    CQL_TRY(backward_items_long_impl(st, o.early_items, o.early_fix));
  }
  // the part of dH that needs nothing from the loss, off the chain the next prologue waits for
  CQL_TRY(cql_qhead_dh_finish(w.ws_qb, B, N, d, w.lse, nullptr, w.act, p.Eout_b, st.alpha_scale, w.dH, s, 1));
  CQL_TRY(cqlrec_gather_dot(w.hb, p.Eout_b, p.b_out, w.act, B, d, w.q_a, s));
  // ---- branch B
  CQL_TRY(cqlrec_gather_pool_fwd(p.Ein_b, c->offsets, c->items, w.users, w.tpos, 1, B, W, d, nullptr, w.h0b + Bd, nullptr, sb));
  CQL_TRY(cqlrec_gather_pool_fwd(p.tEin_b, c->offsets, c->items, w.users, w.tpos, 1, B, W, d, nullptr, w.h0b_t, nullptr, sb));
  CQL_TRY(cqlrec_encoder_fwd(w.h0b + Bd, p.W1_b, p.b1, p.W2_b, p.b2, B, d, w.zb + Bd, w.hb + Bd, sb));
  CQL_TRY(cqlrec_encoder_fwd(w.h0b_t, p.tW1_b, p.tb1, p.tW2_b, p.tb2, B, d, w.zb_t, w.hb_t, sb));
  if (o.eout_ready && par) CQL_HIP_TRY(hipStreamWaitEvent(ss.st_branch, o.eout_ready, 0), "train_step_forward");
  CQL_TRY(cql_qhead_argmax_step(w.hb + Bd, B, p.Eout_b, p.b_out, N, d, w.ws_q2, w.ws_q_bytes, w.maxv, w.a_star, sb));
  CQL_TRY(cqlrec_gather_dot(w.hb_t, p.tEout_b, p.tb_out, w.a_star, B, d, w.q_targ, sb));
  if (par && (hipEventRecord(ss.join2, ss.st_branch) != hipSuccess || hipStreamWaitEvent(s, ss.join2, 0) != hipSuccess)) {
    cql_set_error("train_step_forward: joining the forward branches failed");
    return CQLREC_ERR_HIP;
  }
  // loss + dQ coefficients
  CQL_TRY(cql_td_coef(w.q_a, w.lse, w.q_targ, w.rew, w.done, B, (float)c->gamma, (float)c->alpha, st.inv_batch(), w.coef, w.y,
                      w.term, s));
  if (o.loss_sum_deferred) *o.loss_sum_deferred = true;
  else CQL_TRY(loss_sum_impl(st, loss_out, s));
  mark(2, MK_NEXT_LOSS, s);
  return CQLREC_OK;
}

// ---- item-side backward ----------------------------------------------------------------------------------------------------
// ctx->grads is zero on entry (contract of the step).  Three parts, the sum of a gradient row formed in ONE order on every
// path (pipelined, phased, strict) so that they stay bit-identical:
//   row = ((scale * dE piece holding stage 0) + one-hot part) + scale * cut pieces, in block order
// (1) the long kernel WRITES its rows (nothing to read, nothing to wait for but the forward's -lse: the pipelined driver
//     launches it as soon as the fused forward has finished, under the rest of the forward and the loss),
// (2) the one-hot part -- the only part that needs the loss's coefficients -- is added as a segmented sum,
// (3) the cut pieces: fix-up launch here, or left to the item-side optimizer (CqlAdamFix).
int backward_items_long_impl(const Step& st, hipStream_t s, CqlAdamFix* fix) {
  const StepWs& w = st.w;
  return cql_qhead_bwd_items_long(w.hb, w.nlse2, w.coef, w.act, st.B, st.p.Eout_b, st.p.b_out, st.N, st.d, st.alpha_scale,
                                  w.ws_qb2, w.ws_qb_bytes, st.g_E_out(), st.g_b_out(), s, fix, w.nlse_nat);
}
int backward_items_onehot_impl(const Step& st, hipStream_t s) {
  SideStream& ss = side_stream();
  // the (action, transition) pairs were sorted ahead of time on another stream (same event as the window pairs)
  if (ss.ok) CQL_HIP_TRY(hipStreamWaitEvent(s, ss.sorted[st.step & 1], 0), "train_step_backward_items");
  return cql_onehot_apply(st.w.coef, st.w.hb, st.B, st.N, st.d, st.w.ws_oh, st.g_E_out(), st.g_b_out(), s, 1);
}
// all three in program order; defer != NULL: leave (3) to the caller's optimizer launch
int backward_items_impl(const Step& st, hipStream_t s, CqlAdamFix* defer) {
  CqlAdamFix fix = {};
  CQL_TRY(backward_items_long_impl(st, s, &fix));
  CQL_TRY(backward_items_onehot_impl(st, s));
  if (defer) *defer = fix;
  else CQL_TRY(cql_qde_fixup_deferred(fix, st.g_E_out(), st.g_b_out(), s));
  return CQLREC_OK;
}

// ---- state-side backward ---------------------------------------------------------------------------------------------------
// records `dh` behind dh_finish, the last reader of the E_out shadow on this stream: the item-side Adam waits for it
int backward_states_impl(const Step& st, hipStream_t s) {
  const StepWs& w = st.w;
  // the catalogue pass was done by the forward: only the slabs are combined here (scale, exp(m - lse), + coef * E[a])
  // (the soft part was formed by the forward, right behind the catalogue pass: here only the term that needs the loss)
  CQL_TRY(cql_qhead_dh_finish(w.ws_qb, st.B, st.N, st.d, w.lse, w.coef, w.act, st.p.Eout_b, st.alpha_scale, w.dH, s, 2));
  SideStream& ss = side_stream();
  if (ss.ok) CQL_HIP_TRY(hipEventRecord(ss.dh, s), "train_step_backward_rest");
  return CQLREC_OK;
}

// the chain behind dH: encoder backward, window-gather backward
int backward_chain_impl(const Step& st, hipStream_t s) {
  const StepWs& w = st.w;
  const StepPtrs& p = st.p;
  const cqlrec_layout& L = st.L;
  float* g = st.c->grads;
  // The window-gather backward needs dh0 only: the weight / bias gradients of the encoder (two launches reading dA1) go
  // to the branch stream, idle in the backward, and join before this function returns.
  SideStream& ss = side_stream();
  const bool split = ss.ok && ss.st_branch && ss.st_branch != s;
  CQL_TRY(cql_encoder_bwd_parts(w.dH, w.zb, w.h0b, p.W1_b, p.W2_b, st.B, st.d, w.ws_enc, w.ws_enc_bytes, g + L.off_W1,
                                g + L.off_b1, g + L.off_W2, g + L.off_b2, w.dh0, split ? 1 : 3, s));
  if (split) {
    CQL_HIP_TRY(hipEventRecord(ss.fork2, s), "train_step_backward_rest");
    CQL_HIP_TRY(hipStreamWaitEvent(ss.st_branch, ss.fork2, 0), "train_step_backward_rest");
    CQL_TRY(cql_encoder_bwd_parts(w.dH, w.zb, w.h0b, p.W1_b, p.W2_b, st.B, st.d, w.ws_enc, w.ws_enc_bytes, g + L.off_W1,
                                  g + L.off_b1, g + L.off_W2, g + L.off_b2, w.dh0, 2, ss.st_branch));
    CQL_HIP_TRY(hipEventRecord(ss.join2, ss.st_branch), "train_step_backward_rest");
  }
  mark(1, MK_ENC_DX, s);
  if (ss.ok) CQL_HIP_TRY(hipStreamWaitEvent(s, ss.sorted[st.step & 1], 0), "train_step_backward_rest");
  CQL_TRY(cqlrec_gather_pool_bwd_apply(w.dh0, st.B, st.W, st.d, st.N, w.ws_gb, w.ws_gb_bytes, g + L.off_E_in, s));
  mark(1, MK_GATHER_BWD, s);
  if (split) CQL_HIP_TRY(hipStreamWaitEvent(s, ss.join2, 0), "train_step_backward_rest");
  return CQLREC_OK;
}

int backward_rest_impl(const Step& st, hipStream_t s) {
  CQL_TRY(backward_states_impl(st, s));
  return backward_chain_impl(st, s);
}

// ---- optimizer -------------------------------------------------------------------------------------------------------------
// the two per-step scalars of the optimizer, formed in double and rounded once: these float values are normative
void adam_step_scalars(const cqlrec_train_ctx* c, uint64_t step, float* step_size, float* sqrt_bc2) {
  const double t = (double)(step + 1);
  const double bc1 = 1.0 - pow((double)c->beta1, t);
  const double bc2 = 1.0 - pow((double)c->beta2, t);
  *step_size = (float)((double)c->lr / bc1);
  *sqrt_bc2 = (float)sqrt(bc2);
}
// Adam + target + shadows (+ zero grads) over elements [lo, hi) of the flat buffers (multiples of 4); it reads no workspace,
// so it takes the ctx and not a Step
int update_range_impl(const cqlrec_train_ctx* c, uint64_t step, int64_t lo, int64_t hi, hipStream_t s, const CqlAdamFix* fix,
                      int zero_grads) {
  CQL_REQUIRE(lo >= 0 && hi <= c->layout.total && lo < hi && lo % 4 == 0 && hi % 4 == 0,
              "train_step_update_range: bad range [%lld, %lld)", (long long)lo, (long long)hi);
  float step_size, sqrt_bc2;
  adam_step_scalars(c, step, &step_size, &sqrt_bc2);
  return cql_adam_ema_fix(c->theta + lo, c->grads + lo, c->adam_m + lo, c->adam_v + lo, c->target + lo, c->theta_b + lo,
                          c->target_b + lo, hi - lo, step_size, sqrt_bc2, (float)c->beta1, (float)c->beta2, (float)c->eps,
                          (float)c->tau, zero_grads, fix, s);
}

// ---- early launches of the long item-side kernel (cqlrec_train_step_forward_early_items) that still wait for their
// backward_items call.  A record is identified by what identifies the step's data -- workspace, gradient buffer, step and
// the stream the kernel went to -- never by the host address of the ctx struct (callers copy that struct).  Per device slot
// a small table: two contexts at both parities.  A record that is missing (dropped, or pushed out by a fifth one) only costs
// the fast path: backward_items then runs all three parts, and the long kernel stores every row (accumulate = 0) before the
// one-hot part, so whatever an earlier launch of it left is overwritten.
struct EarlyItems {
  bool live = false;
  const void* ws = nullptr;
  const float* grads = nullptr;
  uint64_t step = 0;
  hipStream_t items_stream = nullptr;
  CqlAdamFix fix = {};
};
constexpr int EARLY_SLOTS = 4;
EarlyItems g_early[CQL_MAX_DEVICES][EARLY_SLOTS];
int g_early_next[CQL_MAX_DEVICES] = {};

// a new forward of this workspace at this parity overwrites the step vectors the recorded launch belongs to
void early_drop(const cqlrec_train_ctx* c, uint64_t step) {
  for (EarlyItems& e : g_early[cql_device_slot()])
    if (e.live && e.ws == c->ws && ((e.step ^ step) & 1) == 0) e.live = false;
}
EarlyItems* early_find(const cqlrec_train_ctx* c, uint64_t step) {
  for (EarlyItems& e : g_early[cql_device_slot()])
    if (e.live && e.ws == c->ws && e.grads == c->grads && e.step == step) return &e;
  return nullptr;
}
EarlyItems& early_take_slot() {
  const int dev = cql_device_slot();
  for (EarlyItems& e : g_early[dev])
    if (!e.live) return e;
  EarlyItems& e = g_early[dev][g_early_next[dev]];      // full: the oldest goes (its step falls back to the full form)
  g_early_next[dev] = (g_early_next[dev] + 1) % EARLY_SLOTS;
  return e;
}

// phase 1: sample + forward + loss (+ the sorts for the backward, forked onto the item-side stream), the Q-head kernels
// behind `items_ready` (may be NULL).  With an `items_stream` of its own (and the side streams up) also the long kernel of
// phase 2 (see the header): the cut pieces of that kernel wait, in the record above, for the backward_items call of the step.
int forward_entry(const cqlrec_train_ctx* c, uint64_t step, float* loss_out, cqlrec_stream stream, void* items_ready,
                  cqlrec_stream items_stream) {
  CQL_TRY(check_ctx(c));
  const bool early = items_stream && items_stream != stream && side_stream().ok;
  early_drop(c, step);
  CqlAdamFix fix = {};
  FwdOpts o;
  o.eout_ready = (hipEvent_t)items_ready;
  o.early_items = early ? (hipStream_t)items_stream : nullptr;
  o.early_fix = &fix;
  CQL_TRY(forward_impl(Step(c, step), loss_out, (hipStream_t)stream, o));
  if (early) early_take_slot() = EarlyItems{true, c->ws, c->grads, step, (hipStream_t)items_stream, fix};
  return CQLREC_OK;
}
}  // namespace

extern "C" int cqlrec_train_step_forward(const cqlrec_train_ctx* c, uint64_t step, float* loss_out,
                                         cqlrec_stream stream) {
  return forward_entry(c, step, loss_out, stream, nullptr, nullptr);
}
extern "C" int cqlrec_train_step_forward_after(const cqlrec_train_ctx* c, uint64_t step, float* loss_out,
                                               cqlrec_stream stream, void* items_ready) {
  return forward_entry(c, step, loss_out, stream, items_ready, nullptr);
}
extern "C" int cqlrec_train_step_forward_early_items(const cqlrec_train_ctx* c, uint64_t step, float* loss_out,
                                                     cqlrec_stream stream, void* items_ready, cqlrec_stream items_stream) {
  return forward_entry(c, step, loss_out, stream, items_ready, items_stream);
}

// phase 2: the catalogue-side gradients g_E_out, g_b_out (half of the gradient bytes; a data-parallel caller starts
// their all-reduce while phase 3 runs)
extern "C" int cqlrec_train_step_backward_items(const cqlrec_train_ctx* c, uint64_t step, cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  hipStream_t s = (hipStream_t)stream;
  const Step st(c, step);
  if (EarlyItems* e = early_find(c, step)) {
    // the long kernel is running (or done) on e->items_stream; on any other stream the parts below would race with it
    CQL_REQUIRE(s == e->items_stream,
                "train_step_backward_items: step %llu was started by forward_early_items; call it on that call's "
                "item-side stream (items_stream)", (unsigned long long)step);
    const CqlAdamFix fix = e->fix;
    e->live = false;
    CQL_TRY(backward_items_onehot_impl(st, s));      // one-hot rows, then the cut pieces
    return cql_qde_fixup_deferred(fix, st.g_E_out(), st.g_b_out(), s);
  }
  return backward_items_impl(st, s, nullptr);
}

// phase 3: dH, encoder backward, window-gather backward (joins the side stream)
extern "C" int cqlrec_train_step_backward_rest(const cqlrec_train_ctx* c, uint64_t step, cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  return backward_rest_impl(Step(c, step), (hipStream_t)stream);
}

extern "C" int cqlrec_train_step_fwd_bwd(const cqlrec_train_ctx* c, uint64_t step, float* loss_out,
                                         cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  early_drop(c, step);
  const Step st(c, step);
  hipStream_t s = (hipStream_t)stream;
  CQL_TRY(forward_impl(st, loss_out, s, FwdOpts()));
  // The item-side backward (one long MFMA-bound kernel) runs on its own stream UNDER the state-side chain (dh_finish,
  // encoder and window-gather backward: latency / HBM bound).  Fork after the loss, join before returning.
  SideStream& ss = side_stream();
  if (ss.ok && hipEventRecord(ss.loss, s) == hipSuccess && hipStreamWaitEvent(ss.st_items, ss.loss, 0) == hipSuccess) {
    CQL_TRY(backward_items_impl(st, ss.st_items, nullptr));
    CQL_HIP_TRY(hipEventRecord(ss.items_done, ss.st_items), "train_step_fwd_bwd");
    CQL_TRY(backward_rest_impl(st, s));
    CQL_HIP_TRY(hipStreamWaitEvent(s, ss.items_done, 0), "train_step_fwd_bwd");
    return CQLREC_OK;
  }
  CQL_TRY(backward_rest_impl(st, s));
  return backward_items_impl(st, s, nullptr);
}

extern "C" int cqlrec_train_step_update_range(const cqlrec_train_ctx* c, uint64_t step, int64_t lo, int64_t hi,
                                              cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  return update_range_impl(c, step, lo, hi, (hipStream_t)stream, nullptr, 1);
}

extern "C" int cqlrec_train_step_update(const cqlrec_train_ctx* c, uint64_t step, cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  return update_range_impl(c, step, 0, c->layout.total, (hipStream_t)stream, nullptr, 1);
}

// ---- cqlrec_train_steps ----------------------------------------------------------------------------------------------------
// n_steps whole steps (sample .. Adam) of a single-rank job, software-pipelined across the two halves of the model:
//   * item-side stream: item-side backward (dE_out, db_out) of step t, then Adam on the E_out/b_out range;
//   * main stream: state-side backward (dH, encoder, window gather) of step t, then Adam on E_in + encoder -- HBM-bound,
//     it runs under the MFMA-bound item-side kernel -- then ALREADY the prologue of step t+1 (sample, window gathers,
//     encoder: they read only E_in / W), which waits for the item-side Adam only in front of its Q-head kernels;
//   * sample-ahead stream: the sample and the pair sorts of step t+1.
// Same dataflow as fwd_bwd + update per step; joined before returning.  world must be 1 (no all-reduce in here).
//
// Steps that have a successor in the same call leave the gradient buffer as it is instead of zeroing it ("lean"):
//   * [off_E_out, off_W1): the next writer is the long item-side kernel of step t+1, which stores every row of g_E_out and
//     every element of g_b_out (qde_kernel, qde2_kernel, qde3_kernel: store_piece of the piece holding stage 0, plain
//     stores with accumulate = 0, in either placement of that kernel); the one-hot part and the cut pieces go on top.
//   * E_in: the window-gather backward writes only the rows of the batch, so the step's row map (built with the sorted
//     pairs, by parity) tells the optimizer which rows to read; the others take g = 0 unread and whatever an earlier step
//     left in them is dead.
// The last step of a call runs the zeroing forms (E_in still through its map, so that stale rows count as zero and are
// cleared), which leaves ctx->grads all zeros as the phase entry points expect.  A single-step call runs the full forms only.
//
// The E_in launch is also deferred per row (adam.hip, adam_ema_rows_deferred_kernel): a row without a gradient that the
// NEXT step's forward does not gather is left behind and only its age (workspace, zero when a call starts) moves on; the
// launch that needs it replays the missed steps.  The next step's read map comes from sample_ahead under an event of its
// own; a step whose successor was not sampled ahead, and the last step of a call, bring every row up to date, so the
// caller finds all six buffers complete.  After an error return from the middle of a call E_in may be behind (cqlrec.h).
namespace {
// what one step of a call hands to the next
struct Carry {
  hipEvent_t pending = nullptr;   // item-side Adam of the previous step
  hipEvent_t sampled = nullptr;   // transitions + sorted pairs of this step, prepared during the previous backward
  bool grads_dirty = false;       // a lean step has run: the gradient buffer holds dead data until the last step clears it
  CqlAdamSteps adam_tab = {};     // (step_size, sqrt_bc2) of the steps of this call, slot = step % CQL_ADAM_DEFER_CAP
};

// everything of step `st` behind its loss (ss.loss is recorded on s), on the side streams.  next: the step after it in this
// call (NULL: none); use_map: E_in goes through the row map and per-row deferral; early: the long item-side kernel was
// launched by the forward, `fix` holds its cut pieces; sum_deferred: the forward left the loss value to us.
int pipelined_step(const Step& st, const Step* next, float* loss_out, hipStream_t s, bool use_map, bool early, CqlAdamFix fix,
                   bool sum_deferred, Carry& k) {
  const cqlrec_train_ctx* c = st.c;
  const cqlrec_layout& L = st.L;
  SideStream& ss = side_stream();
  const bool lean = use_map && next;
  if (next && hipStreamWaitEvent(ss.st_ahead, ss.loss, 0) == hipSuccess) {
    // the sum of the loss terms goes to the head of the sample-ahead stream (it has slack)
    if (sum_deferred) {
      CQL_TRY(loss_sum_impl(st, loss_out, ss.st_ahead));
      sum_deferred = false;
    }
    // the next step's transitions depend on (seed, step) only: sample them now, on a stream of their own, and sort
    // the pairs its backward will need (two radix sorts, ~35 small launches) behind that
    CQL_TRY(sample_ahead(*next, ss.st_ahead, ss.presample, ss.read_map));
    CQL_HIP_TRY(hipEventRecord(ss.sorted[next->step & 1], ss.st_ahead), "train_steps");
    mark(1, MK_SORT_NEXT, ss.st_ahead);
    k.sampled = ss.presample;
  }
  if (sum_deferred) CQL_TRY(loss_sum_impl(st, loss_out, s));      // (the sample-ahead stream could not take it)
  CQL_HIP_TRY(hipStreamWaitEvent(ss.st_items, ss.loss, 0), "train_steps");
  // the long dE_out kernel, then the one-hot part; the sum of its cut pieces is left to the item-side Adam below
  if (early)            // the long kernel is running (or done) already: the one-hot part on top
    CQL_TRY(backward_items_onehot_impl(st, ss.st_items));
  else
    CQL_TRY(backward_items_impl(st, ss.st_items, &fix));
  mark(1, MK_DE, ss.st_items);
  CQL_TRY(backward_states_impl(st, s));                      // dh_finish, records ss.dh
  mark(1, MK_DH, s);
  CQL_TRY(backward_chain_impl(st, s));                       // encoder, window gather
  mark(1, MK_CHAIN, s);
  CQL_TRY(update_range_impl(c, st.step, L.off_W1, L.total, s, nullptr, 1));
  if (use_map) {
    const int slot = (int)(st.step % CQL_ADAM_DEFER_CAP);
    adam_step_scalars(c, st.step, &k.adam_tab.step_size[slot], &k.adam_tab.sqrt_bc2[slot]);
    const uint8_t* read_next = nullptr;      // NULL: bring every row up to date
    if (lean && k.sampled) {
      CQL_HIP_TRY(hipStreamWaitEvent(s, ss.read_map, 0), "train_steps");
      read_next = next->w.read_map;
    }
    CQL_TRY(cql_adam_ema_rows_deferred(c->theta, c->grads, c->adam_m, c->adam_v, c->target, c->theta_b, c->target_b,
                                       L.off_E_out, k.adam_tab, st.step, (float)c->beta1, (float)c->beta2, (float)c->eps,
                                       (float)c->tau, lean ? 0 : 1, st.w.row_map, read_next, st.w.age, L.d, L.n_items, s));
  } else {
    CQL_TRY(update_range_impl(c, st.step, 0, L.off_E_out, s, nullptr, 1));
  }
  mark(1, MK_ADAM_IN, s);
  // The two Adam launches are HBM-bound and run side by side: serialising them, state side first so that the next
  // prologue runs under the item-side Adam, was measured no faster (0.802 vs 0.796 ms per step at cfg3).
  CQL_HIP_TRY(hipStreamWaitEvent(ss.st_items, ss.dh, 0), "train_steps");     // dh_finish reads the E_out shadow
  fix.rows_off = 0;
  fix.cs_off = L.off_b_out - L.off_E_out;
  CQL_TRY(update_range_impl(c, st.step, L.off_E_out, L.off_W1, ss.st_items, &fix, lean ? 0 : 1));
  k.grads_dirty = lean;
  CQL_HIP_TRY(hipEventRecord(ss.eout, ss.st_items), "train_steps");
  mark(1, MK_ADAM_OUT, ss.st_items);
  k.pending = ss.eout;
  return CQLREC_OK;
}

// the same step behind its loss without side streams: everything on s, the full (zeroing) forms
int serial_step(const Step& st, float* loss_out, hipStream_t s, bool sum_deferred, const Carry& k) {
  // (the serial form needs a zeroed gradient buffer; the side streams do not go away in the middle of a call)
  CQL_REQUIRE(!k.grads_dirty, "train_steps: lost the side streams in the middle of a call");
  if (sum_deferred) CQL_TRY(loss_sum_impl(st, loss_out, s));
  CQL_TRY(backward_rest_impl(st, s));
  CQL_TRY(backward_items_impl(st, s, nullptr));
  return update_range_impl(st.c, st.step, 0, st.L.total, s, nullptr, 1);
}
}  // namespace

extern "C" int cqlrec_train_steps(const cqlrec_train_ctx* c, uint64_t step0, int32_t n_steps, float* loss_out,
                                  cqlrec_stream stream) {
  CQL_TRY(check_ctx(c));
  CQL_REQUIRE(n_steps >= 0, "train_steps: n_steps=%d", n_steps);
  CQL_REQUIRE(c->world == 1, "train_steps: world=%d; data-parallel callers use the phase entry points", c->world);
  // CQL_EARLY_DE=0: the long item-side kernel behind the loss (A/B knob); default: behind the fused forward
  static const int early_de = !(getenv("CQL_EARLY_DE") && getenv("CQL_EARLY_DE")[0] == '0');
  hipStream_t s = (hipStream_t)stream;
  SideStream& ss = side_stream();
  for (int32_t i = 0; i < n_steps && i < 2; ++i) early_drop(c, step0 + (uint64_t)i);      // (the parities this call overwrites)
  const bool use_map = n_steps > 1 && c->layout.off_E_in == 0;
  std::optional<Step> by_parity[2];      // this step and the one sampled ahead: each carved once
  if (n_steps > 0) by_parity[step0 & 1].emplace(c, step0);
  if (use_map)                    // every E_in row is up to date when a call starts
    CQL_HIP_TRY(hipMemsetAsync(by_parity[step0 & 1]->w.age, 0, (size_t)c->layout.n_items, s), "train_steps");
  Carry k;
  for (int32_t i = 0; i < n_steps; ++i) {
    const uint64_t step = step0 + (uint64_t)i;
    const Step& st = *by_parity[step & 1];
    const Step* next = i + 1 < n_steps ? &by_parity[(step + 1) & 1].emplace(c, step + 1) : nullptr;
    float* loss_i = loss_out ? loss_out + i : nullptr;
    const bool early = early_de && ss.ok && ss.st_items;
    CqlAdamFix fix = {};
    bool sum_deferred = false;
    FwdOpts o;
    o.eout_ready = k.pending;
    o.presampled = k.sampled;
    o.early_items = early ? ss.st_items : nullptr;
    o.early_fix = &fix;
    // the sum of the loss terms goes to the sample-ahead stream when that stream is used
    o.loss_sum_deferred = (ss.ok && ss.st_ahead && next) ? &sum_deferred : nullptr;
    o.want_row_map = use_map;
    CQL_TRY(forward_impl(st, loss_i, s, o));
    k.pending = k.sampled = nullptr;
    if (g_marks_on && n_steps >= 4) {   // marks: backward of step n/2 (phase 1), forward of step n/2 + 1 (phase 2)
      if (i == n_steps / 2) g_mark_phase = 1;
      else if (i == n_steps / 2 + 1) g_mark_phase = 0;
    }
    mark(1, MK_LOSS, s);
    if (ss.ok && hipEventRecord(ss.loss, s) == hipSuccess) {
      CQL_TRY(pipelined_step(st, next, loss_i, s, use_map, early, fix, sum_deferred, k));
      if (g_mark_phase == 1) g_mark_phase = 2;
    } else {
      CQL_TRY(serial_step(st, loss_i, s, sum_deferred, k));
    }
  }
  g_mark_phase = 0;
  if (k.pending) CQL_HIP_TRY(hipStreamWaitEvent(s, k.pending, 0), "train_steps");
  return CQLREC_OK;
}

// ---- workspace queries (host only) -----------------------------------------------------------------------------------------
extern "C" int64_t cqlrec_train_ws_bytes(int32_t batch, int64_t n_items, int32_t d, int32_t window) {
  return carve_step(nullptr, batch, n_items, d, window, 0).total + 256;
}
extern "C" int cqlrec_train_views_get(const cqlrec_train_ctx* c, uint64_t step, cqlrec_train_views* out) {
  CQL_TRY(check_ctx(c));
  CQL_REQUIRE(out != nullptr, "train_views_get: out is NULL");
  const Step st(c, step);
  const StepWs& w = st.w;
  out->users = w.users; out->tpos = w.tpos; out->act = w.act; out->a_star = w.a_star;
  out->rew = w.rew; out->done = w.done; out->q_a = w.q_a; out->lse = w.lse; out->q_targ = w.q_targ;
  out->y = w.y; out->coef = w.coef; out->dH = w.dH; out->dh0 = w.dh0; out->h0_s = w.h0_s;
  out->hb_s = w.hb; out->hb_sn = w.hb + (int64_t)st.B * st.d; out->hb_tn = w.hb_t;
  return CQLREC_OK;
}
