// f4 continued: every metric of replay/metrics on the device, from any recommendation FRAME (not only a model's block).
//   (a) frame -> block   get_top_k_recs + sorter (replay/metrics/base_metric.py:22-51, :121-134): three stable rocPRIM
//                        radix sorts (item asc, relevance desc, user), a boundary scan, one thread per user to cut,
//                        drop repeated items and compact;
//   (b) per-user extras  RocAuc (rocauc.py:43-60), Unexpectedness (unexpectedness.py:40-46), Surprisal
//                        (surprisal.py:65-68), NCISPrecision (ncis_precision.py:24-30) with the activations and the
//                        clipping of NCISMetric (base_metric.py:429-488);
//   (c) item side        distinct users per item (surprisal.py:57-63, distributions.py:74-78), Coverage's best position
//                        per item (coverage.py:90-112).
// All arithmetic in fp64; sums are per-block partials + one final pass (as eval_topk_kernel); the only atomics are
// integer atomicMin / atomicAdd, whose results do not depend on the order of arrival.
#include <climits>

#include "segment_common.h"

#define MX_MAX_KS 8
struct MxKs {
  int32_t k[MX_MAX_KS];
  int32_t n;
};

// ks: host array, ascending, within 1..kmax
static int mx_take_ks(const int32_t* ks, int32_t n_ks, int32_t kmax, const char* who, MxKs* out) {
  CQL_REQUIRE(ks != nullptr, "%s: NULL pointer", who);
  CQL_REQUIRE(n_ks > 0 && n_ks <= MX_MAX_KS, "%s: n_ks=%d out of range (1..%d)", who, n_ks, MX_MAX_KS);
  out->n = n_ks;
  for (int i = 0; i < MX_MAX_KS; ++i) out->k[i] = 0;
  for (int i = 0; i < n_ks; ++i) {
    CQL_REQUIRE(ks[i] > 0 && (kmax <= 0 || ks[i] <= kmax) && (i == 0 || ks[i] > ks[i - 1]),
                "%s: ks must be ascending and within 1..kmax", who);
    out->k[i] = ks[i];
  }
  return CQLREC_OK;
}

// =============================================================================================================
// (a) frame -> block
// =============================================================================================================
__global__ void mx_key_item_kernel(const int32_t* __restrict__ item, const uint32_t* __restrict__ perm, int64_t n,
                                   uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) key[i] = (uint64_t)((uint32_t)item[perm[i]] ^ 0x80000000u);
}
// larger relevance <=> SMALLER key (the sort is ascending); -0.0 and +0.0 get one key
__global__ void mx_key_rel_kernel(const double* __restrict__ rel, const uint32_t* __restrict__ perm, int64_t n,
                                  uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t b = (uint64_t)__double_as_longlong(rel[perm[i]]);
  if ((b << 1) == 0) b = 0;
  const uint64_t up = (b >> 63) ? ~b : (b | (1ull << 63));
  key[i] = ~up;
}
// rows outside 0..n_users-1 (users that are not evaluated) go to bucket n_users, behind every user
__global__ void mx_key_row_kernel(const int32_t* __restrict__ row, const uint32_t* __restrict__ perm, int64_t n,
                                  int64_t n_users, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = row[perm[i]];
  key[i] = (uint64_t)((r < 0 || r >= n_users) ? n_users : r);
}
__global__ __launch_bounds__(256) void mx_block_kernel(const int64_t* __restrict__ off, const uint32_t* __restrict__ perm,
                                                       const int32_t* __restrict__ item, const double* __restrict__ rel,
                                                       const double* __restrict__ payload, int64_t n_users, int kmax,
                                                       int dedup, int32_t* __restrict__ rec_idx,
                                                       double* __restrict__ rec_val, int32_t* __restrict__ rec_pos,
                                                       double* __restrict__ rec_w) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  int64_t s = 0, c = 0;
  if (off) {
    s = off[u];
    c = off[u + 1] - s;
    if (c > kmax) c = kmax;                      // get_top_k_recs: the cut comes BEFORE the repeats are dropped
  }
  int32_t* row = rec_idx + u * kmax;
  int out = 0;
  for (int j = 0; j < (int)c; ++j) {
    const uint32_t p = perm[s + j];
    const int32_t it = item[p];
    bool dup = false;
    if (dedup)
      for (int t = 0; t < out; ++t) dup = dup || (row[t] == it);
    if (dup) continue;
    row[out] = it;
    if (rec_val) rec_val[u * kmax + out] = rel[p];
    if (rec_pos) rec_pos[u * kmax + out] = j + 1;      // row_number before the repeats are dropped, 1-based
    if (rec_w) rec_w[u * kmax + out] = payload[p];
    ++out;
  }
  for (int t = out; t < kmax; ++t) {
    row[t] = -1;
    if (rec_val) rec_val[u * kmax + t] = 0.0;
    if (rec_pos) rec_pos[u * kmax + t] = 0;
    if (rec_w) rec_w[u * kmax + t] = 0.0;
  }
}

extern "C" int64_t cqlrec_recs_frame_to_block_ws_bytes(int64_t n_rows, int64_t n_users) {
  if (n_rows < 0 || n_users < 0) return -1;
  return CqlPermSort::bytes(n_rows) + cql_align256((n_users + 2) * 8) + cql_sort_temp_cap(n_rows) + 256;
}

extern "C" int cqlrec_recs_frame_to_block(const int32_t* row, const int32_t* item_idx, const double* relevance,
                                          const double* payload, int64_t n_rows, int64_t n_users, int32_t kmax,
                                          int32_t dedup, void* ws, int64_t ws_bytes, int32_t* rec_idx, double* rec_val,
                                          int32_t* rec_pos, double* rec_w, cqlrec_stream stream) {
  CQL_REQUIRE(rec_idx && ws && (n_rows == 0 || (row && item_idx && relevance)), "recs_frame_to_block: NULL pointer");
  // an empty frame has no payload to point at: rec_w, if asked for, comes out all padding
  CQL_REQUIRE(n_rows == 0 || (payload != nullptr) == (rec_w != nullptr), "recs_frame_to_block: payload and rec_w go together");
  CQL_REQUIRE(n_rows >= 0 && n_rows < (1ll << 32) && n_users > 0 && n_users < (1ll << 31) && kmax > 0,
              "recs_frame_to_block: n_rows=%lld n_users=%lld kmax=%d", (long long)n_rows, (long long)n_users, kmax);
  CQL_REQUIRE(ws_bytes >= cqlrec_recs_frame_to_block_ws_bytes(n_rows, n_users), "recs_frame_to_block: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(256), ugrid(cql_ceil_div(n_users, 256));
  if (n_rows == 0) {   // an empty frame: every user gets an empty list
    hipLaunchKernelGGL(mx_block_kernel, ugrid, block, 0, s, (const int64_t*)nullptr, (const uint32_t*)nullptr, item_idx,
                       relevance, payload, n_users, (int)kmax, (int)dedup, rec_idx, rec_val, rec_pos, rec_w);
    CQL_LAUNCH_CHECK("recs_frame_to_block");
    return CQLREC_OK;
  }
  char* p = (char*)ws;
  CqlPermSort ps(p, n_rows, s);
  int64_t* off = (int64_t*)p;       p += cql_align256((n_users + 2) * 8);
  ps.temp = p;
  const dim3 grid(cql_ceil_div(n_rows, 256));
  cql_iota(ps.perm, n_rows, false, s);
  // LSD over (user, relevance desc, item asc): the least significant key first, every pass a STABLE sort
  int rc;
  hipLaunchKernelGGL(mx_key_item_kernel, grid, block, 0, s, item_idx, ps.perm, n_rows, ps.keys<uint64_t>());
  if ((rc = ps.pass<uint64_t>("recs_frame_to_block", 32)) != CQLREC_OK) return rc;
  hipLaunchKernelGGL(mx_key_rel_kernel, grid, block, 0, s, relevance, ps.perm, n_rows, ps.keys<uint64_t>());
  if ((rc = ps.pass<uint64_t>("recs_frame_to_block", 64)) != CQLREC_OK) return rc;
  hipLaunchKernelGGL(mx_key_row_kernel, grid, block, 0, s, row, ps.perm, n_rows, n_users, ps.keys<uint64_t>());
  if ((rc = ps.pass<uint64_t>("recs_frame_to_block", cql_bits_for(n_users + 1))) != CQLREC_OK) return rc;   // bucket n_users
  // off[u] = first sorted position whose bucket >= u, u = 0..n_users+1
  cql_segment_bounds(CqlGroupOfKey<uint64_t>{ps.sorted<uint64_t>()}, n_rows, n_users + 1, off, nullptr, s);
  hipLaunchKernelGGL(mx_block_kernel, ugrid, block, 0, s, off, ps.perm, item_idx, relevance, payload, n_users, (int)kmax,
                     (int)dedup, rec_idx, rec_val, rec_pos, rec_w);
  CQL_LAUNCH_CHECK("recs_frame_to_block");
  return CQLREC_OK;
}

// ---- the join of prev_policy_weights onto the frame's rows (base_metric.py:535-542) --------------------------------
__global__ void mx_join_kernel(const uint64_t* __restrict__ keys, const double* __restrict__ vals, int64_t n_keys,
                               const int32_t* __restrict__ user, const int32_t* __restrict__ item, int64_t n_rows,
                               double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  const uint64_t k = (user ? ((uint64_t)(uint32_t)user[i] << 32) : 0ull) | (uint64_t)(uint32_t)item[i];
  int64_t lo = 0, hi = n_keys;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  out[i] = (lo < n_keys && keys[lo] == k) ? vals[lo] : 0.0;     // .na.fill(0.0)
}

extern "C" int cqlrec_recs_join_prev(const uint64_t* keys, const double* vals, int64_t n_keys, const int32_t* user_idx,
                                     const int32_t* item_idx, int64_t n_rows, double* out, cqlrec_stream stream) {
  CQL_REQUIRE(item_idx && out && (n_keys == 0 || (keys && vals)), "recs_join_prev: NULL pointer");
  CQL_REQUIRE(n_keys >= 0 && n_rows > 0, "recs_join_prev: n_keys=%lld n_rows=%lld", (long long)n_keys, (long long)n_rows);
  hipLaunchKernelGGL(mx_join_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, (hipStream_t)stream, keys, vals, n_keys,
                     user_idx, item_idx, n_rows, out);
  CQL_LAUNCH_CHECK("recs_join_prev");
  return CQLREC_OK;
}

// ---- NCIS weights of a cut, NOT yet de-duplicated block: activation per user over the kept rows, weigh and clip, then
// ---- sorter(extra_position=2): later repeats of an item leave, together with their weight ---------------------------
__global__ __launch_bounds__(256) void mx_ncis_kernel(int32_t* __restrict__ rec_idx, double* __restrict__ rec_val,
                                                      double* __restrict__ rec_w, int64_t n_users, int kmax,
                                                      int activation, double threshold) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  int32_t* idx = rec_idx + u * kmax;
  double* val = rec_val + u * kmax;
  double* w = rec_w + u * kmax;
  int np = 0;
  while (np < kmax && idx[np] >= 0) ++np;
  if (activation == CQLREC_NCIS_SOFTMAX) {          // _softmax_by_user: exp(x - min) / sum, each column on its own
    double mv = __builtin_inf(), mw = __builtin_inf();
    for (int j = 0; j < np; ++j) {
      mv = fmin(mv, val[j]);
      mw = fmin(mw, w[j]);
    }
    double sv = 0.0, sw = 0.0;
    for (int j = 0; j < np; ++j) {
      val[j] = exp(val[j] - mv);
      w[j] = exp(w[j] - mw);
      sv += val[j];
      sw += w[j];
    }
    for (int j = 0; j < np; ++j) {
      val[j] = val[j] / sv;
      w[j] = w[j] / sw;
    }
  } else if (activation == CQLREC_NCIS_SIGMOID) {   // _sigmoid
    for (int j = 0; j < np; ++j) {
      val[j] = 1.0 / (1.0 + exp(-val[j]));
      w[j] = 1.0 / (1.0 + exp(-w[j]));
    }
  }
  const double lower = 1.0 / threshold, upper = threshold;
  int out = 0;
  for (int j = 0; j < np; ++j) {
    const double prev = w[j], unb = val[j] / prev;   // _weigh_and_clip
    const double wt = (prev == 0.0) ? upper : (unb < lower) ? lower : (unb > upper) ? upper : unb;
    const int32_t it = idx[j];
    const double v = val[j];
    bool dup = false;
    for (int t = 0; t < out; ++t) dup = dup || (idx[t] == it);
    if (dup) continue;
    idx[out] = it;
    val[out] = v;
    w[out] = wt;
    ++out;
  }
  for (int t = out; t < np; ++t) {
    idx[t] = -1;
    val[t] = 0.0;
    w[t] = 0.0;
  }
}

extern "C" int cqlrec_recs_ncis_weights(int32_t* rec_idx, double* rec_val, double* rec_w, int64_t n_users, int32_t kmax,
                                        int32_t activation, double threshold, cqlrec_stream stream) {
  CQL_REQUIRE(rec_idx && rec_val && rec_w, "recs_ncis_weights: NULL pointer");
  CQL_REQUIRE(n_users > 0 && kmax > 0, "recs_ncis_weights: n_users=%lld kmax=%d", (long long)n_users, kmax);
  CQL_REQUIRE(activation >= CQLREC_NCIS_NONE && activation <= CQLREC_NCIS_SOFTMAX, "recs_ncis_weights: unknown activation %d",
              activation);
  CQL_REQUIRE(threshold > 0.0, "recs_ncis_weights: threshold must be positive");
  hipLaunchKernelGGL(mx_ncis_kernel, dim3(cql_ceil_div(n_users, 256)), dim3(256), 0, (hipStream_t)stream, rec_idx, rec_val,
                     rec_w, n_users, (int)kmax, (int)activation, threshold);
  CQL_LAUNCH_CHECK("recs_ncis_weights");
  return CQLREC_OK;
}

// =============================================================================================================
// (b) per-user extras
// =============================================================================================================
__global__ __launch_bounds__(256) void mx_extras_kernel(const int32_t* __restrict__ rec_idx, int64_t n_users, int kmax,
                                                        const int32_t* __restrict__ rec_rows,
                                                        const int64_t* __restrict__ gt_off,
                                                        const int32_t* __restrict__ gt_items,
                                                        const int32_t* __restrict__ base_idx, int kb,
                                                        const double* __restrict__ item_w, int64_t n_item_w,
                                                        const double* __restrict__ rec_w, MxKs ks,
                                                        double* __restrict__ per_user, double* __restrict__ block_sums) {
  __shared__ double red[256];
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double vals[CQLREC_EVAL_EXTRAS][MX_MAX_KS];
#pragma unroll
  for (int m = 0; m < CQLREC_EVAL_EXTRAS; ++m)
#pragma unroll
    for (int q = 0; q < MX_MAX_KS; ++q) vals[m][q] = 0.0;
  if (u < n_users) {
    const int32_t* pred = rec_idx + u * kmax;
    int64_t g0 = 0;
    int ngt = 0;
    if (gt_off) {
      const int64_t row = rec_rows ? (int64_t)rec_rows[u] : u;
      g0 = gt_off[row];
      ngt = (int)(gt_off[row + 1] - g0);
    }
    int npred = 0;
    while (npred < kmax && pred[npred] >= 0) ++npred;
    int nbase = 0;
    if (base_idx)
      while (nbase < kb && base_idx[u * kb + nbase] >= 0) ++nbase;
    int fp_cur = 0, fp_cum = 0;
    double wsum = 0.0, whit = 0.0, surp = 0.0;
    int q = 0;
    for (int j = 0; j < kmax && q < ks.n; ++j) {
      if (j < npred) {
        const int32_t it = pred[j];
        bool hit = false;
        if (ngt > 0) {
          int lo = 0, hi = ngt;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (gt_items[g0 + mid] < it) lo = mid + 1; else hi = mid;
          }
          hit = lo < ngt && gt_items[g0 + lo] == it;
        }
        if (hit) fp_cum += fp_cur; else ++fp_cur;                       // rocauc.py:51-55
        if (rec_w) {
          const double w = rec_w[u * kmax + j];
          wsum += w;
          if (hit) whit += w;
        }
        if (item_w) surp += (it < n_item_w) ? item_w[it] : 1.0;         // .fillna(1.0): an item the log never saw
      }
      while (q < ks.n && ks.k[q] == j + 1) {
        const int k = j + 1;
        const int len = k < npred ? k : npred;
        const bool ok = npred > 0 && ngt > 0;
        double roc = 0.0;                                               // rocauc.py:45-60
        if (ok && fp_cur != len) roc = (fp_cum == 0) ? 1.0 : 1.0 - (double)fp_cum / (double)(fp_cur * (len - fp_cur));
        vals[0][q] = roc;
        if (base_idx && npred > 0) {                                    // unexpectedness.py:44-46
          const int nb = k < nbase ? k : nbase;
          int common = 0;
          for (int a = 0; a < len; ++a) {
            const int32_t it = pred[a];
            for (int b = 0; b < nb; ++b) common += (base_idx[u * kb + b] == it) ? 1 : 0;
          }
          vals[1][q] = 1.0 - (double)common / (double)k;
        }
        vals[2][q] = surp / (double)k;                                  // surprisal.py:66-68
        vals[3][q] = (rec_w && ok) ? whit / wsum : 0.0;                 // ncis_precision.py:27-30
        ++q;
      }
    }
    if (per_user) {
      for (int m = 0; m < CQLREC_EVAL_EXTRAS; ++m)
        for (int qq = 0; qq < ks.n; ++qq) per_user[(u * CQLREC_EVAL_EXTRAS + m) * ks.n + qq] = vals[m][qq];
    }
  }
  // deterministic block sums
  for (int m = 0; m < CQLREC_EVAL_EXTRAS; ++m) {
    for (int qq = 0; qq < ks.n; ++qq) {
      red[threadIdx.x] = vals[m][qq];
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
      }
      if (threadIdx.x == 0) block_sums[((int64_t)blockIdx.x * CQLREC_EVAL_EXTRAS + m) * ks.n + qq] = red[0];
      __syncthreads();
    }
  }
}

__global__ void mx_final_kernel(const double* __restrict__ block_sums, int nblocks, int nvals, double* __restrict__ sums) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nvals) return;
  double s = 0.0;
  for (int b = 0; b < nblocks; ++b) s += block_sums[(int64_t)b * nvals + v];
  sums[v] = s;
}

extern "C" int64_t cqlrec_eval_extras_ws_bytes(int64_t n_users, int32_t n_ks) {
  if (n_users < 0 || n_ks < 0) return -1;
  return cql_align256((int64_t)cql_ceil_div(n_users, 256) * CQLREC_EVAL_EXTRAS * n_ks * 8) + 256;
}

extern "C" int cqlrec_eval_extras(const int32_t* rec_idx, int64_t n_users, int32_t kmax, const int32_t* rec_rows,
                                  const int64_t* gt_off, const int32_t* gt_items, const int32_t* base_idx, int32_t kb,
                                  const double* item_w, int64_t n_item_w, const double* rec_w, const int32_t* ks,
                                  int32_t n_ks, void* ws, int64_t ws_bytes, double* per_user, double* sums,
                                  cqlrec_stream stream) {
  CQL_REQUIRE(rec_idx && ks && ws && sums, "eval_extras: NULL pointer");
  CQL_REQUIRE((gt_off != nullptr) == (gt_items != nullptr), "eval_extras: gt_off and gt_items go together");
  CQL_REQUIRE(n_users > 0 && kmax > 0, "eval_extras: n_users=%lld kmax=%d", (long long)n_users, kmax);
  CQL_REQUIRE(!base_idx || kb > 0, "eval_extras: kb=%d", kb);
  CQL_REQUIRE(!item_w || n_item_w > 0, "eval_extras: n_item_w=%lld", (long long)n_item_w);
  MxKs e;
  const int rc = mx_take_ks(ks, n_ks, kmax, "eval_extras", &e);
  if (rc != CQLREC_OK) return rc;
  CQL_REQUIRE(ws_bytes >= cqlrec_eval_extras_ws_bytes(n_users, n_ks), "eval_extras: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int nblocks = cql_ceil_div(n_users, 256);
  hipLaunchKernelGGL(mx_extras_kernel, dim3(nblocks), dim3(256), 0, s, rec_idx, n_users, (int)kmax, rec_rows, gt_off,
                     gt_items, base_idx, (int)kb, item_w, n_item_w, rec_w, e, per_user, (double*)ws);
  const int nvals = CQLREC_EVAL_EXTRAS * n_ks;
  hipLaunchKernelGGL(mx_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, nblocks, nvals, sums);
  CQL_LAUNCH_CHECK("eval_extras");
  return CQLREC_OK;
}

// =============================================================================================================
// (c) item side
// =============================================================================================================
__global__ void mx_pair_key_kernel(const int32_t* __restrict__ item, const int32_t* __restrict__ user, int64_t n,
                                   uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) key[i] = ((uint64_t)(uint32_t)user[i] << 32) | (uint64_t)(uint32_t)item[i];
}
// run heads of the sorted (user, item) pairs: one per distinct pair -> cnt[item]; one per distinct user -> n_distinct
__global__ void mx_pair_heads_kernel(const uint64_t* __restrict__ key, int64_t n, int64_t n_items, int32_t* __restrict__ cnt,
                                     unsigned long long* __restrict__ n_distinct) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  const bool pair_head = i == 0 || key[i - 1] != k;
  const bool user_head = i == 0 || (key[i - 1] >> 32) != (k >> 32);
  const int64_t it = (int64_t)(uint32_t)k;
  if (pair_head && it < n_items) atomicAdd(&cnt[it], 1);
  if (user_head) atomicAdd(n_distinct, 1ull);
}

extern "C" int64_t cqlrec_eval_item_user_counts_ws_bytes(int64_t n_rows) {
  if (n_rows < 0) return -1;
  return 2 * cql_align256(n_rows * 8) + cql_sort_temp_cap(n_rows) + 256;
}

extern "C" int cqlrec_eval_item_user_counts(const int32_t* item_idx, const int32_t* user_idx, int64_t n_rows,
                                            int64_t n_items, void* ws, int64_t ws_bytes, int32_t* cnt,
                                            int64_t* n_distinct_users, cqlrec_stream stream) {
  CQL_REQUIRE(item_idx && user_idx && ws && cnt && n_distinct_users, "eval_item_user_counts: NULL pointer");
  CQL_REQUIRE(n_rows > 0 && n_rows < (1ll << 32) && n_items > 0, "eval_item_user_counts: n_rows=%lld n_items=%lld",
              (long long)n_rows, (long long)n_items);
  CQL_REQUIRE(ws_bytes >= cqlrec_eval_item_user_counts_ws_bytes(n_rows), "eval_item_user_counts: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)ws;
  uint64_t* key_a = (uint64_t*)p;   p += cql_align256(n_rows * 8);
  uint64_t* key_b = (uint64_t*)p;   p += cql_align256(n_rows * 8);
  void* temp = p;
  const size_t temp_cap = (size_t)cql_sort_temp_cap(n_rows);
  const dim3 grid(cql_ceil_div(n_rows, 256)), block(256);
  hipLaunchKernelGGL(mx_pair_key_kernel, grid, block, 0, s, item_idx, user_idx, n_rows, key_a);
  const int rc = cql_sort_keys("eval_item_user_counts", temp, temp_cap, key_a, key_b, n_rows, 64, s);
  if (rc != CQLREC_OK) return rc;
  CQL_MEMSET(cnt, 0, (size_t)n_items * 4, s, "eval_item_user_counts");
  CQL_MEMSET(n_distinct_users, 0, 8, s, "eval_item_user_counts");
  hipLaunchKernelGGL(mx_pair_heads_kernel, grid, block, 0, s, key_b, n_rows, n_items, cnt,
                     (unsigned long long*)n_distinct_users);
  CQL_LAUNCH_CHECK("eval_item_user_counts");
  return CQLREC_OK;
}

// w = log2(n_users / cnt) / log2(n_users) (surprisal.py:57-63); an item nobody touched keeps the cold weight 1.0
__global__ void mx_surprisal_w_kernel(const int32_t* __restrict__ cnt, int64_t n_items, double n_users, double* __restrict__ w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  const int32_t c = cnt[i];
  w[i] = c > 0 ? log2(n_users / (double)c) / log2(n_users) : 1.0;
}

extern "C" int cqlrec_eval_surprisal_weights(const int32_t* cnt, int64_t n_items, int64_t n_users, double* w,
                                             cqlrec_stream stream) {
  CQL_REQUIRE(cnt && w, "eval_surprisal_weights: NULL pointer");
  CQL_REQUIRE(n_items > 0, "eval_surprisal_weights: n_items=%lld", (long long)n_items);
  CQL_REQUIRE(n_users > 1, "eval_surprisal_weights: n_users=%lld (a log of one user has no self-information scale)",
              (long long)n_users);
  hipLaunchKernelGGL(mx_surprisal_w_kernel, dim3(cql_ceil_div(n_items, 256)), dim3(256), 0, (hipStream_t)stream, cnt,
                     n_items, (double)n_users, w);
  CQL_LAUNCH_CHECK("eval_surprisal_weights");
  return CQLREC_OK;
}

// ---- Coverage: best position per item, then how many items have one within k -----------------------------------------
__global__ void mx_cov_init_kernel(int32_t* __restrict__ best, int64_t n_items, unsigned long long* __restrict__ counts,
                                   int n_ks) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_items) best[i] = INT_MAX;
  if (i < n_ks) counts[i] = 0ull;
}
__global__ void mx_cov_best_kernel(const int32_t* __restrict__ rec_idx, const int32_t* __restrict__ rec_pos, int64_t n_cells,
                                   int64_t n_items, int32_t* __restrict__ best) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const int32_t it = rec_idx[i];
  if (it >= 0 && it < n_items) atomicMin(&best[it], rec_pos[i]);
}
__global__ __launch_bounds__(256) void mx_cov_count_kernel(const int32_t* __restrict__ best, int64_t n_items, MxKs ks,
                                                           unsigned long long* __restrict__ counts) {
  __shared__ int red[256];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int32_t b = i < n_items ? best[i] : INT_MAX;
  for (int q = 0; q < ks.n; ++q) {
    red[threadIdx.x] = b <= ks.k[q] ? 1 : 0;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0 && red[0] > 0) atomicAdd(&counts[q], (unsigned long long)red[0]);
    __syncthreads();
  }
}

extern "C" int cqlrec_eval_coverage(const int32_t* rec_idx, const int32_t* rec_pos, int64_t n_users, int32_t kmax,
                                    int64_t n_items, const int32_t* ks, int32_t n_ks, int32_t* best, int64_t* counts,
                                    cqlrec_stream stream) {
  CQL_REQUIRE(rec_idx && rec_pos && ks && best && counts, "eval_coverage: NULL pointer");
  CQL_REQUIRE(n_users > 0 && kmax > 0 && n_items > 0, "eval_coverage: n_users=%lld kmax=%d n_items=%lld",
              (long long)n_users, kmax, (long long)n_items);
  MxKs e;
  const int rc = mx_take_ks(ks, n_ks, 0, "eval_coverage", &e);    // a cut-off beyond kmax is legal (coverage.py:106-112)
  if (rc != CQLREC_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(256), igrid(cql_ceil_div(n_items, 256));
  hipLaunchKernelGGL(mx_cov_init_kernel, igrid, block, 0, s, best, n_items, (unsigned long long*)counts, (int)n_ks);
  hipLaunchKernelGGL(mx_cov_best_kernel, dim3(cql_ceil_div(n_users * kmax, 256)), block, 0, s, rec_idx, rec_pos,
                     n_users * (int64_t)kmax, n_items, best);
  hipLaunchKernelGGL(mx_cov_count_kernel, igrid, block, 0, s, (const int32_t*)best, n_items, e, (unsigned long long*)counts);
  CQL_LAUNCH_CHECK("eval_coverage");
  return CQLREC_OK;
}

// ---- rec_count of item_distribution: a block cut at k with repeats dropped holds an item once per user ---------------
__global__ void mx_item_hist_kernel(const int32_t* __restrict__ rec_idx, int64_t n_cells, int64_t n_items,
                                    int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const int32_t it = rec_idx[i];
  if (it >= 0 && it < n_items) atomicAdd(&cnt[it], 1);
}

extern "C" int cqlrec_eval_item_hist(const int32_t* rec_idx, int64_t n_users, int32_t kmax, int64_t n_items, int32_t* cnt,
                                     cqlrec_stream stream) {
  CQL_REQUIRE(rec_idx && cnt, "eval_item_hist: NULL pointer");
  CQL_REQUIRE(n_users > 0 && kmax > 0 && n_items > 0, "eval_item_hist: n_users=%lld kmax=%d n_items=%lld", (long long)n_users,
              kmax, (long long)n_items);
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(cnt, 0, (size_t)n_items * 4, s, "eval_item_hist");
  hipLaunchKernelGGL(mx_item_hist_kernel, dim3(cql_ceil_div(n_users * kmax, 256)), dim3(256), 0, s, rec_idx,
                     n_users * (int64_t)kmax, n_items, cnt);
  CQL_LAUNCH_CHECK("eval_item_hist");
  return CQLREC_OK;
}
