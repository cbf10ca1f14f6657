// f8  neighbourhood models on the device (replay/models/knn.py, NeighbourRec of replay/models/base_rec.py): the row-wise
// top-k of a sparse x sparse product -- expand, sort, reduce, select -- with the FIT epilogue of ItemKNN (cosine with a
// shrink term, ties by j descending) and the PREDICT epilogue of NeighbourRec (item mask, seen lists, ties by j ascending),
// and the small kernels around it: row weights (tf-idf, bm25), item norms, pair scores.  f10 (association rules,
// replay/models/association_rules.py) is a third epilogue on the same chunk loop.  The rules of f5 - f7 hold:
// integer atomics only, no floating-point atomics, the same input gives the same bytes.  Built with -ffp-contract=off:
// every expression below is evaluated as written.
//
// The terms of one (row, j) sum are added in an order fixed by their POSITION in the sum -- L-entry order, then R-entry
// order, which the expansion produces and the stable sort keeps: up to NB_SHORT terms left to right by one thread, more
// by one wave (lane l takes the terms l, l + 64, ... in that order, then a butterfly over the lanes).  How the query
// rows are cut into chunks therefore never shows in the result.
#include "segment_common.h"

static const int64_t NB_MAX = 1ll << 31;
static const int NB_SHORT = 32;
static const uint32_t NB_PAD = 0xFFFFFFFFu;

__device__ __forceinline__ double nb_wave_sum(double acc) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
  return acc;
}

// order-preserving map double -> uint64 (a larger double has a larger key)
__device__ __forceinline__ uint64_t f64_order_key(double x) {
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

// =============================================================================================================
// row weights
// =============================================================================================================
__global__ void neighbour_weights_kernel(const int32_t* __restrict__ user, const int32_t* __restrict__ item,
                                         const double* __restrict__ relevance, const int32_t* __restrict__ ucount,
                                         const int32_t* __restrict__ icount, int64_t n, double n_items, double avgdl,
                                         int weighting, double k1, double b, double* __restrict__ w) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double rel = relevance ? relevance[r] : 1.0;
  if (weighting != CQLREC_NEIGHBOUR_WEIGHT_NONE) {
    const double df = (double)ucount[user[r]];
    double idf;
    if (weighting == CQLREC_NEIGHBOUR_WEIGHT_TF_IDF) {
      idf = log1p(n_items / df);
    } else {
      const double cnt = (double)icount[item[r]];
      rel = rel * (k1 + 1.0) / (rel + k1 * (1.0 - b + b * (cnt / avgdl)));
      idf = log1p((n_items - df + 0.5) / (df + 0.5));
    }
    rel = rel * idf;
  }
  w[r] = rel;
}

extern "C" int cqlrec_neighbour_weights(const int32_t* user_idx, const int32_t* item_idx, const double* relevance,
                                        const int32_t* ucount, const int32_t* icount, int64_t n_rows, int64_t n_items,
                                        int32_t weighting, double k1, double b, double* w, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < NB_MAX && n_items >= 0 && n_items < NB_MAX,
              "neighbour_weights: n_rows=%lld n_items=%lld out of range", (long long)n_rows, (long long)n_items);
  CQL_REQUIRE(weighting >= CQLREC_NEIGHBOUR_WEIGHT_NONE && weighting <= CQLREC_NEIGHBOUR_WEIGHT_BM25,
              "neighbour_weights: unknown weighting %d", weighting);
  if (n_rows == 0) return CQLREC_OK;
  CQL_REQUIRE(w, "neighbour_weights: NULL pointer");
  CQL_REQUIRE(weighting == CQLREC_NEIGHBOUR_WEIGHT_NONE || (user_idx && item_idx && ucount && icount && n_items > 0),
              "neighbour_weights: weighting %d needs the id columns, both counts and n_items > 0 (NULL pointer)", weighting);
  hipStream_t s = (hipStream_t)stream;
  const double avgdl = n_items > 0 ? (double)n_rows / (double)n_items : 1.0;
  hipLaunchKernelGGL(neighbour_weights_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, user_idx, item_idx, relevance,
                     ucount, icount, n_rows, (double)n_items, avgdl, (int)weighting, k1, b, w);
  CQL_LAUNCH_CHECK("neighbour_weights");
  return CQLREC_OK;
}

// =============================================================================================================
// norms: one wave per group
// =============================================================================================================
__global__ __launch_bounds__(256) void neighbour_norms_kernel(const int32_t* __restrict__ perm,
                                                              const int64_t* __restrict__ offsets,
                                                              const double* __restrict__ w, int64_t n_groups,
                                                              double* __restrict__ norm) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= n_groups) return;
  const int64_t a = offsets[g], b = offsets[g + 1];
  double acc = 0.0;
  for (int64_t p = a + lane; p < b; p += 64) {
    const double x = w[perm[p]];
    acc += x * x;
  }
  acc = nb_wave_sum(acc);
  if (lane == 0) norm[g] = sqrt(acc);
}

extern "C" int cqlrec_neighbour_norms(const int32_t* perm, const int64_t* offsets, const double* w, int64_t n_rows,
                                      int64_t n_groups, double* norm, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < NB_MAX && n_groups > 0 && n_groups < NB_MAX,
              "neighbour_norms: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(norm, "neighbour_norms: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(norm, 0, (size_t)n_groups * 8, s, "neighbour_norms");
    return CQLREC_OK;
  }
  CQL_REQUIRE(perm && offsets && w, "neighbour_norms: NULL pointer");
  hipLaunchKernelGGL(neighbour_norms_kernel, dim3(cql_ceil_div(n_groups, 4)), dim3(256), 0, s, perm, offsets, w, n_groups,
                     norm);
  CQL_LAUNCH_CHECK("neighbour_norms");
  return CQLREC_OK;
}

// =============================================================================================================
// the count pass
// =============================================================================================================
__global__ void neighbour_len_kernel(const int32_t* __restrict__ l_col, const int64_t* __restrict__ r_off, int64_t nnz,
                                     int64_t* __restrict__ len) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e > nnz) return;
  int64_t v = 0;
  if (e < nnz) {
    const int64_t m = l_col[e];
    v = r_off[m + 1] - r_off[m];
  }
  len[e] = v;
}
__global__ void neighbour_row_prefix_kernel(const int64_t* __restrict__ l_off, const int64_t* __restrict__ eprefix,
                                            int64_t n_q, int64_t nnz, int64_t* __restrict__ row_prefix,
                                            int64_t* __restrict__ stats) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > n_q) return;
  const int64_t p = eprefix[l_off[q]];
  row_prefix[q] = p;
  if (q < n_q) {
    const int64_t mine = eprefix[l_off[q + 1]] - p;
    if (mine > 0) atomicMax((unsigned long long*)&stats[1], (unsigned long long)mine);
  } else {
    stats[0] = eprefix[nnz];
  }
}

extern "C" int64_t cqlrec_neighbour_count_ws_bytes(int64_t nnz_l) {
  if (nnz_l < 0 || nnz_l >= NB_MAX) return 0;
  return cql_align256((nnz_l + 1) * 8) + cql_scan_temp_cap(nnz_l + 1) + 256;
}

extern "C" int cqlrec_neighbour_count(const int64_t* l_off, const int32_t* l_col, int64_t n_q, int64_t nnz_l,
                                      const int64_t* r_off, int64_t n_mid, void* ws, int64_t ws_bytes,
                                      int64_t* entry_prefix, int64_t* row_prefix, int64_t* stats, cqlrec_stream stream) {
  CQL_REQUIRE(n_q >= 0 && n_q < NB_MAX && nnz_l >= 0 && nnz_l < NB_MAX && n_mid >= 0 && n_mid < NB_MAX,
              "neighbour_count: n_q=%lld nnz_l=%lld n_mid=%lld out of range", (long long)n_q, (long long)nnz_l,
              (long long)n_mid);
  CQL_REQUIRE(stats, "neighbour_count: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_q > 0) {
    CQL_REQUIRE(l_off && entry_prefix && row_prefix && ws && (nnz_l == 0 || (l_col && r_off)), "neighbour_count: NULL pointer");
    CQL_REQUIRE(ws_bytes >= cqlrec_neighbour_count_ws_bytes(nnz_l), "neighbour_count: workspace too small");
  }
  CQL_MEMSET(stats, 0, 16, s, "neighbour_count");
  if (n_q == 0) return CQLREC_OK;
  char* p = (char*)ws;
  int64_t* len = (int64_t*)p;  p += cql_align256((nnz_l + 1) * 8);
  void* temp = p;
  const size_t cap = (size_t)cql_scan_temp_cap(nnz_l + 1);
  hipLaunchKernelGGL(neighbour_len_kernel, dim3(cql_ceil_div(nnz_l + 1, 256)), dim3(256), 0, s, l_col, r_off, nnz_l, len);
  const int rc = cql_exclusive_scan("neighbour_count", temp, cap, len, entry_prefix, (int64_t)0, nnz_l + 1, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(neighbour_row_prefix_kernel, dim3(cql_ceil_div(n_q + 1, 256)), dim3(256), 0, s, l_off, entry_prefix, n_q,
                     nnz_l, row_prefix, stats);
  CQL_LAUNCH_CHECK("neighbour_count");
  return CQLREC_OK;
}

// =============================================================================================================
// expand, sort, reduce, select
// =============================================================================================================
struct NbChunk {
  int64_t q0, rows;     // the chunk's first query row and how many it holds
  int64_t g0, T;        // its first tuple in the whole expansion and how many it holds
  unsigned jbits;       // the key of a tuple is (local row << jbits) | j
};

// one tuple per thread: the L entry by binary search in the entry prefix, the query row by binary search in l_off.
// RULES (f10): the value is min(a, b) instead of a * b, and a tuple with j == q is dropped here, so that the run length of
// a (row, j) is its pair count.
template <bool RULES>
__global__ void neighbour_expand_kernel(NbChunk C, const int64_t* __restrict__ l_off, const int32_t* __restrict__ l_col,
                                        const double* __restrict__ l_val, const int64_t* __restrict__ r_off,
                                        const int32_t* __restrict__ r_col, const double* __restrict__ r_val,
                                        const int64_t* __restrict__ eprefix, int64_t n_cols, uint64_t* __restrict__ key,
                                        double* __restrict__ val) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= C.T) return;
  const int64_t g = C.g0 + t;
  const int64_t e_lo = l_off[C.q0], e_hi = l_off[C.q0 + C.rows];
  int64_t a = e_lo, b = e_hi;                // the first entry in [e_lo, e_hi] whose prefix is > g
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    if (eprefix[mid] > g) b = mid; else a = mid + 1;
  }
  const int64_t e = a - 1;
  uint64_t k = (uint64_t)C.rows << C.jbits;  // a row past the chunk: a tuple the prefixes do not account for is dropped
  double v = 0.0;
  if (e >= e_lo) {
    const int64_t m = l_col[e];
    const int64_t r = r_off[m] + (g - eprefix[e]);
    if (r < r_off[m + 1]) {
      const int64_t j = r_col[r];
      int64_t qa = C.q0, qb = C.q0 + C.rows; // the first row whose entries end behind e
      while (qa < qb) {
        const int64_t mid = qa + ((qb - qa) >> 1);
        if (l_off[mid + 1] > e) qb = mid; else qa = mid + 1;
      }
      if (j >= 0 && j < n_cols && qa < C.q0 + C.rows && !(RULES && j == qa)) {
        k = ((uint64_t)(qa - C.q0) << C.jbits) | (uint64_t)j;
        if (RULES) {
          const double a = l_val[e], b = r_val[r];
          v = b < a ? b : a;
        } else {
          v = l_val[e] * r_val[r];
        }
      }
    }
  }
  key[t] = k;
  val[t] = v;
}

// sums of up to NB_SHORT terms, left to right; the longer ones are listed for the wave kernel
__global__ void neighbour_sum_short_kernel(const double* __restrict__ val, const uint32_t* __restrict__ seg_off,
                                           const uint32_t* __restrict__ runs, const size_t* __restrict__ n_runs,
                                           double* __restrict__ csum, uint32_t* __restrict__ long_list,
                                           uint32_t* __restrict__ n_long) {
  const int64_t sg = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sg >= (int64_t)*n_runs) return;
  const uint32_t len = runs[sg];
  if (len > (uint32_t)NB_SHORT) {
    long_list[atomicAdd(n_long, 1u)] = (uint32_t)sg;
    return;
  }
  const double* v = val + seg_off[sg];
  double acc = 0.0;
  for (uint32_t i = 0; i < len; ++i) acc += v[i];
  csum[sg] = acc;
}
__global__ __launch_bounds__(256) void neighbour_sum_long_kernel(const double* __restrict__ val,
                                                                 const uint32_t* __restrict__ seg_off,
                                                                 const uint32_t* __restrict__ runs,
                                                                 const uint32_t* __restrict__ long_list,
                                                                 const uint32_t* __restrict__ n_long,
                                                                 double* __restrict__ csum) {
  const int lane = threadIdx.x & 63;
  const uint32_t n = *n_long;
  for (uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6); w < n; w += gridDim.x * 4) {
    const uint32_t sg = long_list[w];
    const double* v = val + seg_off[sg];
    const uint32_t len = runs[sg];
    double acc = 0.0;
    for (uint32_t i = lane; i < len; i += 64) acc += v[i];
    acc = nb_wave_sum(acc);
    if (lane == 0) csum[sg] = acc;
  }
}

struct NbEpilogue {
  int mode;
  const double *norm_q, *norm_j;
  double shrink;
  const uint8_t* mask;
  const int64_t* seen_off;
  const int32_t* seen_col;
};

// the value of every (row, j) and whether it is a candidate; the selection key is the inverted order image of the value,
// so that an ascending stable sort gives value descending.  Ties keep the order they enter the sort in: j ascending for
// PREDICT, and FIT enters them reversed.
__global__ void neighbour_epilogue_kernel(NbChunk C, NbEpilogue E, const uint64_t* __restrict__ ukey,
                                          const size_t* __restrict__ n_runs, double* __restrict__ csum,
                                          uint64_t* __restrict__ skey, uint32_t* __restrict__ payload) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.T) return;
  const int64_t n = (int64_t)*n_runs;
  uint64_t sk = ~0ull;
  uint32_t pl = NB_PAD;
  if (i < n) {
    const int64_t sg = E.mode == CQLREC_NEIGHBOUR_FIT ? n - 1 - i : i;
    const uint64_t key = ukey[sg];
    const int64_t row = (int64_t)(key >> C.jbits);
    const int64_t j = (int64_t)(key & ((1ull << C.jbits) - 1));
    if (row < C.rows) {
      const int64_t q = C.q0 + row;
      double v = csum[sg];
      bool ok = true;
      if (E.mode == CQLREC_NEIGHBOUR_FIT) {
        const double den = E.norm_q[q] * E.norm_j[j] + E.shrink;
        ok = j != q && den != 0.0;
        v = v / den;
      } else {
        if (E.mask && E.mask[j] == 0) ok = false;
        if (ok && E.seen_off) {
          const int64_t end = E.seen_off[q + 1];
          int64_t lo = E.seen_off[q], hi = end;
          while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)E.seen_col[mid] < j) lo = mid + 1; else hi = mid;
          }
          ok = !(lo < end && (int64_t)E.seen_col[lo] == j);
        }
      }
      if (ok) {
        csum[sg] = v;
        sk = ~f64_order_key(v + 0.0);        // -0.0 and +0.0 are one value
        pl = (uint32_t)sg;
      }
    }
  }
  skey[i] = sk;
  payload[i] = pl;
}

__global__ void neighbour_row_key_kernel(NbChunk C, const uint64_t* __restrict__ ukey, const uint32_t* __restrict__ payload,
                                         uint32_t* __restrict__ row_key) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.T) return;
  const uint32_t p = payload[i];
  row_key[i] = p == NB_PAD ? (uint32_t)C.rows : (uint32_t)(ukey[p] >> C.jbits);
}
__global__ void neighbour_write_kernel(NbChunk C, const uint64_t* __restrict__ ukey, const double* __restrict__ csum,
                                       const uint32_t* __restrict__ row_key, const uint32_t* __restrict__ payload,
                                       const int64_t* __restrict__ row_start, int32_t k, int32_t* __restrict__ ids,
                                       double* __restrict__ vals, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.T) return;
  const int64_t row = row_key[i];
  if (row >= C.rows) return;
  const int64_t first = row_start[row];
  const int64_t rank = i - first;
  if (rank >= k) return;
  const uint32_t sg = payload[i];
  const int64_t o = (C.q0 + row) * k + rank;
  ids[o] = (int32_t)(ukey[sg] & ((1ull << C.jbits) - 1));
  vals[o] = csum[sg];
  if (rank == 0) {
    const int64_t n = row_start[row + 1] - first;
    count[C.q0 + row] = (int32_t)(n < k ? n : k);
  }
}
__global__ void neighbour_fill_kernel(int64_t n, int32_t* __restrict__ ids, double* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  ids[i] = -1;
  vals[i] = 0.0;
}

// ---- f10: the association-rules epilogue -----------------------------------------------------------------------------------
struct NbRules {
  const double* item_rel;   // [n_q]: the summed weight of every item (antecedent and consequent alike)
  double n;                 // (double)num_sessions
  int64_t min_pair_count;
  double *lift, *gain;      // the second and third value plane; the first is `vals`
};
// the three measures of a pair, each expression evaluated as written (the file is built with -ffp-contract=off)
__device__ __forceinline__ double rules_confidence(double p, double A) { return p / A; }
__device__ __forceinline__ double rules_lift(double p, double A, double Cr, double n) { return (n * (p / A)) / Cr; }
__device__ __forceinline__ double rules_gain(double p, double A, double Cr, double n) {
  const double d = Cr - p;
  return d == 0.0 ? __longlong_as_double(0x7FF0000000000000ll) : ((p / A) * (n - A)) / d;
}

// item_rel[g] = the sum of the group's values, one wave per group in an order fixed by position
__global__ __launch_bounds__(256) void rules_item_relevance_kernel(const int64_t* __restrict__ offsets,
                                                                   const double* __restrict__ val, int64_t n_groups,
                                                                   double* __restrict__ item_rel) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= n_groups) return;
  const int64_t a = offsets[g], b = offsets[g + 1];
  double acc = 0.0;
  for (int64_t p = a + lane; p < b; p += 64) acc += val[p];
  acc = nb_wave_sum(acc);
  if (lane == 0) item_rel[g] = acc;
}

// candidates: pair_count (the run length) >= min_pair_count and both item relevances non-zero; the selection key is the
// lift; csum keeps the pair relevance.  Candidates enter reversed, as in FIT: ties fall to the larger consequent id.
__global__ void rules_epilogue_kernel(NbChunk C, NbRules U, const uint64_t* __restrict__ ukey,
                                      const uint32_t* __restrict__ runs, const size_t* __restrict__ n_runs,
                                      const double* __restrict__ csum, uint64_t* __restrict__ skey,
                                      uint32_t* __restrict__ payload) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.T) return;
  const int64_t n = (int64_t)*n_runs;
  uint64_t sk = ~0ull;
  uint32_t pl = NB_PAD;
  if (i < n) {
    const int64_t sg = n - 1 - i;
    const uint64_t key = ukey[sg];
    const int64_t row = (int64_t)(key >> C.jbits);
    const int64_t j = (int64_t)(key & ((1ull << C.jbits) - 1));
    if (row < C.rows) {
      const double A = U.item_rel[C.q0 + row], Cr = U.item_rel[j];
      if ((int64_t)runs[sg] >= U.min_pair_count && A != 0.0 && Cr != 0.0) {
        sk = ~f64_order_key(rules_lift(csum[sg], A, Cr, U.n) + 0.0);   // -0.0 and +0.0 are one value
        pl = (uint32_t)sg;
      }
    }
  }
  skey[i] = sk;
  payload[i] = pl;
}
__global__ void rules_write_kernel(NbChunk C, NbRules U, const uint64_t* __restrict__ ukey, const double* __restrict__ csum,
                                   const uint32_t* __restrict__ row_key, const uint32_t* __restrict__ payload,
                                   const int64_t* __restrict__ row_start, int32_t k, int32_t* __restrict__ ids,
                                   double* __restrict__ confidence, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C.T) return;
  const int64_t row = row_key[i];
  if (row >= C.rows) return;
  const int64_t first = row_start[row];
  const int64_t rank = i - first;
  if (rank >= k) return;
  const uint32_t sg = payload[i];
  const int64_t o = (C.q0 + row) * k + rank;
  const int64_t j = (int64_t)(ukey[sg] & ((1ull << C.jbits) - 1));
  const double p = csum[sg], A = U.item_rel[C.q0 + row], Cr = U.item_rel[j];
  ids[o] = (int32_t)j;
  confidence[o] = rules_confidence(p, A);
  U.lift[o] = rules_lift(p, A, Cr, U.n);
  U.gain[o] = rules_gain(p, A, Cr, U.n);
  if (rank == 0) {
    const int64_t n = row_start[row + 1] - first;
    count[C.q0 + row] = (int32_t)(n < k ? n : k);
  }
}

static inline int64_t nb_cap(int64_t max_tuples, int64_t largest_row) {
  const int64_t c = max_tuples > largest_row ? max_tuples : largest_row;
  return c > 1 ? c : 1;
}

extern "C" int64_t cqlrec_neighbour_topk_ws_bytes(int64_t n_q, int64_t n_cols, int64_t max_tuples, int64_t largest_row,
                                                  int32_t k) {
  if (n_q < 0 || n_q >= NB_MAX || n_cols < 0 || n_cols >= NB_MAX || max_tuples < 1 || largest_row < 0 || k < 1 ||
      k > CQLREC_NEIGHBOUR_MAX_K)
    return 0;
  const int64_t cap = nb_cap(max_tuples, largest_row);
  if (cap >= NB_MAX) return 0;
  return 4 * cql_align256(cap * 8) + 6 * cql_align256(cap * 4) + cql_align256((n_q + 2) * 8) + 256 + cql_sort_temp_cap(cap) +
         256;
}

// the two CSR matrices of a call, the count pass's prefixes and how the query rows are cut
struct NbProduct {
  const int64_t* l_off;
  const int32_t* l_col;
  const double* l_val;
  const int64_t* r_off;
  const int32_t* r_col;
  const double* r_val;
  const int64_t *entry_prefix, *row_prefix_host;
  int64_t n_q, n_cols, max_tuples, largest_row;
  int32_t k;
};

// the host-side checks of the row prefix that both entry points make before any launch
static int nb_check_prefix(const char* what, const NbProduct& P) {
  CQL_REQUIRE(P.row_prefix_host[0] == 0 && P.row_prefix_host[P.n_q] >= 0, "%s: the row prefix does not start at 0", what);
  for (int64_t q = 0; q < P.n_q; ++q) {
    const int64_t mine = P.row_prefix_host[q + 1] - P.row_prefix_host[q];
    CQL_REQUIRE(mine >= 0 && mine <= P.largest_row, "%s: row %lld expands to %lld tuples, largest_row is %lld", what,
                (long long)q, (long long)mine, (long long)P.largest_row);
  }
  return CQLREC_OK;
}

// The chunk loop of cqlrec_neighbour_topk and cqlrec_rules_topk, after the outputs are filled: expand, sort, reduce,
// select, write.  U == nullptr: E's epilogue, one value plane; otherwise the rules epilogue (min instead of the product,
// j == q dropped in the expansion, three planes).
static int nb_chunks(const char* what, const NbProduct& P, const NbEpilogue& E, const NbRules* U, void* ws, int32_t* ids,
                     double* vals, int32_t* count, hipStream_t s) {
  const dim3 block(256);
  const int64_t n_q = P.n_q, max_tuples = P.max_tuples;
  const int64_t* row_prefix_host = P.row_prefix_host;
  const int64_t cap = nb_cap(max_tuples, P.largest_row);
  char* p = (char*)ws;
  uint64_t* A8 = (uint64_t*)p;      p += cql_align256(cap * 8);
  uint64_t* B8 = (uint64_t*)p;      p += cql_align256(cap * 8);
  double* C8 = (double*)p;          p += cql_align256(cap * 8);
  double* D8 = (double*)p;          p += cql_align256(cap * 8);
  uint32_t* seg_off = (uint32_t*)p; p += cql_align256(cap * 4);
  uint32_t* runs = (uint32_t*)p;    p += cql_align256(cap * 4);
  uint32_t* F4 = (uint32_t*)p;      p += cql_align256(cap * 4);
  uint32_t* G4 = (uint32_t*)p;      p += cql_align256(cap * 4);
  uint32_t* H4 = (uint32_t*)p;      p += cql_align256(cap * 4);
  uint32_t* I4 = (uint32_t*)p;      p += cql_align256(cap * 4);
  int64_t* row_start = (int64_t*)p; p += cql_align256((n_q + 2) * 8);
  size_t* n_runs = (size_t*)p;
  uint32_t* n_long = (uint32_t*)(p + 8);
  p += 256;
  void* temp = p;
  const size_t temp_cap = (size_t)cql_sort_temp_cap(cap);

  const unsigned jbits = cql_bits_for(P.n_cols);
  int64_t q0 = 0;
  while (q0 < n_q) {
    int64_t q1 = q0 + 1;
    while (q1 < n_q && row_prefix_host[q1 + 1] - row_prefix_host[q0] <= max_tuples) ++q1;
    NbChunk C;
    C.q0 = q0;
    C.rows = q1 - q0;
    C.g0 = row_prefix_host[q0];
    C.T = row_prefix_host[q1] - C.g0;
    C.jbits = jbits;
    q0 = q1;
    if (C.T == 0) continue;
    const int64_t T = C.T;
    const dim3 grid(cql_ceil_div(T, 256));
    const unsigned qbits = cql_bits_for(C.rows + 1);         // the row past the chunk is representable
    int rc;
    // expand: (A8, C8); sort: (B8, D8)
    if (U)
      hipLaunchKernelGGL(neighbour_expand_kernel<true>, grid, block, 0, s, C, P.l_off, P.l_col, P.l_val, P.r_off, P.r_col,
                         P.r_val, P.entry_prefix, P.n_cols, A8, C8);
    else
      hipLaunchKernelGGL(neighbour_expand_kernel<false>, grid, block, 0, s, C, P.l_off, P.l_col, P.l_val, P.r_off, P.r_col,
                         P.r_val, P.entry_prefix, P.n_cols, A8, C8);
    if ((rc = cql_sort_pairs(what, temp, temp_cap, A8, B8, C8, D8, T, jbits + qbits, s)) != CQLREC_OK) return rc;
    // reduce: the distinct keys (A8), their run lengths and first positions, their sums (C8)
    if ((rc = cql_run_length_encode(what, temp, temp_cap, B8, T, A8, runs, n_runs, s)) != CQLREC_OK) return rc;
    if ((rc = cql_exclusive_scan(what, temp, temp_cap, runs, seg_off, 0u, T, s)) != CQLREC_OK) return rc;
    CQL_MEMSET(n_long, 0, 4, s, what);
    hipLaunchKernelGGL(neighbour_sum_short_kernel, grid, block, 0, s, D8, seg_off, runs, n_runs, C8, H4, n_long);
    const int long_blocks = cql_ceil_div(T / NB_SHORT + 1, 4) < 2048 ? cql_ceil_div(T / NB_SHORT + 1, 4) : 2048;
    hipLaunchKernelGGL(neighbour_sum_long_kernel, dim3(long_blocks), block, 0, s, D8, seg_off, runs, H4, n_long, C8);
    // select: by value (B8, F4) -> (D8 as keys, G4), then by row (H4, G4) -> (I4, F4)
    if (U)
      hipLaunchKernelGGL(rules_epilogue_kernel, grid, block, 0, s, C, *U, A8, runs, n_runs, C8, B8, F4);
    else
      hipLaunchKernelGGL(neighbour_epilogue_kernel, grid, block, 0, s, C, E, A8, n_runs, C8, B8, F4);
    if ((rc = cql_sort_pairs(what, temp, temp_cap, B8, (uint64_t*)D8, F4, G4, T, 64, s)) != CQLREC_OK) return rc;
    hipLaunchKernelGGL(neighbour_row_key_kernel, grid, block, 0, s, C, A8, G4, H4);
    if ((rc = cql_sort_pairs(what, temp, temp_cap, H4, I4, G4, F4, T, qbits, s)) != CQLREC_OK) return rc;
    // row_start[g] = the first sorted position whose row is >= g, for g in [0, rows + 1]
    cql_segment_bounds(CqlGroupOfKey<uint32_t>{I4}, T, C.rows + 1, row_start, nullptr, s);
    if (U)
      hipLaunchKernelGGL(rules_write_kernel, grid, block, 0, s, C, *U, A8, C8, I4, F4, row_start, P.k, ids, vals, count);
    else
      hipLaunchKernelGGL(neighbour_write_kernel, grid, block, 0, s, C, A8, C8, I4, F4, row_start, P.k, ids, vals, count);
    CQL_LAUNCH_CHECK(what);
  }
  return CQLREC_OK;
}

extern "C" int cqlrec_neighbour_topk(int32_t mode, const int64_t* l_off, const int32_t* l_col, const double* l_val,
                                     int64_t n_q, int64_t nnz_l, const int64_t* r_off, const int32_t* r_col,
                                     const double* r_val, int64_t n_mid, int64_t n_cols, const int64_t* entry_prefix,
                                     const int64_t* row_prefix_host, int64_t max_tuples, int64_t largest_row, int32_t k,
                                     const double* norm_q, const double* norm_j, double shrink, const uint8_t* mask,
                                     const int64_t* seen_off, const int32_t* seen_col, void* ws, int64_t ws_bytes,
                                     int32_t* ids, double* vals, int32_t* count, cqlrec_stream stream) {
  const char* what = "neighbour_topk";
  CQL_REQUIRE(mode == CQLREC_NEIGHBOUR_FIT || mode == CQLREC_NEIGHBOUR_PREDICT, "neighbour_topk: unknown mode %d", mode);
  CQL_REQUIRE(n_q >= 0 && n_q < NB_MAX && nnz_l >= 0 && nnz_l < NB_MAX && n_mid >= 0 && n_mid < NB_MAX && n_cols >= 0 &&
                  n_cols < NB_MAX,
              "neighbour_topk: n_q=%lld nnz_l=%lld n_mid=%lld n_cols=%lld out of range", (long long)n_q, (long long)nnz_l,
              (long long)n_mid, (long long)n_cols);
  CQL_REQUIRE(k >= 1 && k <= CQLREC_NEIGHBOUR_MAX_K, "neighbour_topk: k=%d out of range (1..%d)", k,
              CQLREC_NEIGHBOUR_MAX_K);
  CQL_REQUIRE(max_tuples >= 1 && largest_row >= 0 && nb_cap(max_tuples, largest_row) < NB_MAX,
              "neighbour_topk: max_tuples=%lld largest_row=%lld out of range (a chunk holds fewer than 2^31 tuples)",
              (long long)max_tuples, (long long)largest_row);
  CQL_REQUIRE(n_q * (int64_t)k < (1ll << 38), "neighbour_topk: n_q * k = %lld is beyond 2^38", (long long)(n_q * (int64_t)k));
  if (n_q == 0) return CQLREC_OK;
  CQL_REQUIRE(ids && vals && count && row_prefix_host, "neighbour_topk: NULL pointer");
  const NbProduct P = {l_off, l_col, l_val, r_off, r_col, r_val, entry_prefix, row_prefix_host, n_q, n_cols, max_tuples,
                       largest_row, k};
  const int rc = nb_check_prefix(what, P);
  if (rc != CQLREC_OK) return rc;
  const int64_t total = row_prefix_host[n_q];
  CQL_REQUIRE(total == 0 || (l_off && l_col && l_val && r_off && r_col && r_val && entry_prefix && ws),
              "neighbour_topk: NULL pointer");
  CQL_REQUIRE(mode != CQLREC_NEIGHBOUR_FIT || total == 0 || (norm_q && norm_j), "neighbour_topk: FIT needs the norms (NULL pointer)");
  CQL_REQUIRE((seen_off == nullptr) == (seen_col == nullptr) || total == 0,
              "neighbour_topk: the seen lists need offsets and columns (NULL pointer)");
  CQL_REQUIRE(total == 0 || ws_bytes >= cqlrec_neighbour_topk_ws_bytes(n_q, n_cols, max_tuples, largest_row, k),
              "neighbour_topk: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(neighbour_fill_kernel, dim3(cql_ceil_div(n_q * (int64_t)k, 256)), dim3(256), 0, s, n_q * (int64_t)k, ids,
                     vals);
  CQL_MEMSET(count, 0, (size_t)n_q * 4, s, what);
  if (total == 0) {
    CQL_LAUNCH_CHECK(what);
    return CQLREC_OK;
  }
  NbEpilogue E = {};
  E.mode = mode;
  E.norm_q = norm_q;
  E.norm_j = norm_j;
  E.shrink = shrink;
  E.mask = mask;
  E.seen_off = seen_off;
  E.seen_col = seen_col;
  return nb_chunks(what, P, E, nullptr, ws, ids, vals, count, s);
}

// =============================================================================================================
// f10  association rules: the distinct rows of the log, and the rules epilogue on the engine above
// =============================================================================================================
// keep[perm[i]] = 1 for the first position of every distinct (session, item[, relevance]) in an ordering that brings equal
// triples together; -0.0 and +0.0 are one relevance
__global__ void rules_mark_kernel(const int32_t* __restrict__ session, const int32_t* __restrict__ item,
                                  const double* __restrict__ relevance, const int32_t* __restrict__ perm, int64_t n,
                                  uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = perm[i];
  if (r < 0 || r >= n) return;                       // no permutation of the rows: nothing is written for this position
  uint8_t first = 1;
  if (i > 0) {
    const int64_t q = perm[i - 1];
    if (q >= 0 && q < n)
      first = session[q] != session[r] || item[q] != item[r] || (relevance && !(relevance[q] == relevance[r]));
  }
  keep[r] = first;
}

extern "C" int cqlrec_rules_distinct(const int32_t* session, const int32_t* item, const double* relevance,
                                     const int32_t* perm, int64_t n_rows, uint8_t* keep, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < NB_MAX, "rules_distinct: n_rows=%lld out of range", (long long)n_rows);
  if (n_rows == 0) return CQLREC_OK;
  CQL_REQUIRE(session && item && perm && keep, "rules_distinct: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(keep, 0, (size_t)n_rows, s, "rules_distinct");
  hipLaunchKernelGGL(rules_mark_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, session, item, relevance, perm,
                     n_rows, keep);
  CQL_LAUNCH_CHECK("rules_distinct");
  return CQLREC_OK;
}

extern "C" int64_t cqlrec_rules_topk_ws_bytes(int64_t n_items, int64_t max_tuples, int64_t largest_row, int32_t k) {
  return cqlrec_neighbour_topk_ws_bytes(n_items, n_items, max_tuples, largest_row, k);
}

extern "C" int cqlrec_rules_topk(const int64_t* l_off, const int32_t* l_col, const double* l_val, int64_t n_items,
                                 int64_t nnz_l, const int64_t* r_off, const int32_t* r_col, const double* r_val,
                                 int64_t n_sessions, const int64_t* entry_prefix, const int64_t* row_prefix_host,
                                 int64_t max_tuples, int64_t largest_row, int32_t k, int64_t num_sessions,
                                 int64_t min_pair_count, void* ws, int64_t ws_bytes, int32_t* ids, double* confidence,
                                 double* lift, double* confidence_gain, int32_t* count, double* item_relevance,
                                 cqlrec_stream stream) {
  const char* what = "rules_topk";
  CQL_REQUIRE(n_items >= 0 && n_items < NB_MAX && nnz_l >= 0 && nnz_l < NB_MAX && n_sessions >= 0 && n_sessions < NB_MAX,
              "rules_topk: n_items=%lld nnz_l=%lld n_sessions=%lld out of range", (long long)n_items, (long long)nnz_l,
              (long long)n_sessions);
  CQL_REQUIRE(k >= 1 && k <= CQLREC_NEIGHBOUR_MAX_K, "rules_topk: k=%d out of range (1..%d)", k, CQLREC_NEIGHBOUR_MAX_K);
  CQL_REQUIRE(max_tuples >= 1 && largest_row >= 0 && nb_cap(max_tuples, largest_row) < NB_MAX,
              "rules_topk: max_tuples=%lld largest_row=%lld out of range (a chunk holds fewer than 2^31 tuples)",
              (long long)max_tuples, (long long)largest_row);
  CQL_REQUIRE(num_sessions >= 0 && num_sessions <= n_sessions, "rules_topk: num_sessions=%lld out of range (0..%lld)",
              (long long)num_sessions, (long long)n_sessions);
  CQL_REQUIRE(n_items * (int64_t)k < (1ll << 38), "rules_topk: n_items * k = %lld is beyond 2^38",
              (long long)(n_items * (int64_t)k));
  if (n_items == 0) return CQLREC_OK;
  CQL_REQUIRE(ids && confidence && lift && confidence_gain && count && item_relevance && row_prefix_host && l_off,
              "rules_topk: NULL pointer");
  const NbProduct P = {l_off, l_col, l_val, r_off, r_col, r_val, entry_prefix, row_prefix_host, n_items, n_items, max_tuples,
                       largest_row, k};
  const int rc = nb_check_prefix(what, P);
  if (rc != CQLREC_OK) return rc;
  const int64_t total = row_prefix_host[n_items];
  CQL_REQUIRE(nnz_l == 0 || l_val, "rules_topk: NULL pointer");
  CQL_REQUIRE(total == 0 || (l_col && r_off && r_col && r_val && entry_prefix && ws), "rules_topk: NULL pointer");
  CQL_REQUIRE(total == 0 || ws_bytes >= cqlrec_rules_topk_ws_bytes(n_items, max_tuples, largest_row, k),
              "rules_topk: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int64_t cells = n_items * (int64_t)k;
  hipLaunchKernelGGL(neighbour_fill_kernel, dim3(cql_ceil_div(cells, 256)), dim3(256), 0, s, cells, ids, confidence);
  CQL_MEMSET(lift, 0, (size_t)cells * 8, s, what);
  CQL_MEMSET(confidence_gain, 0, (size_t)cells * 8, s, what);
  CQL_MEMSET(count, 0, (size_t)n_items * 4, s, what);
  hipLaunchKernelGGL(rules_item_relevance_kernel, dim3(cql_ceil_div(n_items, 4)), dim3(256), 0, s, l_off, l_val, n_items,
                     item_relevance);
  if (total == 0) {
    CQL_LAUNCH_CHECK(what);
    return CQLREC_OK;
  }
  NbRules U;
  U.item_rel = item_relevance;
  U.n = (double)num_sessions;
  U.min_pair_count = min_pair_count;
  U.lift = lift;
  U.gain = confidence_gain;
  return nb_chunks(what, P, NbEpilogue{}, &U, ws, ids, confidence, count, s);
}

// =============================================================================================================
// pair scores
// =============================================================================================================
__global__ void neighbour_pair_scores_kernel(const int32_t* __restrict__ pair_user, const int32_t* __restrict__ pair_item,
                                             int64_t n_pairs, const int64_t* __restrict__ h_off,
                                             const int32_t* __restrict__ h_item, int64_t n_users,
                                             const int64_t* __restrict__ s_off, const int32_t* __restrict__ s_col,
                                             const double* __restrict__ s_val, int64_t n_s_rows,
                                             double* __restrict__ score, uint8_t* __restrict__ present) {
  const int64_t pr = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pr >= n_pairs) return;
  const int64_t u = pair_user[pr], j = pair_item[pr];
  double acc = 0.0;
  uint8_t any = 0;
  if (u >= 0 && u < n_users) {
    const int64_t hb = h_off[u + 1];
    for (int64_t h = h_off[u]; h < hb; ++h) {
      const int64_t i = h_item[h];
      if (i < 0 || i >= n_s_rows) continue;
      const int64_t end = s_off[i + 1];
      int64_t lo = s_off[i], hi = end;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)s_col[mid] < j) lo = mid + 1; else hi = mid;
      }
      if (lo < end && (int64_t)s_col[lo] == j) {
        acc += s_val[lo];
        any = 1;
      }
    }
  }
  score[pr] = acc;
  present[pr] = any;
}

extern "C" int cqlrec_neighbour_pair_scores(const int32_t* pair_user, const int32_t* pair_item, int64_t n_pairs,
                                            const int64_t* h_off, const int32_t* h_item, int64_t n_users,
                                            const int64_t* s_off, const int32_t* s_col, const double* s_val,
                                            int64_t n_s_rows, double* score, uint8_t* present, cqlrec_stream stream) {
  CQL_REQUIRE(n_pairs >= 0 && n_pairs < NB_MAX && n_users >= 0 && n_users < NB_MAX && n_s_rows >= 0 && n_s_rows < NB_MAX,
              "neighbour_pair_scores: n_pairs=%lld n_users=%lld n_s_rows=%lld out of range", (long long)n_pairs,
              (long long)n_users, (long long)n_s_rows);
  if (n_pairs == 0) return CQLREC_OK;
  CQL_REQUIRE(pair_user && pair_item && score && present && (n_users == 0 || h_off) && (n_s_rows == 0 || s_off),
              "neighbour_pair_scores: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(neighbour_pair_scores_kernel, dim3(cql_ceil_div(n_pairs, 256)), dim3(256), 0, s, pair_user, pair_item,
                     n_pairs, h_off, h_item, n_users, s_off, s_col, s_val, n_s_rows, score, present);
  CQL_LAUNCH_CHECK("neighbour_pair_scores");
  return CQLREC_OK;
}
