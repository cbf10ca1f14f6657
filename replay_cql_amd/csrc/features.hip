// f7  history-based features on the device (replay/history_based_fp.py): sorted segments per group, fp64 segment
// statistics (count, mean, sample std, three quantile picks), a segmented mean of a per-row expression, distinct-key
// counts, (entity, category) pair counts, and the fused kernel that writes the feature block of a frame of pairs.
// The rules of f5 / f6 hold: integer atomics only, no floating-point atomics, the same input gives the same bytes.
// Built with -ffp-contract=off: the quantile rank p * n is one IEEE double multiply, and every expression below is
// evaluated as written.
//
// A floating-point sum over a segment is formed in an order fixed by POSITION inside the segment: the segment is cut
// into pieces of FEAT_SUB consecutive sorted rows, counted from the segment's first row; one wave sums a piece (lane l
// takes the rows l, l + 64, ... in that order, then a butterfly over the lanes), and one wave per group sums the
// group's pieces the same way.  No thread walks more than FEAT_SUB / 64 rows, nor more than n_rows / (64 * FEAT_SUB)
// pieces (< 2^15 for n_rows < 2^31), whatever the group sizes are.
#include "segment_common.h"

static const int64_t FEAT_MAX_ROWS = 1ll << 31;
static const int FEAT_SUB = 1024;

// =============================================================================================================
// day = floor(key / unit)
// =============================================================================================================
__global__ void features_day_kernel(const int64_t* __restrict__ key, int64_t n, int64_t unit, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t k = key[i];
  int64_t q = k / unit;
  if (k % unit < 0) --q;                     // C division truncates: step down to the floor
  out[i] = q;
}

extern "C" int cqlrec_features_day(const int64_t* key, int64_t n, int64_t unit, int64_t* day, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 0 && n < FEAT_MAX_ROWS && unit > 0, "features_day: n=%lld unit=%lld out of range", (long long)n,
              (long long)unit);
  if (n == 0) return CQLREC_OK;
  CQL_REQUIRE(key && day, "features_day: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(features_day_kernel, dim3(cql_ceil_div(n, 256)), dim3(256), 0, s, key, n, unit, day);
  CQL_LAUNCH_CHECK("features_day");
  return CQLREC_OK;
}

// =============================================================================================================
// segments: rows ordered by (group, key, input row index) ascending
// =============================================================================================================
__global__ void features_sort_key_kernel(const int64_t* __restrict__ key, int64_t n, uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint64_t)key[i] ^ (1ull << 63);
}

extern "C" int64_t cqlrec_features_segments_ws_bytes(int64_t n_rows, int64_t n_groups) {
  if (n_rows < 0 || n_groups < 0) return 0;
  return CqlPermSort::bytes(n_rows) + cql_sort_temp_cap(n_rows) + 256;
}

extern "C" int cqlrec_features_segments(const int32_t* group, const int64_t* key, int64_t n_rows, int64_t n_groups,
                                        void* ws, int64_t ws_bytes, int32_t* perm, int64_t* offsets,
                                        cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < FEAT_MAX_ROWS && n_groups > 0 && n_groups < FEAT_MAX_ROWS,
              "features_segments: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(offsets, "features_segments: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(offsets, 0, (size_t)(n_groups + 1) * 8, s, "features_segments");
    return CQLREC_OK;
  }
  CQL_REQUIRE(group && ws && perm, "features_segments: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_features_segments_ws_bytes(n_rows, n_groups), "features_segments: workspace too small");
  char* p = (char*)ws;
  CqlPermSort ps(p, n_rows, s);
  ps.temp = p;
  int rc;
  cql_iota(ps.perm, n_rows, false, s);
  if (key) {  // least significant: the key, over all 64 bits (the permutation is still the identity)
    hipLaunchKernelGGL(features_sort_key_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, key, n_rows,
                       ps.keys<uint64_t>());
    if ((rc = ps.pass<uint64_t>("features_segments", 64)) != CQLREC_OK) return rc;
  }
  cql_group_key(group, ps.perm, n_rows, ps.keys<uint32_t>(), s);
  if ((rc = ps.pass<uint32_t>("features_segments", cql_bits_for(n_groups), (uint32_t*)perm)) != CQLREC_OK) return rc;
  cql_segment_bounds(CqlGroupOfPerm{group, ps.perm}, n_rows, n_groups, offsets, nullptr, s);
  CQL_LAUNCH_CHECK("features_segments");
  return CQLREC_OK;
}

// =============================================================================================================
// segmented sums in an order fixed by position, and what is made of them
// =============================================================================================================
enum { FEAT_EXPR_VALUE = 100, FEAT_EXPR_SQDEV = 101 };   // internal rules next to the public CQLREC_FEATURES_MEAN_*

struct FeatExpr {
  int rule;
  const double* value;    // [n_rows]
  const int32_t* other;   // [n_rows] the id of the other entity
  const double* tab_a;    // indexed other * stride
  const double* tab_b;
  int64_t stride;
  const double* center;   // indexed group * cstride (SQDEV)
  int64_t cstride;
  double lo, span;
};

__device__ __forceinline__ double feat_expr(const FeatExpr& E, int64_t row, int64_t g) {
  switch (E.rule) {
    case FEAT_EXPR_VALUE:
      return E.value[row];
    case FEAT_EXPR_SQDEV: {
      const double d = E.value[row] - E.center[g * E.cstride];
      return d * d;
    }
    case CQLREC_FEATURES_MEAN_GATHER:
      return E.tab_a[(int64_t)E.other[row] * E.stride];
    case CQLREC_FEATURES_MEAN_ABNORMALITY:
      return fabs(E.value[row] - E.tab_a[(int64_t)E.other[row] * E.stride]);
    default: {  // CQLREC_FEATURES_MEAN_ABNORMALITY_CR
      const int64_t o = (int64_t)E.other[row] * E.stride;
      const double a = fabs(E.value[row] - E.tab_a[o]);
      const double c = 1.0 - (E.tab_b[o] - E.lo) / E.span;
      const double x = a * c;
      return x * x;
    }
  }
}

__device__ __forceinline__ double feat_wave_sum(double acc) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
  return acc;
}

__global__ void features_nsub_kernel(const int64_t* __restrict__ offsets, int64_t n_groups, int64_t* __restrict__ nsub) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n_groups) return;
  nsub[g] = g < n_groups ? (offsets[g + 1] - offsets[g] + FEAT_SUB - 1) / FEAT_SUB : 0;
}

// one wave per piece; piece w belongs to the group g with sub_off[g] <= w < sub_off[g + 1]
__global__ __launch_bounds__(256) void features_partial_kernel(FeatExpr E, const int32_t* __restrict__ perm,
                                                               const int64_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ sub_off, int64_t n_groups,
                                                               double* __restrict__ partial) {
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= sub_off[n_groups]) return;
  int64_t lo = 0, hi = n_groups;             // the first index in [0, n_groups] with sub_off[index] > w
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sub_off[mid] > w) hi = mid; else lo = mid + 1;
  }
  const int64_t g = lo - 1;
  const int64_t a = offsets[g] + (w - sub_off[g]) * FEAT_SUB;
  const int64_t end = offsets[g + 1];
  const int64_t b = a + FEAT_SUB < end ? a + FEAT_SUB : end;
  double acc = 0.0;
  for (int64_t p = a + lane; p < b; p += 64) acc += feat_expr(E, perm[p], g);
  acc = feat_wave_sum(acc);
  if (lane == 0) partial[w] = acc;
}

// one wave per group: the sum of its pieces, then the statistic.  finish 0: sum / n; finish 1: sqrt(sum / (n - 1)), 0 for
// n = 1.  A group without rows gets 0.  count_out (or NULL) receives n as a double, with out's stride.
__global__ __launch_bounds__(256) void features_combine_kernel(const double* __restrict__ partial,
                                                               const int64_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ sub_off, int64_t n_groups,
                                                               int finish, double* __restrict__ out, int64_t ostride,
                                                               double* __restrict__ count_out) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (g >= n_groups) return;
  const int64_t a = sub_off[g], b = sub_off[g + 1];
  double acc = 0.0;
  for (int64_t p = a + lane; p < b; p += 64) acc += partial[p];
  acc = feat_wave_sum(acc);
  if (lane != 0) return;
  const int64_t n = offsets[g + 1] - offsets[g];
  double r = 0.0;
  if (n > 0) {
    if (finish == 0) r = acc / (double)n;
    else if (n > 1) r = sqrt(acc / (double)(n - 1));
  }
  out[g * ostride] = r;
  if (count_out) count_out[g * ostride] = (double)n;
}

__global__ void features_pick_kernel(const int32_t* __restrict__ perm, const int64_t* __restrict__ offsets,
                                     const double* __restrict__ value, int64_t n_groups, double* __restrict__ out,
                                     int64_t ostride) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const int64_t a = offsets[g], n = offsets[g + 1] - a;
  const double ps[3] = {0.05, 0.5, 0.95};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double r = 0.0;
    if (n > 0) {
      int64_t k = (int64_t)ceil(ps[j] * (double)n);      // 1-based rank
      k = k < 1 ? 1 : (k > n ? n : k);
      r = value[perm[a + k - 1]];
    }
    out[g * ostride + j] = r;
  }
}

static inline int64_t feat_max_pieces(int64_t n_rows, int64_t n_groups) { return n_rows / FEAT_SUB + n_groups; }

static int64_t feat_sum_ws_bytes(int64_t n_rows, int64_t n_groups) {
  return 2 * cql_align256((n_groups + 1) * 8) + cql_align256(feat_max_pieces(n_rows, n_groups) * 8) +
         cql_scan_temp_cap(n_groups + 1) + 256;
}

struct FeatSumWs {
  int64_t *nsub, *sub_off;
  double* partial;
  void* temp;
};
static FeatSumWs feat_sum_carve(void* ws, int64_t n_rows, int64_t n_groups) {
  FeatSumWs w;
  char* p = (char*)ws;
  w.nsub = (int64_t*)p;     p += cql_align256((n_groups + 1) * 8);
  w.sub_off = (int64_t*)p;  p += cql_align256((n_groups + 1) * 8);
  w.partial = (double*)p;   p += cql_align256(feat_max_pieces(n_rows, n_groups) * 8);
  w.temp = p;
  return w;
}
// sub_off [n_groups + 1]: the first piece of every group, and the number of pieces at the end
static int feat_pieces(const int64_t* offsets, int64_t n_groups, const FeatSumWs& w, hipStream_t s, const char* what) {
  hipLaunchKernelGGL(features_nsub_kernel, dim3(cql_ceil_div(n_groups + 1, 256)), dim3(256), 0, s, offsets, n_groups,
                     w.nsub);
  return cql_exclusive_scan(what, w.temp, (size_t)cql_scan_temp_cap(n_groups + 1), w.nsub, w.sub_off, (int64_t)0, n_groups + 1,
                            s);
}
static void feat_sum(const FeatExpr& E, const int32_t* perm, const int64_t* offsets, int64_t n_rows, int64_t n_groups,
                     const FeatSumWs& w, int finish, double* out, int64_t ostride, double* count_out, hipStream_t s) {
  hipLaunchKernelGGL(features_partial_kernel, dim3(cql_ceil_div(feat_max_pieces(n_rows, n_groups), 4)), dim3(256), 0, s, E,
                     perm, offsets, w.sub_off, n_groups, w.partial);
  hipLaunchKernelGGL(features_combine_kernel, dim3(cql_ceil_div(n_groups, 4)), dim3(256), 0, s, w.partial, offsets,
                     w.sub_off, n_groups, finish, out, ostride, count_out);
}

extern "C" int64_t cqlrec_features_segment_stats_ws_bytes(int64_t n_rows, int64_t n_groups) {
  if (n_rows < 0 || n_groups < 0) return 0;
  return feat_sum_ws_bytes(n_rows, n_groups);
}

extern "C" int cqlrec_features_segment_stats(const int32_t* perm, const int64_t* offsets, const double* value,
                                             int64_t n_rows, int64_t n_groups, void* ws, int64_t ws_bytes, double* out,
                                             cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < FEAT_MAX_ROWS && n_groups > 0 && n_groups < FEAT_MAX_ROWS,
              "features_segment_stats: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(out, "features_segment_stats: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(out, 0, (size_t)n_groups * CQLREC_FEATURES_STATS * 8, s, "features_segment_stats");
    return CQLREC_OK;
  }
  CQL_REQUIRE(perm && offsets && value && ws, "features_segment_stats: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_features_segment_stats_ws_bytes(n_rows, n_groups),
              "features_segment_stats: workspace too small");
  const FeatSumWs w = feat_sum_carve(ws, n_rows, n_groups);
  const int rc = feat_pieces(offsets, n_groups, w, s, "features_segment_stats");
  if (rc != CQLREC_OK) return rc;
  FeatExpr E = {};
  E.rule = FEAT_EXPR_VALUE;
  E.value = value;
  feat_sum(E, perm, offsets, n_rows, n_groups, w, 0, out + 1, CQLREC_FEATURES_STATS, out, s);   // count, mean
  E.rule = FEAT_EXPR_SQDEV;                  // the second pass of the two-pass variance, around the mean just written
  E.center = out + 1;
  E.cstride = CQLREC_FEATURES_STATS;
  feat_sum(E, perm, offsets, n_rows, n_groups, w, 1, out + 2, CQLREC_FEATURES_STATS, nullptr, s);
  hipLaunchKernelGGL(features_pick_kernel, dim3(cql_ceil_div(n_groups, 256)), dim3(256), 0, s, perm, offsets, value,
                     n_groups, out + 3, (int64_t)CQLREC_FEATURES_STATS);
  CQL_LAUNCH_CHECK("features_segment_stats");
  return CQLREC_OK;
}

extern "C" int64_t cqlrec_features_segment_mean_ws_bytes(int64_t n_rows, int64_t n_groups) {
  if (n_rows < 0 || n_groups < 0) return 0;
  return feat_sum_ws_bytes(n_rows, n_groups);
}

extern "C" int cqlrec_features_segment_mean(int32_t rule, const int32_t* perm, const int64_t* offsets, const double* value,
                                            const int32_t* other, const double* tab_a, const double* tab_b,
                                            int64_t tab_stride, double min_std, double max_std, int64_t n_rows,
                                            int64_t n_groups, void* ws, int64_t ws_bytes, double* out,
                                            cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < FEAT_MAX_ROWS && n_groups > 0 && n_groups < FEAT_MAX_ROWS,
              "features_segment_mean: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(rule >= CQLREC_FEATURES_MEAN_GATHER && rule <= CQLREC_FEATURES_MEAN_ABNORMALITY_CR,
              "features_segment_mean: unknown rule %d", rule);
  CQL_REQUIRE(out, "features_segment_mean: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(out, 0, (size_t)n_groups * 8, s, "features_segment_mean");
    return CQLREC_OK;
  }
  CQL_REQUIRE(perm && offsets && ws && other && tab_a && tab_stride > 0, "features_segment_mean: NULL pointer");
  CQL_REQUIRE(rule == CQLREC_FEATURES_MEAN_GATHER || value, "features_segment_mean: rule %d needs the value column", rule);
  CQL_REQUIRE(rule != CQLREC_FEATURES_MEAN_ABNORMALITY_CR || (tab_b && max_std - min_std > 0.0),
              "features_segment_mean: ABNORMALITY_CR needs the std column and min_std < max_std (%g, %g)", min_std, max_std);
  CQL_REQUIRE(ws_bytes >= cqlrec_features_segment_mean_ws_bytes(n_rows, n_groups),
              "features_segment_mean: workspace too small");
  const FeatSumWs w = feat_sum_carve(ws, n_rows, n_groups);
  const int rc = feat_pieces(offsets, n_groups, w, s, "features_segment_mean");
  if (rc != CQLREC_OK) return rc;
  FeatExpr E = {};
  E.rule = rule;
  E.value = value;
  E.other = other;
  E.tab_a = tab_a;
  E.tab_b = tab_b;
  E.stride = tab_stride;
  E.lo = min_std;
  E.span = max_std - min_std;
  feat_sum(E, perm, offsets, n_rows, n_groups, w, 0, out, 1, nullptr, s);
  CQL_LAUNCH_CHECK("features_segment_mean");
  return CQLREC_OK;
}

// =============================================================================================================
// distinct keys per group, over an ordering by (group, key): the heads of the runs are counted
// =============================================================================================================
__global__ void features_heads_kernel(const int32_t* __restrict__ group, const int32_t* __restrict__ perm,
                                      const int64_t* __restrict__ offsets, const int64_t* __restrict__ key, int64_t n,
                                      int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t r = perm[p];
  const int32_t g = group[r];
  if (p == offsets[g] || key[r] != key[perm[p - 1]]) atomicAdd(&out[g], 1);
}

extern "C" int cqlrec_features_segment_distinct(const int32_t* group, const int32_t* perm, const int64_t* offsets,
                                                const int64_t* key, int64_t n_rows, int64_t n_groups, int32_t* out,
                                                cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < FEAT_MAX_ROWS && n_groups > 0 && n_groups < FEAT_MAX_ROWS,
              "features_segment_distinct: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(out && (n_rows == 0 || (group && perm && offsets && key)), "features_segment_distinct: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(out, 0, (size_t)n_groups * 4, s, "features_segment_distinct");
  if (n_rows == 0) return CQLREC_OK;
  hipLaunchKernelGGL(features_heads_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, group, perm, offsets, key,
                     n_rows, out);
  CQL_LAUNCH_CHECK("features_segment_distinct");
  return CQLREC_OK;
}

// =============================================================================================================
// (entity, category) pair counts: sorted distinct composite keys and the share of the entity's rows each holds
// =============================================================================================================
__global__ void features_pair_key_kernel(const int32_t* __restrict__ entity, const int32_t* __restrict__ other,
                                         const int32_t* __restrict__ code, int64_t n, int64_t n_cat,
                                         int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int64_t)entity[i] * (n_cat + 1) + (int64_t)code[other[i]];
}
// pop[i] = the share of the entity's rows; entity_off[e] = the first distinct key of an entity >= e
__global__ void features_pair_pop_kernel(const int64_t* __restrict__ keys, const uint32_t* __restrict__ runs,
                                         const int64_t* __restrict__ n_out, const int32_t* __restrict__ entity_count,
                                         int64_t n_cat, int64_t n_entity, double* __restrict__ pop,
                                         int64_t* __restrict__ entity_off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t m = *n_out;
  if (i > m) return;
  const int64_t cur = (i < m) ? keys[i] / (n_cat + 1) : n_entity;
  const int64_t prev = (i > 0) ? keys[i - 1] / (n_cat + 1) : -1;
  cql_fill_gap(prev, cur, i, entity_off);
  if (i < m) pop[i] = (double)runs[i] / (double)entity_count[cur];
}

extern "C" int64_t cqlrec_features_pair_counts_ws_bytes(int64_t n_rows) {
  if (n_rows < 0) return 0;
  return 2 * cql_align256(n_rows * 8) + cql_align256(n_rows * 4) + cql_sort_temp_cap(n_rows) + 256;
}

extern "C" int cqlrec_features_pair_counts(const int32_t* entity, const int32_t* other, const int32_t* code,
                                           const int32_t* entity_count, int64_t n_rows, int64_t n_entity, int64_t n_cat,
                                           void* ws, int64_t ws_bytes, int64_t* keys, double* pop, int64_t* entity_off,
                                           int64_t* n_out, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < FEAT_MAX_ROWS && n_entity > 0 && n_entity < FEAT_MAX_ROWS && n_cat >= 0 &&
                  n_cat < FEAT_MAX_ROWS - 1,
              "features_pair_counts: n_rows=%lld n_entity=%lld n_cat=%lld out of range", (long long)n_rows,
              (long long)n_entity, (long long)n_cat);
  CQL_REQUIRE(n_out && entity_off, "features_pair_counts: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(n_out, 0, 8, s, "features_pair_counts");
    CQL_MEMSET(entity_off, 0, (size_t)(n_entity + 1) * 8, s, "features_pair_counts");
    return CQLREC_OK;
  }
  CQL_REQUIRE(entity && other && code && entity_count && ws && keys && pop, "features_pair_counts: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_features_pair_counts_ws_bytes(n_rows), "features_pair_counts: workspace too small");
  char* p = (char*)ws;
  int64_t* raw = (int64_t*)p;     p += cql_align256(n_rows * 8);
  int64_t* sorted = (int64_t*)p;  p += cql_align256(n_rows * 8);
  uint32_t* runs = (uint32_t*)p;  p += cql_align256(n_rows * 4);
  void* temp = p;
  const size_t cap = (size_t)cql_sort_temp_cap(n_rows);
  const unsigned bits = cql_bits_for(n_entity * (n_cat + 1));        // the keys are non-negative and below that product
  hipLaunchKernelGGL(features_pair_key_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, entity, other, code, n_rows,
                     n_cat, raw);
  int rc = cql_sort_keys("features_pair_counts", temp, cap, raw, sorted, n_rows, bits, s);
  if (rc == CQLREC_OK)
    rc = cql_run_length_encode("features_pair_counts", temp, cap, sorted, n_rows, keys, runs, (size_t*)n_out, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(features_pair_pop_kernel, dim3(cql_ceil_div(n_rows + 1, 256)), dim3(256), 0, s, keys, runs, n_out,
                     entity_count, n_cat, n_entity, pop, entity_off);
  CQL_LAUNCH_CHECK("features_pair_counts");
  return CQLREC_OK;
}

// =============================================================================================================
// the feature block of a frame of pairs, in one launch
// =============================================================================================================
struct FeatBlockArgs {
  const int64_t *user, *item;
  int64_t n_pairs;
  const double *utab, *itab;
  const int32_t *ucount, *icount;
  int64_t n_users, n_items;
  int32_t fu, fi, n_cols, n_pop;
  cqlrec_features_pop pop[CQLREC_FEATURES_MAX_POP];
  int8_t kind[CQLREC_FEATURES_MAX_COLS], a[CQLREC_FEATURES_MAX_COLS], b[CQLREC_FEATURES_MAX_COLS];
};

// the popularity of (entity, category of `other`) and whether the pair has none
__device__ __forceinline__ double feat_pop_lookup(const cqlrec_features_pop& P, int64_t pair, int64_t u, int64_t i,
                                                  bool* na) {
  const int64_t e = P.entity_is_item ? i : u, o = P.entity_is_item ? u : i;
  int64_t c = P.n_cat;                       // the null category: an id the features did not list
  if (P.pair_code) c = P.pair_code[pair];
  else if (o >= 0 && o < P.n_code) c = P.code[o];
  *na = true;
  if (e < 0 || e >= P.n_entity || c < 0 || c >= P.n_cat) return 0.0;   // a null never equals a null in a join
  const int64_t v = e * (P.n_cat + 1) + c;
  const int64_t end = P.entity_off[e + 1];
  int64_t lo = P.entity_off[e], hi = end;    // the first j among the entity's keys with keys[j] >= v: at most n_cat + 1 of them
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (P.keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  if (lo >= end || P.keys[lo] != v) return 0.0;
  *na = false;
  return P.pop[lo];
}

// Lanes run across the ELEMENTS of the row-major block: every lane forms 16 consecutive bytes of it (4 floats or
// 2 doubles) and stores them at once, so a wave writes 1 KiB contiguously and reads the table rows of the few pairs it
// covers in contiguous runs.
template <typename T>
__global__ __launch_bounds__(256) void features_block_kernel(FeatBlockArgs A, T* __restrict__ out) {
  constexpr int V = 16 / sizeof(T);
  const int64_t total = A.n_pairs * A.n_cols;
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (e0 >= total) return;
  int64_t pair = e0 / A.n_cols;
  int col = (int)(e0 - pair * A.n_cols);
  int64_t loaded = -1, u = 0, i = 0;
  bool ucold = true, icold = true, pop_na = true;
  int pop_of = -1;
  int64_t pop_pair = -1;
  double pop_value = 0.0;
  T v[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    v[k] = (T)0;
    if (e0 + k >= total) continue;
    if (pair != loaded) {
      loaded = pair;
      u = A.user[pair];
      i = A.item[pair];
      ucold = A.fu == 0 || u < 0 || u >= A.n_users || A.ucount[u] == 0;
      icold = A.fi == 0 || i < 0 || i >= A.n_items || A.icount[i] == 0;
    }
    const int ca = A.a[col], cb = A.b[col];
    double x;
    switch (A.kind[col]) {
      case CQLREC_FEATURES_COL_USER:
        x = ucold ? 0.0 : A.utab[u * A.fu + ca];
        break;
      case CQLREC_FEATURES_COL_ITEM:
        x = icold ? 0.0 : A.itab[i * A.fi + ca];
        break;
      case CQLREC_FEATURES_COL_NA_USER:
        x = ucold ? 1.0 : 0.0;
        break;
      case CQLREC_FEATURES_COL_NA_ITEM:
        x = icold ? 1.0 : 0.0;
        break;
      case CQLREC_FEATURES_COL_DIFF_USER:       // user column a minus item column b, both after the zero fill
        x = (ucold ? 0.0 : A.utab[u * A.fu + ca]) - (icold ? 0.0 : A.itab[i * A.fi + cb]);
        break;
      case CQLREC_FEATURES_COL_DIFF_ITEM:       // item column a minus user column b
        x = (icold ? 0.0 : A.itab[i * A.fi + ca]) - (ucold ? 0.0 : A.utab[u * A.fu + cb]);
        break;
      default:                                  // CQLREC_FEATURES_COL_POP / _POP_NA: one search serves both
        if (pop_of != ca || pop_pair != pair) {
          pop_of = ca;
          pop_pair = pair;
          pop_value = feat_pop_lookup(A.pop[ca], pair, u, i, &pop_na);
        }
        x = A.kind[col] == CQLREC_FEATURES_COL_POP ? pop_value : (pop_na ? 1.0 : 0.0);
        break;
    }
    v[k] = (T)x;
    if (++col == A.n_cols) {
      col = 0;
      ++pair;
    }
  }
  if (e0 + V <= total) {
    if constexpr (V == 4) *(float4*)(out + e0) = make_float4(v[0], v[1], v[2], v[3]);
    else *(double2*)(out + e0) = make_double2(v[0], v[1]);
  } else {
    for (int k = 0; k < V; ++k)
      if (e0 + k < total) out[e0 + k] = v[k];
  }
}

extern "C" int cqlrec_features_block(const int64_t* user_idx, const int64_t* item_idx, int64_t n_pairs, const double* utab,
                                     const int32_t* ucount, int64_t n_users, int32_t fu, const double* itab,
                                     const int32_t* icount, int64_t n_items, int32_t fi, const int32_t* colmap,
                                     int32_t n_cols, const cqlrec_features_pop* pops, int32_t n_pop, int32_t dtype,
                                     void* block, cqlrec_stream stream) {
  CQL_REQUIRE(n_pairs >= 0 && n_pairs < FEAT_MAX_ROWS && n_users >= 0 && n_users < FEAT_MAX_ROWS && n_items >= 0 &&
                  n_items < FEAT_MAX_ROWS,
              "features_block: n_pairs=%lld n_users=%lld n_items=%lld out of range", (long long)n_pairs,
              (long long)n_users, (long long)n_items);
  CQL_REQUIRE(n_cols > 0 && n_cols <= CQLREC_FEATURES_MAX_COLS && fu >= 0 && fu <= CQLREC_FEATURES_MAX_COLS && fi >= 0 &&
                  fi <= CQLREC_FEATURES_MAX_COLS && n_pop >= 0 && n_pop <= CQLREC_FEATURES_MAX_POP,
              "features_block: n_cols=%d fu=%d fi=%d n_pop=%d out of range", n_cols, fu, fi, n_pop);
  CQL_REQUIRE(dtype == CQLREC_FEATURES_F32 || dtype == CQLREC_FEATURES_F64, "features_block: unknown dtype %d", dtype);
  CQL_REQUIRE(colmap && (n_pop == 0 || pops), "features_block: NULL pointer");
  CQL_REQUIRE((fu == 0 || n_users == 0 || (utab && ucount)) && (fi == 0 || n_items == 0 || (itab && icount)),
              "features_block: NULL pointer");
  FeatBlockArgs args = {};
  for (int c = 0; c < n_cols; ++c) {
    const int32_t kind = colmap[3 * c], a = colmap[3 * c + 1], b = colmap[3 * c + 2];
    bool ok;
    switch (kind) {
      case CQLREC_FEATURES_COL_USER:
        ok = a >= 0 && a < fu;
        break;
      case CQLREC_FEATURES_COL_ITEM:
        ok = a >= 0 && a < fi;
        break;
      case CQLREC_FEATURES_COL_NA_USER:
      case CQLREC_FEATURES_COL_NA_ITEM:
        ok = true;
        break;
      case CQLREC_FEATURES_COL_DIFF_USER:
        ok = a >= 0 && a < fu && b >= 0 && b < fi;
        break;
      case CQLREC_FEATURES_COL_DIFF_ITEM:
        ok = a >= 0 && a < fi && b >= 0 && b < fu;
        break;
      case CQLREC_FEATURES_COL_POP:
      case CQLREC_FEATURES_COL_POP_NA:
        ok = a >= 0 && a < n_pop;
        break;
      default:
        ok = false;
        break;
    }
    CQL_REQUIRE(ok, "features_block: column %d: kind %d with (%d, %d) out of range", c, kind, a, b);
    args.kind[c] = (int8_t)kind;
    args.a[c] = (int8_t)a;
    args.b[c] = (int8_t)b;
  }
  for (int q = 0; q < n_pop; ++q) {
    const cqlrec_features_pop& P = pops[q];
    CQL_REQUIRE(P.m >= 0 && P.m < FEAT_MAX_ROWS && P.n_cat >= 0 && P.n_cat < FEAT_MAX_ROWS - 1 && P.n_code >= 0 &&
                    P.n_code < FEAT_MAX_ROWS && P.n_entity >= 0 && P.n_entity < FEAT_MAX_ROWS,
                "features_block: popularity table %d: sizes out of range", q);
    CQL_REQUIRE((P.n_entity == 0 || P.entity_off) && (P.m == 0 || (P.keys && P.pop)) &&
                    (P.n_code == 0 || P.code || P.pair_code),
                "features_block: popularity table %d: NULL pointer", q);
    args.pop[q] = P;
  }
  if (n_pairs == 0) return CQLREC_OK;
  CQL_REQUIRE(user_idx && item_idx && block, "features_block: NULL pointer");
  args.user = user_idx;
  args.item = item_idx;
  args.n_pairs = n_pairs;
  args.utab = utab;
  args.itab = itab;
  args.ucount = ucount;
  args.icount = icount;
  args.n_users = (fu == 0) ? 0 : n_users;
  args.n_items = (fi == 0) ? 0 : n_items;
  args.fu = fu;
  args.fi = fi;
  args.n_cols = n_cols;
  args.n_pop = n_pop;
  hipStream_t s = (hipStream_t)stream;
  const int64_t total = n_pairs * (int64_t)n_cols;
  if (dtype == CQLREC_FEATURES_F32) {
    hipLaunchKernelGGL(features_block_kernel<float>, dim3(cql_ceil_div((total + 3) / 4, 256)), dim3(256), 0, s, args,
                       (float*)block);
  } else {
    hipLaunchKernelGGL(features_block_kernel<double>, dim3(cql_ceil_div((total + 1) / 2, 256)), dim3(256), 0, s, args,
                       (double*)block);
  }
  CQL_LAUNCH_CHECK("features_block");
  return CQLREC_OK;
}
