// f6  log preparation on the device (replay/filters.py, replay/data_preparator.py's Indexer): a ranking inside each
// user with a secondary key, per-group counts and int64 extremes, one row predicate for the six filters, a stable
// compaction, and the Indexer's distinct / lookup / gather.  Integer work; the only atomics are integer ones, so the
// same input gives the same bytes.  The two double expressions (the rating comparison, the float day bound: one add or
// subtract) are single IEEE operations -- the file is built with -ffp-contract=off.
//
// Order inside a user: (key, key2, input row index), ranked DESCENDING as cqlrec_split_rank does -- stable LSD radix
// passes over a row permutation that starts REVERSED (stability then keeps later rows first): key2, then key, then
// user.  The ascending row number is count[u] + 1 - rank.
#include "segment_common.h"

static const int64_t PREPARE_MAX_ROWS = 1ll << 31;

// =============================================================================================================
// rank inside the user under (key desc, key2 desc, row index desc)
// =============================================================================================================
// sort keys of the rows in their current order, for an ASCENDING sort: key2 and key reversed
__global__ void prepare_key2_kernel(const int32_t* __restrict__ key2, const uint32_t* __restrict__ perm, int64_t n,
                                    uint32_t top, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = top - (uint32_t)key2[perm[i]];
}
__global__ void prepare_key_kernel(const int64_t* __restrict__ key, const uint32_t* __restrict__ perm, int64_t n,
                                   uint64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = ~((uint64_t)key[perm[i]] ^ (1ull << 63));
}

extern "C" int64_t cqlrec_prepare_rank_ws_bytes(int64_t n_rows, int64_t n_users) {
  return cql_rank_ws_bytes(n_rows, n_users);
}

extern "C" int cqlrec_prepare_rank(const int32_t* user_idx, const int64_t* key, const int32_t* key2, int64_t n_rows,
                                   int64_t n_users, int64_t n_key2, void* ws, int64_t ws_bytes, int32_t* rank,
                                   int32_t* count, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS && n_users > 0 && n_users < PREPARE_MAX_ROWS,
              "prepare_rank: n_rows=%lld n_users=%lld out of range", (long long)n_rows, (long long)n_users);
  CQL_REQUIRE(!key2 || (n_key2 > 0 && n_key2 < PREPARE_MAX_ROWS), "prepare_rank: n_key2=%lld out of range",
              (long long)n_key2);
  CQL_REQUIRE(count, "prepare_rank: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(count, 0, (size_t)n_users * 4, s, "prepare_rank");
    return CQLREC_OK;
  }
  CQL_REQUIRE(user_idx && key && ws && rank, "prepare_rank: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_rank_ws_bytes(n_rows, n_users), "prepare_rank: workspace too small");
  char* p = (char*)ws;
  CqlPermSort ps(p, n_rows, s);
  int64_t* offsets = (int64_t*)p;  p += cql_align256((n_users + 1) * 8);
  ps.temp = p;
  const dim3 grid(cql_ceil_div(n_rows, 256)), block(256);
  int rc;
  cql_iota(ps.perm, n_rows, true, s);
  if (key2) {  // least significant: key2 descending, over the bits a value below n_key2 can have
    hipLaunchKernelGGL(prepare_key2_kernel, grid, block, 0, s, key2, ps.perm, n_rows, (uint32_t)(n_key2 - 1),
                       ps.keys<uint32_t>());
    if ((rc = ps.pass<uint32_t>("prepare_rank", cql_bits_for(n_key2))) != CQLREC_OK) return rc;
  }
  hipLaunchKernelGGL(prepare_key_kernel, grid, block, 0, s, key, ps.perm, n_rows, ps.keys<uint64_t>());
  if ((rc = ps.pass<uint64_t>("prepare_rank", 64)) != CQLREC_OK) return rc;
  return cql_rank_tail(ps, user_idx, n_users, offsets, rank, count, nullptr, "prepare_rank");
}

// =============================================================================================================
// per-group count, per-group and global int64 min / max
// =============================================================================================================
__global__ void prepare_count_kernel(const int32_t* __restrict__ ids, int64_t n, int32_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&count[ids[i]], 1);
}

extern "C" int cqlrec_prepare_count(const int32_t* ids, int64_t n_rows, int64_t n_groups, int32_t* count,
                                    cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS && n_groups > 0 && n_groups < PREPARE_MAX_ROWS,
              "prepare_count: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(count && (ids || n_rows == 0), "prepare_count: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(count, 0, (size_t)n_groups * 4, s, "prepare_count");
  if (n_rows == 0) return CQLREC_OK;
  hipLaunchKernelGGL(prepare_count_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, ids, n_rows, count);
  CQL_LAUNCH_CHECK("prepare_count");
  return CQLREC_OK;
}

__global__ void prepare_minmax_init_kernel(int64_t n_groups, int64_t* __restrict__ gmin, int64_t* __restrict__ gmax) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g < n_groups) {
    gmin[g] = INT64_MAX;
    gmax[g] = INT64_MIN;
  }
}
__global__ void prepare_group_minmax_kernel(const int32_t* __restrict__ group, const int64_t* __restrict__ key, int64_t n,
                                            int64_t* __restrict__ gmin, int64_t* __restrict__ gmax) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t g = group[i];
  const long long k = (long long)key[i];
  atomicMin((long long*)&gmin[g], k);
  atomicMax((long long*)&gmax[g], k);
}
// the whole column: a grid-stride pass, a block reduction in LDS, one pair of atomics per block
__global__ __launch_bounds__(256) void prepare_global_minmax_kernel(const int64_t* __restrict__ key, int64_t n,
                                                                   int64_t* __restrict__ gmin,
                                                                   int64_t* __restrict__ gmax) {
  __shared__ long long lo[256], hi[256];
  long long a = INT64_MAX, b = INT64_MIN;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const long long k = (long long)key[i];
    a = k < a ? k : a;
    b = k > b ? k : b;
  }
  lo[threadIdx.x] = a;
  hi[threadIdx.x] = b;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const long long a2 = lo[threadIdx.x + w], b2 = hi[threadIdx.x + w];
      if (a2 < lo[threadIdx.x]) lo[threadIdx.x] = a2;
      if (b2 > hi[threadIdx.x]) hi[threadIdx.x] = b2;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicMin((long long*)gmin, lo[0]);
    atomicMax((long long*)gmax, hi[0]);
  }
}

extern "C" int cqlrec_prepare_minmax(const int32_t* group, const int64_t* key, int64_t n_rows, int64_t n_groups,
                                     int64_t* gmin, int64_t* gmax, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS && n_groups > 0 && n_groups < PREPARE_MAX_ROWS,
              "prepare_minmax: n_rows=%lld n_groups=%lld out of range", (long long)n_rows, (long long)n_groups);
  CQL_REQUIRE(group || n_groups == 1, "prepare_minmax: no group column means one group, not %lld", (long long)n_groups);
  CQL_REQUIRE(gmin && gmax && (key || n_rows == 0), "prepare_minmax: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(prepare_minmax_init_kernel, dim3(cql_ceil_div(n_groups, 256)), dim3(256), 0, s, n_groups, gmin,
                     gmax);
  if (n_rows > 0) {
    if (group) {
      hipLaunchKernelGGL(prepare_group_minmax_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, group, key, n_rows,
                         gmin, gmax);
    } else {
      const int blocks = cql_ceil_div(n_rows, 256) < 2048 ? cql_ceil_div(n_rows, 256) : 2048;
      hipLaunchKernelGGL(prepare_global_minmax_kernel, dim3(blocks), dim3(256), 0, s, key, n_rows, gmin, gmax);
    }
  }
  CQL_LAUNCH_CHECK("prepare_minmax");
  return CQLREC_OK;
}

// =============================================================================================================
// the row predicate of the six filters
// =============================================================================================================
__device__ __forceinline__ int64_t sat_add(int64_t a, int64_t b) {
  int64_t r;
  if (__builtin_add_overflow(a, b, &r)) return b > 0 ? INT64_MAX : INT64_MIN;
  return r;
}
__device__ __forceinline__ int64_t sat_sub(int64_t a, int64_t b) {
  int64_t r;
  if (__builtin_sub_overflow(a, b, &r)) return b > 0 ? INT64_MIN : INT64_MAX;
  return r;
}
// data.timestamp_key of a double, back to the double (the map is its own inverse)
__device__ __forceinline__ double key_to_double(int64_t k) {
  return __longlong_as_double(k < 0 ? (k ^ 0x7FFFFFFFFFFFFFFFll) : k);
}

__global__ void prepare_keep_kernel(int rule, const int32_t* __restrict__ group, const int64_t* __restrict__ key,
                                    const double* __restrict__ value, const int32_t* __restrict__ rank,
                                    const int32_t* __restrict__ count, const int64_t* __restrict__ extreme, int64_t n_rows,
                                    int64_t n, int first, int float_key, int64_t lo, int64_t hi, int open_end, double x,
                                    uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  bool k;
  switch (rule) {
    case CQLREC_KEEP_MIN_COUNT:
      k = (int64_t)count[group[i]] >= n;
      break;
    case CQLREC_KEEP_MIN_VALUE:
      k = value[i] >= x;
      break;
    case CQLREC_KEEP_NUM_INTERACTIONS: {
      const int64_t r = rank[i];
      k = (first ? (int64_t)count[group[i]] + 1 - r : r) <= n;
    } break;
    case CQLREC_KEEP_DAYS_USER:
    case CQLREC_KEEP_DAYS_GLOBAL: {
      const int64_t e = extreme[rule == CQLREC_KEEP_DAYS_USER ? group[i] : 0];
      if (float_key) {
        const double t = key_to_double(key[i]), m = key_to_double(e);
        k = first ? t < m + x : t > m - x;
      } else {
        k = first ? key[i] < sat_add(e, n) : key[i] > sat_sub(e, n);
      }
    } break;
    default:  // CQLREC_KEEP_PERIOD
      k = key[i] >= lo && (open_end || key[i] < hi);
      break;
  }
  keep[i] = k ? 1 : 0;
}

extern "C" int cqlrec_prepare_keep(int32_t rule, const int32_t* group, const int64_t* key, const double* value,
                                   const int32_t* rank, const int32_t* count, const int64_t* extreme, int64_t n_rows,
                                   int64_t n, int32_t first, int32_t float_key, int64_t lo, int64_t hi, int32_t open_end,
                                   double x, uint8_t* keep, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS, "prepare_keep: n_rows=%lld out of range", (long long)n_rows);
  CQL_REQUIRE(rule >= CQLREC_KEEP_MIN_COUNT && rule <= CQLREC_KEEP_PERIOD, "prepare_keep: unknown rule %d", rule);
  if (n_rows == 0) return CQLREC_OK;
  CQL_REQUIRE(keep, "prepare_keep: NULL pointer");
  bool ok = true;
  switch (rule) {
    case CQLREC_KEEP_MIN_COUNT:
      ok = group && count;
      break;
    case CQLREC_KEEP_MIN_VALUE:
      ok = value != nullptr;
      break;
    case CQLREC_KEEP_NUM_INTERACTIONS:
      ok = rank && (!first || (group && count));
      break;
    case CQLREC_KEEP_DAYS_USER:
      ok = group && key && extreme && (!float_key || x == x);
      break;
    case CQLREC_KEEP_DAYS_GLOBAL:
      ok = key && extreme && (!float_key || x == x);
      break;
    default:
      ok = key != nullptr;
      break;
  }
  CQL_REQUIRE(ok, "prepare_keep: rule %d: NULL pointer or parameter out of range (x=%g)", rule, x);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(prepare_keep_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, rule, group, key, value, rank,
                     count, extreme, n_rows, n, first ? 1 : 0, float_key ? 1 : 0, lo, hi, open_end ? 1 : 0, x, keep);
  CQL_LAUNCH_CHECK("prepare_keep");
  return CQLREC_OK;
}

// =============================================================================================================
// stable compaction of one keep byte per row
// =============================================================================================================
extern "C" int64_t cqlrec_prepare_compact_ws_bytes(int64_t n_rows) {
  if (n_rows < 0) return 0;
  return cql_align256(n_rows * 8) + (16ll << 20) + 256;
}

extern "C" int cqlrec_prepare_compact(const uint8_t* keep, int64_t n_rows, void* ws, int64_t ws_bytes, int64_t* rows,
                                      int64_t* n_kept, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS, "prepare_compact: n_rows=%lld out of range", (long long)n_rows);
  CQL_REQUIRE(n_kept, "prepare_compact: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(n_kept, 0, 8, s, "prepare_compact");
    return CQLREC_OK;
  }
  CQL_REQUIRE(keep && ws && rows, "prepare_compact: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_compact_ws_bytes(n_rows), "prepare_compact: workspace too small");
  const size_t cap = (size_t)(cqlrec_prepare_compact_ws_bytes(n_rows) - 256);
  const int rc = cql_select_rows("prepare_compact", ws, cap, keep, rows, n_kept, n_rows, s);
  if (rc != CQLREC_OK) return rc;
  CQL_LAUNCH_CHECK("prepare_compact");
  return CQLREC_OK;
}

// =============================================================================================================
// Indexer: distinct sorted ids, labels sorted with their index, lookup, gather
// =============================================================================================================
extern "C" int64_t cqlrec_prepare_distinct_ws_bytes(int64_t n) {
  if (n < 0) return 0;
  return cql_align256(n * 8) + cql_sort_temp_cap(n) + 256;
}

extern "C" int cqlrec_prepare_distinct(const int64_t* ids, int64_t n, void* ws, int64_t ws_bytes, int64_t* out,
                                       int64_t* n_out, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 0 && n < PREPARE_MAX_ROWS, "prepare_distinct: n=%lld out of range", (long long)n);
  CQL_REQUIRE(n_out, "prepare_distinct: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    CQL_MEMSET(n_out, 0, 8, s, "prepare_distinct");
    return CQLREC_OK;
  }
  CQL_REQUIRE(ids && ws && out, "prepare_distinct: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_distinct_ws_bytes(n), "prepare_distinct: workspace too small");
  int64_t* sorted = (int64_t*)ws;
  void* temp = (char*)ws + cql_align256(n * 8);
  const size_t cap = (size_t)cql_sort_temp_cap(n);
  int rc = cql_sort_keys("prepare_distinct", temp, cap, ids, sorted, n, 64, s);
  if (rc == CQLREC_OK) rc = cql_unique("prepare_distinct", temp, cap, sorted, out, n_out, n, s);
  if (rc != CQLREC_OK) return rc;
  CQL_LAUNCH_CHECK("prepare_distinct");
  return CQLREC_OK;
}

extern "C" int64_t cqlrec_prepare_sort_labels_ws_bytes(int64_t m) {
  if (m < 0) return 0;
  return cql_align256(m * 4) + cql_sort_temp_cap(m) + 256;
}

extern "C" int cqlrec_prepare_sort_labels(const int64_t* labels, int64_t m, void* ws, int64_t ws_bytes, int64_t* sorted,
                                          int32_t* sorted_idx, cqlrec_stream stream) {
  CQL_REQUIRE(m >= 0 && m < PREPARE_MAX_ROWS - 1, "prepare_sort_labels: m=%lld out of range", (long long)m);
  if (m == 0) return CQLREC_OK;
  CQL_REQUIRE(labels && ws && sorted && sorted_idx, "prepare_sort_labels: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_sort_labels_ws_bytes(m), "prepare_sort_labels: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int32_t* iota = (int32_t*)ws;
  void* temp = (char*)ws + cql_align256(m * 4);
  cql_iota((uint32_t*)iota, m, false, s);                 // m < 2^31: the same bits as int32
  const int rc = cql_sort_pairs("prepare_sort_labels", temp, (size_t)cql_sort_temp_cap(m), labels, sorted, iota, sorted_idx, m,
                                64, s);
  if (rc != CQLREC_OK) return rc;
  CQL_LAUNCH_CHECK("prepare_sort_labels");
  return CQLREC_OK;
}

// out[i] = sorted_idx[j] for the j with sorted[j] == ids[i] (binary search), or -1 and *miss = 1
__global__ void prepare_lookup_kernel(const int64_t* __restrict__ ids, int64_t n, const int64_t* __restrict__ sorted,
                                      const int32_t* __restrict__ sorted_idx, int64_t m, int32_t* __restrict__ out,
                                      int32_t* __restrict__ miss) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t v = ids[i];
  int64_t lo = 0, hi = m;                 // the first j in [0, m] with sorted[j] >= v
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < v) lo = mid + 1; else hi = mid;
  }
  if (lo < m && sorted[lo] == v) {
    out[i] = sorted_idx[lo];
  } else {
    out[i] = -1;
    atomicOr(miss, 1);
  }
}

extern "C" int cqlrec_prepare_lookup(const int64_t* ids, int64_t n_rows, const int64_t* sorted, const int32_t* sorted_idx,
                                     int64_t m, int32_t* out, int32_t* miss, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS && m >= 0 && m < PREPARE_MAX_ROWS - 1,
              "prepare_lookup: n_rows=%lld m=%lld out of range", (long long)n_rows, (long long)m);
  CQL_REQUIRE(miss && (n_rows == 0 || (ids && out && (m == 0 || (sorted && sorted_idx)))), "prepare_lookup: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(miss, 0, 4, s, "prepare_lookup");
  if (n_rows == 0) return CQLREC_OK;
  hipLaunchKernelGGL(prepare_lookup_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, ids, n_rows, sorted,
                     sorted_idx, m, out, miss);
  CQL_LAUNCH_CHECK("prepare_lookup");
  return CQLREC_OK;
}

// out[i] = labels[idx[i]]; an index outside [0, m) gives 0 and *bad = 1
__global__ void prepare_gather_kernel(const int64_t* __restrict__ idx, int64_t n, const int64_t* __restrict__ labels,
                                      int64_t m, int64_t* __restrict__ out, int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t j = idx[i];
  if (j >= 0 && j < m) {
    out[i] = labels[j];
  } else {
    out[i] = 0;
    atomicOr(bad, 1);
  }
}

extern "C" int cqlrec_prepare_gather(const int64_t* idx, int64_t n_rows, const int64_t* labels, int64_t m, int64_t* out,
                                     int32_t* bad, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS && m >= 0 && m < PREPARE_MAX_ROWS - 1,
              "prepare_gather: n_rows=%lld m=%lld out of range", (long long)n_rows, (long long)m);
  CQL_REQUIRE(bad && (n_rows == 0 || (idx && out && (m == 0 || labels))), "prepare_gather: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CQL_MEMSET(bad, 0, 4, s, "prepare_gather");
  if (n_rows == 0) return CQLREC_OK;
  hipLaunchKernelGGL(prepare_gather_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, idx, n_rows, labels, m, out,
                     bad);
  CQL_LAUNCH_CHECK("prepare_gather");
  return CQLREC_OK;
}
