// f6  log preparation on the device (replay/filters.py, replay/data_preparator.py's Indexer): a ranking inside each
// user with a secondary key, per-group counts and int64 extremes, one row predicate for the six filters, a stable
// compaction, and the Indexer's distinct / lookup / gather.  Integer work; the only atomics are integer ones, so the
// same input gives the same bytes.  The two double expressions (the rating comparison, the float day bound: one add or
// subtract) are single IEEE operations -- the file is built with -ffp-contract=off.
//
// Order inside a user: (key, key2, input row index), ranked DESCENDING as cqlrec_split_rank does -- stable LSD radix
// passes over a row permutation that starts REVERSED (stability then keeps later rows first): key2, then key, then
// user.  The ascending row number is count[u] + 1 - rank.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

static inline int64_t a256(int64_t x) { return (x + 255) / 256 * 256; }
static const int64_t PREPARE_MAX_ROWS = 1ll << 31;
// scratch left for rocPRIM behind the explicit buffers (the bound split.hip and prep.hip use)
static inline int64_t sort_temp_cap(int64_t n) { return a256(4 * n * 8) + (16ll << 20); }

#define PREPARE_ROCPRIM(call, what)                                                      \
  do {                                                                                   \
    hipError_t e__ = (call);                                                             \
    if (e__ != hipSuccess) {                                                             \
      cql_set_error("%s: rocPRIM failed: %s", what, hipGetErrorString(e__));             \
      return CQLREC_ERR_HIP;                                                             \
    }                                                                                    \
  } while (0)
#define PREPARE_TEMP_FITS(need, cap, what)                                               \
  do {                                                                                   \
    if ((need) > (size_t)(cap)) {                                                        \
      cql_set_error("%s: rocPRIM needs %zu bytes of scratch (have %zu)", what, (size_t)(need), (size_t)(cap)); \
      return CQLREC_ERR_HIP;                                                             \
    }                                                                                    \
  } while (0)
#define PREPARE_MEMSET(ptr, val, bytes, what)                                            \
  do {                                                                                   \
    if (hipMemsetAsync(ptr, val, bytes, s) != hipSuccess) {                              \
      cql_set_error("%s: memset failed", what);                                          \
      return CQLREC_ERR_HIP;                                                             \
    }                                                                                    \
  } while (0)

static inline unsigned bits_for(int64_t n) {
  unsigned bits = 1;
  while (bits < 32 && (1ll << bits) < n) ++bits;
  return bits;
}

// =============================================================================================================
// rank inside the user under (key desc, key2 desc, row index desc)
// =============================================================================================================
__global__ void prepare_perm_init_kernel(int64_t n, uint32_t* __restrict__ perm) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = (uint32_t)(n - 1 - i);
}
// sort keys of the rows in their current order, for an ASCENDING sort: key2 and key reversed, the user as it is
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
__global__ void prepare_user_key_kernel(const int32_t* __restrict__ user_idx, const uint32_t* __restrict__ perm,
                                        int64_t n, uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint32_t)user_idx[perm[i]];
}
// offsets[u] = first sorted position whose user >= u
__global__ void prepare_bounds_kernel(const int32_t* __restrict__ user_idx, const uint32_t* __restrict__ perm, int64_t n,
                                      int64_t n_users, int64_t* __restrict__ offsets) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const int64_t cur = (i < n) ? (int64_t)user_idx[perm[i]] : n_users;
  const int64_t prev = (i > 0) ? (int64_t)user_idx[perm[i - 1]] : -1;
  for (int64_t u = prev + 1; u <= cur; ++u) offsets[u] = i;
}
__global__ void prepare_rank_finish_kernel(const int32_t* __restrict__ user_idx, const uint32_t* __restrict__ perm,
                                           int64_t n, const int64_t* __restrict__ offsets, int32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = perm[i];
  rank[r] = (int32_t)(i - offsets[user_idx[r]] + 1);
}
__global__ void prepare_rank_count_kernel(const int64_t* __restrict__ offsets, int64_t n_users,
                                          int32_t* __restrict__ count) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_users) count[u] = (int32_t)(offsets[u + 1] - offsets[u]);
}

extern "C" int64_t cqlrec_prepare_rank_ws_bytes(int64_t n_rows, int64_t n_users) {
  if (n_rows < 0 || n_users < 0) return 0;
  return 2 * a256(n_rows * 4) + 2 * a256(n_rows * 8) + a256((n_users + 1) * 8) + sort_temp_cap(n_rows) + 256;
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
    PREPARE_MEMSET(count, 0, (size_t)n_users * 4, "prepare_rank");
    return CQLREC_OK;
  }
  CQL_REQUIRE(user_idx && key && ws && rank, "prepare_rank: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_rank_ws_bytes(n_rows, n_users), "prepare_rank: workspace too small");
  char* p = (char*)ws;
  uint32_t* cur = (uint32_t*)p;    p += a256(n_rows * 4);
  uint32_t* other = (uint32_t*)p;  p += a256(n_rows * 4);
  uint64_t* key_a = (uint64_t*)p;  p += a256(n_rows * 8);
  uint64_t* key_b = (uint64_t*)p;  p += a256(n_rows * 8);
  int64_t* offsets = (int64_t*)p;  p += a256((n_users + 1) * 8);
  void* temp = p;
  const size_t temp_cap = (size_t)sort_temp_cap(n_rows);
  const dim3 grid(cql_ceil_div(n_rows, 256)), block(256);
  uint32_t* k32_a = (uint32_t*)key_a;
  uint32_t* k32_b = (uint32_t*)key_b;
  size_t need = 0;
  hipLaunchKernelGGL(prepare_perm_init_kernel, grid, block, 0, s, n_rows, cur);
  if (key2) {  // least significant: key2 descending, over the bits a value below n_key2 can have
    const unsigned bits = bits_for(n_key2);
    hipLaunchKernelGGL(prepare_key2_kernel, grid, block, 0, s, key2, cur, n_rows, (uint32_t)(n_key2 - 1), k32_a);
    PREPARE_ROCPRIM(rocprim::radix_sort_pairs(nullptr, need, k32_a, k32_b, cur, other, (size_t)n_rows, 0u, bits, s),
                    "prepare_rank");
    PREPARE_TEMP_FITS(need, temp_cap, "prepare_rank");
    PREPARE_ROCPRIM(rocprim::radix_sort_pairs(temp, need, k32_a, k32_b, cur, other, (size_t)n_rows, 0u, bits, s),
                    "prepare_rank");
    uint32_t* t = cur;  cur = other;  other = t;
  }
  hipLaunchKernelGGL(prepare_key_kernel, grid, block, 0, s, key, cur, n_rows, key_a);
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(nullptr, need, key_a, key_b, cur, other, (size_t)n_rows, 0u, 64u, s),
                  "prepare_rank");
  PREPARE_TEMP_FITS(need, temp_cap, "prepare_rank");
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(temp, need, key_a, key_b, cur, other, (size_t)n_rows, 0u, 64u, s),
                  "prepare_rank");
  {
    uint32_t* t = cur;  cur = other;  other = t;
  }
  const unsigned ubits = bits_for(n_users);
  hipLaunchKernelGGL(prepare_user_key_kernel, grid, block, 0, s, user_idx, cur, n_rows, k32_a);
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(nullptr, need, k32_a, k32_b, cur, other, (size_t)n_rows, 0u, ubits, s),
                  "prepare_rank");
  PREPARE_TEMP_FITS(need, temp_cap, "prepare_rank");
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(temp, need, k32_a, k32_b, cur, other, (size_t)n_rows, 0u, ubits, s),
                  "prepare_rank");
  cur = other;
  hipLaunchKernelGGL(prepare_bounds_kernel, dim3(cql_ceil_div(n_rows + 1, 256)), block, 0, s, user_idx, cur, n_rows,
                     n_users, offsets);
  hipLaunchKernelGGL(prepare_rank_finish_kernel, grid, block, 0, s, user_idx, cur, n_rows, offsets, rank);
  hipLaunchKernelGGL(prepare_rank_count_kernel, dim3(cql_ceil_div(n_users, 256)), block, 0, s, offsets, n_users, count);
  CQL_LAUNCH_CHECK("prepare_rank");
  return CQLREC_OK;
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
  PREPARE_MEMSET(count, 0, (size_t)n_groups * 4, "prepare_count");
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
  return a256(n_rows * 8) + (16ll << 20) + 256;
}

extern "C" int cqlrec_prepare_compact(const uint8_t* keep, int64_t n_rows, void* ws, int64_t ws_bytes, int64_t* rows,
                                      int64_t* n_kept, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < PREPARE_MAX_ROWS, "prepare_compact: n_rows=%lld out of range", (long long)n_rows);
  CQL_REQUIRE(n_kept, "prepare_compact: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    PREPARE_MEMSET(n_kept, 0, 8, "prepare_compact");
    return CQLREC_OK;
  }
  CQL_REQUIRE(keep && ws && rows, "prepare_compact: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_compact_ws_bytes(n_rows), "prepare_compact: workspace too small");
  const size_t cap = (size_t)(cqlrec_prepare_compact_ws_bytes(n_rows) - 256);
  static_assert(sizeof(size_t) == sizeof(int64_t), "the count is written as size_t");
  rocprim::counting_iterator<int64_t> all_rows(0);
  size_t need = 0;
  PREPARE_ROCPRIM(rocprim::select(nullptr, need, all_rows, keep, rows, (size_t*)n_kept, (size_t)n_rows, s),
                  "prepare_compact");
  PREPARE_TEMP_FITS(need, cap, "prepare_compact");
  PREPARE_ROCPRIM(rocprim::select(ws, need, all_rows, keep, rows, (size_t*)n_kept, (size_t)n_rows, s), "prepare_compact");
  CQL_LAUNCH_CHECK("prepare_compact");
  return CQLREC_OK;
}

// =============================================================================================================
// Indexer: distinct sorted ids, labels sorted with their index, lookup, gather
// =============================================================================================================
extern "C" int64_t cqlrec_prepare_distinct_ws_bytes(int64_t n) {
  if (n < 0) return 0;
  return a256(n * 8) + sort_temp_cap(n) + 256;
}

extern "C" int cqlrec_prepare_distinct(const int64_t* ids, int64_t n, void* ws, int64_t ws_bytes, int64_t* out,
                                       int64_t* n_out, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 0 && n < PREPARE_MAX_ROWS, "prepare_distinct: n=%lld out of range", (long long)n);
  CQL_REQUIRE(n_out, "prepare_distinct: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    PREPARE_MEMSET(n_out, 0, 8, "prepare_distinct");
    return CQLREC_OK;
  }
  CQL_REQUIRE(ids && ws && out, "prepare_distinct: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_distinct_ws_bytes(n), "prepare_distinct: workspace too small");
  int64_t* sorted = (int64_t*)ws;
  void* temp = (char*)ws + a256(n * 8);
  const size_t cap = (size_t)sort_temp_cap(n);
  static_assert(sizeof(size_t) == sizeof(int64_t), "the count is written as size_t");
  size_t need = 0;
  PREPARE_ROCPRIM(rocprim::radix_sort_keys(nullptr, need, ids, sorted, (size_t)n, 0u, 64u, s), "prepare_distinct");
  PREPARE_TEMP_FITS(need, cap, "prepare_distinct");
  PREPARE_ROCPRIM(rocprim::radix_sort_keys(temp, need, ids, sorted, (size_t)n, 0u, 64u, s), "prepare_distinct");
  PREPARE_ROCPRIM(rocprim::unique(nullptr, need, sorted, out, (size_t*)n_out, (size_t)n, rocprim::equal_to<int64_t>(), s),
                  "prepare_distinct");
  PREPARE_TEMP_FITS(need, cap, "prepare_distinct");
  PREPARE_ROCPRIM(rocprim::unique(temp, need, sorted, out, (size_t*)n_out, (size_t)n, rocprim::equal_to<int64_t>(), s),
                  "prepare_distinct");
  CQL_LAUNCH_CHECK("prepare_distinct");
  return CQLREC_OK;
}

__global__ void prepare_iota_kernel(int64_t m, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = (int32_t)i;
}

extern "C" int64_t cqlrec_prepare_sort_labels_ws_bytes(int64_t m) {
  if (m < 0) return 0;
  return a256(m * 4) + sort_temp_cap(m) + 256;
}

extern "C" int cqlrec_prepare_sort_labels(const int64_t* labels, int64_t m, void* ws, int64_t ws_bytes, int64_t* sorted,
                                          int32_t* sorted_idx, cqlrec_stream stream) {
  CQL_REQUIRE(m >= 0 && m < PREPARE_MAX_ROWS - 1, "prepare_sort_labels: m=%lld out of range", (long long)m);
  if (m == 0) return CQLREC_OK;
  CQL_REQUIRE(labels && ws && sorted && sorted_idx, "prepare_sort_labels: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_prepare_sort_labels_ws_bytes(m), "prepare_sort_labels: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int32_t* iota = (int32_t*)ws;
  void* temp = (char*)ws + a256(m * 4);
  hipLaunchKernelGGL(prepare_iota_kernel, dim3(cql_ceil_div(m, 256)), dim3(256), 0, s, m, iota);
  size_t need = 0;
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(nullptr, need, labels, sorted, iota, sorted_idx, (size_t)m, 0u, 64u, s),
                  "prepare_sort_labels");
  PREPARE_TEMP_FITS(need, sort_temp_cap(m), "prepare_sort_labels");
  PREPARE_ROCPRIM(rocprim::radix_sort_pairs(temp, need, labels, sorted, iota, sorted_idx, (size_t)m, 0u, 64u, s),
                  "prepare_sort_labels");
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
  PREPARE_MEMSET(miss, 0, 4, "prepare_lookup");
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
  PREPARE_MEMSET(bad, 0, 4, "prepare_gather");
  if (n_rows == 0) return CQLREC_OK;
  hipLaunchKernelGGL(prepare_gather_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, idx, n_rows, labels, m, out,
                     bad);
  CQL_LAUNCH_CHECK("prepare_gather");
  return CQLREC_OK;
}
