// f5  train/test splitters on the device (replay/splitters/{user_log_splitter,log_splitter,base_splitter}.py): a ranking
// inside each user, a row predicate, the cold / zero-relevance filters and a stable compaction.  Integer work; the only
// atomics are integer ones, so the same input gives the same bytes.
//
// Tie-break of the ranking: the reference's row_number().over(partitionBy(user).orderBy(ts.desc())) leaves rows of equal
// timestamp to Spark; here rank orders a user's rows by (key DESCENDING, input row index DESCENDING) -- of equal
// timestamps the later input row is the "more recent" one.  Done the way prep.hip builds the CSR: stable LSD radix
// passes over a row permutation (which starts REVERSED, so that stability keeps later rows first), then one kernel that
// turns sorted position into rank.
//
// Random draws: h(x) = mix64(mix64(seed) ^ x), u(x) = ((h >> 11) + 0.5) * 2^-53 -- data._mix64 / data._u01 bit for bit
// (the double add rounds to nearest even in both; the multiply by a power of two is exact).
#include "segment_common.h"

static const int64_t SPLIT_MAX_ROWS = 1ll << 31;

__host__ __device__ __forceinline__ uint64_t split_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ double split_u01(uint64_t h) { return ((double)(h >> 11) + 0.5) * 0x1p-53; }

// =============================================================================================================
// rank inside the user
// =============================================================================================================
// perm[i] = n-1-i (reversed), sort key of that row for an ASCENDING sort = complement of the order-preserving
// unsigned image of the key (or of h(row) when shuffled)
__global__ void rank_init_kernel(const int64_t* __restrict__ key, int64_t n, int shuffle, uint64_t seed_mixed,
                                 uint32_t* __restrict__ perm, uint64_t* __restrict__ skey) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = n - 1 - i;
  const uint64_t k = shuffle ? split_mix64(seed_mixed ^ (uint64_t)r) : ((uint64_t)key[r] ^ (1ull << 63));
  perm[i] = (uint32_t)r;
  skey[i] = ~k;
}

extern "C" int64_t cqlrec_split_rank_ws_bytes(int64_t n_rows, int64_t n_users) {
  return cql_rank_ws_bytes(n_rows, n_users);
}

extern "C" int cqlrec_split_rank(const int32_t* user_idx, const int64_t* key, int64_t n_rows, int64_t n_users,
                                 int32_t shuffle, uint64_t seed, void* ws, int64_t ws_bytes, int32_t* rank,
                                 int32_t* count, int64_t* n_present, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < SPLIT_MAX_ROWS && n_users > 0 && n_users < SPLIT_MAX_ROWS,
              "split_rank: n_rows=%lld n_users=%lld out of range", (long long)n_rows, (long long)n_users);
  CQL_REQUIRE(count, "split_rank: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(count, 0, (size_t)n_users * 4, s, "split_rank");
    if (n_present) CQL_MEMSET(n_present, 0, 8, s, "split_rank");
    return CQLREC_OK;
  }
  CQL_REQUIRE(user_idx && ws && rank && (key || shuffle), "split_rank: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_rank_ws_bytes(n_rows, n_users), "split_rank: workspace too small");
  char* p = (char*)ws;
  CqlPermSort ps(p, n_rows, s);
  int64_t* offsets = (int64_t*)p;   p += cql_align256((n_users + 1) * 8);
  ps.temp = p;
  hipLaunchKernelGGL(rank_init_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, key, n_rows, shuffle ? 1 : 0,
                     split_mix64(seed), ps.perm, ps.keys<uint64_t>());
  // by key descending (ascending over the complemented key); stable, so equal keys keep later rows first
  const int rc = ps.pass<uint64_t>("split_rank", 64);
  if (rc != CQLREC_OK) return rc;
  return cql_rank_tail(ps, user_idx, n_users, offsets, rank, count, n_present, "split_rank");
}

// =============================================================================================================
// order statistics
// =============================================================================================================
__global__ void pick_kth_kernel(const int64_t* __restrict__ sorted, int64_t m, int64_t* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *out = sorted[m - 1];
}

extern "C" int64_t cqlrec_split_kth_key_ws_bytes(int64_t n) {
  if (n < 0) return 0;
  return cql_align256(n * 8) + cql_sort_temp_cap(n) + 256;
}

extern "C" int cqlrec_split_kth_key(const int64_t* key, int64_t n, int64_t m, void* ws, int64_t ws_bytes, int64_t* out,
                                    cqlrec_stream stream) {
  CQL_REQUIRE(n > 0 && n < SPLIT_MAX_ROWS, "split_kth_key: n=%lld out of range", (long long)n);
  CQL_REQUIRE(m >= 1 && m <= n, "split_kth_key: m=%lld outside 1..%lld", (long long)m, (long long)n);
  CQL_REQUIRE(key && ws && out, "split_kth_key: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_kth_key_ws_bytes(n), "split_kth_key: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  int64_t* sorted = (int64_t*)ws;
  void* temp = (char*)ws + cql_align256(n * 8);
  const int rc = cql_sort_keys("split_kth_key", temp, (size_t)cql_sort_temp_cap(n), key, sorted, n, 64, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(pick_kth_kernel, dim3(1), dim3(64), 0, s, sorted, m, out);
  CQL_LAUNCH_CHECK("split_kth_key");
  return CQLREC_OK;
}

__global__ void user_start_init_kernel(int64_t* __restrict__ user_start, int32_t* __restrict__ cnt, int64_t n_users) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_users) {
    user_start[u] = INT64_MAX;
    cnt[u] = 0;
  }
}
__global__ void user_start_kernel(const int32_t* __restrict__ user_idx, const int64_t* __restrict__ key, int64_t n,
                                  int64_t* __restrict__ user_start, int32_t* __restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t u = user_idx[i];
  atomicMin((long long*)&user_start[u], (long long)key[i]);
  atomicAdd(&cnt[u], 1);
}
// one block: T = users with a row; the sorted starts of users without one (INT64_MAX) lie behind the first T entries
// (a real start of INT64_MAX ties with them, and equal values are interchangeable).  c = the least number of users
// with (double)c >= (double)T * test_size, at least 1; threshold = the c-th largest start.
__global__ __launch_bounds__(1024) void new_users_threshold_kernel(const int64_t* __restrict__ sorted,
                                                                   const int32_t* __restrict__ cnt, int64_t n_users,
                                                                   double test_size, int64_t* __restrict__ threshold) {
  __shared__ long long red[1024];
  long long t = 0;
  for (int64_t u = threadIdx.x; u < n_users; u += 1024) t += cnt[u] > 0 ? 1 : 0;
  red[threadIdx.x] = t;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long T = red[0];
    long long c = (long long)ceil((double)T * test_size);
    if (c < 1) c = 1;
    if (c > T) c = T;
    *threshold = T > 0 ? sorted[T - c] : INT64_MAX;
  }
}

extern "C" int64_t cqlrec_split_new_users_ws_bytes(int64_t n_users) {
  if (n_users < 0) return 0;
  return cql_align256(n_users * 8) + cql_align256(n_users * 4) + cql_sort_temp_cap(n_users) + 256;
}

extern "C" int cqlrec_split_new_users(const int32_t* user_idx, const int64_t* key, int64_t n_rows, int64_t n_users,
                                      double test_size, void* ws, int64_t ws_bytes, int64_t* user_start,
                                      int64_t* threshold, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows > 0 && n_rows < SPLIT_MAX_ROWS && n_users > 0 && n_users < SPLIT_MAX_ROWS,
              "split_new_users: n_rows=%lld n_users=%lld out of range", (long long)n_rows, (long long)n_users);
  CQL_REQUIRE(test_size >= 0.0 && test_size <= 1.0, "split_new_users: test_size=%g outside [0, 1]", test_size);
  CQL_REQUIRE(user_idx && key && ws && user_start && threshold, "split_new_users: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_new_users_ws_bytes(n_users), "split_new_users: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)ws;
  int64_t* sorted = (int64_t*)p;  p += cql_align256(n_users * 8);
  int32_t* cnt = (int32_t*)p;     p += cql_align256(n_users * 4);
  void* temp = p;
  const dim3 block(256);
  hipLaunchKernelGGL(user_start_init_kernel, dim3(cql_ceil_div(n_users, 256)), block, 0, s, user_start, cnt, n_users);
  hipLaunchKernelGGL(user_start_kernel, dim3(cql_ceil_div(n_rows, 256)), block, 0, s, user_idx, key, n_rows, user_start,
                     cnt);
  const int rc = cql_sort_keys("split_new_users", temp, (size_t)cql_sort_temp_cap(n_users), user_start, sorted, n_users, 64, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(new_users_threshold_kernel, dim3(1), dim3(1024), 0, s, sorted, cnt, n_users, test_size, threshold);
  CQL_LAUNCH_CHECK("split_new_users");
  return CQLREC_OK;
}

// =============================================================================================================
// user_test_size: the n_pick present users with the smallest h(user), ties by user id ascending
// =============================================================================================================
__global__ void pick_init_kernel(int64_t n_users, uint64_t seed_mixed, uint32_t* __restrict__ perm,
                                 uint64_t* __restrict__ hkey) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_users) return;
  perm[u] = (uint32_t)u;
  hkey[u] = split_mix64(seed_mixed ^ (uint64_t)u);
}
__global__ void pick_absent_key_kernel(const int32_t* __restrict__ count, const uint32_t* __restrict__ perm,
                                       int64_t n_users, uint32_t* __restrict__ akey) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_users) akey[i] = count[perm[i]] > 0 ? 0u : 1u;
}
__global__ void pick_mark_kernel(const int32_t* __restrict__ count, const uint32_t* __restrict__ perm, int64_t n_users,
                                 int64_t n_pick, uint8_t* __restrict__ test_user) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_users) return;
  const uint32_t u = perm[i];
  test_user[u] = (i < n_pick && count[u] > 0) ? 1 : 0;
}

extern "C" int64_t cqlrec_split_pick_users_ws_bytes(int64_t n_users) {
  if (n_users < 0) return 0;
  return CqlPermSort::bytes(n_users) + cql_sort_temp_cap(n_users) + 256;
}

extern "C" int cqlrec_split_pick_users(const int32_t* count, int64_t n_users, uint64_t seed, int64_t n_pick, void* ws,
                                       int64_t ws_bytes, uint8_t* test_user, cqlrec_stream stream) {
  CQL_REQUIRE(n_users > 0 && n_users < SPLIT_MAX_ROWS && n_pick >= 0, "split_pick_users: n_users=%lld n_pick=%lld",
              (long long)n_users, (long long)n_pick);
  CQL_REQUIRE(count && ws && test_user, "split_pick_users: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_pick_users_ws_bytes(n_users), "split_pick_users: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  char* p = (char*)ws;
  CqlPermSort ps(p, n_users, s);
  ps.temp = p;
  const dim3 grid(cql_ceil_div(n_users, 256)), block(256);
  hipLaunchKernelGGL(pick_init_kernel, grid, block, 0, s, n_users, split_mix64(seed), ps.perm, ps.keys<uint64_t>());
  int rc = ps.pass<uint64_t>("split_pick_users", 64);
  if (rc != CQLREC_OK) return rc;
  // users without rows go behind the others (one stable pass over one bit)
  hipLaunchKernelGGL(pick_absent_key_kernel, grid, block, 0, s, count, ps.perm, n_users, ps.keys<uint32_t>());
  rc = ps.pass<uint32_t>("split_pick_users", 1);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(pick_mark_kernel, grid, block, 0, s, count, ps.perm, n_users, n_pick, test_user);
  CQL_LAUNCH_CHECK("split_pick_users");
  return CQLREC_OK;
}

// =============================================================================================================
// classify
// =============================================================================================================
__global__ void classify_kernel(int rule, const int32_t* __restrict__ user_idx, const int64_t* __restrict__ key,
                                const int32_t* __restrict__ rank, const int32_t* __restrict__ count,
                                const uint8_t* __restrict__ test_user, const int64_t* __restrict__ user_start,
                                const int64_t* __restrict__ threshold, int64_t n_rows, int64_t n, int64_t fold, double frac,
                                uint64_t seed_mixed, uint8_t* __restrict__ is_train, uint8_t* __restrict__ is_test) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows) return;
  bool test = false, train;
  switch (rule) {
    case CQLREC_SPLIT_QUANTITY: {
      test = (int64_t)rank[i] <= n && (!test_user || test_user[user_idx[i]]);
      train = !test;
    } break;
    case CQLREC_SPLIT_PROPORTION: {
      const int32_t u = user_idx[i];
      test = (double)rank[i] / (double)count[u] <= frac && (!test_user || test_user[u]);
      train = !test;
    } break;
    case CQLREC_SPLIT_DATE:
      test = key[i] >= *threshold;
      train = !test;
      break;
    case CQLREC_SPLIT_RANDOM_ROW:
      test = split_u01(split_mix64(seed_mixed ^ (uint64_t)i)) >= frac;
      train = !test;
      break;
    case CQLREC_SPLIT_RANDOM_USER:
      test = split_u01(split_mix64(seed_mixed ^ (uint64_t)(int64_t)user_idx[i])) >= frac;
      train = !test;
      break;
    case CQLREC_SPLIT_NEW_USERS: {
      const int64_t thr = *threshold;
      train = key[i] < thr;
      test = user_start[user_idx[i]] >= thr;
    } break;
    default:  // CQLREC_SPLIT_FOLD
      test = (int64_t)rank[i] % n == fold;
      train = !test;
      break;
  }
  is_train[i] = train ? 1 : 0;
  is_test[i] = test ? 1 : 0;
}

extern "C" int cqlrec_split_classify(int32_t rule, const int32_t* user_idx, const int64_t* key, const int32_t* rank,
                                     const int32_t* count, const uint8_t* test_user, const int64_t* user_start,
                                     const int64_t* threshold, int64_t n_rows, int64_t n, int64_t fold, double frac,
                                     uint64_t seed, uint8_t* is_train, uint8_t* is_test, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < SPLIT_MAX_ROWS, "split_classify: n_rows=%lld out of range", (long long)n_rows);
  CQL_REQUIRE(rule >= CQLREC_SPLIT_QUANTITY && rule <= CQLREC_SPLIT_FOLD, "split_classify: unknown rule %d", rule);
  if (n_rows == 0) return CQLREC_OK;
  CQL_REQUIRE(is_train && is_test, "split_classify: NULL pointer");
  bool ok = true;
  switch (rule) {
    case CQLREC_SPLIT_QUANTITY:
      ok = rank && (user_idx || !test_user) && n >= 1;
      break;
    case CQLREC_SPLIT_PROPORTION:
      ok = rank && count && user_idx && frac == frac;
      break;
    case CQLREC_SPLIT_DATE:
      ok = key && threshold;
      break;
    case CQLREC_SPLIT_RANDOM_ROW:
      ok = frac == frac;
      break;
    case CQLREC_SPLIT_RANDOM_USER:
      ok = user_idx && frac == frac;
      break;
    case CQLREC_SPLIT_NEW_USERS:
      ok = key && threshold && user_idx && user_start;
      break;
    default:
      ok = rank && n >= 1 && fold >= 0 && fold < n;
      break;
  }
  CQL_REQUIRE(ok, "split_classify: rule %d: NULL pointer or parameter out of range (n=%lld fold=%lld frac=%g)", rule,
              (long long)n, (long long)fold, frac);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(classify_kernel, dim3(cql_ceil_div(n_rows, 256)), dim3(256), 0, s, rule, user_idx, key, rank, count,
                     test_user, user_start, threshold, n_rows, n, fold, frac, split_mix64(seed), is_train, is_test);
  CQL_LAUNCH_CHECK("split_classify");
  return CQLREC_OK;
}

// =============================================================================================================
// cold / zero-relevance filters of the test part
// =============================================================================================================
__global__ void presence_kernel(const int32_t* __restrict__ user_idx, const int32_t* __restrict__ item_idx,
                                const uint8_t* __restrict__ is_train, int64_t n_rows, uint32_t* __restrict__ user_bits,
                                uint32_t* __restrict__ item_bits) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows || !is_train[i]) return;
  if (user_bits) {
    const uint32_t u = (uint32_t)user_idx[i];
    atomicOr(&user_bits[u >> 5], 1u << (u & 31));
  }
  if (item_bits) {
    const uint32_t it = (uint32_t)item_idx[i];
    atomicOr(&item_bits[it >> 5], 1u << (it & 31));
  }
}
__global__ void filter_test_kernel(const int32_t* __restrict__ user_idx, const int32_t* __restrict__ item_idx,
                                   const double* __restrict__ relevance, int64_t n_rows,
                                   const uint32_t* __restrict__ user_bits, const uint32_t* __restrict__ item_bits,
                                   uint8_t* __restrict__ is_test) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows || !is_test[i]) return;
  bool keep = true;
  if (item_bits) {
    const uint32_t it = (uint32_t)item_idx[i];
    keep = keep && ((item_bits[it >> 5] >> (it & 31)) & 1u);
  }
  if (user_bits) {
    const uint32_t u = (uint32_t)user_idx[i];
    keep = keep && ((user_bits[u >> 5] >> (u & 31)) & 1u);
  }
  if (relevance) keep = keep && relevance[i] > 0.0;
  if (!keep) is_test[i] = 0;
}

static inline int64_t bitmap_bytes(int64_t n) { return cql_align256((n + 31) / 32 * 4); }

extern "C" int64_t cqlrec_split_filter_test_ws_bytes(int64_t n_users, int64_t n_items) {
  if (n_users < 0 || n_items < 0) return 0;
  return bitmap_bytes(n_users) + bitmap_bytes(n_items) + 256;
}

extern "C" int cqlrec_split_filter_test(const int32_t* user_idx, const int32_t* item_idx, const double* relevance,
                                        const uint8_t* is_train, int64_t n_rows, int64_t n_users, int64_t n_items,
                                        int32_t drop_cold_users, int32_t drop_cold_items, int32_t drop_zero_rel, void* ws,
                                        int64_t ws_bytes, uint8_t* is_test, cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < SPLIT_MAX_ROWS && n_users > 0 && n_users < SPLIT_MAX_ROWS && n_items > 0 &&
                  n_items < SPLIT_MAX_ROWS,
              "split_filter_test: n_rows=%lld n_users=%lld n_items=%lld out of range", (long long)n_rows,
              (long long)n_users, (long long)n_items);
  if (n_rows == 0 || (!drop_cold_users && !drop_cold_items && !drop_zero_rel)) return CQLREC_OK;
  CQL_REQUIRE(is_train && is_test && ws, "split_filter_test: NULL pointer");
  CQL_REQUIRE((!drop_cold_users || user_idx) && (!drop_cold_items || item_idx) && (!drop_zero_rel || relevance),
              "split_filter_test: a requested filter has no column");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_filter_test_ws_bytes(n_users, n_items), "split_filter_test: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  uint32_t* user_bits = drop_cold_users ? (uint32_t*)ws : nullptr;
  uint32_t* item_bits = drop_cold_items ? (uint32_t*)((char*)ws + bitmap_bytes(n_users)) : nullptr;
  const dim3 grid(cql_ceil_div(n_rows, 256)), block(256);
  if (user_bits || item_bits) {
    CQL_MEMSET(ws, 0, (size_t)(bitmap_bytes(n_users) + bitmap_bytes(n_items)), s, "split_filter_test");
    hipLaunchKernelGGL(presence_kernel, grid, block, 0, s, user_idx, item_idx, is_train, n_rows, user_bits, item_bits);
  }
  hipLaunchKernelGGL(filter_test_kernel, grid, block, 0, s, user_idx, item_idx, drop_zero_rel ? relevance : nullptr,
                     n_rows, user_bits, item_bits, is_test);
  CQL_LAUNCH_CHECK("split_filter_test");
  return CQLREC_OK;
}

// =============================================================================================================
// stable compaction
// =============================================================================================================
extern "C" int64_t cqlrec_split_compact_ws_bytes(int64_t n_rows) {
  if (n_rows < 0) return 0;
  return cql_align256(n_rows * 8) + (16ll << 20) + 256;
}

extern "C" int cqlrec_split_compact(const uint8_t* is_train, const uint8_t* is_test, int64_t n_rows, void* ws,
                                    int64_t ws_bytes, int64_t* train_rows, int64_t* test_rows, int64_t* counts,
                                    cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < SPLIT_MAX_ROWS, "split_compact: n_rows=%lld out of range", (long long)n_rows);
  CQL_REQUIRE(counts, "split_compact: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  if (n_rows == 0) {
    CQL_MEMSET(counts, 0, 16, s, "split_compact");
    return CQLREC_OK;
  }
  CQL_REQUIRE(is_train && is_test && ws && train_rows && test_rows, "split_compact: NULL pointer");
  CQL_REQUIRE(ws_bytes >= cqlrec_split_compact_ws_bytes(n_rows), "split_compact: workspace too small");
  const size_t cap = (size_t)(cqlrec_split_compact_ws_bytes(n_rows) - 256);
  const uint8_t* flags[2] = {is_train, is_test};
  int64_t* outs[2] = {train_rows, test_rows};
  for (int w = 0; w < 2; ++w) {
    const int rc = cql_select_rows("split_compact", ws, cap, flags[w], outs[w], counts + w, n_rows, s);
    if (rc != CQLREC_OK) return rc;
  }
  CQL_LAUNCH_CHECK("split_compact");
  return CQLREC_OK;
}
