// The sort / segment layer under every prepared-data entry point (prep, metrics, split, prepare, features, neighbour, als,
// gbwd): the only home of the rocPRIM plumbing those files share.  DESIGN section 3.11.
//
//   sizes    cql_sort_temp_cap / cql_scan_temp_cap bound rocPRIM's scratch (the *_ws_bytes formulas are built from them);
//            cql_bits_for(n) is the end bit of a radix sort over keys below n.
//   rocPRIM  cql_rocprim runs one algorithm: size query, fit check against the cap, the real call, ONE error text;
//            cql_sort_pairs / _keys, cql_exclusive_scan, cql_run_length_encode, cql_select_rows, cql_unique are thin
//            wrappers that hand their iterators through unchanged (rocPRIM picks its kernels from these types).
//   perm     CqlPermSort is the stable LSD driver: the caller's kernel writes the keys of the rows in their current order,
//            pass() sorts (key, perm) and swaps the two perm buffers.  The key kernels stay with their files.
//   kernels  iota (forward / reversed), the gather of a uint32 group key, segment bounds with the gap fill, and the tail
//            of the rank inside a group (segment_common.hip holds the non-template ones, once per program).
// These files are compiled with different floating-point flags: nothing here may hold a floating-point expression.
#pragma once
#include <iterator>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "common.h"

// ---- scratch bounds and bit counts -------------------------------------------------------------------------------------
// a radix sort without double buffers keeps one more copy of keys and values in its scratch
static inline int64_t cql_sort_temp_cap(int64_t n) { return cql_align256(4 * n * 8) + (16ll << 20); }
static inline int64_t cql_scan_temp_cap(int64_t n) { return cql_align256(n * 8) + (1ll << 20); }
// the bits a value below n can have, at least 1
static inline unsigned cql_bits_for(int64_t n) {
  unsigned bits = 1;
  while (bits < 62 && (1ll << bits) < n) ++bits;
  return bits;
}

// ---- one error path ----------------------------------------------------------------------------------------------------
#define CQL_MEMSET(ptr, val, bytes, stream, what)                      \
  do {                                                                 \
    if (hipMemsetAsync(ptr, val, bytes, stream) != hipSuccess) {       \
      cql_set_error("%s: memset failed", what);                        \
      return CQLREC_ERR_HIP;                                           \
    }                                                                  \
  } while (0)

// call: (void* temp, size_t& need) -> hipError_t, one rocPRIM algorithm; with temp == nullptr it only reports its need
template <typename F>
static inline int cql_rocprim(const char* what, void* temp, size_t temp_cap, F&& call) {
  size_t need = 0;
  hipError_t e = call(nullptr, need);
  if (e == hipSuccess && need > temp_cap) e = hipErrorOutOfMemory;
  if (e == hipSuccess) e = call(temp, need);
  if (e != hipSuccess) {
    cql_set_error("%s: rocPRIM failed: %s (%zu bytes of scratch needed, %zu there)", what, hipGetErrorString(e), need,
                  temp_cap);
    return CQLREC_ERR_HIP;
  }
  return CQLREC_OK;
}

// stable, ascending over the bits [0, bits) of the keys
template <typename KI, typename KO, typename VI, typename VO>
static inline int cql_sort_pairs(const char* what, void* temp, size_t temp_cap, KI keys_in, KO keys_out, VI vals_in,
                                 VO vals_out, int64_t n, unsigned bits, hipStream_t s) {
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::radix_sort_pairs(t, need, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, bits, s);
  });
}
template <typename KI, typename KO>
static inline int cql_sort_keys(const char* what, void* temp, size_t temp_cap, KI keys_in, KO keys_out, int64_t n,
                                unsigned bits, hipStream_t s) {
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::radix_sort_keys(t, need, keys_in, keys_out, (size_t)n, 0u, bits, s);
  });
}
// out[i] = init + in[0] + ... + in[i - 1]
template <typename In, typename Out, typename T>
static inline int cql_exclusive_scan(const char* what, void* temp, size_t temp_cap, In in, Out out, T init, int64_t n,
                                     hipStream_t s) {
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::exclusive_scan(t, need, in, out, init, (size_t)n, rocprim::plus<T>(), s);
  });
}
// the distinct values of a sorted sequence, their run lengths, and how many there are (*n_runs, on the device)
template <typename In, typename UO, typename CO>
static inline int cql_run_length_encode(const char* what, void* temp, size_t temp_cap, In in, int64_t n, UO unique_out,
                                        CO counts_out, size_t* n_runs, hipStream_t s) {
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::run_length_encode(t, need, in, (unsigned int)n, unique_out, counts_out, n_runs, s);
  });
}
// the row numbers i in [0, n) with flags[i] != 0, in order, and how many (*n_out, on the device)
static_assert(sizeof(size_t) == sizeof(int64_t), "device-side counts are written as size_t and read as int64_t");
static inline int cql_select_rows(const char* what, void* temp, size_t temp_cap, const uint8_t* flags, int64_t* rows_out,
                                  int64_t* n_out, int64_t n, hipStream_t s) {
  rocprim::counting_iterator<int64_t> rows(0);
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::select(t, need, rows, flags, rows_out, (size_t*)n_out, (size_t)n, s);
  });
}
// the distinct values of a sorted sequence and how many (*n_out, on the device)
template <typename In, typename Out>
static inline int cql_unique(const char* what, void* temp, size_t temp_cap, In in, Out out, int64_t* n_out, int64_t n,
                             hipStream_t s) {
  typedef typename std::iterator_traits<In>::value_type T;
  return cql_rocprim(what, temp, temp_cap, [&](void* t, size_t& need) {
    return rocprim::unique(t, need, in, out, (size_t*)n_out, (size_t)n, rocprim::equal_to<T>(), s);
  });
}

// ---- the permutation-sort driver ---------------------------------------------------------------------------------------
// Stable LSD sort of a row permutation, least significant key first.  One pass: the caller's kernel writes keys<K>()[i] =
// the key of row perm[i]; pass<K>() sorts (key, perm) over `bits` bits into the other buffers and makes them current.
// After a pass sorted<K>() holds the sorted keys of that pass.  key_a / key_b hold n uint64 (or uint32) each.
struct CqlPermSort {
  uint32_t *perm, *perm_alt;   // the current permutation and the buffer the next pass writes
  uint64_t *key_a, *key_b;
  void* temp;
  size_t temp_cap;
  int64_t n;
  hipStream_t s;

  // carve: perm | perm_alt | key_a | key_b from p (advanced past them); the caller places temp
  CqlPermSort(char*& p, int64_t n_, hipStream_t s_) : temp(nullptr), temp_cap((size_t)cql_sort_temp_cap(n_)), n(n_), s(s_) {
    perm = (uint32_t*)p;      p += cql_align256(n * 4);
    perm_alt = (uint32_t*)p;  p += cql_align256(n * 4);
    key_a = (uint64_t*)p;     p += cql_align256(n * 8);
    key_b = (uint64_t*)p;     p += cql_align256(n * 8);
  }
  static int64_t bytes(int64_t n) { return 2 * cql_align256(n * 4) + 2 * cql_align256(n * 8); }
  template <typename K> K* keys() const { return (K*)key_a; }
  template <typename K> const K* sorted() const { return (const K*)key_b; }
  // `out`: the buffer that receives the permutation instead of perm_alt (a caller's own array, for the last pass)
  template <typename K>
  int pass(const char* what, unsigned bits, uint32_t* out = nullptr) {
    uint32_t* dst = out ? out : perm_alt;
    const int rc = cql_sort_pairs(what, temp, temp_cap, (K*)key_a, (K*)key_b, perm, dst, n, bits, s);
    if (!out) perm_alt = perm;
    perm = dst;
    return rc;
  }
};

// ---- shared kernels ----------------------------------------------------------------------------------------------------
// perm[i] = i, or n - 1 - i (a stable sort of a reversed permutation keeps LATER rows first among equal keys)
void cql_iota(uint32_t* perm, int64_t n, bool reversed, hipStream_t s);
// out[i] = (uint32_t)group[perm[i]]
void cql_group_key(const int32_t* group, const uint32_t* perm, int64_t n, uint32_t* out, hipStream_t s);

// offsets[g] = i for every group g in (prev, cur]: position i is the first one whose group is >= g.  prev / cur are the
// groups of the sorted positions i - 1 and i (-1 in front of the first, the end bucket behind the last), so one thread
// fills the whole gap of empty groups in front of its position.
static __device__ __forceinline__ void cql_fill_gap(int64_t prev, int64_t cur, int64_t i, int64_t* __restrict__ offsets) {
  for (int64_t g = prev + 1; g <= cur; ++g) offsets[g] = i;
}
// the group of a sorted position: through the permutation, or from the sorted keys themselves
struct CqlGroupOfPerm {
  const int32_t* group;
  const uint32_t* perm;
  __device__ __forceinline__ int64_t operator()(int64_t i) const { return (int64_t)group[perm[i]]; }
};
template <typename K>
struct CqlGroupOfKey {
  const K* key;
  __device__ __forceinline__ int64_t operator()(int64_t i) const { return (int64_t)key[i]; }
};
// offsets[0 .. end]; n_present (or NULL) counts the groups that have a row
template <typename G>
__global__ void cql_bounds_kernel(G group_at, int64_t n, int64_t end, int64_t* __restrict__ offsets,
                                  unsigned long long* __restrict__ n_present) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const int64_t cur = (i < n) ? group_at(i) : end;
  const int64_t prev = (i > 0) ? group_at(i - 1) : -1;
  cql_fill_gap(prev, cur, i, offsets);
  if (n_present && i < n && cur != prev) atomicAdd(n_present, 1ull);
}
template <typename G>
static inline void cql_segment_bounds(G group_at, int64_t n, int64_t end, int64_t* offsets, unsigned long long* n_present,
                                      hipStream_t s) {
  hipLaunchKernelGGL(cql_bounds_kernel<G>, dim3(cql_ceil_div(n + 1, 256)), dim3(256), 0, s, group_at, n, end, offsets,
                     n_present);
}

// ---- rank inside the user ----------------------------------------------------------------------------------------------
// workspace of a rank routine: the driver's buffers | offsets [n_users + 1] | sort scratch
static inline int64_t cql_rank_ws_bytes(int64_t n_rows, int64_t n_users) {
  if (n_rows < 0 || n_users < 0) return 0;
  return CqlPermSort::bytes(n_rows) + cql_align256((n_users + 1) * 8) + cql_sort_temp_cap(n_rows) + 256;
}
// The tail of cqlrec_split_rank and cqlrec_prepare_rank, after their own passes over the keys: the most significant pass
// (by user), the bounds, rank[r] = position inside the user + 1, count[u]; n_present (or NULL) = users with a row.
int cql_rank_tail(CqlPermSort& ps, const int32_t* user_idx, int64_t n_users, int64_t* offsets, int32_t* rank, int32_t* count,
                  int64_t* n_present, const char* what);
