// Wave-level selection over 64-bit keys in LDS, one wave per row: the only home of the exact "threshold algorithm"
// pieces that topk.hip (two-pass cqlrec_score_topk), item_knn.hip (get_nearest_items) and pairs_topk.hip (predict_pairs
// with k) share.  The three walks over the groups / chunks of a row stay in their files.
//
//   key      order(value) << 32 | id field; a larger key is a better entry.  The id field is ~id where ties go to the
//            smaller id (topk, pairs) and the id itself where they go to the larger one (kNN).
//   buffer   admissible keys are appended (sel_append); when it cannot take another batch, sel_keep_topk keeps the k
//            largest and hands back tau, the k-th largest: from then on only keys above tau are worth appending, and a
//            group whose bound cannot beat tau is not visited.
//   finally  sel_emit ranks the survivors and writes (id, value), the -1 / -inf padding and the count.
// These files are compiled with different floating-point flags: nothing here may hold a floating-point expression (the
// MFMA builtin and integer code are fine).
#pragma once
#include "common.h"

// ---- keys ------------------------------------------------------------------------------------------------------------
// COMPL: the id is stored complemented (equal values order by id ascending); else as it is (id descending)
template <bool COMPL>
static __device__ __forceinline__ uint64_t sel_make_key(float value, uint32_t id) {
  return ((uint64_t)f32_order_key(value) << 32) | (uint64_t)(COMPL ? ~id : id);
}
template <bool COMPL>
static __device__ __forceinline__ void sel_write_key(uint64_t key, int32_t* out_idx, float* out_val) {
  const uint32_t f = (uint32_t)(key & 0xFFFFFFFFull);
  *out_idx = (int32_t)(COMPL ? ~f : f);
  *out_val = f32_from_order_key((uint32_t)(key >> 32));
}

static __device__ __forceinline__ uint64_t sel_wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
static __device__ __forceinline__ uint64_t sel_wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off);
    v = o < v ? o : v;
  }
  return v;
}
// smallest key of buf[0..n)
static __device__ __forceinline__ uint64_t sel_buf_min(const uint64_t* buf, int n, int lane) {
  uint64_t m = ~0ull;
  for (int i = lane; i < n; i += 64) m = buf[i] < m ? buf[i] : m;
  return sel_wave_min_u64(m);
}

// append this lane's key (if valid) behind buf[0..n), in lane order; the caller has made room for 64 keys
static __device__ __forceinline__ void sel_append(uint64_t* buf, int& n, bool valid, uint64_t key, int lane) {
  const unsigned long long m = __ballot(valid);
  if (valid) buf[n + __popcll(m & ((1ull << lane) - 1))] = key;
  n += __popcll(m);
}

// is `id` in the ascending list[lo..hi)?  (P: LDS or global pointer; I: int, or int64_t for offsets into a whole CSR)
template <typename P, typename I>
static __device__ __forceinline__ bool sel_seen(P list, I lo, I hi, int32_t id) {
  const I end = hi;
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (list[mid] < id) lo = mid + 1; else hi = mid;
  }
  return lo < end && list[lo] == id;
}

// ---- radix select ----------------------------------------------------------------------------------------------------
// with the histogram of the current digit in hist[] (256 LDS words), find the digit that holds the `need`-th largest
// element; returns (digit, rank inside that digit's bin) wave-uniformly
static __device__ __forceinline__ void sel_radix_pick(const uint32_t* hist, int lane, int& need, int& digit) {
  uint32_t bins[4];
  uint32_t local = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    bins[b] = hist[lane * 4 + b];
    local += bins[b];
  }
  uint32_t suf = local;  // inclusive suffix sum over lanes >= lane
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_down(suf, off);
    if (lane + off < 64) suf += t;
  }
  const uint32_t above = suf - local;
  const bool mine = (above < (uint32_t)need) && ((uint32_t)need <= suf);
  int dg = 0, need_new = need;
  if (mine) {
    uint32_t c = above;
#pragma unroll
    for (int b = 3; b >= 0; --b) {
      if (c + bins[b] >= (uint32_t)need) {
        dg = lane * 4 + b;
        need_new = need - (int)c;
        break;
      }
      c += bins[b];
    }
  }
  const unsigned long long m = __ballot(mine);
  const int src = __ffsll((long long)m) - 1;
  digit = __shfl(dg, src);
  need = __shfl(need_new, src);
}

// k-th largest (1-based) of n 64-bit keys in LDS; the whole wave takes part.  Equal keys are counted as often as they
// occur (the histograms count elements, not values), so for a multiset this is its k-th largest element, and need_eq is
// the number of keys equal to it that belong to the k largest.
static __device__ uint64_t sel_radix_kth(const uint64_t* buf, int n, int kth, uint32_t* hist, int lane, int& need_eq) {
  uint64_t prefix = 0;
  int need = kth;
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = lane; i < 256; i += 64) hist[i] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
      const uint64_t key = buf[i];
      const bool match = (shift == 56) || ((key >> (shift + 8)) == (prefix >> (shift + 8)));
      if (match) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    int digit;
    sel_radix_pick(hist, lane, need, digit);
    prefix |= (uint64_t)digit << shift;
    __syncthreads();
  }
  need_eq = need;
  return prefix;
}

// keep the k largest keys of buf[0..n) at the front, in buffer order: every key above the k-th largest and the first
// need_eq of those equal to it.  Returns the new count, exactly min(n, k); from n >= k on, tau = the k-th largest key.
// MULTISET = false: the caller's keys are distinct, so "every key >= the k-th" is the same set and the equal-key count is
// compiled out (topk_select_kernel inlines its in-tile keep once per key slot: profiles/select_refactor_ab.md).
template <bool MULTISET = true>
static __device__ int sel_keep_topk(uint64_t* buf, int n, int k, uint32_t* hist, int lane, uint64_t& tau) {
  if (n < k) return n;
  if (n == k) {
    tau = sel_buf_min(buf, n, lane);
    return n;
  }
  int need_eq;
  const uint64_t thr = sel_radix_kth(buf, n, k, hist, lane, need_eq);
  const unsigned long long lt_mask = (1ull << lane) - 1;
  int cnt = 0, eq_seen = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const uint64_t key = (i < n) ? buf[i] : 0;
    bool keep = (i < n) && (key >= thr);
    if (MULTISET) {
      const bool is_eq = (i < n) && (key == thr);
      const unsigned long long me = __ballot(is_eq);
      keep = (i < n) && (key > thr || (is_eq && eq_seen + __popcll(me & lt_mask) < need_eq));
      eq_seen += __popcll(me);
    }
    const unsigned long long m = __ballot(keep);
    const int pos = cnt + __popcll(m & lt_mask);
    __syncthreads();
    if (keep) buf[pos] = key;
    cnt += __popcll(m);
    __syncthreads();
  }
  tau = thr;
  return cnt;
}
// the same for a caller that keeps tau its own way
template <bool MULTISET = true>
static __device__ int sel_keep_topk(uint64_t* buf, int n, int k, uint32_t* hist, int lane) {
  uint64_t tau;
  return sel_keep_topk<MULTISET>(buf, n, k, hist, lane, tau);
}

// ---- epilogue --------------------------------------------------------------------------------------------------------
// slots n..k-1 of a row's output and its count
static __device__ __forceinline__ void sel_pad(int n, int k, int lane, int32_t* out_idx, float* out_val, int32_t* out_cnt) {
  for (int i = n + lane; i < k; i += 64) {
    out_idx[i] = -1;
    out_val[i] = NEG_INF_F;
  }
  if (lane == 0) *out_cnt = n;
}
// rank the n <= k DISTINCT keys of buf and write the row (pairs_topk.hip ranks equal keys too: its pt_emit)
template <bool COMPL>
static __device__ __forceinline__ void sel_emit(const uint64_t* buf, int n, int k, int lane, int32_t* out_idx,
                                                float* out_val, int32_t* out_cnt) {
  for (int i = lane; i < n; i += 64) {
    const uint64_t ck = buf[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (buf[j] > ck) ? 1 : 0;
    sel_write_key<COMPL>(ck, out_idx + rank, out_val + rank);
  }
  sel_pad(n, k, lane, out_idx, out_val, out_cnt);
}

// ---- exact re-scoring of one tile of 32 candidate rows ---------------------------------------------------------------
// the MFMA chain of pass 1 (K steps ascending; A = candidate row `arow` of this lane, B = the row's vector in hf) on the
// caller's initial accumulator; the 32 scores land in scores[] (LDS), visible to the wave on return
template <int D>
static __device__ __forceinline__ void sel_score_tile(const uint16_t* __restrict__ E_b, int64_t arow,
                                                      const bf16x8 (&hf)[D / 16], f32x16 acc, float* scores, int r, int h) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s) {
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(E_b + arow * D + 16 * s + 8 * h);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, hf[s], acc, 0, 0, 0);
  }
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) scores[mfma_row(i, h)] = acc[i];
  }
  __syncthreads();
}

// ---- host: groups of candidate tiles, the transposed bound table -----------------------------------------------------
#define SEL_MAX_GROUPS 4096     // bounds per row (topk.hip keeps their keys in registers, item_knn.hip in 16 KiB of LDS)
struct SelGroups {
  int tg, ngroups, gstride;     // tiles of 32 candidates per group; groups; row stride of the transposed table
};
static inline SelGroups sel_groups(int64_t n_cand) {
  const int64_t tiles = (n_cand + 31) / 32;
  SelGroups g;
  g.tg = 1;
  while ((tiles + g.tg - 1) / g.tg > SEL_MAX_GROUPS) g.tg *= 2;
  g.ngroups = (int)((tiles + g.tg - 1) / g.tg);
  g.gstride = (g.ngroups + 63) / 64 * 64;
  return g;
}
// [groups][rows] -> [rows][gstride], the padding of a row filled with -inf (select_common.hip)
void cql_sel_transpose(const float* src, int ngroups, int64_t n_rows, float* dst, int gstride, hipStream_t s);
