// Wave-level selection helpers over 64-bit keys in LDS (one wave per block; the scheme of topk.hip): shared by
// item_knn.hip and pairs_topk.hip.
#pragma once
#include "common.h"

// ---- selection helpers (one wave; the scheme of topk.hip) -----------------------------------------------------------
// with the histogram of the current digit in hist[], find the digit that holds the `need`-th largest element
static __device__ __forceinline__ void knn_radix_pick(const uint32_t* hist, int lane, int& need, int& digit) {
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

// k-th largest (1-based) of n 64-bit keys in LDS.  Equal keys are counted as often as they occur (the histograms count
// elements, not values), so for a multiset this is its k-th largest element: pairs_topk.hip relies on that.
static __device__ uint64_t knn_radix_kth(const uint64_t* buf, int n, int kth, uint32_t* hist, int lane) {
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
    knn_radix_pick(hist, lane, need, digit);
    prefix |= (uint64_t)digit << shift;
    __syncthreads();
  }
  return prefix;
}

// keep the k largest keys of buf[0..n) at the front (unordered); returns the new count
static __device__ int knn_keep_topk(uint64_t* buf, int n, int k, uint32_t* hist, int lane) {
  if (n <= k) return n;
  const uint64_t thr = knn_radix_kth(buf, n, k, hist, lane);
  int cnt = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    const uint64_t key = (i < n) ? buf[i] : 0;
    const bool keep = (i < n) && (key >= thr);
    const unsigned long long m = __ballot(keep);
    const int pos = cnt + __popcll(m & ((1ull << lane) - 1));
    __syncthreads();
    if (keep) buf[pos] = key;
    cnt += __popcll(m);
    __syncthreads();
  }
  return cnt;
}

static __device__ __forceinline__ uint64_t knn_wave_max_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t o = __shfl_xor(v, off);
    v = o > v ? o : v;
  }
  return v;
}
