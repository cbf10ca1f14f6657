// Item-to-item nearest neighbours (get_nearest_items, replay/models/base_rec.py:851-936, :955-1030) without
// materialising the queries x candidates similarity matrix.  Operand: the bf16 shadow rows of E_out; arithmetic fp32.
//
//   norms   item_norms_kernel: n_j = sum_t v_j[t]^2 (fp32; the products of bf16 values are exact).
//   gather  knn_gather_kernel: the query rows as one compact bf16 block + their norms.
//   pass 1  knn_bound_kernel: 256 queries per block stay in registers as MFMA B fragments, candidate rows stream
//           through LDS in stages of 64 rows (32 for d = 256; double buffered), dots from v_mfma_f32_32x32x16_bf16.  Per
//           (query, group of 32*tg candidates) ONE float leaves the chip: an upper bound of the metric over the group,
//           bound[group][query] (then transposed to [query][group]).  The bound is
//             dot_product             max of the dots                                  (= the group maximum, bit for bit)
//             euclidean_distance_sim  f(min x), x = (n_i + n_j) - 2 dot, f = 1/(1+sqrt(max(x,0)))  (f is non-increasing
//                                     under correctly rounded max / sqrt / + / divide: again the exact maximum)
//             cosine_similarity       max(dot * r_j) * r_i, r = 1/sqrt(n), pushed up by 2^-20 relative + 1e-30: two
//                                     multiplications instead of a division per pair.  The value proper,
//                                     dot / (sqrt(n_i) * sqrt(n_j)), and this product differ by at most six roundings
//                                     (< 2^-21 relative), so the inflated product is >= every value of the group.
//           Neither the self pair nor a zero-norm candidate nor the padding of the last stage (copies of the last
//           candidate) is masked here: a maximum over a superset is still an upper bound.
//   pass 2  knn_select_kernel, one wave per query, the exact threshold algorithm on the pieces of select_common.h.
//           Specific to this file: the bounds' keys live in LDS (gkey) and the groups are visited one at a time in
//           descending order of their bound; a group is re-scored with the SAME MFMA chain (acc = 0) followed by the
//           metric in the normative operation order; keys hold the neighbour id itself, not its complement: the
//           reference orders by (value desc, neighbour id DESC), base_rec.py:911-917.  The walk stops when the best
//           unvisited bound is below the value of the k-th best key so far.  Whatever pass 1 wrote only steers which
//           groups are re-scored; every value that is returned comes from pass 2.
//   No float atomics; the same call gives the same bits twice.  This file is compiled with -ffp-contract=off: the
//   metric expressions are normative in their operation order (NumPy float32 doing the same gives the same bits).
#include <stdlib.h>
#include "common.h"
#include "select_common.h"

#define KNN_MAX_K 512
#define KNN_CB 1024             // candidate keys in LDS per query (8 KiB)
// sel_keep_topk leaves at most k <= KNN_MAX_K keys, so a tile of 32 more always fits behind them
static_assert(KNN_CB >= 2 * KNN_MAX_K, "knn_select_kernel: no room to append after a tighten");
#define KNN_UNIT 64             // candidate slices start on multiples of this many rows
#define KNN_QPB 256             // queries per block of pass 1: 4 waves x 2 groups of 32
#define KNN_TARGET_BLOCKS 1024

// value of one pair in the normative operation order; false: the pair is not admissible (cosine with a zero denominator)
template <int M>
__device__ __forceinline__ bool knn_value(float dot, float ni, float nj, float& v) {
  if constexpr (M == CQLREC_SIM_DOT) {
    v = dot;
    return true;
  } else if constexpr (M == CQLREC_SIM_COSINE) {
    const float den = sqrtf(ni) * sqrtf(nj);
    v = dot / den;
    return den != 0.0f;
  } else {
    const float x = (ni + nj) - 2.0f * dot;
    v = 1.0f / (1.0f + sqrtf(fmaxf(x, 0.0f)));
    return true;
  }
}

__device__ __forceinline__ int64_t knn_clamp_row(int64_t r, int64_t n_rows) {
  return r < 0 ? 0 : (r >= n_rows ? n_rows - 1 : r);
}

// ---- squared norms: 8 lanes per row ---------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void item_norms_kernel(const uint16_t* __restrict__ E_b, int64_t n_rows,
                                                         float* __restrict__ norms) {
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7;
  float acc = 0.0f;
  if (row < n_rows) {
#pragma unroll
    for (int c = 0; c < D / 64; ++c) {
      const uint4 v = *reinterpret_cast<const uint4*>(E_b + row * D + (c * 8 + sub) * 8);
      float f[8];
      unpack_bf16x8(v, f);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc += f[j] * f[j];
    }
  }
#pragma unroll
  for (int off = 4; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  if (row < n_rows && sub == 0) norms[row] = acc;
}

// ---- query rows -> compact block ------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void knn_gather_kernel(const uint16_t* __restrict__ E_b, const float* __restrict__ norms,
                                                         int64_t n_rows, const int32_t* __restrict__ query_rows,
                                                         int64_t n_query, uint16_t* __restrict__ Qb,
                                                         float* __restrict__ qn) {
  constexpr int CH = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t q = i / CH;
  const int ch = (int)(i % CH);
  if (q >= n_query) return;
  const int64_t row = knn_clamp_row(query_rows[q], n_rows);
  *reinterpret_cast<uint4*>(Qb + q * D + ch * 8) = *reinterpret_cast<const uint4*>(E_b + row * D + ch * 8);
  if (ch == 0) qn[q] = norms[row];
}

// ---- pass 1 ---------------------------------------------------------------------------------------------------------
template <int D, int M>
__global__ __launch_bounds__(256) void knn_bound_kernel(const uint16_t* __restrict__ Qb, const float* __restrict__ qn,
                                                        int64_t n_query, const uint16_t* __restrict__ E_b,
                                                        const float* __restrict__ norms, int64_t n_rows,
                                                        const int32_t* __restrict__ cand_rows, int64_t n_cand,
                                                        int64_t split_rows, int tg, float* __restrict__ bound) {
  // stage = TPS tiles of 32 candidate rows: 64 rows (d <= 128), 32 rows (d = 256); two stage buffers of 16 KiB at most
  constexpr int KS = D / 16, CH = D / 8, TPS = (D == 256) ? 1 : 2, KNN_TC = 32 * TPS, NPF = KNN_TC * CH / 256;
  __shared__ __attribute__((aligned(16))) uint16_t tile[2][KNN_TC * D];
  __shared__ __attribute__((aligned(16))) float sv[2][KNN_TC];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t c_begin = (int64_t)blockIdx.y * split_rows;
  const int64_t c_end = (c_begin + split_rows < n_cand) ? c_begin + split_rows : n_cand;
  if (c_begin >= n_cand) return;
  const int nstages = (int)((c_end - c_begin + KNN_TC - 1) / KNN_TC);
  const int64_t t_last = (n_cand - 1) / 32;

  // query fragments of this wave's two groups (rows past the end repeat the last query; their bounds are not written)
  bf16x8 hf[2][KS];
  float ni[2];
  int64_t qrow[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    qrow[g] = (int64_t)blockIdx.x * KNN_QPB + wave * 64 + g * 32 + r;
    const int64_t q = qrow[g] < n_query ? qrow[g] : n_query - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) hf[g][s] = *reinterpret_cast<const bf16x8*>(Qb + q * D + 16 * s + 8 * h);
    const float n = qn[q];
    ni[g] = (M == CQLREC_SIM_COSINE) ? (n > 0.0f ? 1.0f / sqrtf(n) : 0.0f) : n;
  }

  auto table_row = [&](int64_t c) -> int64_t {
    const int64_t cc = c < n_cand ? c : n_cand - 1;
    return knn_clamp_row(cand_rows ? (int64_t)cand_rows[cc] : cc, n_rows);
  };
  uint4 pf[NPF];
  float pf_s = 0.0f;
  auto fetch = [&](int st) {
    const int64_t c0 = c_begin + (int64_t)st * KNN_TC;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int ci = tid + 256 * j, row = ci / CH, ch = ci % CH;
      pf[j] = *reinterpret_cast<const uint4*>(E_b + table_row(c0 + row) * D + ch * 8);
    }
    if (M != CQLREC_SIM_DOT && tid < KNN_TC) {
      const float n = norms[table_row(c0 + tid)];
      pf_s = (M == CQLREC_SIM_COSINE) ? (n > 0.0f ? 1.0f / sqrtf(n) : 0.0f) : n;
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int ci = tid + 256 * j, row = ci / CH, ch = ci % CH;
      *reinterpret_cast<uint4*>(&tile[buf][(row * CH + swz_chunk<D>(row, ch)) * 8]) = pf[j];
    }
    if (M != CQLREC_SIM_DOT && tid < KNN_TC) sv[buf][tid] = pf_s;
  };

  const float init = (M == CQLREC_SIM_EUCLID) ? __builtin_inff() : NEG_INF_F;
  float gm[2] = {init, init};
  fetch(0);
  stash(0);
  __syncthreads();
  for (int st = 0; st < nstages; ++st) {
    const int buf = st & 1;
    if (st + 1 < nstages) fetch(st + 1);
    const int64_t c0 = c_begin + (int64_t)st * KNN_TC;
#pragma unroll
    for (int t = 0; t < TPS; ++t) {
      const int64_t T = c0 / 32 + t;         // global tile index (c_begin is a multiple of 64)
      if (T > t_last) break;
      f32x16 acc[2];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        acc[0][i] = 0.0f;
        acc[1][i] = 0.0f;
      }
      const int row = t * 32 + r;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(&tile[buf][(row * CH + swz_chunk<D>(row, 2 * s + h)) * 8]);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, hf[0][s], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, hf[1][s], acc[1], 0, 0, 0);
      }
      const bool flush = ((T + 1) % tg == 0) || (T == t_last);
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        float m = gm[g];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float s4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
          if (M != CQLREC_SIM_DOT) {
            const float4 t4 = *reinterpret_cast<const float4*>(&sv[buf][t * 32 + 8 * j + 4 * h]);
            s4[0] = t4.x; s4[1] = t4.y; s4[2] = t4.z; s4[3] = t4.w;
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float dot = acc[g][4 * j + e];
            if (M == CQLREC_SIM_DOT) m = fmaxf(m, dot);
            else if (M == CQLREC_SIM_COSINE) m = fmaxf(m, dot * s4[e]);
            else m = fminf(m, (ni[g] + s4[e]) - 2.0f * dot);
          }
        }
        gm[g] = m;
        if (flush) {
          const float o = __shfl_xor(m, 32);
          m = (M == CQLREC_SIM_EUCLID) ? fminf(m, o) : fmaxf(m, o);
          float b;
          if (M == CQLREC_SIM_DOT) b = m;
          else if (M == CQLREC_SIM_COSINE) {
            b = m * ni[g];
            b = b + (fabsf(b) * 9.5367431640625e-07f + 1e-30f);      // 2^-20 relative: see the head of this file
          } else b = 1.0f / (1.0f + sqrtf(fmaxf(m, 0.0f)));
          if (h == 0 && qrow[g] < n_query) bound[(T / tg) * n_query + qrow[g]] = b;
          gm[g] = init;
        }
      }
    }
    if (st + 1 < nstages) stash(buf ^ 1);
    __syncthreads();
  }
}

// ---- pass 2 ---------------------------------------------------------------------------------------------------------
template <int D, int M>
__global__ __launch_bounds__(64) void knn_select_kernel(const uint16_t* __restrict__ Qb, const float* __restrict__ qn,
                                                        const int32_t* __restrict__ query_rows, int64_t n_query,
                                                        const uint16_t* __restrict__ E_b, const float* __restrict__ norms,
                                                        int64_t n_rows, const int32_t* __restrict__ cand_rows,
                                                        int64_t n_cand, const float* __restrict__ bound_t, int gstride,
                                                        int ngroups, int tg, int k, int32_t* __restrict__ out_idx,
                                                        float* __restrict__ out_val, int32_t* __restrict__ out_cnt) {
  constexpr int KS = D / 16;
  __shared__ uint32_t hist[256];
  __shared__ float scores[32];
  __shared__ uint64_t cand[KNN_CB];
  __shared__ uint32_t gkey[SEL_MAX_GROUPS];      // order keys of the bounds; 0 = visited

  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int64_t u = blockIdx.x;
  const int32_t my_id = query_rows[u];
  const float ni = qn[u];

  int ncand = 0;
  const bool dead = (M == CQLREC_SIM_COSINE) && !(sqrtf(ni) != 0.0f);    // every denominator is 0: no admissible pair
  if (!dead) {
    for (int g = lane; g < ngroups; g += 64) gkey[g] = f32_order_key(bound_t[u * gstride + g]);
    __syncthreads();
    bf16x8 hf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) hf[s] = *reinterpret_cast<const bf16x8*>(Qb + u * D + 16 * s + 8 * h);

    // this lane's best unvisited group (groups lane, lane + 64, ...)
    uint32_t bk = 0;
    int bg = 0;
    auto rescan = [&]() {
      bk = 0;
      bg = 0;
      for (int g = lane; g < ngroups; g += 64) {
        const uint32_t kk = gkey[g];
        if (kk > bk) {
          bk = kk;
          bg = g;
        }
      }
    };
    rescan();

    uint64_t tau = 0;        // k-th best key so far (valid once have_k)
    bool have_k = false;
    auto tighten = [&]() {
      ncand = sel_keep_topk(cand, ncand, k, hist, lane, tau);
      have_k = ncand >= k;
    };

    // exact re-scoring of one group (wave-uniform g): tg tiles of 32 candidates -> admissible ones appended to cand[]
    auto rescore = [&](int g) {
      for (int t = 0; t < tg; ++t) {
        const int64_t item0 = ((int64_t)g * tg + t) * 32;
        if (item0 >= n_cand) break;
        if (ncand + 32 > KNN_CB) tighten();
        const int64_t ca = (item0 + r < n_cand) ? item0 + r : n_cand - 1;
        const int64_t arow = knn_clamp_row(cand_rows ? (int64_t)cand_rows[ca] : ca, n_rows);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        sel_score_tile<D>(E_b, arow, hf, acc, scores, r, h);
        bool valid = false;
        uint64_t ck = 0;
        if (lane < 32 && item0 + lane < n_cand) {
          float v;
          const bool ok = knn_value<M>(scores[lane], ni, norms[arow], v);
          ck = sel_make_key<false>(v, (uint32_t)arow);
          valid = ok && ((int32_t)arow != my_id) && (!have_k || ck > tau);
        }
        sel_append(cand, ncand, valid, ck, lane);
        __syncthreads();
      }
    };

    const int slack = (k / 8 > 1) ? k / 8 : 1;
    for (;;) {
      const uint64_t c1 = bk ? (((uint64_t)bk << 32) | (uint64_t)(~(uint32_t)bg)) : 0ull;
      const uint64_t cw = sel_wave_max_u64(c1);
      if (cw == 0) break;                                                  // every group visited
      // a key of this group is at most (bound, largest id): it can enter only if the bound reaches tau's value
      if (have_k && (uint32_t)(cw >> 32) < (uint32_t)(tau >> 32)) break;
      const int g = (int)(~(uint32_t)(cw & 0xFFFFFFFFull));
      if (c1 == cw) {
        gkey[g] = 0;
        rescan();
      }
      rescore(g);
      if (ncand >= k && (!have_k || ncand - k >= slack)) tighten();
    }
    ncand = sel_keep_topk(cand, ncand, k, hist, lane);
    __syncthreads();
    // The ranking epilogue is written out here, not sel_emit behind the block: with the shared form the dot-product
    // instantiation ran 1 % slower than before (profiles/select_refactor_ab.md, "kNN").  ncand <= k, so every rank is
    // below k.  Candidate rows listed twice (outside the ABI's contract) give equal keys, which share a rank: one slot
    // of the row then stays unwritten, as before.
    for (int i = lane; i < ncand; i += 64) {
      const uint64_t ck = cand[i];
      int rank = 0;
      for (int j = 0; j < ncand; ++j) rank += (cand[j] > ck) ? 1 : 0;
      out_idx[u * k + rank] = (int32_t)(uint32_t)(ck & 0xFFFFFFFFull);
      out_val[u * k + rank] = f32_from_order_key((uint32_t)(ck >> 32));
    }
  }
  for (int i = ncand + lane; i < k; i += 64) {
    out_idx[u * k + i] = -1;
    out_val[u * k + i] = NEG_INF_F;
  }
  if (lane == 0) out_cnt[u] = ncand;
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct KnnWs {
  int64_t off_q, off_qn, off_b, off_bt, total;
  SelGroups g;
};
static KnnWs knn_ws_layout(int64_t n_query, int64_t n_cand, int32_t d) {
  KnnWs w;
  w.g = sel_groups(n_cand);
  w.off_q = 0;
  w.off_qn = w.off_q + cql_align256(n_query * d * 2);
  w.off_b = w.off_qn + cql_align256(n_query * 4);
  w.off_bt = w.off_b + cql_align256((int64_t)w.g.ngroups * n_query * 4);
  w.total = w.off_bt + cql_align256((int64_t)w.g.gstride * n_query * 4) + 256;
  return w;
}

extern "C" int64_t cqlrec_item_knn_ws_bytes(int64_t n_query, int64_t n_cand, int32_t d, int32_t k) {
  (void)k;
  if (n_query <= 0 || n_cand <= 0 || !cql_d_ok(d)) return 0;
  return knn_ws_layout(n_query, n_cand, d).total;
}

extern "C" int cqlrec_item_norms(const uint16_t* E_b, int64_t n_rows, int32_t d, float* norms, cqlrec_stream stream) {
  CQL_REQUIRE(E_b && norms, "item_norms: NULL pointer");
  CQL_REQUIRE(cql_d_ok(d), "item_norms: d=%d unsupported", d);
  CQL_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "item_norms: n_rows=%lld", (long long)n_rows);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cql_ceil_div(n_rows * 8, 256)), block(256);
  const int rc = cql_by_d(d, [&](auto D) {
    hipLaunchKernelGGL((item_norms_kernel<decltype(D)::value>), grid, block, 0, s, E_b, n_rows, norms);
  });
  CQL_LAUNCH_CHECK("item_norms");
  return rc;
}

template <int D, int M>
static void knn_launch(const uint16_t* E_b, const float* norms, int64_t n_rows, const int32_t* query_rows, int64_t n_query,
                       const int32_t* cand_rows, int64_t n_cand, int32_t k, char* ws, const KnnWs& w, int32_t* out_idx,
                       float* out_val, int32_t* out_cnt, hipStream_t s) {
  uint16_t* Qb = (uint16_t*)(ws + w.off_q);
  float* qn = (float*)(ws + w.off_qn);
  float* bound = (float*)(ws + w.off_b);
  float* bound_t = (float*)(ws + w.off_bt);
  hipLaunchKernelGGL((knn_gather_kernel<D>), dim3(cql_ceil_div(n_query * (D / 8), 256)), dim3(256), 0, s, E_b, norms, n_rows,
                     query_rows, n_query, Qb, qn);
  // candidate slices: whole groups and whole stages, enough blocks to fill the chip
  const int64_t unit = (32 * w.g.tg > KNN_UNIT) ? 32 * w.g.tg : KNN_UNIT;
  const int64_t units = (n_cand + unit - 1) / unit;
  const int64_t qblocks = (n_query + KNN_QPB - 1) / KNN_QPB;
  int64_t nsplit = (KNN_TARGET_BLOCKS + qblocks - 1) / qblocks;
  if (nsplit > units) nsplit = units;
  if (nsplit > 65535) nsplit = 65535;
  const int64_t split_rows = (units + nsplit - 1) / nsplit * unit;
  nsplit = (n_cand + split_rows - 1) / split_rows;
  hipLaunchKernelGGL((knn_bound_kernel<D, M>), dim3((unsigned)qblocks, (unsigned)nsplit), dim3(256), 0, s,
                     (const uint16_t*)Qb, (const float*)qn, n_query, E_b, norms, n_rows, cand_rows, n_cand, split_rows, w.g.tg,
                     bound);
  cql_sel_transpose(bound, w.g.ngroups, n_query, bound_t, w.g.gstride, s);
  hipLaunchKernelGGL((knn_select_kernel<D, M>), dim3((unsigned)n_query), dim3(64), 0, s, (const uint16_t*)Qb,
                     (const float*)qn, query_rows, n_query, E_b, norms, n_rows, cand_rows, n_cand, (const float*)bound_t,
                     w.g.gstride, w.g.ngroups, w.g.tg, k, out_idx, out_val, out_cnt);
}

extern "C" int cqlrec_item_knn(const uint16_t* E_b, const float* norms, int64_t n_rows, int32_t d, const int32_t* query_rows,
                               int64_t n_query, const int32_t* cand_rows, int64_t n_cand, int32_t metric, int32_t k, void* ws,
                               int64_t ws_bytes, int32_t* out_idx, float* out_val, int32_t* out_cnt, cqlrec_stream stream) {
  CQL_REQUIRE(E_b && norms && query_rows && ws && out_idx && out_val && out_cnt, "item_knn: NULL pointer");
  CQL_REQUIRE(cql_d_ok(d), "item_knn: d=%d unsupported", d);
  CQL_REQUIRE(n_rows > 0 && n_rows < (1ll << 31), "item_knn: n_rows=%lld", (long long)n_rows);
  CQL_REQUIRE(n_query > 0 && n_query < (1ll << 31), "item_knn: n_query=%lld", (long long)n_query);
  CQL_REQUIRE(n_cand > 0 && n_cand <= n_rows, "item_knn: n_cand=%lld (1..n_rows=%lld)", (long long)n_cand, (long long)n_rows);
  CQL_REQUIRE(cand_rows != nullptr || n_cand == n_rows, "item_knn: cand_rows is NULL, so n_cand must equal n_rows");
  CQL_REQUIRE(metric == CQLREC_SIM_DOT || metric == CQLREC_SIM_COSINE || metric == CQLREC_SIM_EUCLID,
              "item_knn: metric=%d (CQLREC_SIM_DOT, _COSINE or _EUCLID)", metric);
  CQL_REQUIRE(k > 0 && k <= KNN_MAX_K, "item_knn: k=%d out of range (1..%d)", k, KNN_MAX_K);
  const KnnWs w = knn_ws_layout(n_query, n_cand, d);
  CQL_REQUIRE(ws_bytes >= w.total, "item_knn: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const int rc = cql_by_d(d, [&](auto D) {
    cql_dispatch<CQLREC_SIM_DOT, CQLREC_SIM_COSINE, CQLREC_SIM_EUCLID>(metric, [&](auto M) {   // metric: checked above
      knn_launch<decltype(D)::value, decltype(M)::value>(E_b, norms, n_rows, query_rows, n_query, cand_rows, n_cand, k,
                                                         (char*)ws, w, out_idx, out_val, out_cnt, s);
    });
  });
  CQL_LAUNCH_CHECK("item_knn");
  return rc;
}
