// Ranking of per-row candidate lists (predict_pairs with k, replay/models/base_rec.py:725-782): scores of a ragged CSR
// of (row, item) pairs and, per row, the k best admissible pairs -- without expanding the state vectors to one per pair.
//
//   unit of work  a PIECE: a contiguous run of one row's candidates, handled by one wave (one 64-thread block).  A row is
//                 one piece unless it is longer than the piece length P = max(4096, L / 8192), L = the summed length of
//                 all rows above 4096 (pt_plan_kernel: one integer sum).  Such a row is cut into ceil(len / P) pieces; the
//                 pieces after the first go to a table of at most 8192 entries (sum of (ceil(len/P) - 1) <= L / P), so
//                 the workspace depends on k alone and rows of any length run in one launch sequence.
//   score         the wave holds its row's h in registers (read once per piece): lane c of a group of d/8 lanes keeps
//                 elements 8c..8c+7.  64 / (d/8) groups each gather one E_out row per step, four steps in flight
//                 (4 rows in flight per lane group: 4 KiB per wave), the next steps' item ids already loaded.  Arithmetic
//                 is gather_dot_kernel's (state_side.hip), operation for operation: eight sequential fmaf from 0 per lane, the
//                 xor butterfly over the group, + b[item] -- the same bits, which is what lets predict_pairs(k) return
//                 the frame the host path returned.  Scores of a chunk of 256 candidates wait in LDS.
//   admit         all 64 lanes then take one candidate each: the score goes to out_score (coalesced), the row's seen
//                 list is searched, admissible pairs become keys (score desc, item id asc) in an LDS buffer of 1024;
//                 once a k-th best key tau is known only keys above it are appended (select_common.h).
//   select        when the buffer cannot take another chunk: sel_keep_topk.  A candidate listed twice gives the same
//                 key twice; the shared select counts such keys as often as they occur.
//                 At the end the survivors are ranked (rank = keys above + equal keys before) and written: to the row's
//                 output (the only or first piece) or, as keys, to the piece's slot of the workspace.
//   merge         one wave per cut row: the keys of its output and of its further pieces through the same buffer.
//   Integer atomics hand out table slots (their order varies; what the slots hold does not); no float atomics, every
//   output is a pure function of the inputs.  Compiled with -ffp-contract=off like state_side.hip.
#include "common.h"
#include "select_common.h"

#define PT_MAX_K CQLREC_PAIRS_MAX_K
#define PT_CB 1024          // keys in LDS per wave (8 KiB) >= PT_MAX_K + 2 * PT_CHUNK
#define PT_CHUNK 256        // candidates scored between two admit phases
#define PT_PIECE_MIN 4096   // rows up to this length are never cut
#define PT_MAX_EXTRA 8192   // pieces beyond the first of their row
#define PT_MAX_ROWS (1ll << 26)   // rows per call: one block of 64 threads each, 2^32 threads per launch
#define PT_DIRECT 256       // lists up to this length are ranked without a radix select first

struct PtHeader {
  unsigned long long long_total;   // summed length of the selected rows above PT_PIECE_MIN
  uint32_t n_extra, n_long;
};
struct PtLong { int32_t sel, pbase, extra, pad; };
struct PtPiece { int32_t sel, q; };       // sel < 0: unused slot

struct PtArgs {
  const uint16_t* H;
  const uint16_t* E;
  const float* b;
  int64_t n_items;
  const int64_t* pair_off;
  const int32_t* pair_items;
  const int32_t* rows;
  int64_t n_sel;
  const int64_t* seen_off;
  const int32_t* seen_items;
  int32_t k;
  float* out_score;
  int32_t* out_idx;
  float* out_val;
  int32_t* out_cnt;
  PtHeader* hdr;
  PtLong* long_tab;
  PtPiece* piece_tab;
  uint64_t* part;                // [PT_MAX_EXTRA][k] keys, 0 = none
};

__device__ __forceinline__ int64_t pt_piece_len(unsigned long long long_total) {
  const int64_t p = (int64_t)((long_total + PT_MAX_EXTRA - 1) / PT_MAX_EXTRA);
  return p < PT_PIECE_MIN ? PT_PIECE_MIN : p;
}
__device__ __forceinline__ void pt_row_range(const PtArgs& a, int64_t i, int64_t& r, int64_t& lo, int64_t& len) {
  r = a.rows ? (int64_t)a.rows[i] : i;
  lo = a.pair_off[r];
  len = a.pair_off[r + 1] - lo;
  if (len < 0) len = 0;
}

// ---- plan: L ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pt_plan_kernel(PtArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned long long v = 0;
  if (i < a.n_sel) {
    int64_t r, lo, len;
    pt_row_range(a, i, r, lo, len);
    if (len > PT_PIECE_MIN) v = (unsigned long long)len;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.hdr->long_total, v);
}

// ---- the k largest keys of a buffer, duplicates counted --------------------------------------------------------------
struct PtSel {
  int ncand;
  uint64_t tau;   // k-th best key so far (valid once have_k)
  bool have_k;
};

// (every caller has more than k keys in the buffer; at exactly k, tau would be their minimum: also a valid bound)
static __device__ void pt_tighten(uint64_t* buf, PtSel& s, int k, uint32_t* hist, int lane) {
  s.ncand = sel_keep_topk(buf, s.ncand, k, hist, lane, s.tau);
  s.have_k = s.ncand >= k;
}

// rank the survivors and write them: to the row's output, or as keys to part_dst[0..k)
static __device__ void pt_emit(uint64_t* buf, PtSel& s, int k, uint32_t* hist, int lane, int32_t* out_idx,
                               float* out_val, int32_t* out_cnt, uint64_t* part_dst) {
  if (s.ncand > k && s.ncand > PT_DIRECT) pt_tighten(buf, s, k, hist, lane);
  const int n = s.ncand;
  if ((n & 1) && lane == 0) buf[n] = 0;       // n odd => n < PT_CB: the pair-wise loop below reads one key past the end
  __syncthreads();
  for (int i = lane; i < n; i += 64) {
    const uint64_t key = buf[i];
    int rank = 0;
    for (int j = 0; j < n; j += 2) {
      const ulonglong2 kk = *reinterpret_cast<const ulonglong2*>(&buf[j]);
      rank += (kk.x > key || (kk.x == key && j < i)) ? 1 : 0;
      rank += (kk.y > key || (kk.y == key && j + 1 < i)) ? 1 : 0;
    }
    if (rank < k) {
      if (part_dst) part_dst[rank] = key;
      else sel_write_key<true>(key, out_idx + rank, out_val + rank);
    }
  }
  const int cnt = n < k ? n : k;
  for (int i = cnt + lane; i < k; i += 64) {
    if (part_dst) part_dst[i] = 0;
    else {
      out_idx[i] = -1;
      out_val[i] = NEG_INF_F;
    }
  }
  if (!part_dst && lane == 0) *out_cnt = cnt;
}

// ---- one piece: candidates [lo, lo + n) of CSR row r, state vector i -------------------------------------------------
template <int D>
static __device__ void pt_run_piece(const PtArgs& a, int64_t i, int64_t r, int64_t lo, int64_t n,
                                    uint64_t* part_dst, uint64_t* buf, float* sc, uint32_t* hist) {
  constexpr int LPR = D / 8, RPW = 64 / LPR, U = 4, STEP = RPW * U;
  const int lane = threadIdx.x, g = lane / LPR, c = lane % LPR;
  const int k = a.k;
  const int32_t last_item = (int32_t)(a.n_items - 1);

  float hf[8];
  unpack_bf16x8(*reinterpret_cast<const uint4*>(a.H + i * D + c * 8), hf);
  int64_t s_lo = 0, s_hi = 0;
  if (a.seen_off) {
    s_lo = a.seen_off[r];
    s_hi = a.seen_off[r + 1];
  }
  PtSel sel = {0, 0ull, false};

  for (int64_t c0 = 0; c0 < n; c0 += PT_CHUNK) {
    const int m = (int)((n - c0 < PT_CHUNK) ? n - c0 : PT_CHUNK);
    const int32_t* __restrict__ items = a.pair_items + lo + c0;
    // score: sc[j] = <h, E[items[j]]> + b[items[j]], gather_dot_kernel's operation order
    int32_t nxt[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = u * RPW + g;
      nxt[u] = (j < m) ? items[j] : 0;
    }
    for (int j0 = 0; j0 < m; j0 += STEP) {
      int32_t it[U];
      uint4 ev[U];
      float bb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t raw = nxt[u];
        it[u] = raw < 0 ? 0 : (raw > last_item ? last_item : raw);     // loads stay inside the table whatever the list holds
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ev[u] = *reinterpret_cast<const uint4*>(a.E + (int64_t)it[u] * D + c * 8);
        bb[u] = a.b[it[u]];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + STEP + u * RPW + g;
        nxt[u] = (j < m) ? items[j] : 0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float ef[8];
        unpack_bf16x8(ev[u], ef);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s = fmaf(hf[e], ef[e], s);
#pragma unroll
        for (int off = 1; off < LPR; off <<= 1) s += __shfl_xor(s, off);
        const int j = j0 + u * RPW + g;
        if (j < m && c == 0) sc[j] = s + bb[u];
      }
    }
    __syncthreads();
    // admit: one candidate per lane
    if (k > 0 && sel.ncand + PT_CHUNK > PT_CB) pt_tighten(buf, sel, k, hist, lane);
    for (int j0 = 0; j0 < m; j0 += 64) {
      const int j = j0 + lane;
      const bool ok = j < m;
      const int32_t item = ok ? items[j] : 0;
      const float s = ok ? sc[j] : 0.f;
      if (ok && a.out_score) a.out_score[lo + c0 + j] = s;
      if (k > 0) {
        const bool adm = ok && !sel_seen(a.seen_items, s_lo, s_hi, item);
        const uint64_t key = sel_make_key<true>(s, (uint32_t)item);
        sel_append(buf, sel.ncand, adm && (!sel.have_k || key > sel.tau), key, lane);
      }
    }
    __syncthreads();
  }
  if (k > 0)
    pt_emit(buf, sel, k, hist, lane, a.out_idx + i * k, a.out_val + i * k, a.out_cnt + i, part_dst);
}

// one wave per selected row: the whole row, or the first piece of a cut row (whose further pieces it registers)
template <int D>
__global__ __launch_bounds__(64) void pt_row_kernel(PtArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t buf[PT_CB];
  __shared__ float sc[PT_CHUNK];
  __shared__ uint32_t hist[256];
  const int lane = threadIdx.x;
  const int64_t i = blockIdx.x;
  int64_t r, lo, len;
  pt_row_range(a, i, r, lo, len);
  const int64_t P = pt_piece_len(a.hdr->long_total);
  int64_t n0 = len;
  if (len > P) {
    const int64_t extra64 = (len + P - 1) / P - 1;       // <= len / P <= PT_MAX_EXTRA
    int extra = extra64 > PT_MAX_EXTRA ? 0 : (int)extra64;
    int pbase = 0;
    if (lane == 0 && extra > 0) {
      pbase = (int)atomicAdd(&a.hdr->n_extra, (uint32_t)extra);
      // cannot overflow while the rows are distinct (the bound above); if it does, this wave takes the whole row
      if ((int64_t)pbase + extra > PT_MAX_EXTRA) extra = 0;
      else {
        const int slot = (int)atomicAdd(&a.hdr->n_long, 1u);
        a.long_tab[slot] = PtLong{(int32_t)i, pbase, extra, 0};
      }
    }
    extra = __shfl(extra, 0);
    pbase = __shfl(pbase, 0);
    for (int q = lane; q < extra; q += 64) a.piece_tab[pbase + q] = PtPiece{(int32_t)i, q + 1};
    if (extra > 0) n0 = P;
  }
  pt_run_piece<D>(a, i, r, lo, n0, nullptr, buf, sc, hist);
}

// the further pieces of the cut rows
template <int D>
__global__ __launch_bounds__(64) void pt_piece_kernel(PtArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t buf[PT_CB];
  __shared__ float sc[PT_CHUNK];
  __shared__ uint32_t hist[256];
  const int p = blockIdx.x;
  const PtPiece e = a.piece_tab[p];
  if (e.sel < 0) return;
  const int64_t i = e.sel;
  int64_t r, lo, len;
  pt_row_range(a, i, r, lo, len);
  const int64_t P = pt_piece_len(a.hdr->long_total);
  const int64_t begin = (int64_t)e.q * P;
  if (begin >= len) return;
  const int64_t n = (len - begin < P) ? len - begin : P;
  pt_run_piece<D>(a, i, r, lo + begin, n, a.part + (int64_t)p * a.k, buf, sc, hist);
}

// one wave per cut row: its output (the first piece's list) and the lists of its further pieces -> its output
__global__ __launch_bounds__(64) void pt_merge_kernel(PtArgs a) {
  __shared__ __attribute__((aligned(16))) uint64_t buf[PT_CB];
  __shared__ uint32_t hist[256];
  const int lane = threadIdx.x;
  if (blockIdx.x >= a.hdr->n_long) return;
  const PtLong e = a.long_tab[blockIdx.x];
  const int64_t i = e.sel;
  const int k = a.k;
  PtSel sel = {0, 0ull, false};
  const int cnt0 = a.out_cnt[i];
  for (int t = lane; t < cnt0; t += 64)
    buf[t] = sel_make_key<true>(a.out_val[i * k + t], (uint32_t)a.out_idx[i * k + t]);
  sel.ncand = cnt0;
  __syncthreads();
  const uint64_t* __restrict__ src = a.part + (int64_t)e.pbase * k;
  const int64_t total = (int64_t)e.extra * k;
  for (int64_t t0 = 0; t0 < total; t0 += 64) {
    if (sel.ncand + 64 > PT_CB) pt_tighten(buf, sel, k, hist, lane);
    const int64_t t = t0 + lane;
    const uint64_t key = (t < total) ? src[t] : 0ull;
    sel_append(buf, sel.ncand, key != 0ull && (!sel.have_k || key > sel.tau), key, lane);
    __syncthreads();
  }
  pt_emit(buf, sel, k, hist, lane, a.out_idx + i * k, a.out_val + i * k, a.out_cnt + i, nullptr);
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct PtWs {
  int64_t off_long, off_piece, off_part, total;
};
static PtWs pt_ws_layout(int32_t k) {
  PtWs w;
  w.off_long = 256;
  w.off_piece = w.off_long + (int64_t)PT_MAX_EXTRA * (int64_t)sizeof(PtLong);
  w.off_part = w.off_piece + (int64_t)PT_MAX_EXTRA * (int64_t)sizeof(PtPiece);
  w.total = w.off_part + (int64_t)PT_MAX_EXTRA * k * 8 + 256;
  return w;
}

extern "C" int64_t cqlrec_pairs_topk_ws_bytes(int64_t n_sel, int64_t nnz, int32_t d, int32_t k) {
  if (n_sel <= 0 || n_sel > PT_MAX_ROWS || nnz < 0 || !cql_d_ok(d) || k < 0 || k > PT_MAX_K) return 0;
  return pt_ws_layout(k).total;       // the piece table is bounded whatever the list lengths: see the head of this file
}

extern "C" int cqlrec_pairs_topk(const uint16_t* H_b, const uint16_t* E_b, const float* b, int64_t n_items, int32_t d,
                                 const int64_t* pair_off, const int32_t* pair_items, const int32_t* rows, int64_t n_sel,
                                 const int64_t* seen_off, const int32_t* seen_items, int32_t k, void* ws,
                                 int64_t ws_bytes, float* out_score, int32_t* out_idx, float* out_val, int32_t* out_cnt,
                                 cqlrec_stream stream) {
  CQL_REQUIRE(H_b && E_b && b && pair_off && pair_items && ws, "pairs_topk: NULL pointer");
  CQL_REQUIRE(cql_d_ok(d), "pairs_topk: d=%d unsupported", d);
  CQL_REQUIRE(k >= 0 && k <= PT_MAX_K, "pairs_topk: k=%d out of range (0..%d)", k, PT_MAX_K);
  CQL_REQUIRE(n_items > 0 && n_items < (1ll << 31), "pairs_topk: n_items=%lld", (long long)n_items);
  // one 64-thread block per row: 2^26 rows are the 2^32 threads a launch may have
  CQL_REQUIRE(n_sel >= 0 && n_sel <= PT_MAX_ROWS, "pairs_topk: n_sel=%lld out of range (0..%lld per call)", (long long)n_sel,
              (long long)PT_MAX_ROWS);
  CQL_REQUIRE((seen_off == nullptr) == (seen_items == nullptr), "pairs_topk: seen_off and seen_items go together");
  if (k == 0) {
    CQL_REQUIRE(out_score != nullptr, "pairs_topk: k=0 asks for scores only, out_score is NULL");
    CQL_REQUIRE(!out_idx && !out_val && !out_cnt, "pairs_topk: k=0, so out_idx / out_val / out_cnt must be NULL");
  } else {
    CQL_REQUIRE(out_idx && out_val && out_cnt, "pairs_topk: NULL output pointer");
  }
  const PtWs w = pt_ws_layout(k);
  CQL_REQUIRE(ws_bytes >= w.total, "pairs_topk: workspace too small");
  if (n_sel == 0) return CQLREC_OK;
  hipStream_t s = (hipStream_t)stream;
  char* base = (char*)ws;
  PtArgs a;
  a.H = H_b; a.E = E_b; a.b = b; a.n_items = n_items;
  a.pair_off = pair_off; a.pair_items = pair_items; a.rows = rows; a.n_sel = n_sel;
  a.seen_off = seen_off; a.seen_items = seen_items; a.k = k;
  a.out_score = out_score; a.out_idx = out_idx; a.out_val = out_val; a.out_cnt = out_cnt;
  a.hdr = (PtHeader*)base;
  a.long_tab = (PtLong*)(base + w.off_long);
  a.piece_tab = (PtPiece*)(base + w.off_piece);
  a.part = (uint64_t*)(base + w.off_part);
  if (hipMemsetAsync(base, 0, 256, s) != hipSuccess ||
      hipMemsetAsync(base + w.off_piece, 0xFF, (size_t)PT_MAX_EXTRA * sizeof(PtPiece), s) != hipSuccess) {
    cql_set_error("pairs_topk: hipMemsetAsync failed");
    return CQLREC_ERR_HIP;
  }
  hipLaunchKernelGGL(pt_plan_kernel, dim3(cql_ceil_div(n_sel, 256)), dim3(256), 0, s, a);
  const int rc = cql_by_d(d, [&](auto D) {
    hipLaunchKernelGGL(pt_row_kernel<decltype(D)::value>, dim3((unsigned)n_sel), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pt_piece_kernel<decltype(D)::value>, dim3(PT_MAX_EXTRA), dim3(64), 0, s, a);
  });
  if (rc != CQLREC_OK) return rc;
  if (k > 0) hipLaunchKernelGGL(pt_merge_kernel, dim3(PT_MAX_EXTRA), dim3(64), 0, s, a);
  CQL_LAUNCH_CHECK("pairs_topk");
  return CQLREC_OK;
}
