// f11  dense fp64 linear algebra on the device, and ADMM SLIM on top of it (ADMMSLIM of replay/models/admm_slim.py;
// DESIGN.md section 3.14 is the normative text): a GEMM on the fp64 matrix pipe, the dense Gram matrix of a log, the
// explicit inverse of a symmetric positive definite matrix by a blocked Cholesky factorisation, one ADMM iteration as
// that GEMM with a fused element-wise epilogue, and dense -> CSR.
// The rules of f5 - f10 hold: integer atomics only, no floating-point atomics, the same input gives the same bytes.
// Built with -ffp-contract=off: every element-wise expression is evaluated as written.
//
// The GEMM.  One workgroup of four waves owns a 128 x 128 tile of D, each wave a 64 x 64 quarter of it as 4 x 4
// accumulators of v_mfma_f64_16x16x4_f64.  That instruction has a layout of its own:
//   A operand   lane l holds A[row l & 15][k = l >> 4]         (one fp64 per lane)
//   B operand   lane l holds B[k = l >> 4][col l & 15]
//   C / D       lane l, register r of 4: row = (l >> 4) + 4 r, col = l & 15
// k runs in slabs of 16 through LDS, both operands stored [k][x] with a row stride of 144 doubles: the 16 lanes of
// one k read 128 consecutive bytes and the next k starts 128 bytes further modulo the 256 bytes of all banks, so a
// ds_read_b64 of 32 lanes touches every bank once.  LDS holds two slabs: the next one travels from memory through
// registers into the other buffer while the matrix pipe works on the current one, one barrier per slab.  Edges are predicated: a row, column or k beyond the matrix reads +0.0 and is not
// stored.  An element of D is the sum over k ascending -- slab after slab, four k per instruction -- whatever the
// grid: there is no split over k.

#include "common.h"

typedef __attribute__((ext_vector_type(4))) double f64x4;

#define DG_BM 128
#define DG_BK 16
#define DG_LD 144
#define DG_NB CQLREC_DENSE_BLOCK
enum { DG_LOWER_ONLY = 1, DG_K_FROM_DIAG = 2 };
enum { DG_AXPBY = 0, DG_ADMM = 1 };
static const int64_t DG_MAX_MN = 1ll << 22, DG_MAX_K = 1ll << 31, DG_MAX_N = 1ll << 16;

struct DgArgs {
  const double* A;                  // op(A) is m x k
  const double* B;                  // op(B) is k x n
  const double* E;                  // m x n, read when beta != 0 (ADMM: P)
  double* D;                        // m x n (ADMM: unused)
  int64_t lda, ldb, lde, ldd;
  int32_t m, n, k, ta, tb, flags;
  double alpha, beta;
  // the ADMM epilogue: A is W, B is rho C - Gamma, E is P; all n x n with the leading dimension n
  const double* v;                  // [n] T_jj / W_jj
  double* C;
  double* Gm;
  double* part;                     // [tiles][5]
  double rho, coef;
};

// eight consecutive elements of one operand slab per thread.  contig_k: element (x, kk) lies at P[x * ld + kk] (thread t:
// x = t / 2, kk = 8 (t & 1) ..); otherwise at P[kk * ld + x] (thread t: kk = t / 16, x = 8 (t & 15) ..)
static __device__ __forceinline__ void dg_load(double (&r)[8], const double* __restrict__ P, int64_t ld, bool contig_k,
                                               int x0, int xmax, int k0, int kmax, int t) {
  int row, colb, rmax, cmax;        // the operand as stored: row-major [row][col], eight consecutive columns
  if (contig_k) { row = x0 + (t >> 1); colb = k0 + (t & 1) * 8; rmax = xmax; cmax = kmax; }
  else { row = k0 + (t >> 4); colb = x0 + (t & 15) * 8; rmax = kmax; cmax = xmax; }
  const double* p = P + (int64_t)row * ld + colb;
  if (row < rmax && colb + 8 <= cmax && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double2 w = q[j];
      r[2 * j] = w.x;
      r[2 * j + 1] = w.y;
    }
  } else if (row < rmax && colb + 8 <= cmax) {          // an odd leading dimension: one element, three aligned pairs, one element
    const double2* q = reinterpret_cast<const double2*>(p + 1);
    r[0] = p[0];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double2 w = q[j];
      r[2 * j + 1] = w.x;
      r[2 * j + 2] = w.y;
    }
    r[7] = p[7];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (row < rmax && colb + j < cmax) ? p[j] : 0.0;
  }
}
static __device__ __forceinline__ void dg_store(double (*S)[DG_LD], const double (&r)[8], bool contig_k, int t) {
  if (contig_k) {
    const int x = t >> 1, kb = (t & 1) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) S[kb + j][x] = r[j];
  } else {
    const int kk = t >> 4, xb = (t & 15) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) S[kk][xb + j] = r[j];
  }
}

static __device__ __forceinline__ double dg_wave_sum(double x) {      // butterfly: every lane ends with the same sum
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x = x + __shfl_xor(x, o, 64);
  return x;
}

template <int MODE>
__global__ __launch_bounds__(256) void dense_gemm_kernel(DgArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dg_smem[];
  double (*As)[DG_BK][DG_LD] = reinterpret_cast<double (*)[DG_BK][DG_LD]>(dg_smem);     // [2]: the slab at work, the next one
  double (*Bs)[DG_BK][DG_LD] = As + 2;
  __shared__ double red[4][5];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row0 = blockIdx.y * DG_BM, col0 = blockIdx.x * DG_BM;
  if ((g.flags & DG_LOWER_ONLY) && row0 + DG_BM <= col0) return;
  const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
  const int lr = lane & 15, lk = lane >> 4;
  const bool a_ck = g.ta == 0, b_ck = g.tb != 0;

  f64x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  int k0 = 0, buf = 0;
  if (g.flags & DG_K_FROM_DIAG) k0 = (row0 > col0 ? row0 : col0) / DG_BK * DG_BK;   // the terms in front are exact zeros
  double ra[8], rb[8];
  if (k0 < g.k) {
    dg_load(ra, g.A, g.lda, a_ck, row0, g.m, k0, g.k, t);
    dg_load(rb, g.B, g.ldb, b_ck, col0, g.n, k0, g.k, t);
    dg_store(As[0], ra, a_ck, t);
    dg_store(Bs[0], rb, b_ck, t);
  }
  __syncthreads();
  for (; k0 < g.k; k0 += DG_BK, buf ^= 1) {
    const bool more = k0 + DG_BK < g.k;
    if (more) {                                        // the next slab travels while the matrix pipe works on this one
      dg_load(ra, g.A, g.lda, a_ck, row0, g.m, k0 + DG_BK, g.k, t);
      dg_load(rb, g.B, g.ldb, b_ck, col0, g.n, k0 + DG_BK, g.k, t);
    }
#pragma unroll
    for (int ks = 0; ks < DG_BK; ks += 4) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = As[buf][ks + lk][wr + i * 16 + lr];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Bs[buf][ks + lk][wc + j * 16 + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if (more) {                                        // the other buffer was last read before the barrier of the slab in front
      dg_store(As[buf ^ 1], ra, a_ck, t);
      dg_store(Bs[buf ^ 1], rb, b_ck, t);
    }
    __syncthreads();
  }

  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  if constexpr (MODE == DG_AXPBY) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + wr + i * 16 + lk + 4 * r, col = col0 + wc + j * 16 + lr;
          if (row >= g.m || col >= g.n) continue;
          double d = g.alpha * acc[i][j][r];
          if (g.beta != 0.0) d = d + g.beta * g.E[(int64_t)row * g.lde + col];
          g.D[(int64_t)row * g.ldd + col] = d;
        }
  } else {
    // One accumulator (four elements of one column) at a time, and the inputs of the next one are asked for before
    // the results of this one are stored: a load issued behind a store to memory that may alias waits for it, and 64
    // such round trips in a row cost a third of the product's time.  The order of every sum stays (i, j, r).
    struct AdmmIn { double e[4], w[4], gm[4], c[4], v; };
    auto fetch = [&](int idx, AdmmIn& in) {
      const int col = col0 + wc + (idx & 3) * 16 + lr;
      in.v = col < g.n ? g.v[col] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr + (idx >> 2) * 16 + lk + 4 * r;
        const bool ok = row < g.m && col < g.n;
        const int64_t at = (int64_t)row * g.n + col;
        in.e[r] = ok ? g.E[at] : 0.0;
        in.w[r] = ok ? g.A[at] : 0.0;
        in.gm[r] = ok ? g.Gm[at] : 0.0;
        in.c[r] = ok ? g.C[at] : 0.0;
      }
    };
    AdmmIn cur, nxt;
    fetch(0, cur);
#pragma unroll
    for (int idx = 0; idx < 16; ++idx) {
      if (idx + 1 < 16) fetch(idx + 1, nxt);
      const int col = col0 + wc + (idx & 3) * 16 + lr;
      double c_new[4], g_new[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr + (idx >> 2) * 16 + lk + 4 * r;
        const double T = cur.e[r] + acc[idx >> 2][idx & 3][r];
        const double Bv = T - cur.w[r] * cur.v;
        const double S = Bv + cur.gm[r] / g.rho;
        c_new[r] = fmax(S - g.coef, 0.0) - fmax(-S - g.coef, 0.0);
        g_new[r] = cur.gm[r] + g.rho * (Bv - c_new[r]);
        if (row < g.m && col < g.n) {
          const double d1 = Bv - c_new[r], d2 = c_new[r] - cur.c[r];
          s0 = s0 + d1 * d1;
          s1 = s1 + d2 * d2;
          s2 = s2 + Bv * Bv;
          s3 = s3 + c_new[r] * c_new[r];
          s4 = s4 + g_new[r] * g_new[r];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + wr + (idx >> 2) * 16 + lk + 4 * r;
        if (row < g.m && col < g.n) {
          const int64_t at = (int64_t)row * g.n + col;
          g.C[at] = c_new[r];
          g.Gm[at] = g_new[r];
        }
      }
      cur = nxt;
    }
  }
  if constexpr (MODE == DG_ADMM) {
    s0 = dg_wave_sum(s0); s1 = dg_wave_sum(s1); s2 = dg_wave_sum(s2); s3 = dg_wave_sum(s3); s4 = dg_wave_sum(s4);
    if (lane == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; red[wave][4] = s4; }
    __syncthreads();
    if (t < 5) {
      const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
      g.part[tile * 5 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
    }
  }
}

static int dg_launch(const DgArgs& g, int mode, hipStream_t s) {
  const dim3 grid((unsigned)cql_ceil_div(g.n, DG_BM), (unsigned)cql_ceil_div(g.m, DG_BM));
  const int smem = 2 * 2 * DG_BK * DG_LD * 8;
  static bool attr_set_dev[CQL_MAX_DEVICES] = {};   // > 64 KiB of dynamic LDS needs the opt-in once per kernel and device
  bool& attr_set = attr_set_dev[cql_device_slot()];
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)dense_gemm_kernel<DG_AXPBY>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    (void)hipFuncSetAttribute((const void*)dense_gemm_kernel<DG_ADMM>, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    attr_set = true;
  }
  if (mode == DG_AXPBY) hipLaunchKernelGGL(dense_gemm_kernel<DG_AXPBY>, grid, dim3(256), smem, s, g);
  else hipLaunchKernelGGL(dense_gemm_kernel<DG_ADMM>, grid, dim3(256), smem, s, g);
  CQL_LAUNCH_CHECK("dense_gemm");
  return CQLREC_OK;
}
static int dg_gemm(const double* A, int64_t lda, int ta, const double* B, int64_t ldb, int tb, const double* E, int64_t lde,
                   double alpha, double beta, int64_t m, int64_t n, int64_t k, double* D, int64_t ldd, int flags,
                   hipStream_t s) {
  DgArgs g = {};
  g.A = A; g.B = B; g.E = E; g.D = D;
  g.lda = lda; g.ldb = ldb; g.lde = lde; g.ldd = ldd;
  g.m = (int32_t)m; g.n = (int32_t)n; g.k = (int32_t)k; g.ta = ta; g.tb = tb; g.flags = flags;
  g.alpha = alpha; g.beta = beta;
  return dg_launch(g, DG_AXPBY, s);
}

extern "C" int cqlrec_dense_gemm_f64(const double* A, int64_t lda, int32_t trans_a, const double* B, int64_t ldb,
                                     int32_t trans_b, const double* E, int64_t lde, double alpha, double beta, int64_t m,
                                     int64_t n, int64_t k, double* D, int64_t ldd, cqlrec_stream stream) {
  CQL_REQUIRE(m >= 1 && m <= DG_MAX_MN && n >= 1 && n <= DG_MAX_MN && k >= 1 && k < DG_MAX_K,
              "dense_gemm_f64: m=%lld n=%lld k=%lld out of range (m, n 1..%lld, k below 2^31)", (long long)m, (long long)n,
              (long long)k, (long long)DG_MAX_MN);
  CQL_REQUIRE((trans_a == 0 || trans_a == 1) && (trans_b == 0 || trans_b == 1), "dense_gemm_f64: trans_a=%d trans_b=%d out of range (0, 1)",
              trans_a, trans_b);
  CQL_REQUIRE(A && B && D && (E || beta == 0.0), "dense_gemm_f64: NULL pointer");
  CQL_REQUIRE(lda >= (trans_a ? m : k) && ldb >= (trans_b ? k : n) && ldd >= n && (beta == 0.0 || lde >= n),
              "dense_gemm_f64: a leading dimension (lda=%lld ldb=%lld lde=%lld ldd=%lld) is shorter than its row", (long long)lda,
              (long long)ldb, (long long)lde, (long long)ldd);
  return dg_gemm(A, lda, trans_a, B, ldb, trans_b, E, lde, alpha, beta, m, n, k, D, ldd, 0, (hipStream_t)stream);
}

// ---- small pieces shared below ---------------------------------------------------------------------------------
// in place: v[0] = 0, v[i + 1] = the sum of the counts that stood at v[1 .. i + 1]; v[n + 1 .. n_out] = the total
__global__ __launch_bounds__(256) void dense_scan_kernel(int64_t* v, int64_t n, int64_t n_out) {
  __shared__ int64_t part[256];
  const int t = threadIdx.x;
  const int64_t chunk = (n + 255) / 256, lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
  int64_t s = 0;
  for (int64_t i = lo; i < hi; ++i) s += v[i + 1];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int i = 0; i < 256; ++i) { const int64_t x = part[i]; part[i] = run; run += x; }
    v[0] = 0;
  }
  __syncthreads();
  s = part[t];
  for (int64_t i = lo; i < hi; ++i) { s += v[i + 1]; v[i + 1] = s; }
  __syncthreads();                                     // the global writes of this one workgroup are visible behind it
  const int64_t total = v[n];
  for (int64_t i = n + 1 + t; i <= n_out; i += 256) v[i] = total;
}

// ---- the Gram matrix of a log ------------------------------------------------------------------------------------
// One workgroup per item row i walks the users of i in ascending order; for a user it adds x_ui * x_uj to G[i][j] for
// every j of the user's row, one thread per j, and a barrier closes the user: G[i][j] is summed users ascending.  A run
// of entries with one (user, item) is one entry whose value is the sum of the run in row order.  An item row of more
// than CQLREC_DENSE_GRAM_PIECE entries is cut: one workgroup per piece sums into a row of the workspace and the finishing
// launch adds those rows in piece order from +0.0; a run belongs to the piece its first entry lies in.
struct GramArgs {
  const int64_t* i_off; const int32_t* i_user; const double* i_val;
  const int64_t* u_off; const int32_t* u_item; const double* u_val;
  int64_t* piece_off;               // [n_items + 1]
  double* part;                     // [n_pieces][n_items]
  double* G;
  int64_t n_items, n_users, n_pieces;
};
enum { GRAM_SETUP = 0, GRAM_SHORT = 1, GRAM_PIECE = 2, GRAM_FINISH = 3 };

static __device__ void gram_walk(const GramArgs& a, int64_t row_lo, int64_t row_hi, int64_t lo, int64_t hi, double* out) {
  const int t = threadIdx.x;
  for (int64_t j = t; j < a.n_items; j += 256) out[j] = 0.0;
  __syncthreads();
  int64_t e = lo;
  if (e > row_lo) while (e < hi && a.i_user[e] == a.i_user[e - 1]) ++e;       // the run belongs to the piece in front
  while (e < hi) {
    const int32_t u = a.i_user[e];
    double x = a.i_val[e];
    int64_t e2 = e + 1;
    for (; e2 < row_hi && a.i_user[e2] == u; ++e2) x = x + a.i_val[e2];
    if (u >= 0 && u < a.n_users) {
      const int64_t us = a.u_off[u], ue = a.u_off[u + 1];
      for (int64_t q = us + t; q < ue; q += 256) {
        const int32_t j = a.u_item[q];
        if ((q > us && a.u_item[q - 1] == j) || j < 0 || j >= a.n_items) continue;
        double y = a.u_val[q];
        for (int64_t q2 = q + 1; q2 < ue && a.u_item[q2] == j; ++q2) y = y + a.u_val[q2];
        out[j] = out[j] + x * y;
      }
    }
    __syncthreads();
    e = e2;
  }
}

template <int PHASE>
__global__ __launch_bounds__(256) void dense_gram_kernel(GramArgs a) {
  const int64_t b = blockIdx.x;
  const int t = threadIdx.x;
  if constexpr (PHASE == GRAM_SETUP) {                 // piece counts, scanned by dense_scan_kernel
    const int64_t i = b * 256 + t;
    if (i < a.n_items) {
      const int64_t len = a.i_off[i + 1] - a.i_off[i];
      a.piece_off[i + 1] = len > CQLREC_DENSE_GRAM_PIECE ? (len + CQLREC_DENSE_GRAM_PIECE - 1) / CQLREC_DENSE_GRAM_PIECE : 0;
    }
  } else if constexpr (PHASE == GRAM_SHORT) {
    const int64_t lo = a.i_off[b], hi = a.i_off[b + 1];
    if (hi - lo > CQLREC_DENSE_GRAM_PIECE) return;
    gram_walk(a, lo, hi, lo, hi, a.G + b * a.n_items);
  } else if constexpr (PHASE == GRAM_PIECE) {
    if (b >= a.piece_off[a.n_items]) return;
    int64_t l = 0, h = a.n_items;                      // the largest row with piece_off[row] <= b
    while (h - l > 1) {
      const int64_t mid = (l + h) >> 1;
      if (a.piece_off[mid] <= b) l = mid; else h = mid;
    }
    const int64_t row_lo = a.i_off[l], row_hi = a.i_off[l + 1];
    const int64_t lo = row_lo + (b - a.piece_off[l]) * CQLREC_DENSE_GRAM_PIECE;
    const int64_t hi = lo + CQLREC_DENSE_GRAM_PIECE < row_hi ? lo + CQLREC_DENSE_GRAM_PIECE : row_hi;
    gram_walk(a, row_lo, row_hi, lo, hi, a.part + b * a.n_items);
  } else {
    const int64_t p0 = a.piece_off[b], p1 = a.piece_off[b + 1];
    if (p1 == p0) return;
    const bool announced = p1 <= a.n_pieces;
    for (int64_t j = t; j < a.n_items; j += 256) {
      double s = 0.0;
      for (int64_t p = p0; p < p1 && announced; ++p) s = s + a.part[p * a.n_items + j];
      a.G[b * a.n_items + j] = announced ? s : __builtin_nan("");
    }
  }
}

extern "C" int64_t cqlrec_dense_gram_ws_bytes(int64_t n_items, int64_t n_pieces) {
  if (n_items < 1 || n_items > DG_MAX_N || n_pieces < 0 || n_pieces >= DG_MAX_K) return 0;
  return cql_align256((n_items + 1) * 8) + cql_align256(n_pieces * n_items * 8) + 256;
}
extern "C" int cqlrec_dense_gram(const int64_t* i_off, const int32_t* i_user, const double* i_val, const int64_t* u_off,
                                 const int32_t* u_item, const double* u_val, int64_t n_items, int64_t n_users,
                                 int64_t n_pieces, void* ws, int64_t ws_bytes, double* G, cqlrec_stream stream) {
  CQL_REQUIRE(n_items >= 1 && n_items <= DG_MAX_N && n_users >= 0 && n_users < DG_MAX_K && n_pieces >= 0 && n_pieces < DG_MAX_K,
              "dense_gram: n_items=%lld (1..%lld) n_users=%lld n_pieces=%lld out of range", (long long)n_items, (long long)DG_MAX_N,
              (long long)n_users, (long long)n_pieces);
  CQL_REQUIRE(i_off && u_off && G && ws, "dense_gram: NULL pointer");
  const int64_t need = cqlrec_dense_gram_ws_bytes(n_items, n_pieces);
  CQL_REQUIRE(ws_bytes >= need, "dense_gram: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  GramArgs a = {i_off, i_user, i_val, u_off, u_item, u_val, nullptr, nullptr, G, n_items, n_users, n_pieces};
  char* base = static_cast<char*>(ws);
  a.piece_off = reinterpret_cast<int64_t*>(base);
  a.part = reinterpret_cast<double*>(base + cql_align256((n_items + 1) * 8));
  hipLaunchKernelGGL(dense_gram_kernel<GRAM_SETUP>, dim3(cql_ceil_div(n_items, 256)), dim3(256), 0, s, a);
  hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(256), 0, s, a.piece_off, n_items, n_items);
  hipLaunchKernelGGL(dense_gram_kernel<GRAM_SHORT>, dim3((unsigned)n_items), dim3(256), 0, s, a);
  if (n_pieces > 0) {
    hipLaunchKernelGGL(dense_gram_kernel<GRAM_PIECE>, dim3((unsigned)n_pieces), dim3(256), 0, s, a);
    hipLaunchKernelGGL(dense_gram_kernel<GRAM_FINISH>, dim3((unsigned)n_items), dim3(256), 0, s, a);
  }
  CQL_LAUNCH_CHECK("dense_gram");
  return CQLREC_OK;
}

// ---- the inverse of a symmetric positive definite matrix ---------------------------------------------------------
// Recursive over the diagonal: a range of at most CQLREC_DENSE_BLOCK rows is factorised (A = L L^T, right-looking) and
// L inverted (forward substitution, one thread per column) by one workgroup in LDS.  A longer range [lo, hi) is cut at
// mid -- half of it, rounded up to whole blocks -- and with 1 = [lo, mid), 2 = [mid, hi):
//   the first half          gives L11^-1
//   L21 = A21 L11^-T        GEMM; it is parked where L^-1 21 will stand
//   A22 <- A22 - L21 L21^T  GEMM over the tiles that touch the lower triangle
//   the second half         gives L22^-1
//   L^-1 21 = -L22^-1 (L21 L11^-1)        two GEMMs, the product in between in a buffer of its own
// and at the end X = L^-T L^-1: one GEMM over the lower tiles whose k starts at the tile's diagonal, then the mirror.
// L itself is never stored.  The workspace: the working copy of A, L^-1, and the buffer of the largest in-between product.
__global__ void dense_copy_shift_kernel(const double* A, int64_t lda, int64_t n, double shift, double* out) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n * n) return;
  const int64_t i = at / n, j = at - i * n;
  const double x = A[i * lda + j];
  out[at] = i == j ? x + shift : x;
}
__global__ void dense_mirror_kernel(double* X, int64_t n) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= n * n) return;
  const int64_t i = at / n, j = at - i * n;
  if (j > i) X[at] = X[j * n + i];
}

__global__ __launch_bounds__(256) void dense_chol_block_kernel(const double* Wk, double* Li, int64_t ld, int b, int32_t base,
                                                               int32_t* status) {
  __shared__ double A[DG_NB][DG_NB + 1];
  __shared__ double X[DG_NB][DG_NB + 1];
  const int t = threadIdx.x;
  for (int at = t; at < DG_NB * DG_NB; at += 256) {
    const int i = at / DG_NB, j = at % DG_NB;
    A[i][j] = (i < b && j <= i) ? Wk[(int64_t)i * ld + j] : (i == j ? 1.0 : 0.0);
    X[i][j] = 0.0;
  }
  for (int j = 0; j < b; ++j) {
    __syncthreads();
    double p = A[j][j];
    if (!(p > 0.0)) {                                  // not positive definite: flag it, stay finite, go on
      if (t == 0) atomicCAS(status, 0, base + j + 1);
      p = 1.0;
    }
    const double l = sqrt(p);
    __syncthreads();
    if (t < b && t >= j) A[t][j] = t == j ? l : A[t][j] / l;
    __syncthreads();
    for (int at = t; at < DG_NB * DG_NB; at += 256) {
      const int i = at / DG_NB, k = at % DG_NB;
      if (k > j && k <= i && i < b) A[i][k] = A[i][k] - A[i][j] * A[k][j];
    }
  }
  __syncthreads();
  if (t < b) {                                         // column t of L^-1, rows top to bottom
    for (int i = t; i < b; ++i) {
      double s = i == t ? 1.0 : 0.0;
      for (int k = t; k < i; ++k) s = s - A[i][k] * X[k][t];
      X[i][t] = s / A[i][i];
    }
  }
  __syncthreads();
  for (int at = t; at < b * b; at += 256) {
    const int i = at / b, j = at % b;
    Li[(int64_t)i * ld + j] = j <= i ? X[i][j] : 0.0;
  }
}

static inline int64_t spd_mid(int64_t lo, int64_t hi) {
  return lo + ((hi - lo + 1) / 2 + DG_NB - 1) / DG_NB * DG_NB;
}
struct SpdCtx { double* Wk; double* Li; double* tmp; int64_t n; int32_t* status; hipStream_t s; };

static int spd_node(const SpdCtx& c, int64_t lo, int64_t hi) {
  const int64_t n = c.n;
  if (hi - lo <= DG_NB) {
    hipLaunchKernelGGL(dense_chol_block_kernel, dim3(1), dim3(256), 0, c.s, c.Wk + lo * n + lo, c.Li + lo * n + lo, n,
                       (int)(hi - lo), (int32_t)lo, c.status);
    CQL_LAUNCH_CHECK("dense_spd_inverse");
    return CQLREC_OK;
  }
  const int64_t mid = spd_mid(lo, hi), s1 = mid - lo, s2 = hi - mid;
  double* L11 = c.Li + lo * n + lo;
  double* L21 = c.Li + mid * n + lo;
  double* L22 = c.Li + mid * n + mid;
  int rc = spd_node(c, lo, mid);
  if (rc == CQLREC_OK) rc = dg_gemm(c.Wk + mid * n + lo, n, 0, L11, n, 1, nullptr, 0, 1.0, 0.0, s2, s1, s1, L21, n, 0, c.s);
  if (rc == CQLREC_OK)
    rc = dg_gemm(L21, n, 0, L21, n, 1, c.Wk + mid * n + mid, n, -1.0, 1.0, s2, s2, s1, c.Wk + mid * n + mid, n, DG_LOWER_ONLY, c.s);
  if (rc == CQLREC_OK) rc = spd_node(c, mid, hi);
  if (rc == CQLREC_OK) rc = dg_gemm(L21, n, 0, L11, n, 0, nullptr, 0, 1.0, 0.0, s2, s1, s1, c.tmp, s1, 0, c.s);
  if (rc == CQLREC_OK) rc = dg_gemm(L22, n, 0, c.tmp, s1, 0, nullptr, 0, -1.0, 0.0, s2, s1, s2, L21, n, 0, c.s);
  return rc;
}

static int64_t spd_tmp_elems(int64_t lo, int64_t hi) {  // the largest in-between product of the tree below [lo, hi)
  if (hi - lo <= DG_NB) return 0;
  const int64_t mid = spd_mid(lo, hi);
  int64_t best = (mid - lo) * (hi - mid);
  const int64_t a = spd_tmp_elems(lo, mid), b = spd_tmp_elems(mid, hi);
  if (a > best) best = a;
  return b > best ? b : best;
}
extern "C" int64_t cqlrec_dense_spd_inverse_ws_bytes(int64_t n) {
  if (n < 1 || n > DG_MAX_N) return 0;
  return 2 * cql_align256(n * n * 8) + cql_align256(spd_tmp_elems(0, n) * 8) + 256;
}
extern "C" int cqlrec_dense_spd_inverse(const double* A, int64_t lda, int64_t n, double shift, void* ws, int64_t ws_bytes,
                                        double* X, int32_t* status, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 1 && n <= DG_MAX_N, "dense_spd_inverse: n=%lld out of range (1..%lld)", (long long)n, (long long)DG_MAX_N);
  CQL_REQUIRE(A && X && status && ws, "dense_spd_inverse: NULL pointer");
  CQL_REQUIRE(lda >= n, "dense_spd_inverse: lda=%lld is shorter than a row of %lld", (long long)lda, (long long)n);
  const int64_t need = cqlrec_dense_spd_inverse_ws_bytes(n);
  CQL_REQUIRE(ws_bytes >= need, "dense_spd_inverse: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes,
              (long long)need);
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  const int64_t mat = cql_align256(n * n * 8);
  SpdCtx c = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + mat), reinterpret_cast<double*>(base + 2 * mat), n,
              status, s};
  if (hipMemsetAsync(status, 0, 4, s) != hipSuccess || hipMemsetAsync(c.Li, 0, (size_t)(n * n * 8), s) != hipSuccess) {
    cql_set_error("dense_spd_inverse: hipMemsetAsync failed");
    return CQLREC_ERR_HIP;
  }
  const unsigned blocks = (unsigned)((n * n + 255) / 256);
  hipLaunchKernelGGL(dense_copy_shift_kernel, dim3(blocks), dim3(256), 0, s, A, lda, n, shift, c.Wk);
  CQL_LAUNCH_CHECK("dense_spd_inverse");
  int rc = spd_node(c, 0, n);
  if (rc != CQLREC_OK) return rc;
  rc = dg_gemm(c.Li, n, 1, c.Li, n, 0, nullptr, 0, 1.0, 0.0, n, n, n, X, n, DG_LOWER_ONLY | DG_K_FROM_DIAG, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(dense_mirror_kernel, dim3(blocks), dim3(256), 0, s, X, n);
  CQL_LAUNCH_CHECK("dense_spd_inverse");
  return CQLREC_OK;
}

// ---- one ADMM iteration --------------------------------------------------------------------------------------------
//   M = rho C - Gamma                          element-wise, into the workspace
//   v_j = (P_jj + sum_k W_jk M_kj) / W_jj       one lane per j: k in four quarters, each added k ascending, the quarters in order
//   per element, behind the GEMM T = P + W M:  B = T - W_ij v_j;  S = B + Gamma / rho;  C' = max(S - c, 0) - max(-S - c, 0);
//                                              Gamma' = Gamma + rho (B - C');  C and Gamma are updated in place, B is not stored
//   sums[5] = the sums of squares of B - C', C' - C, B, C', Gamma': per thread in register order, per wave by a butterfly, per
//             tile the four waves in order, then the tiles in an order fixed by the tile index (admm_sums_kernel)
__global__ void admm_operand_kernel(const double* C, const double* Gm, double rho, int64_t total, double* M) {
  const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (at < total) M[at] = rho * C[at] - Gm[at];
}
// 64 consecutive j per workgroup, one lane per j; wave w of four takes the w-th quarter of k (in whole slabs of 16) and
// adds its terms k ascending; the four partial sums are added in wave order.  A slab of W (64 rows of j, 16 k) goes
// through LDS so that W is read along its rows and M along its rows too: a lane reading M[k][j] down a column of its
// own would touch one cache line and one page per element.
__global__ __launch_bounds__(256) void admm_diag_kernel(const double* W, const double* P, const double* M, int64_t n, double* v) {
  __shared__ double tile[4][64][17];
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * 64, j = j0 + lane;
  const int64_t slabs = (n + 15) / 16, per = (slabs + 3) / 4;
  const int64_t k_lo = wave * per * 16, k_end = (wave + 1) * per * 16 < n ? (wave + 1) * per * 16 : n;
  double s = 0.0;
  for (int64_t k0 = k_lo; k0 < k_end; k0 += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = (lane >> 4) + 4 * i, kk = lane & 15;
      tile[wave][r][kk] = (j0 + r < n && k0 + kk < k_end) ? W[(j0 + r) * n + k0 + kk] : 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (j < n)
      for (int kk = 0; kk < 16 && k0 + kk < k_end; ++kk) s = s + tile[wave][lane][kk] * M[(k0 + kk) * n + j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && j < n) {
    const double sum = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    v[j] = (P[j * n + j] + sum) / W[j * n + j];
  }
}
// thread t adds the tiles t, t + 256, ... in that order, then the 256 partial sums meet in a fixed tree: the order depends
// on the number of tiles alone.  (One thread walking all tiles waits out one memory latency per tile.)
__global__ __launch_bounds__(256) void admm_sums_kernel(const double* part, int64_t tiles, double* sums) {
  __shared__ double red[5][256];
  const int t = threadIdx.x;
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = t; i < tiles; i += 256)
#pragma unroll
    for (int q = 0; q < 5; ++q) s[q] = s[q] + part[i * 5 + q];
#pragma unroll
  for (int q = 0; q < 5; ++q) red[q][t] = s[q];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o)
#pragma unroll
      for (int q = 0; q < 5; ++q) red[q][t] = red[q][t] + red[q][t + o];
    __syncthreads();
  }
  if (t < 5) sums[t] = red[t][0];
}

static inline int64_t admm_tiles(int64_t n) { const int64_t e = (n + DG_BM - 1) / DG_BM; return e * e; }
extern "C" int64_t cqlrec_admm_iteration_ws_bytes(int64_t n) {
  if (n < 1 || n > DG_MAX_N) return 0;
  return cql_align256(n * n * 8) + cql_align256(n * 8) + cql_align256(admm_tiles(n) * 5 * 8) + 256;
}
extern "C" int cqlrec_admm_iteration(const double* W, const double* P, double* C, double* Gamma, int64_t n, double rho,
                                     double lambda_1, void* ws, int64_t ws_bytes, double* sums, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 1 && n <= DG_MAX_N, "admm_iteration: n=%lld out of range (1..%lld)", (long long)n, (long long)DG_MAX_N);
  CQL_REQUIRE(rho > 0.0 && lambda_1 >= 0.0, "admm_iteration: rho=%g (above 0) or lambda_1=%g (0 or more) out of range", rho, lambda_1);
  CQL_REQUIRE(W && P && C && Gamma && sums && ws, "admm_iteration: NULL pointer");
  const int64_t need = cqlrec_admm_iteration_ws_bytes(n);
  CQL_REQUIRE(ws_bytes >= need, "admm_iteration: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  double* M = reinterpret_cast<double*>(base);
  double* v = reinterpret_cast<double*>(base + cql_align256(n * n * 8));
  double* part = reinterpret_cast<double*>(base + cql_align256(n * n * 8) + cql_align256(n * 8));
  hipLaunchKernelGGL(admm_operand_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, s, C, Gamma, rho, n * n, M);
  hipLaunchKernelGGL(admm_diag_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, s, W, P, M, n, v);
  CQL_LAUNCH_CHECK("admm_iteration");
  DgArgs g = {};
  g.A = W; g.B = M; g.E = P;
  g.lda = g.ldb = g.lde = g.ldd = n;
  g.m = g.n = g.k = (int32_t)n;
  g.alpha = 1.0; g.beta = 1.0;
  g.v = v; g.C = C; g.Gm = Gamma; g.part = part;
  g.rho = rho; g.coef = lambda_1 / rho;
  const int rc = dg_launch(g, DG_ADMM, s);
  if (rc != CQLREC_OK) return rc;
  hipLaunchKernelGGL(admm_sums_kernel, dim3(1), dim3(256), 0, s, part, admm_tiles(n), sums);
  CQL_LAUNCH_CHECK("admm_iteration");
  return CQLREC_OK;
}

// ---- dense -> CSR ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void admm_count_kernel(const double* C, int64_t n, int64_t* offsets) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  int cnt = 0;
  for (int64_t j = lane; j < n; j += 64) cnt += C[row * n + j] != 0.0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) offsets[row + 1] = cnt;
}
__global__ __launch_bounds__(256) void admm_write_kernel(const double* C, int64_t n, const int64_t* offsets, int32_t* col,
                                                         double* val) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  int64_t at = offsets[row];
  for (int64_t j0 = 0; j0 < n; j0 += 64) {
    const int64_t j = j0 + lane;
    const double x = j < n ? C[row * n + j] : 0.0;
    const bool nz = x != 0.0;
    const uint64_t mask = __ballot(nz);
    if (nz) {
      const int64_t to = at + __popcll(mask & ((1ull << lane) - 1));
      col[to] = (int32_t)j;
      val[to] = x;
    }
    at += __popcll(mask);
  }
}
extern "C" int cqlrec_admm_compact(const double* C, int64_t n, int64_t n_rows, int64_t* offsets, int32_t* col, double* val,
                                   cqlrec_stream stream) {
  CQL_REQUIRE(n >= 1 && n <= DG_MAX_N && n_rows >= n && n_rows < DG_MAX_K, "admm_compact: n=%lld (1..%lld) n_rows=%lld (n or more) out of range",
              (long long)n, (long long)DG_MAX_N, (long long)n_rows);
  CQL_REQUIRE(C && offsets && ((col == nullptr) == (val == nullptr)), "admm_compact: NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + 3) / 4);
  if (!col) {
    hipLaunchKernelGGL(admm_count_kernel, dim3(blocks), dim3(256), 0, s, C, n, offsets);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(256), 0, s, offsets, n, n_rows);
  } else {
    hipLaunchKernelGGL(admm_write_kernel, dim3(blocks), dim3(256), 0, s, C, n, offsets, col, val);
  }
  CQL_LAUNCH_CHECK("admm_compact");
  return CQLREC_OK;
}
