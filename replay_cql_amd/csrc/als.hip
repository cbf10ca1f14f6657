// f9  alternating least squares on the device (ALSWrap of replay/models/als.py; the solver is Spark ML's ALS at the
// settings that wrapper uses -- DESIGN.md section 3.10 is the normative text): the Gram matrix of a factor table, the
// fp64 normal equations of a list of destination rows, the whole update of one side (accumulate, Cholesky, solve, fp32
// store), and prediction (dense fp32 scores with the exact wave-level selection of select_common.h, pair scores).
// The rules of f5 - f8 hold: integer atomics only, no floating-point atomics, the same input gives the same bytes.
// Built with -ffp-contract=off: every expression is evaluated as written, a fused operation is an explicit fma().
//
// One matrix, one layout.  The (rank + 1) x (rank + 1) lower triangle [A b; b^T .] of a row is cut into T x T blocks;
// thread t of a group owns block (bi, bj), bj <= bi, and keeps it in registers from the first term to the last
// elimination step.  Element (i, j) therefore has ONE chain of operations, whichever group shape the rank selects:
//   accumulate   acc = fma(left_i, y_j, acc) over the entries of a piece, left to right from +0.0; left_i = c * y_i for
//                i < rank and the weight of b for i = rank (b is row `rank` of the matrix)
//   pieces       a row of more than CQLREC_ALS_PIECE entries is ALWAYS cut: one group per piece writes its registers
//                to the workspace, the finishing group adds the pieces in piece order (plain +); a shorter row is one piece
//   G, reg       acc = acc + G[i][j] last; the solver then adds reg * n_expl to the diagonal
//   Cholesky     right-looking on the registers: step k publishes column k (times 1 / sqrt(pivot)) in LDS and every
//                live block takes acc = fma(-l_ik, l_jk, acc): the accumulate loop with the column as the vector.
//                Row `rank` comes out as z = L^-1 b, so the forward substitution costs nothing; the back
//                substitution runs on one wave with z in registers and the reciprocals of the diagonal from LDS.
// Nothing depends on the grid, on which wave takes a row or on the other rows of a launch.

#include "segment_common.h"
#include "select_common.h"

static const int64_t ALS_MAX = 1ll << 31;
#define ALS_CH 16                   // entries staged in LDS at once
#define ALS_TOPK_ROWS 4             // query rows per wave of the top-k kernel: they share the loads of the item table
static inline int als_topk_cb(int k) { return 2 * k < 128 ? 128 : 2 * k; }   // keys per selection buffer: k and room for batches of 64


enum { ALS_SHORT = 0, ALS_PIECE = 1, ALS_FINISH = 2 };

struct AlsShape {
  int T, GT, nb;                    // block edge, threads per group, blocks per side: nb * T >= rank + 1
  int ntri() const { return nb * (nb + 1) / 2; }
  int64_t part_stride() const { return (int64_t)ntri() * T * T; }          // doubles per piece in the workspace
  int64_t group_bytes(int rank) const {                                    // LDS of one group
    const int64_t tri = (int64_t)(rank + 1) * (rank + 2) / 2, rp = (int64_t)nb * T;
    return (8 * (tri + 2 * rp + 2 * ALS_CH + 2) + 4 * ALS_CH * rp + 15) / 16 * 16;
  }
};
static inline AlsShape als_shape(int rank) {
  AlsShape s;
  if (rank + 1 <= 20) { s.T = 2; s.GT = 64; }
  else if (rank + 1 <= 40) { s.T = 4; s.GT = 64; }
  else if (rank + 1 <= 88) { s.T = 4; s.GT = 256; }
  else { s.T = 8; s.GT = 256; }
  s.nb = (rank + 1 + s.T - 1) / s.T;
  return s;
}

struct AlsArgs {
  const int64_t* offsets;           // [n_dst + 1]
  const int32_t* src;               // [nnz], NULL: entry e is source row e (the Gram matrix)
  const double* rating;             // [nnz], NULL: c = 1, no b
  const float* F;                   // [n_src][rank]
  const double* G;                  // [rank][rank] or NULL
  const int32_t* rows;              // [n_list] or NULL: row l is l
  const int64_t* piece_off;         // [n_list + 1]: first piece of a listed row longer than `piece`
  double* part;                     // [n_pieces][part_stride]
  int32_t* part_n;                  // [n_pieces]
  float* X;                         // solve: [n_dst][rank]
  uint8_t* has;                     //        [n_dst]
  int32_t* n_failed;
  double* A;                        // dump: [n_list][rank][rank]
  double* b;                        //       [n_list][rank] or NULL
  int32_t* n_expl;                  //       [n_list] or NULL
  int64_t n_src, n_dst, n_list, n_pieces, part_stride, piece;
  double alpha, reg;
  int32_t rank, nb, implicit, phase, dump;
};

// 1 / sqrt(d) for d > 0: the hardware estimate and two Newton steps, y <- y + (y / 2)(1 - d y^2).  It sits on the
// critical path of every elimination step, where sqrt() followed by a division costs several times as much.
static __device__ __forceinline__ double als_rsqrt(double d) {
  double y = __builtin_amdgcn_rsq(d);
  double e = fma(-d * y, y, 1.0);
  y = fma(y * 0.5, e, y);
  e = fma(-d * y, y, 1.0);
  y = fma(y * 0.5, e, y);
  return y;
}

template <int GT>
static __device__ __forceinline__ void als_sync() {
  if constexpr (GT == 64) {         // one wave: its LDS operations complete in order; only the compiler has to be held
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __syncthreads();
  }
}

// the listed row that piece p belongs to
static __device__ __forceinline__ int64_t als_row_of_piece(const int64_t* piece_off, int64_t n_list, int64_t p) {
  int64_t lo = 0, hi = n_list;      // largest l with piece_off[l] <= p
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (piece_off[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

template <int T, int GT>
__global__ __launch_bounds__(256) void als_kernel(AlsArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char als_smem[];
  constexpr int NG = 256 / GT;
  const int g = threadIdx.x / GT, t = threadIdx.x % GT;
  const int r = a.rank, nb = a.nb, rp = nb * T;
  const int ntri = nb * (nb + 1) / 2;
  const int64_t tri = (int64_t)(r + 1) * (r + 2) / 2;
  const int64_t gbytes = (8 * (tri + 2 * rp + 2 * ALS_CH + 2) + 4 * ALS_CH * rp + 15) / 16 * 16;
  double* Lm = reinterpret_cast<double*>(als_smem + (int64_t)g * gbytes);   // packed lower triangle of L, row `r` = z
  double* col = Lm + tri;                                                  // [rp] column k of the current step
  double* dinv = col + rp;                                                 // [rp] 1 / l_kk
  double* cw = dinv + rp;                                                  // [ALS_CH][2] = (c, weight of b)
  double* piv = cw + 2 * ALS_CH;
  int* cnt_s = reinterpret_cast<int*>(piv + 1);
  float* stage = reinterpret_cast<float*>(piv + 2);                        // [ALS_CH][rp], padded with zeros

  const bool active = t < ntri;
  int bi = 0, bj = 0;
  if (active) {
    bi = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (bi * (bi + 1) / 2 > t) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
    bj = t - bi * (bi + 1) / 2;
  }

  // ---- which row, which entries (uniform over the group) ---------------------------------------------------------
  const int64_t item = (int64_t)blockIdx.x * NG + g;
  int64_t l, e0, e1, p0 = 0, np = 0;
  if (a.phase == ALS_SHORT) {
    l = item;
    if (l >= a.n_list) return;
  } else {
    if (item >= a.n_pieces || item >= a.piece_off[a.n_list]) return;
    l = als_row_of_piece(a.piece_off, a.n_list, item);
    p0 = a.piece_off[l];
    np = a.piece_off[l + 1] - p0;
    if (p0 + np > a.n_pieces) return;                     // more pieces than the caller announced: the short phase reports it
    if (a.phase == ALS_FINISH && item != p0) return;
  }
  const int64_t row = a.rows ? (int64_t)a.rows[l] : l;
  if (row < 0 || row >= a.n_dst) return;
  const int64_t r0 = a.offsets[row], r1 = a.offsets[row + 1], n = r1 - r0;
  bool overflow = false;
  if (a.phase == ALS_SHORT) {
    if (n > a.piece) {
      if (a.piece_off[l + 1] <= a.n_pieces) return;       // the piece and finish phases take it
      overflow = true;
    }
    e0 = r0;
    e1 = overflow ? r0 : r1;
  } else if (a.phase == ALS_PIECE) {
    e0 = r0 + (item - p0) * a.piece;
    e1 = e0 + a.piece < r1 ? e0 + a.piece : r1;
  } else {
    e0 = e1 = 0;
  }

  // ---- accumulate ------------------------------------------------------------------------------------------------
  double acc[T][T];
#pragma unroll
  for (int x = 0; x < T; ++x)
#pragma unroll
    for (int y = 0; y < T; ++y) acc[x][y] = 0.0;
  int cnt = 0;
  if (t == 0) *cnt_s = 0;
  for (int64_t base = e0; base < e1; base += ALS_CH) {
    const int m = (int)(e1 - base < ALS_CH ? e1 - base : ALS_CH);
    als_sync<GT>();
    for (int f = t; f < m * rp; f += GT) {                // whole rows, consecutive lanes on consecutive elements
      const int e = f / rp, k = f - e * rp;
      const int64_t s = a.src ? (int64_t)a.src[base + e] : base + e;
      float v = 0.0f;
      if (k < r && s >= 0 && s < a.n_src) v = a.F[s * r + k];
      stage[f] = v;
    }
    if (t < m) {
      const double rho = a.rating ? a.rating[base + t] : 0.0;
      double c = 1.0, w = rho;
      if (a.implicit) {
        c = a.alpha * fabs(rho);
        w = rho > 0.0 ? 1.0 + c : 0.0;
        cnt += rho > 0.0 ? 1 : 0;
      } else {
        cnt += 1;
      }
      cw[2 * t] = c;
      cw[2 * t + 1] = w;
    }
    als_sync<GT>();
    if (active) {
      for (int e = 0; e < m; ++e) {
        const double c = cw[2 * e], w = cw[2 * e + 1];
        const float* y = stage + e * rp;
        double left[T], right[T];
#pragma unroll
        for (int x = 0; x < T; ++x) {                     // the load is unconditional (i < rp): a select, not a branch
          const int i = bi * T + x;
          const double cy = c * (double)y[i];
          left[x] = i == r ? w : cy;
        }
#pragma unroll
        for (int x = 0; x < T; ++x) right[x] = (double)y[bj * T + x];
#pragma unroll
        for (int x = 0; x < T; ++x)
#pragma unroll
          for (int z = 0; z < T; ++z) acc[x][z] = fma(left[x], right[z], acc[x][z]);
      }
    }
  }
  if (cnt) atomicAdd(cnt_s, cnt);
  als_sync<GT>();
  int n_expl = *cnt_s;

  if (a.phase == ALS_PIECE) {                             // registers to the workspace, consecutive threads together
    if (active) {
      double* dst = a.part + item * a.part_stride;
#pragma unroll
      for (int x = 0; x < T; ++x)
#pragma unroll
        for (int z = 0; z < T; ++z) dst[(int64_t)(x * T + z) * ntri + t] = acc[x][z];
    }
    if (t == 0) a.part_n[item] = n_expl;
    return;
  }
  if (a.phase == ALS_FINISH) {                            // the pieces in piece order
    for (int64_t q = 0; q < np; ++q) {
      const double* srcp = a.part + (p0 + q) * a.part_stride;
      if (active) {
#pragma unroll
        for (int x = 0; x < T; ++x) {
#pragma unroll
          for (int z = 0; z < T; ++z) {
            const double v = srcp[(int64_t)(x * T + z) * ntri + t];
            acc[x][z] = q == 0 ? v : acc[x][z] + v;
          }
        }
      }
      n_expl += a.part_n[p0 + q];
    }
  }

  // ---- G last ----------------------------------------------------------------------------------------------------
  if (a.G && active) {
#pragma unroll
    for (int x = 0; x < T; ++x) {
#pragma unroll
      for (int z = 0; z < T; ++z) {
        const int i = bi * T + x, j = bj * T + z;
        if (i < r && j < r) acc[x][z] = acc[x][z] + a.G[i * r + j];
      }
    }
  }

  if (a.dump) {
    const double nan = __builtin_nan("");
    if (active) {
#pragma unroll
      for (int x = 0; x < T; ++x)
#pragma unroll
        for (int z = 0; z < T; ++z) {
          const int i = bi * T + x, j = bj * T + z;
          const double v = overflow ? nan : acc[x][z];
          if (i < r && j <= i) {
            a.A[(l * r + i) * r + j] = v;
            a.A[(l * r + j) * r + i] = v;
          } else if (i == r && j < r && a.b) {
            a.b[l * r + j] = v;
          }
        }
    }
    if (t == 0 && a.n_expl) a.n_expl[l] = overflow ? -1 : n_expl;
    return;
  }

  // ---- solve (A + reg n_expl I) x = b ------------------------------------------------------------------------------
  bool fail = overflow;
  if (n == 0 || fail) {
    for (int k = t; k < r; k += GT) a.X[row * r + k] = 0.0f;
    if (t == 0) {
      a.has[row] = 0;
      if (fail) atomicAdd(a.n_failed, 1);
    }
    return;
  }
  if (active && bi == bj) {
    const double shift = a.reg * (double)n_expl;
#pragma unroll
    for (int x = 0; x < T; ++x)
      if (bi * T + x < r) acc[x][x] = acc[x][x] + shift;
  }
  for (int kb = 0; kb < nb && !fail; ++kb) {
#pragma unroll
    for (int ka = 0; ka < T; ++ka) {
      const int k = kb * T + ka;
      if (k >= r) break;
      if (active && bi == kb && bj == kb) *piv = acc[ka][ka];
      als_sync<GT>();
      const double d = *piv;
      if (!(d > 0.0)) {                                   // not positive definite (NaN included)
        fail = true;
        break;
      }
      const double inv = als_rsqrt(d), sq = d * inv;      // l_kk = d / sqrt(d), l_ik = a_ik * (1 / sqrt(d)): no division
      if (t == 0) dinv[k] = inv;
      if (active && bj == kb) {
#pragma unroll
        for (int x = 0; x < T; ++x) {
          const int i = bi * T + x;
          const double v = i > k ? acc[x][ka] * inv : (i == k ? sq : 0.0);
          col[i] = v;
          if (i >= k && i <= r) Lm[i * (i + 1) / 2 + k] = v;
        }
      }
      als_sync<GT>();
      if (active && bi >= kb) {
        double cl[T], cr[T];
#pragma unroll
        for (int x = 0; x < T; ++x) cl[x] = -col[bi * T + x];
#pragma unroll
        for (int x = 0; x < T; ++x) cr[x] = col[bj * T + x];
#pragma unroll
        for (int x = 0; x < T; ++x)
#pragma unroll
          for (int z = 0; z < T; ++z) acc[x][z] = fma(cl[x], cr[z], acc[x][z]);
      }
    }
  }
  if (fail) {
    for (int k = t; k < r; k += GT) a.X[row * r + k] = 0.0f;
    if (t == 0) {
      a.has[row] = 0;
      atomicAdd(a.n_failed, 1);
    }
    return;
  }
  als_sync<GT>();
  if (t < 64) {                                           // L^T x = z, last row first; lane t holds z_t and z_(t + 64)
    const int zr = r * (r + 1) / 2;
    double z0 = t < r ? Lm[zr + t] : 0.0, z1 = t + 64 < r ? Lm[zr + t + 64] : 0.0;
    double x0 = 0.0, x1 = 0.0;
    for (int k = r - 1; k >= 0; --k) {
      const double* Lk = Lm + k * (k + 1) / 2;
      const double zk = __shfl(k < 64 ? z0 : z1, k & 63);
      const double xk = zk * dinv[k];
      if (t == (k & 63)) {
        if (k < 64) x0 = xk; else x1 = xk;
      }
      if (t < k) z0 = fma(-Lk[t], xk, z0);
      if (t + 64 < k) z1 = fma(-Lk[t + 64], xk, z1);
    }
    if (t < r) a.X[row * r + t] = (float)x0;
    if (t + 64 < r) a.X[row * r + t + 64] = (float)x1;
    if (t == 0) a.has[row] = 1;
  }
}

// pieces per listed row (0 for a row of at most `piece` entries), one more slot for the scan's total
__global__ void als_npieces_kernel(const int64_t* __restrict__ offsets, const int32_t* __restrict__ rows, int64_t n_list,
                                   int64_t n_dst, int64_t piece, int64_t* __restrict__ np) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l > n_list) return;
  int64_t v = 0;
  if (l < n_list) {
    const int64_t row = rows ? (int64_t)rows[l] : l;
    if (row >= 0 && row < n_dst) {
      const int64_t n = offsets[row + 1] - offsets[row];
      if (n > piece) v = (n + piece - 1) / piece;
    }
  }
  np[l] = v;
}
__global__ void als_gram_setup_kernel(int64_t n, int64_t n_pieces, int64_t* off, int64_t* piece_off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    off[0] = 0;
    off[1] = n;
    piece_off[0] = 0;
    piece_off[1] = n_pieces;
  }
}

static int als_launch(const AlsShape& sh, AlsArgs a, int phase, int64_t items, hipStream_t s) {
  if (items <= 0) return CQLREC_OK;
  a.phase = phase;
  const int ng = 256 / sh.GT;
  const size_t smem = (size_t)(ng * sh.group_bytes(a.rank));
  const int64_t grid = (items + ng - 1) / ng;
  CQL_REQUIRE(grid < ALS_MAX && smem <= 160 * 1024, "als: %lld work items or %zu bytes of LDS are out of range",
              (long long)items, smem);
  static bool attr_set_dev[CQL_MAX_DEVICES] = {};   // > 64 KiB of dynamic LDS needs the opt-in once per kernel and device
  bool& attr_set = attr_set_dev[cql_device_slot()];
  if (!attr_set) {
    const int cap = 96 * 1024;
    (void)hipFuncSetAttribute((const void*)als_kernel<2, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    (void)hipFuncSetAttribute((const void*)als_kernel<4, 64>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    (void)hipFuncSetAttribute((const void*)als_kernel<4, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    (void)hipFuncSetAttribute((const void*)als_kernel<8, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    attr_set = true;
  }
  if (sh.T == 2) hipLaunchKernelGGL((als_kernel<2, 64>), dim3((unsigned)grid), dim3(256), smem, s, a);
  else if (sh.T == 4 && sh.GT == 64) hipLaunchKernelGGL((als_kernel<4, 64>), dim3((unsigned)grid), dim3(256), smem, s, a);
  else if (sh.T == 4) hipLaunchKernelGGL((als_kernel<4, 256>), dim3((unsigned)grid), dim3(256), smem, s, a);
  else hipLaunchKernelGGL((als_kernel<8, 256>), dim3((unsigned)grid), dim3(256), smem, s, a);
  CQL_LAUNCH_CHECK("als");
  return CQLREC_OK;
}

// ---- workspace of the row entry points: np | piece_off | scan scratch | part | part_n --------------------------------
struct AlsWs {
  int64_t np, piece_off, temp, part, part_n, total;
};
static AlsWs als_ws(int64_t n_list, int64_t n_pieces, int rank) {
  AlsWs w;
  int64_t o = 0;
  w.np = o; o += cql_align256((n_list + 1) * 8);
  w.piece_off = o; o += cql_align256((n_list + 1) * 8);
  w.temp = o; o += cql_scan_temp_cap(n_list + 1);
  w.part = o; o += cql_align256(n_pieces * als_shape(rank).part_stride() * 8);
  w.part_n = o; o += cql_align256(n_pieces * 4);
  w.total = o;
  return w;
}
static bool als_sizes_ok(int64_t n_list, int64_t n_pieces, int32_t rank) {
  return n_list >= 0 && n_list < ALS_MAX && n_pieces >= 0 && n_pieces < ALS_MAX && rank >= 1 && rank <= CQLREC_ALS_MAX_RANK;
}

static int als_rows(AlsArgs a, void* ws, int64_t ws_bytes, const char* what, hipStream_t s) {
  const AlsShape sh = als_shape(a.rank);
  const AlsWs w = als_ws(a.n_list, a.n_pieces, a.rank);
  CQL_REQUIRE(ws && ws_bytes >= w.total, "%s: the workspace holds %lld bytes, %lld are needed", what, (long long)ws_bytes,
              (long long)w.total);
  char* base = static_cast<char*>(ws);
  int64_t* np = reinterpret_cast<int64_t*>(base + w.np);
  int64_t* piece_off = reinterpret_cast<int64_t*>(base + w.piece_off);
  hipLaunchKernelGGL(als_npieces_kernel, dim3(cql_ceil_div(a.n_list + 1, 256)), dim3(256), 0, s, a.offsets, a.rows, a.n_list,
                     a.n_dst, (int64_t)CQLREC_ALS_PIECE, np);
  CQL_LAUNCH_CHECK(what);
  int rc = cql_exclusive_scan(what, base + w.temp, (size_t)cql_scan_temp_cap(a.n_list + 1), np, piece_off, (int64_t)0,
                              a.n_list + 1, s);
  if (rc != CQLREC_OK) return rc;
  a.piece_off = piece_off;
  a.part = reinterpret_cast<double*>(base + w.part);
  a.part_n = reinterpret_cast<int32_t*>(base + w.part_n);
  a.part_stride = sh.part_stride();
  a.piece = CQLREC_ALS_PIECE;
  a.nb = sh.nb;
  rc = als_launch(sh, a, ALS_SHORT, a.n_list, s);
  if (rc == CQLREC_OK) rc = als_launch(sh, a, ALS_PIECE, a.n_pieces, s);
  if (rc == CQLREC_OK) rc = als_launch(sh, a, ALS_FINISH, a.n_pieces, s);
  return rc;
}

// =============================================================================================================
// Gram matrix
// =============================================================================================================
static inline int64_t als_gram_pieces(int64_t n) {
  return n > CQLREC_ALS_GRAM_BLOCK ? (n + CQLREC_ALS_GRAM_BLOCK - 1) / CQLREC_ALS_GRAM_BLOCK : 0;
}
extern "C" int64_t cqlrec_als_gram_ws_bytes(int64_t n_rows, int32_t rank) {
  if (n_rows < 0 || n_rows >= ALS_MAX || rank < 1 || rank > CQLREC_ALS_MAX_RANK) return 0;
  const int64_t np = als_gram_pieces(n_rows);
  return 256 + 256 + cql_align256(np * als_shape(rank).part_stride() * 8) + cql_align256(np * 4);
}
extern "C" int cqlrec_als_gram(const float* F, int64_t n_rows, int32_t rank, void* ws, int64_t ws_bytes, double* G,
                               cqlrec_stream stream) {
  CQL_REQUIRE(n_rows >= 0 && n_rows < ALS_MAX && rank >= 1 && rank <= CQLREC_ALS_MAX_RANK,
              "als_gram: n_rows=%lld rank=%d out of range (rank 1..%d)", (long long)n_rows, rank, CQLREC_ALS_MAX_RANK);
  CQL_REQUIRE(G && (F || n_rows == 0), "als_gram: NULL pointer");
  const int64_t need = cqlrec_als_gram_ws_bytes(n_rows, rank);
  CQL_REQUIRE(ws && ws_bytes >= need, "als_gram: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes,
              (long long)need);
  hipStream_t s = (hipStream_t)stream;
  const AlsShape sh = als_shape(rank);
  const int64_t np = als_gram_pieces(n_rows);
  char* base = static_cast<char*>(ws);
  int64_t* off = reinterpret_cast<int64_t*>(base);
  int64_t* piece_off = reinterpret_cast<int64_t*>(base + 256);
  hipLaunchKernelGGL(als_gram_setup_kernel, dim3(1), dim3(64), 0, s, n_rows, np, off, piece_off);
  CQL_LAUNCH_CHECK("als_gram");
  AlsArgs a = {};
  a.offsets = off;
  a.F = F;
  a.piece_off = piece_off;
  a.part = reinterpret_cast<double*>(base + 512);
  a.part_n = reinterpret_cast<int32_t*>(base + 512 + cql_align256(np * sh.part_stride() * 8));
  a.A = G;
  a.n_src = n_rows;
  a.n_dst = 1;
  a.n_list = 1;
  a.n_pieces = np;
  a.part_stride = sh.part_stride();
  a.piece = CQLREC_ALS_GRAM_BLOCK;
  a.rank = rank;
  a.nb = sh.nb;
  a.dump = 1;
  int rc = als_launch(sh, a, ALS_SHORT, 1, s);
  if (rc == CQLREC_OK) rc = als_launch(sh, a, ALS_PIECE, np, s);
  if (rc == CQLREC_OK) rc = als_launch(sh, a, ALS_FINISH, np, s);
  return rc;
}

// =============================================================================================================
// normal equations, half step
// =============================================================================================================
extern "C" int64_t cqlrec_als_normal_equations_ws_bytes(int64_t n_list, int64_t n_pieces, int32_t rank) {
  return als_sizes_ok(n_list, n_pieces, rank) ? als_ws(n_list, n_pieces, rank).total : 0;
}
extern "C" int64_t cqlrec_als_half_step_ws_bytes(int64_t n_list, int64_t n_pieces, int32_t rank) {
  return als_sizes_ok(n_list, n_pieces, rank) ? als_ws(n_list, n_pieces, rank).total : 0;
}

static int als_check_common(const char* what, const int64_t* offsets, const int32_t* src, const double* rating,
                            int64_t n_dst, const float* F, int64_t n_src, int32_t rank, int32_t mode, double alpha,
                            int64_t n_list, int64_t n_pieces) {
  CQL_REQUIRE(rank >= 1 && rank <= CQLREC_ALS_MAX_RANK, "%s: rank=%d out of range (1..%d)", what, rank, CQLREC_ALS_MAX_RANK);
  CQL_REQUIRE(n_dst >= 0 && n_dst < ALS_MAX && n_src >= 0 && n_src < ALS_MAX && n_list >= 0 && n_list < ALS_MAX &&
              n_pieces >= 0 && n_pieces < ALS_MAX, "%s: n_dst=%lld n_src=%lld n_list=%lld n_pieces=%lld out of range", what,
              (long long)n_dst, (long long)n_src, (long long)n_list, (long long)n_pieces);
  CQL_REQUIRE(mode == CQLREC_ALS_EXPLICIT || mode == CQLREC_ALS_IMPLICIT, "%s: unknown mode %d", what, mode);
  CQL_REQUIRE(alpha == alpha && alpha >= 0.0, "%s: alpha=%g must be non-negative", what, alpha);
  if (n_list == 0) return CQLREC_OK;
  CQL_REQUIRE(offsets && src && rating && F, "%s: NULL pointer", what);
  return CQLREC_OK;
}

extern "C" int cqlrec_als_normal_equations(const int64_t* offsets, const int32_t* src, const double* rating, int64_t n_dst,
                                           const float* F, int64_t n_src, int32_t rank, const double* G, int32_t mode,
                                           double alpha, const int32_t* rows, int64_t n_list, int64_t n_pieces, void* ws,
                                           int64_t ws_bytes, double* A, double* b, int32_t* n_expl, cqlrec_stream stream) {
  const int rc = als_check_common("als_normal_equations", offsets, src, rating, n_dst, F, n_src, rank, mode, alpha, n_list,
                                  n_pieces);
  if (rc != CQLREC_OK) return rc;
  if (n_list == 0) return CQLREC_OK;
  CQL_REQUIRE(A && b && n_expl, "als_normal_equations: NULL pointer");
  CQL_REQUIRE(rows || n_list == n_dst, "als_normal_equations: without a row list n_list must be n_dst");
  AlsArgs a = {};
  a.offsets = offsets; a.src = src; a.rating = rating; a.F = F; a.G = G; a.rows = rows;
  a.A = A; a.b = b; a.n_expl = n_expl;
  a.n_src = n_src; a.n_dst = n_dst; a.n_list = n_list; a.n_pieces = n_pieces;
  a.alpha = alpha; a.rank = rank; a.implicit = mode == CQLREC_ALS_IMPLICIT; a.dump = 1;
  return als_rows(a, ws, ws_bytes, "als_normal_equations", (hipStream_t)stream);
}

extern "C" int cqlrec_als_half_step(const int64_t* offsets, const int32_t* src, const double* rating, int64_t n_dst,
                                    const float* F, int64_t n_src, int32_t rank, const double* G, int32_t mode, double alpha,
                                    double reg, const int32_t* rows, int64_t n_list, int64_t n_pieces, void* ws,
                                    int64_t ws_bytes, float* X, uint8_t* has_factor, int32_t* n_failed,
                                    cqlrec_stream stream) {
  const int rc = als_check_common("als_half_step", offsets, src, rating, n_dst, F, n_src, rank, mode, alpha, n_list, n_pieces);
  if (rc != CQLREC_OK) return rc;
  CQL_REQUIRE(reg == reg && reg >= 0.0, "als_half_step: reg=%g must be non-negative", reg);
  if (n_list == 0) return CQLREC_OK;
  CQL_REQUIRE(X && has_factor && n_failed, "als_half_step: NULL pointer");
  CQL_REQUIRE(rows || n_list == n_dst, "als_half_step: without a row list n_list must be n_dst");
  CQL_REQUIRE(mode == CQLREC_ALS_EXPLICIT || G, "als_half_step: the implicit mode needs G (NULL pointer)");
  AlsArgs a = {};
  a.offsets = offsets; a.src = src; a.rating = rating; a.F = F; a.G = mode == CQLREC_ALS_IMPLICIT ? G : nullptr; a.rows = rows;
  a.X = X; a.has = has_factor; a.n_failed = n_failed;
  a.n_src = n_src; a.n_dst = n_dst; a.n_list = n_list; a.n_pieces = n_pieces;
  a.alpha = alpha; a.reg = reg; a.rank = rank; a.implicit = mode == CQLREC_ALS_IMPLICIT;
  return als_rows(a, ws, ws_bytes, "als_half_step", (hipStream_t)stream);
}

// =============================================================================================================
// prediction
// =============================================================================================================
// one wave per ALS_TOPK_ROWS query rows: lane l scores item base + l for every row, so a row of V is read once per block
__global__ __launch_bounds__(64) void als_topk_kernel(const int32_t* __restrict__ users, int64_t n_q,
                                                      const float* __restrict__ U, const uint8_t* __restrict__ u_has,
                                                      int64_t n_users, const float* __restrict__ V,
                                                      const uint8_t* __restrict__ v_has, int64_t n_items, int r,
                                                      const uint8_t* __restrict__ mask, const int64_t* __restrict__ seen_off,
                                                      const int32_t* __restrict__ seen_col, int k, int cb,
                                                      int32_t* __restrict__ ids, float* __restrict__ vals,
                                                      int32_t* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) uint64_t als_topk_buf[];   // [ALS_TOPK_ROWS][cb]
  uint64_t* buf[ALS_TOPK_ROWS];
#pragma unroll
  for (int j = 0; j < ALS_TOPK_ROWS; ++j) buf[j] = als_topk_buf + j * cb;
  __shared__ __attribute__((aligned(16))) float xs[ALS_TOPK_ROWS][CQLREC_ALS_MAX_RANK];
  __shared__ uint32_t hist[256];
  const int lane = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * ALS_TOPK_ROWS;
  bool live[ALS_TOPK_ROWS], have[ALS_TOPK_ROWS];   // have: the buffer held k keys at the last selection, tau is their smallest
  int64_t s_lo[ALS_TOPK_ROWS], s_hi[ALS_TOPK_ROWS];
  int n[ALS_TOPK_ROWS];
  uint64_t tau[ALS_TOPK_ROWS];
  bool any = false;
#pragma unroll
  for (int j = 0; j < ALS_TOPK_ROWS; ++j) {
    const int64_t q = q0 + j;
    const int64_t u = q < n_q ? (int64_t)users[q] : -1;
    live[j] = u >= 0 && u < n_users && u_has[u] != 0;
    s_lo[j] = s_hi[j] = 0;
    n[j] = 0;
    tau[j] = 0;
    have[j] = false;
    if (live[j]) {
      any = true;
      for (int c = lane; c < r; c += 64) xs[j][c] = U[u * r + c];
      if (seen_off) {
        s_lo[j] = seen_off[u];
        s_hi[j] = seen_off[u + 1];
      }
    }
  }
  __syncthreads();
  if (any) {
    for (int64_t base = 0; base < n_items; base += 64) {
      const int64_t item = base + lane;
      const bool cand = item < n_items && v_has[item] != 0 && (!mask || mask[item] != 0);
      float sc[ALS_TOPK_ROWS];
#pragma unroll
      for (int j = 0; j < ALS_TOPK_ROWS; ++j) sc[j] = 0.0f;
      if (cand) {
        const float* y = V + item * r;      // a row per lane: the widest loads its alignment allows, the chain order unchanged
        if ((r & 3) == 0) {
          for (int c = 0; c < r; c += 4) {
            const float4 y4 = *reinterpret_cast<const float4*>(y + c);
#pragma unroll
            for (int j = 0; j < ALS_TOPK_ROWS; ++j) {
              const float4 x4 = *reinterpret_cast<const float4*>(&xs[j][c]);
              sc[j] = fmaf(x4.w, y4.w, fmaf(x4.z, y4.z, fmaf(x4.y, y4.y, fmaf(x4.x, y4.x, sc[j]))));
            }
          }
        } else if ((r & 1) == 0) {
          for (int c = 0; c < r; c += 2) {
            const float2 y2 = *reinterpret_cast<const float2*>(y + c);
#pragma unroll
            for (int j = 0; j < ALS_TOPK_ROWS; ++j) sc[j] = fmaf(xs[j][c + 1], y2.y, fmaf(xs[j][c], y2.x, sc[j]));
          }
        } else {
          for (int c = 0; c < r; ++c) {
            const float yc = y[c];
#pragma unroll
            for (int j = 0; j < ALS_TOPK_ROWS; ++j) sc[j] = fmaf(xs[j][c], yc, sc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < ALS_TOPK_ROWS; ++j) {
        if (!live[j]) continue;
        if (n[j] + 64 > cb) {
          __syncthreads();
          n[j] = sel_keep_topk<false>(buf[j], n[j], k, hist, lane, tau[j]);
          have[j] = n[j] >= k;
        }
        const uint64_t key = sel_make_key<true>(sc[j], (uint32_t)item);
        const bool adm = cand && (!have[j] || key > tau[j]) &&
                         !(seen_col && sel_seen(seen_col, s_lo[j], s_hi[j], (int32_t)item));
        sel_append(buf[j], n[j], adm, key, lane);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < ALS_TOPK_ROWS; ++j) {
    const int64_t q = q0 + j;
    if (q >= n_q) continue;
    __syncthreads();
    if (live[j]) n[j] = sel_keep_topk<false>(buf[j], n[j], k, hist, lane, tau[j]);
    __syncthreads();
    sel_emit<true>(buf[j], n[j], k, lane, ids + q * k, vals + q * k, count + q);
  }
}

extern "C" int cqlrec_als_topk(const int32_t* users, int64_t n_q, const float* U, const uint8_t* u_has, int64_t n_users,
                               const float* V, const uint8_t* v_has, int64_t n_items, int32_t rank, const uint8_t* mask,
                               const int64_t* seen_off, const int32_t* seen_col, int32_t k, int32_t* ids, float* vals,
                               int32_t* count, cqlrec_stream stream) {
  CQL_REQUIRE(rank >= 1 && rank <= CQLREC_ALS_MAX_RANK, "als_topk: rank=%d out of range (1..%d)", rank, CQLREC_ALS_MAX_RANK);
  CQL_REQUIRE(k >= 1 && k <= CQLREC_ALS_MAX_K, "als_topk: k=%d out of range (1..%d)", k, CQLREC_ALS_MAX_K);
  CQL_REQUIRE(n_q >= 0 && n_q < ALS_MAX && n_users >= 0 && n_users < ALS_MAX && n_items >= 0 && n_items < ALS_MAX,
              "als_topk: n_q=%lld n_users=%lld n_items=%lld out of range", (long long)n_q, (long long)n_users,
              (long long)n_items);
  if (n_q == 0) return CQLREC_OK;
  CQL_REQUIRE(users && ids && vals && count, "als_topk: NULL pointer");
  CQL_REQUIRE((U && u_has) || n_users == 0, "als_topk: NULL pointer (user factors)");
  CQL_REQUIRE((V && v_has) || n_items == 0, "als_topk: NULL pointer (item factors)");
  CQL_REQUIRE((seen_off == nullptr) == (seen_col == nullptr), "als_topk: seen lists need both arrays (NULL pointer)");
  CQL_REQUIRE(((uintptr_t)V & 15) == 0, "als_topk: the item factors must be 16-byte aligned");
  const int cb = als_topk_cb(k);
  hipLaunchKernelGGL(als_topk_kernel, dim3((unsigned)cql_ceil_div(n_q, ALS_TOPK_ROWS)), dim3(64),
                     (size_t)ALS_TOPK_ROWS * cb * 8, (hipStream_t)stream, users, n_q, U, u_has, n_users, V, v_has, n_items,
                     (int)rank, mask, seen_off, seen_col, (int)k, cb, ids, vals, count);
  CQL_LAUNCH_CHECK("als_topk");
  return CQLREC_OK;
}

__global__ void als_pair_scores_kernel(const int32_t* __restrict__ pu, const int32_t* __restrict__ pi, int64_t n,
                                       const float* __restrict__ U, const uint8_t* __restrict__ u_has, int64_t n_users,
                                       const float* __restrict__ V, const uint8_t* __restrict__ v_has, int64_t n_items, int r,
                                       float* __restrict__ score, uint8_t* __restrict__ valid) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t u = pu[p], i = pi[p];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items && u_has[u] != 0 && v_has[i] != 0;
  float sc = 0.0f;
  if (ok) {
    const float* x = U + u * r;
    const float* y = V + i * r;
    for (int c = 0; c < r; ++c) sc = fmaf(x[c], y[c], sc);
  }
  score[p] = sc;
  valid[p] = ok ? 1 : 0;
}

extern "C" int cqlrec_als_pair_scores(const int32_t* pair_user, const int32_t* pair_item, int64_t n_pairs, const float* U,
                                      const uint8_t* u_has, int64_t n_users, const float* V, const uint8_t* v_has,
                                      int64_t n_items, int32_t rank, float* score, uint8_t* valid, cqlrec_stream stream) {
  CQL_REQUIRE(rank >= 1 && rank <= CQLREC_ALS_MAX_RANK, "als_pair_scores: rank=%d out of range (1..%d)", rank,
              CQLREC_ALS_MAX_RANK);
  CQL_REQUIRE(n_pairs >= 0 && n_pairs < ALS_MAX && n_users >= 0 && n_users < ALS_MAX && n_items >= 0 && n_items < ALS_MAX,
              "als_pair_scores: n_pairs=%lld n_users=%lld n_items=%lld out of range", (long long)n_pairs,
              (long long)n_users, (long long)n_items);
  if (n_pairs == 0) return CQLREC_OK;
  CQL_REQUIRE(pair_user && pair_item && score && valid, "als_pair_scores: NULL pointer");
  CQL_REQUIRE(((U && u_has) || n_users == 0) && ((V && v_has) || n_items == 0), "als_pair_scores: NULL pointer (factors)");
  hipLaunchKernelGGL(als_pair_scores_kernel, dim3(cql_ceil_div(n_pairs, 256)), dim3(256), 0, (hipStream_t)stream, pair_user,
                     pair_item, n_pairs, U, u_has, n_users, V, v_has, n_items, (int)rank, score, valid);
  CQL_LAUNCH_CHECK("als_pair_scores");
  return CQLREC_OK;
}
