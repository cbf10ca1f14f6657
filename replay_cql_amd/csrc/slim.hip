// SLIM on the device (section f12 of include/cqlrec.h; DESIGN.md section 3.15 is the normative text): per target item j
// the elastic-net problem  min 1/(2 nu) |x_j - X w|^2 + lambda |w|_1 + beta/2 |w|^2  over w >= 0, w_j = 0, solved by
// cyclic coordinate descent on the Gram matrix G = X^T X.
//
// One workgroup of SL_T lanes per target column, persistent: workgroup b takes the columns col_begin + b, + gridDim, ...
// Lane t owns the coordinates i = t (mod SL_T): their q_i (dynamic LDS, n doubles), their w_i (a slice of the workspace,
// read and written by that lane alone) and their part of every axpy, so the state of a column needs no barrier of its
// own.  The only exchange is the choice of the next coordinate: all lanes screen the SL_T coordinates of a chunk against
// the current q at once, the lowest index whose update is not zero wins (ballot, one LDS slot per wave, one barrier), its
// axpy is applied by every lane to its own elements, and the lanes behind it screen again.  A coordinate whose update is
// zero leaves q as it is, so this is the ascending cyclic sweep bit for bit, at the cost of its updates, not its visits.
//
// Every value that steers a branch around a barrier (the chosen coordinate, the stopping test, G_jj == 0) is the same in
// all lanes and is passed through readfirstlane, so that the branch is a scalar one: the compiler must not be left to
// linearise such a branch as if lanes could disagree, with lanes parked on one side of a barrier.
//
// Compiled with -ffp-contract=off: the update, the refresh and the certificate are evaluated as written.
#include "common.h"

#include <limits.h>

#define SL_T 1024                      // lanes of a workgroup = coordinates of a chunk
#define SL_WAVES (SL_T / CQL_WAVE)
#define SL_MAX_BLOCKS 512              // workgroups of a launch (two per CU while q takes at most half of the LDS)
#define SL_NONE INT_MAX

struct SlimArgs {
  const double* G;
  int64_t ldg;
  int32_t n, max_iter, col_begin, col_end;
  double nu, nb, nl, beta, lambda, thr;   // n_users, nu * beta, nu * lambda_, beta, lambda_, tol * lambda_
  const double* diag;                     // [n] G_ii
  double* w_all;                          // [blocks][w_stride]
  int64_t w_stride;
  double* S;
  int64_t lds;
  int32_t* sweeps;
  double* kkt;
  int64_t* updates;
};

__global__ __launch_bounds__(256) void slim_diag_kernel(const double* G, int64_t ldg, int32_t n, double* diag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) diag[i] = G[i * ldg + i];
}

static __device__ __forceinline__ int slim_uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// q[e] = op(e, q[e], row[e]) over the elements e = t (mod SL_T) of this lane, four loads in flight: the latency of a row is
// paid once per four elements, the values and their order per element are those of the plain loop
template <typename Op>
static __device__ __forceinline__ void slim_row(const double* __restrict__ row, double* q, int n, int t, Op op) {
  int e = t;
  for (; e + 3 * SL_T < n; e += 4 * SL_T) {
    const double g0 = row[e], g1 = row[e + SL_T], g2 = row[e + 2 * SL_T], g3 = row[e + 3 * SL_T];
    q[e] = op(e, q[e], g0);
    q[e + SL_T] = op(e + SL_T, q[e + SL_T], g1);
    q[e + 2 * SL_T] = op(e + 2 * SL_T, q[e + 2 * SL_T], g2);
    q[e + 3 * SL_T] = op(e + 3 * SL_T, q[e + 3 * SL_T], g3);
  }
  for (; e < n; e += SL_T) q[e] = op(e, q[e], row[e]);
}

// q = G[j, :] - sum over the support, k ascending, of w_k G[k, :], element by element in that order
static __device__ __forceinline__ void slim_refresh(const SlimArgs& a, const double* __restrict__ w, double* q, int j, int t,
                                                    double* s_w, uint64_t* s_mask) {
  const int n = a.n, lane = t & 63, wave = t >> 6;
  slim_row(a.G + (int64_t)j * a.ldg, q, n, t, [](int, double, double g) { return g; });
  for (int c0 = 0; c0 < n; c0 += SL_T) {
    const int i = c0 + t;
    const double wk = i < n ? w[i] : 0.0;
    const uint64_t m = __ballot(wk != 0.0);
    s_w[t] = wk;
    if (lane == 0) s_mask[wave] = m;
    __syncthreads();
    for (int wv = 0; wv < SL_WAVES; ++wv) {
      const uint64_t mv = s_mask[wv];
      uint64_t mm = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(mv >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)(mv & 0xffffffffu));
      while (mm) {
        const int b = __builtin_ctzll(mm);
        mm &= mm - 1;
        const double x = s_w[wv * 64 + b];
        slim_row(a.G + (int64_t)(c0 + wv * 64 + b) * a.ldg, q, n, t, [x](int, double qe, double g) { return qe - x * g; });
      }
    }
    __syncthreads();
  }
}

// at most 64 registers, so that two workgroups share a CU while q takes at most half of its LDS (n <= 9 600 or so)
__global__ __launch_bounds__(SL_T) __attribute__((amdgpu_waves_per_eu(8, 8))) void slim_fit_kernel(SlimArgs a) {
  extern __shared__ double q[];                       // [n]; element e belongs to lane e % SL_T
  __shared__ int32_t s_idx[2][SL_WAVES];
  __shared__ double s_delta[2][SL_WAVES];
  __shared__ double s_w[SL_T];
  __shared__ uint64_t s_mask[SL_WAVES];
  __shared__ double s_red[SL_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, n = a.n;
  double* __restrict__ w = a.w_all + (int64_t)blockIdx.x * a.w_stride;
  for (int j = a.col_begin + (int)blockIdx.x; j < a.col_end; j += (int)gridDim.x) {
    for (int e = t; e < n; e += SL_T) w[e] = 0.0;
    slim_row(a.G + (int64_t)j * a.ldg, q, n, t, [](int, double, double g) { return g; });
    int64_t upd = 0;
    int32_t sweeps = 0;
    double cert = 0.0;
    if (slim_uniform(a.diag[j] != 0.0)) {
      int par = 0;
      for (;;) {
        // ---- one full sweep, coordinates ascending
        for (int c0 = 0; c0 < n; c0 += SL_T) {
          const int i = c0 + t;
          const bool mine = i < n && i != j;
          double wc = 0.0, gii = 0.0, d = 0.0;
          if (mine) {
            wc = w[i];
            gii = a.diag[i];
            d = gii + a.nb;
          }
          bool live = mine && d > 0.0;
          for (;;) {
            double nw = wc;
            if (live) {
              const double r = (q[i] + gii * wc) - a.nl;
              nw = (r > 0.0 ? r : 0.0) / d;
            }
            const bool cand = live && nw != wc;
            const uint64_t m = __ballot(cand);
            if (m ? lane == __builtin_ctzll(m) : lane == 0) {
              s_idx[par][wave] = m ? t : SL_NONE;
              s_delta[par][wave] = nw - wc;
            }
            __syncthreads();
            int sel = SL_NONE;
#pragma unroll
            for (int wv = 0; wv < SL_WAVES; ++wv) sel = min(sel, s_idx[par][wv]);
            sel = slim_uniform(sel);
            if (sel == SL_NONE) {
              par ^= 1;
              break;
            }
            const double delta = s_delta[par][sel >> 6];
            par ^= 1;
            if (t == sel) wc = nw;
            if (t <= sel) live = false;
            slim_row(a.G + (int64_t)(c0 + sel) * a.ldg, q, n, t, [delta](int, double qe, double g) { return qe - delta * g; });
            ++upd;
          }
          if (mine) w[i] = wc;
        }
        ++sweeps;
        // ---- refresh q from w, then the certificate from the refreshed q
        slim_refresh(a, w, q, j, t, s_w, s_mask);
        double mx = 0.0;
        {
          const double nu = a.nu, beta = a.beta, lambda = a.lambda;
          slim_row(w, q, n, t, [&mx, nu, beta, lambda, j](int e, double qe, double we) {   // the "row" is w; q stays
            const double g = ((-qe) / nu + beta * we) + lambda;
            const double v = we > 0.0 ? g : (g < 0.0 ? g : 0.0);
            const double av = e == j ? 0.0 : fabs(v);
            if (av > mx) mx = av;
            return qe;
          });
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
          const double other = __shfl_xor(mx, o, 64);
          if (other > mx) mx = other;
        }
        if (lane == 0) s_red[wave] = mx;
        __syncthreads();
        cert = 0.0;
#pragma unroll
        for (int wv = 0; wv < SL_WAVES; ++wv) cert = s_red[wv] > cert ? s_red[wv] : cert;
        __syncthreads();
        if (slim_uniform(cert <= a.thr || sweeps >= a.max_iter)) break;
      }
    }
    for (int e = t; e < n; e += SL_T) a.S[(int64_t)e * a.lds + j] = w[e];
    if (t == 0) {
      a.sweeps[j] = sweeps;
      a.kkt[j] = cert;
      a.updates[j] = upd;
    }
  }
}

extern "C" int64_t cqlrec_slim_fit_ws_bytes(int64_t n) {
  if (n < 1 || n > CQLREC_SLIM_MAX_ITEMS) return 0;
  return cql_align256(n * 8) * (1 + SL_MAX_BLOCKS);   // G's diagonal, one w per workgroup
}

extern "C" int cqlrec_slim_fit(const double* G, int64_t ldg, int64_t n, int64_t n_users, double beta, double lambda_,
                               double tol, int32_t max_iter, int64_t col_begin, int64_t col_end, void* ws, int64_t ws_bytes,
                               double* S, int64_t lds, int32_t* sweeps, double* kkt, int64_t* updates, cqlrec_stream stream) {
  CQL_REQUIRE(n >= 1 && n <= CQLREC_SLIM_MAX_ITEMS, "slim_fit: n=%lld out of range (1..%lld)", (long long)n,
              (long long)CQLREC_SLIM_MAX_ITEMS);
  CQL_REQUIRE(n_users >= 1 && n_users < (1ll << 31), "slim_fit: n_users=%lld out of range (1..2^31-1)", (long long)n_users);
  CQL_REQUIRE(beta >= 0.0 && beta < __builtin_inf(), "slim_fit: beta=%g out of range (0 or more, finite)", beta);
  CQL_REQUIRE(lambda_ > 0.0 && lambda_ < __builtin_inf(), "slim_fit: lambda_=%g out of range (above 0, finite)", lambda_);
  CQL_REQUIRE(tol > 0.0 && tol < __builtin_inf(), "slim_fit: tol=%g out of range (above 0, finite)", tol);
  CQL_REQUIRE(max_iter >= 1, "slim_fit: max_iter=%d out of range (1 or more)", (int)max_iter);
  CQL_REQUIRE(col_begin >= 0 && col_begin < col_end && col_end <= n, "slim_fit: columns %lld..%lld out of range (0 <= begin < end <= %lld)",
              (long long)col_begin, (long long)col_end, (long long)n);
  CQL_REQUIRE(ldg >= n && lds >= n, "slim_fit: leading dimension ldg=%lld or lds=%lld is shorter than n=%lld", (long long)ldg,
              (long long)lds, (long long)n);
  CQL_REQUIRE(G && S && sweeps && kkt && updates && ws, "slim_fit: NULL pointer");
  const int64_t need = cqlrec_slim_fit_ws_bytes(n);
  CQL_REQUIRE(ws_bytes >= need, "slim_fit: the workspace holds %lld bytes, %lld are needed", (long long)ws_bytes, (long long)need);
  hipStream_t s = (hipStream_t)stream;
  char* base = static_cast<char*>(ws);
  SlimArgs a = {};
  a.G = G; a.ldg = ldg;
  a.n = (int32_t)n; a.max_iter = max_iter; a.col_begin = (int32_t)col_begin; a.col_end = (int32_t)col_end;
  a.nu = (double)n_users; a.nb = a.nu * beta; a.nl = a.nu * lambda_; a.beta = beta; a.lambda = lambda_; a.thr = tol * lambda_;
  double* diag = reinterpret_cast<double*>(base);
  a.diag = diag;
  a.w_stride = cql_align256(n * 8) / 8;
  a.w_all = diag + a.w_stride;
  a.S = S; a.lds = lds; a.sweeps = sweeps; a.kkt = kkt; a.updates = updates;
  static bool attr_set_dev[CQL_MAX_DEVICES] = {};   // > 64 KiB of dynamic LDS needs the opt-in once per kernel and device
  bool& attr_set = attr_set_dev[cql_device_slot()];
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)slim_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, CQLREC_SLIM_MAX_ITEMS * 8);
    attr_set = true;
  }
  hipLaunchKernelGGL(slim_diag_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G, ldg, a.n, diag);
  const int64_t cols = col_end - col_begin;
  const unsigned blocks = (unsigned)(cols < SL_MAX_BLOCKS ? cols : SL_MAX_BLOCKS);
  hipLaunchKernelGGL(slim_fit_kernel, dim3(blocks), dim3(SL_T), (size_t)(n * 8), s, a);
  CQL_LAUNCH_CHECK("slim_fit");
  return CQLREC_OK;
}
