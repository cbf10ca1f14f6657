// Streaming optimizer: fused Adam + Polyak + bf16 shadows (dense, deferred-row and fix-up forms), cast_bf16.
// gfx950 only.  The arithmetic and the one loop body are adam_math.h.
#include "common.h"
#include "adam_math.h"

// =============================================================================================================
// fused Adam + Polyak + bf16 shadows.  Pure HBM streaming: 20 B read + 24 B written per parameter in the full form
// (zero_grads = 1, every gradient element read).  Inside a cqlrec_train_steps call the steps that have a successor run
// leaner (train.hip): the item-side range keeps its gradient (20 B + 20 B: the next long dE_out kernel overwrites every
// row), the E_in range goes through adam_ema_rows_deferred_kernel (16 B + 20 B for a row that is brought up to
// date, + 4 B read if the batch touched it; one byte of age for a row that is left behind).
// Compiled with -ffp-contract=off so the expression order below is the normative one (oracle.adam_ema_step).
// =============================================================================================================
template <bool NT>
__global__ __launch_bounds__(256) void adam_ema_kernel(float4* __restrict__ theta, float4* __restrict__ grads,
                                                       float4* __restrict__ m, float4* __restrict__ v,
                                                       float4* __restrict__ target, uint2* __restrict__ theta_b,
                                                       uint2* __restrict__ target_b, int64_t n4, float step_size,
                                                       float sqrt_bc2, float beta1, float beta2, float eps, float tau,
                                                       int zero_grads) {
  const AdamK k(beta1, beta2, eps, tau);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    adam_ema_body<NT>(theta, grads, m, v, target, theta_b, target_b, i, k, step_size, sqrt_bc2, zero_grads,
                      [](float (&)[4], int64_t) __attribute__((always_inline)) {});
}

// The E_in range of the pipelined single-rank driver.  `row_map[r] != 0` says that the window-gather backward of THIS step
// wrote gradient row r (gbwd.hip, cql_gather_pool_bwd_mark_rows).  Any other row contributes g = +0.0f -- what the full
// form loads from a zeroed buffer -- without being read, so what an earlier step left in it is dead data.  The range starts
// at a row boundary; rows >= n_rows (the pad row, alignment padding) are never written by anyone.  zero_grads = 1 (the
// last step of a call) zeroes every element, stale rows included.
//
// Rows are deferred.  An Adam + Polyak step with g = +0.0f is a pure function of the
// row's own (theta, m, v, target) and of the step's two scalars, so a row that no step reads may stay behind: `age[r]` counts
// the steps row r has missed, and the launch that needs the row -- it has a gradient (row_map), the next step's forward
// gathers it (read_next), its age reaches the table's length, or every row is wanted (read_next == NULL: the last step of a
// call, or a step whose successor was not sampled ahead) -- replays the missed steps in registers, oldest first, each with
// the scalars of its own step from `tab`, then runs this step's: the same adam_ema_elem in the same order as the dense
// form, so the same bits, and the row crosses HBM once.  A row left behind has its age stored and nothing else touched;
// its shadows are stale, and nobody reads them before a later launch has brought the row up to date.
// A row of D floats is D/4 consecutive float4 (16 / 32 / 64 lanes) starting at a multiple of its length: it sits inside
// one wave, whose lanes all load age[r] before the row's first lane stores it (the stored value depends on the load).
// Rows >= n_rows (pad row, alignment padding) have no age: they take one dense step per launch, as in the form above.
// The zero of a replayed step goes through a register the compiler cannot see through: every step of the loop, replayed
// or current, is the one instruction sequence.
template <bool NT>
__global__ __launch_bounds__(256) void adam_ema_rows_deferred_kernel(
    float4* __restrict__ theta, float4* __restrict__ grads, float4* __restrict__ m, float4* __restrict__ v,
    float4* __restrict__ target, uint2* __restrict__ theta_b, uint2* __restrict__ target_b, int64_t n4, CqlAdamSteps tab,
    uint32_t step, float beta1, float beta2, float eps, float tau, int zero_grads, const uint8_t* __restrict__ row_map,
    const uint8_t* __restrict__ read_next, uint8_t* age, int ld4row, int64_t n_rows) {
  __shared__ float2 tab_s[CQL_ADAM_DEFER_CAP];
  if (threadIdx.x < CQL_ADAM_DEFER_CAP)
    tab_s[threadIdx.x] = make_float2(tab.step_size[threadIdx.x], tab.sqrt_bc2[threadIdx.x]);
  __syncthreads();
  const AdamK kk(beta1, beta2, eps, tau);
  float zero = 0.f;
  asm volatile("" : "+v"(zero));
  const int64_t row_lane = ((int64_t)1 << ld4row) - 1;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i >> ld4row;
    bool live = false, go = true;
    int k = 1;                                          // steps to run: the missed ones + this one
    if (row < n_rows) {
      live = row_map[row] != 0;
      k = (int)age[row] + 1;
      go = live || !read_next || read_next[row] != 0 || k >= CQL_ADAM_DEFER_CAP;
      if ((i & row_lane) == 0) age[row] = go ? (uint8_t)0 : (uint8_t)k;
    }
    if (go) {
      Adam4 x = adam_load4<NT>(theta, m, v, target, i);
      float4 g4 = make_float4(zero, zero, zero, zero);
      if (live) g4 = ld4<NT>(grads + i);
      for (int a = k - 1; a >= 0; --a) {
        const float2 sc = tab_s[(step - (uint32_t)a) & (uint32_t)(CQL_ADAM_DEFER_CAP - 1)];
        const float g[4] = {a == 0 ? g4.x : zero, a == 0 ? g4.y : zero, a == 0 ? g4.z : zero, a == 0 ? g4.w : zero};
        x.step(g, kk, sc.x, sc.y);
      }
      adam_store4<NT>(theta, m, v, target, theta_b, target_b, i, x);
    }
    if (zero_grads) st4<NT>(grads + i, 0.f, 0.f, 0.f, 0.f);
  }
}

int cql_adam_ema_rows_deferred(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b,
                               uint16_t* target_b, int64_t n, const CqlAdamSteps& tab, uint64_t step, float beta1, float beta2,
                               float eps, float tau, int32_t zero_grads, const uint8_t* row_map, const uint8_t* read_next,
                               uint8_t* age, int32_t d, int64_t n_rows, hipStream_t stream) {
  CQL_REQUIRE(theta && grads && m && v && target && theta_b && target_b && row_map && age,
              "adam_ema_rows_deferred: NULL pointer");
  CQL_REQUIRE(n > 0 && n % 4 == 0, "adam_ema_rows_deferred: n=%lld must be a positive multiple of 4", (long long)n);
  CQL_REQUIRE(cql_d_ok(d), "adam_ema_rows_deferred: d=%d unsupported", d);
  CQL_REQUIRE(n_rows >= 0 && n_rows * d <= n, "adam_ema_rows_deferred: %lld rows of %d do not fit n=%lld", (long long)n_rows,
              d, (long long)n);
  const int64_t n4 = n / 4;
  CqlProfScope prof(CQLREC_PH_ADAM, stream);
  hipLaunchKernelGGL(adam_ema_rows_deferred_kernel<true>, dim3(float4_stream_grid(n4)), dim3(256), 0, stream, (float4*)theta, (float4*)grads,
                     (float4*)m, (float4*)v, (float4*)target, (uint2*)theta_b, (uint2*)target_b, n4, tab, (uint32_t)step,
                     beta1, beta2, eps, tau, zero_grads, row_map, read_next, age, __builtin_ctz((unsigned)d) - 2, n_rows);
  CQL_LAUNCH_CHECK("adam_ema (deferred rows)");
  return CQLREC_OK;
}

// what qde_fixup_kernel would have added to the four gradient elements 4 i4 .. 4 i4 + 3 (relative to the start of the
// updated range).  D and the items per group are powers of two and every offset is a multiple of 4, so the four elements
// belong to one item (rows) or to four items of one group (column sums); 32-bit arithmetic (the host checks the range).
__device__ __forceinline__ void adam_fix4(const CqlAdamFix& f, float (&g)[4], int64_t i4, int ld, int li) {
  const QdeSlab& s = f.s;
  const int64_t e = 4 * i4;
  uint32_t item;
  int col = -1;
  if (e >= f.rows_off && e < f.rows_off + s.n_items * s.D) {
    const uint64_t r = (uint64_t)(e - f.rows_off);
    item = (uint32_t)(r >> ld);
    col = (int)(r & (uint64_t)(s.D - 1));
  } else if (e >= f.cs_off && e < f.cs_off + s.n_items) {
    item = (uint32_t)(e - f.cs_off);
  } else {
    return;
  }
#ifdef ADAMFIX_ABL_NOLOOP      // timing-only build: the gradient without the slabs
  return;
#endif
  const uint32_t grp = item >> li, row = item & (uint32_t)(s.items - 1);
  // (qde_axpy of qde_pieces.h, kept in place: through it hipcc builds this kernel's grid-stride loop differently -- 9 loops
  // become 6, 4380 bytes 4400.  `g += scale * slab` is its product, then sum: this file is compiled without contraction)
  QDE_FOR_SLAB_PIECES(uint32_t, uint64_t, s.pc, grp, p) {
    if (col >= 0) {
      const float4 s4 = *reinterpret_cast<const float4*>(s.row(p, row) + col);
      g[0] += s.scale * s4.x; g[1] += s.scale * s4.y; g[2] += s.scale * s4.z; g[3] += s.scale * s4.w;
    } else {
      const float* sc = s.cs(p, row);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if ((int64_t)item + k < s.n_items) g[k] += s.scale * sc[k];
    }
  }
}

template <bool NT>
__global__ __launch_bounds__(256) void adam_ema_fix_kernel(float4* __restrict__ theta, float4* __restrict__ grads,
                                                           float4* __restrict__ m, float4* __restrict__ v,
                                                           float4* __restrict__ target, uint2* __restrict__ theta_b,
                                                           uint2* __restrict__ target_b, int64_t n4, float step_size,
                                                           float sqrt_bc2, float beta1, float beta2, float eps, float tau,
                                                           int zero_grads, CqlAdamFix fix) {
  const AdamK k(beta1, beta2, eps, tau);
  const int ld = __builtin_ctz((unsigned)fix.s.D), li = __builtin_ctz((unsigned)fix.s.items);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x)
    adam_ema_body<NT>(theta, grads, m, v, target, theta_b, target_b, i, k, step_size, sqrt_bc2, zero_grads,
                      [&](float (&g)[4], int64_t i4) __attribute__((always_inline)) { adam_fix4(fix, g, i4, ld, li); });
}

// one launch site for the dense form: with `fix` valid the kernel that adds the slab pieces, else the plain one
int cql_adam_ema_fix(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b, uint16_t* target_b,
                     int64_t n, float step_size, float sqrt_bc2, float beta1, float beta2, float eps, float tau,
                     int32_t zero_grads, const CqlAdamFix* fix, hipStream_t stream) {
  const bool on = fix && fix->valid;
  const bool pow2 = on && (fix->s.D & (fix->s.D - 1)) == 0 && (fix->s.items & (fix->s.items - 1)) == 0 &&
                    fix->rows_off % 4 == 0 && fix->cs_off % 4 == 0 &&
                    fix->s.pc.W() * ((int64_t)fix->s.pc.nblk + 1) < (1ll << 31) && fix->s.n_items < (1ll << 31);
  CQL_REQUIRE(!on || pow2, "adam_ema: deferred fix-up outside the supported range");
  CQL_REQUIRE(theta && grads && m && v && target && theta_b && target_b, "adam_ema: NULL pointer");
  CQL_REQUIRE(n > 0 && n % 4 == 0, "adam_ema: n=%lld must be a positive multiple of 4", (long long)n);
  const int64_t n4 = n / 4;
  CqlProfScope prof(CQLREC_PH_ADAM, stream);
#define ADAM_LAUNCH(kernel, ...)                                                                                       \
  hipLaunchKernelGGL(kernel, dim3(float4_stream_grid(n4)), dim3(256), 0, stream, (float4*)theta, (float4*)grads, (float4*)m,    \
                     (float4*)v, (float4*)target, (uint2*)theta_b, (uint2*)target_b, n4, step_size, sqrt_bc2, beta1, beta2, \
                     eps, tau, zero_grads, ##__VA_ARGS__)
  if (on) ADAM_LAUNCH(adam_ema_fix_kernel<true>, *fix);
  else ADAM_LAUNCH(adam_ema_kernel<true>);
#undef ADAM_LAUNCH
  CQL_LAUNCH_CHECK(on ? "adam_ema (deferred fix-up)" : "adam_ema");
  return CQLREC_OK;
}

extern "C" int cqlrec_adam_ema(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b,
                               uint16_t* target_b, int64_t n, float step_size, float sqrt_bc2, float beta1, float beta2,
                               float eps, float tau, int32_t zero_grads, cqlrec_stream stream) {
  return cql_adam_ema_fix(theta, grads, m, v, target, theta_b, target_b, n, step_size, sqrt_bc2, beta1, beta2, eps, tau,
                          zero_grads, nullptr, (hipStream_t)stream);
}

__global__ __launch_bounds__(256) void cast_bf16_kernel(const float4* __restrict__ src, uint2* __restrict__ dst,
                                                        int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = src[i];
    dst[i] = make_uint2(pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w));
  }
}
extern "C" int cqlrec_cast_bf16(const float* src, uint16_t* dst_b, int64_t n, cqlrec_stream stream) {
  CQL_REQUIRE(src && dst_b, "cast_bf16: NULL pointer");
  CQL_REQUIRE(n > 0 && n % 4 == 0, "cast_bf16: n=%lld must be a positive multiple of 4", (long long)n);
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(cast_bf16_kernel, dim3(float4_stream_grid(n4)), dim3(256), 0, (hipStream_t)stream, (const float4*)src,
                     (uint2*)dst_b, n4);
  CQL_LAUNCH_CHECK("cast_bf16");
  return CQLREC_OK;
}
