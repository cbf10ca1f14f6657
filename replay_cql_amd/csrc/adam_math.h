// The Adam + Polyak arithmetic of one parameter and the one loop body the streaming optimizer kernels (adam.hip) are made
// of, plus the internal entry points of those kernels.  The expression order is the normative one (oracle.adam_ema_step):
// no fma contraction, IEEE division and square root -- whichever kernel updates a parameter, the bits are the same.
#pragma once
#include "common.h"
#include "qde_pieces.h"

// the dense launch with the deferred sum of dE_out's slab pieces added to the gradient as it is read (fix NULL or not
// valid: cqlrec_adam_ema)
int cql_adam_ema_fix(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b, uint16_t* target_b,
                     int64_t n, float step_size, float sqrt_bc2, float beta1, float beta2, float eps, float tau,
                     int32_t zero_grads, const CqlAdamFix* fix, hipStream_t stream);
// Adam over the whole embedding rows of E_in inside a cqlrec_train_steps call (adam.hip).  Only the rows
// marked in `row_map` (one byte per row, n_rows of them) carry a gradient this step: the others take g = 0 and their gradient
// elements are not read.  `age[r]` counts the steps row r is behind; a row is brought up to date -- the missed steps replayed in order with g = +0.0f, then this step's -- when it has a
// gradient (`row_map`), when the next step's forward reads it (`read_next`; NULL: every row, the flush), or when its age
// reaches the table's length.  `tab` holds the (step_size, sqrt_bc2) pairs of the last CQL_ADAM_DEFER_CAP steps, slot =
// step % CQL_ADAM_DEFER_CAP, formed on the host in double like the dense launch's two scalars.
#define CQL_ADAM_DEFER_CAP 64
struct CqlAdamSteps {
  float step_size[CQL_ADAM_DEFER_CAP], sqrt_bc2[CQL_ADAM_DEFER_CAP];
};
int cql_adam_ema_rows_deferred(float* theta, float* grads, float* m, float* v, float* target, uint16_t* theta_b,
                               uint16_t* target_b, int64_t n, const CqlAdamSteps& tab, uint64_t step, float beta1, float beta2,
                               float eps, float tau, int32_t zero_grads, const uint8_t* row_map, const uint8_t* read_next,
                               uint8_t* age, int32_t d, int64_t n_rows, hipStream_t stream);

__device__ __forceinline__ void adam_ema_elem(float g, float& p, float& m, float& v, float& t, float step_size, float sqrt_bc2,
                                              float beta1, float beta2, float eps, float tau, float omb1, float omb2,
                                              float omt) {
#pragma clang fp contract(off)
  m = beta1 * m + omb1 * g;
  v = beta2 * v + (omb2 * g) * g;
  const float denom = sqrtf(v) / sqrt_bc2 + eps;
  p = p - step_size * (m / denom);
  t = omt * t + tau * p;
}

// NT: the fp32 streams (read once, written once per step) bypass the caches with non-temporal accesses, so that the
// optimizer does not evict the bf16 E_out shadow -- which the Q-head kernels keep re-reading from L2 / Infinity Cache --
// when it runs next to them; the bf16 shadows it writes stay cacheable (they are what the next kernels read).
template <bool NT>
__device__ __forceinline__ float4 ld4(const float4* p) {
  if constexpr (NT) {
    const float* f = reinterpret_cast<const float*>(p);
    return make_float4(__builtin_nontemporal_load(f), __builtin_nontemporal_load(f + 1), __builtin_nontemporal_load(f + 2),
                       __builtin_nontemporal_load(f + 3));
  } else {
    return *p;
  }
}
template <bool NT>
__device__ __forceinline__ void st4(float4* p, float a, float b, float c, float d) {
  if constexpr (NT) {
    float* f = reinterpret_cast<float*>(p);
    __builtin_nontemporal_store(a, f);
    __builtin_nontemporal_store(b, f + 1);
    __builtin_nontemporal_store(c, f + 2);
    __builtin_nontemporal_store(d, f + 3);
  } else {
    *p = make_float4(a, b, c, d);
  }
}

// ---- the loop body of the streaming kernels: four consecutive parameters (float4 index i of every stream) ------------
struct AdamK {
  float beta1, beta2, eps, tau, omb1, omb2, omt;
  __device__ __forceinline__ AdamK(float b1, float b2, float eps_, float tau_)
      : beta1(b1), beta2(b2), eps(eps_), tau(tau_), omb1(1.0f - b1), omb2(1.0f - b2), omt(1.0f - tau_) {}
};
struct Adam4 {
  float p[4], m[4], v[4], t[4];
  // one step of the four parameters with gradients g
  __device__ __forceinline__ void step(const float (&g)[4], const AdamK& k, float step_size, float sqrt_bc2) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      adam_ema_elem(g[j], p[j], m[j], v[j], t[j], step_size, sqrt_bc2, k.beta1, k.beta2, k.eps, k.tau, k.omb1, k.omb2, k.omt);
  }
};
// The streams travel as separate __restrict__ pointers, as the kernels receive them: gathered in a struct, hipcc places
// the address arithmetic of the grid-stride loops differently.
template <bool NT>
__device__ __forceinline__ Adam4 adam_load4(const float4* __restrict__ theta, const float4* __restrict__ m,
                                            const float4* __restrict__ v, const float4* __restrict__ target, int64_t i) {
  const float4 p4 = ld4<NT>(theta + i), m4 = ld4<NT>(m + i), v4 = ld4<NT>(v + i), t4 = ld4<NT>(target + i);
  return {{p4.x, p4.y, p4.z, p4.w}, {m4.x, m4.y, m4.z, m4.w}, {v4.x, v4.y, v4.z, v4.w}, {t4.x, t4.y, t4.z, t4.w}};
}
// parameters, moments, target and the two bf16 shadows
template <bool NT>
__device__ __forceinline__ void adam_store4(float4* __restrict__ theta, float4* __restrict__ m, float4* __restrict__ v,
                                            float4* __restrict__ target, uint2* __restrict__ theta_b,
                                            uint2* __restrict__ target_b, int64_t i, const Adam4& a) {
  st4<NT>(theta + i, a.p[0], a.p[1], a.p[2], a.p[3]);
  st4<NT>(m + i, a.m[0], a.m[1], a.m[2], a.m[3]);
  st4<NT>(v + i, a.v[0], a.v[1], a.v[2], a.v[3]);
  st4<NT>(target + i, a.t[0], a.t[1], a.t[2], a.t[3]);
  theta_b[i] = make_uint2(pack_bf16x2(a.p[0], a.p[1]), pack_bf16x2(a.p[2], a.p[3]));
  target_b[i] = make_uint2(pack_bf16x2(a.t[0], a.t[1]), pack_bf16x2(a.t[2], a.t[3]));
}
// The dense body: five loads, the gradient through fix(g, i) (nothing, or what the gradient still lacks), one step, the
// stores, the gradient zeroed on request.
template <bool NT, class Fix>
__device__ __forceinline__ void adam_ema_body(float4* __restrict__ theta, float4* __restrict__ grads, float4* __restrict__ m,
                                              float4* __restrict__ v, float4* __restrict__ target,
                                              uint2* __restrict__ theta_b, uint2* __restrict__ target_b, int64_t i,
                                              const AdamK& k, float step_size, float sqrt_bc2, int zero_grads, Fix&& fix) {
  const float4 g4 = ld4<NT>(grads + i);
  Adam4 a = adam_load4<NT>(theta, m, v, target, i);
  float g[4] = {g4.x, g4.y, g4.z, g4.w};
  fix(g, i);
  a.step(g, k, step_size, sqrt_bc2);
  adam_store4<NT>(theta, m, v, target, theta_b, target_b, i, a);
  if (zero_grads) st4<NT>(grads + i, 0.f, 0.f, 0.f, 0.f);
}

// blocks of 256 threads for a grid-stride loop over n4 float4 (the Adam launches and cast_bf16)
static inline int float4_stream_grid(int64_t n4) {
  const int64_t blocks = (n4 + 255) / 256;
  return (int)(blocks > 8192 ? 8192 : blocks);
}
