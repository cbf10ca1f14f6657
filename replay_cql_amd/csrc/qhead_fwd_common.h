// What the one-wave-per-SIMD forward kernels share besides the LDS image (qhead_fwd2.hip, qhead_fwd3.hip; the slice
// preamble also serves qhead_argmax2.hip): which slice of the streamed table a block takes, the fixed reference of the
// exponentials from the slice's first tile, and the store of a (slice, state) partial result.
#pragma once
#include "qhead_image.h"

#define QF_REF_MARGIN 8.0f      // nats between the first tile's maximum and the reference

// block -> (slice of the streamed rows, block of owner rows); TI rows per stage
struct QSlice {
  int split;
  int64_t rblk;
  int64_t s_begin, s_end;     // streamed rows of the slice
  int nst;                    // its stages (<= 0: nothing to do)
  uint32_t gst0;              // index of its first stage in the whole table
};
template <int TI>
__device__ __forceinline__ QSlice slice_preamble(int nsplit, int64_t split_rows, int64_t n_rows) {
  QSlice s;
  s.split = blockIdx.x % nsplit;
  s.rblk = blockIdx.x / nsplit;
  s.s_begin = (int64_t)s.split * split_rows;
  s.s_end = (s.s_begin + split_rows < n_rows) ? (s.s_begin + split_rows) : n_rows;
  s.nst = (s.s_end > s.s_begin) ? (int)((s.s_end - s.s_begin + TI - 1) / TI) : 0;
  s.gst0 = (uint32_t)(s.s_begin / TI);
  return s;
}

// Scores of the slice's first tile (rows in af, bias in sv) for state `row`, through TEMPORARY fragments: their maximum
// fixes the reference.  rl2 = -reference * log2e for the loop; the reference itself is parked in an AccVGPR until the end.
// (The fragments the loop keeps are loaded afterwards and used by the loop only: with one more use in front of the loop
// hipcc rotates them through AccVGPR tuples, four copies per product.)
template <int D>
__device__ __forceinline__ void first_tile_reference(const bf16x8 (&af)[D / 16], const f32x16& sv, const uint16_t* H_b, int64_t row,
                                                     int64_t n_states, int h, float& rl2, float& ref_a) {
  bf16x8 tmpf[D / 16];
  load_owner_frags<D>(H_b, row, n_states, h, tmpf);
  f32x16 t = sv;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) t = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[s], tmpf[s], t, 0, 0, 0);
  float m = t[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = fmaxf(m, t[i]);
  m = fmaxf(m, __shfl_xor(m, 32));
  const float rv = (m == NEG_INF_F) ? 0.f : m + QF_REF_MARGIN;
  rl2 = -rv * CQL_LOG2E;
  asm volatile("v_accvgpr_write_b32 %0, %1" : "=a"(ref_a) : "v"(rv));
  asm volatile("" : "+v"(rl2));      // (keeps the temporaries' uses in front of the loads that follow)
}

// partials of state `row` in slice `split`: the un-normalised slab row, (reference, sum relative to it), overflow flag
template <int D>
__device__ __forceinline__ void store_partials(const QFwd2Args& a, int split, int64_t row, int h, const f32x16 (&y)[D / 32], float cs,
                                               const float& ref_a) {
  const float ls = cs + __shfl_xor(cs, 32);
  if (row < a.n_states) {
    const int64_t pidx = (int64_t)split * a.n_states + row;
    float* dst = a.slab + pidx * D;
#pragma unroll
    for (int ft = 0; ft < D / 32; ++ft)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(dst + ft * 32 + 8 * q + 4 * h) =
            make_float4(y[ft][4 * q + 0], y[ft][4 * q + 1], y[ft][4 * q + 2], y[ft][4 * q + 3]);
    if (h == 0) {
      float rv;
      asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(rv) : "a"(ref_a));
      a.part_a[pidx] = rv;
      a.part_b[pidx] = ls;
      if (!(ls < 3.0e38f) && a.flag) atomicOr(a.flag, 1);      // inf or NaN: the guarded first form redoes the pass
    }
  }
}
