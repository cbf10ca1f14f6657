// The one kernel of select_common.h: pass 1 of topk.hip and of item_knn.hip writes one bound per (group, row); pass 2
// reads a row's bounds as whole lines.
#include "select_common.h"

// [groups][rows] -> [rows][gstride]  (32x32 tiles through LDS; both sides coalesced)
__global__ __launch_bounds__(256) void sel_transpose_kernel(const float* __restrict__ src, int ngroups, int64_t n_rows,
                                                            float* __restrict__ dst, int gstride) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  const int64_t u0 = (int64_t)blockIdx.x * 32;
  const int g0 = blockIdx.y * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = g0 + ty + 8 * j;
    const int64_t u = u0 + tx;
    t[ty + 8 * j][tx] = (g < ngroups && u < n_rows) ? src[(int64_t)g * n_rows + u] : NEG_INF_F;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int64_t u = u0 + ty + 8 * j;
    const int g = g0 + tx;
    if (u < n_rows && g < gstride) dst[u * gstride + g] = t[tx][ty + 8 * j];
  }
}

void cql_sel_transpose(const float* src, int ngroups, int64_t n_rows, float* dst, int gstride, hipStream_t s) {
  hipLaunchKernelGGL(sel_transpose_kernel, dim3(cql_ceil_div(n_rows, 32), cql_ceil_div(gstride, 32)), dim3(256), 0, s, src,
                     ngroups, n_rows, dst, gstride);
}
