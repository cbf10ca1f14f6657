// The non-template kernels of segment_common.h and their launchers, once per program: iota, the group-key gather, and the
// tail of the rank inside a user that cqlrec_split_rank and cqlrec_prepare_rank share.
#include "segment_common.h"

__global__ void cql_iota_kernel(uint32_t* __restrict__ perm, int64_t n, int reversed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = (uint32_t)(reversed ? n - 1 - i : i);
}
void cql_iota(uint32_t* perm, int64_t n, bool reversed, hipStream_t s) {
  hipLaunchKernelGGL(cql_iota_kernel, dim3(cql_ceil_div(n, 256)), dim3(256), 0, s, perm, n, reversed ? 1 : 0);
}

__global__ void cql_group_key_kernel(const int32_t* __restrict__ group, const uint32_t* __restrict__ perm, int64_t n,
                                     uint32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint32_t)group[perm[i]];
}
void cql_group_key(const int32_t* group, const uint32_t* perm, int64_t n, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(cql_group_key_kernel, dim3(cql_ceil_div(n, 256)), dim3(256), 0, s, group, perm, n, out);
}

__global__ void cql_rank_finish_kernel(const int32_t* __restrict__ user_idx, const uint32_t* __restrict__ perm, int64_t n,
                                       const int64_t* __restrict__ offsets, int32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t r = perm[i];
  rank[r] = (int32_t)(i - offsets[user_idx[r]] + 1);
}
__global__ void cql_rank_count_kernel(const int64_t* __restrict__ offsets, int64_t n_users, int32_t* __restrict__ count) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n_users) count[u] = (int32_t)(offsets[u + 1] - offsets[u]);
}

int cql_rank_tail(CqlPermSort& ps, const int32_t* user_idx, int64_t n_users, int64_t* offsets, int32_t* rank, int32_t* count,
                  int64_t* n_present, const char* what) {
  // by user, over the bits a user id below n_users can have
  cql_group_key(user_idx, ps.perm, ps.n, ps.keys<uint32_t>(), ps.s);
  const int rc = ps.pass<uint32_t>(what, cql_bits_for(n_users));
  if (rc != CQLREC_OK) return rc;
  if (n_present) CQL_MEMSET(n_present, 0, 8, ps.s, what);
  cql_segment_bounds(CqlGroupOfPerm{user_idx, ps.perm}, ps.n, n_users, offsets, (unsigned long long*)n_present, ps.s);
  const dim3 block(256);
  hipLaunchKernelGGL(cql_rank_finish_kernel, dim3(cql_ceil_div(ps.n, 256)), block, 0, ps.s, user_idx, ps.perm, ps.n, offsets,
                     rank);
  hipLaunchKernelGGL(cql_rank_count_kernel, dim3(cql_ceil_div(n_users, 256)), block, 0, ps.s, offsets, n_users, count);
  CQL_LAUNCH_CHECK(what);
  return CQLREC_OK;
}
