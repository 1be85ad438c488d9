// The block sum shared by the loss kernels (pointwise.hip, iql.hip).
#pragma once
#include "common.h"

// The block's sums of N values per thread, each in one fixed order, come in two steps.  wave_partials (every thread): a shuffle
// tree per wave, then the waves' partials into red[j][wave] and a barrier.  add_partials (thread 0, inside the branch that uses
// the sums): red[j][0 .. n_waves) added first to last.  n_waves is the launch's blockDim.x >> 6, 16 at the most; a kernel that is
// only ever launched with 256 threads passes the literal 4, which unrolls to red[j][0] + red[j][1] + red[j][2] + red[j][3].
// (Two calls rather than one that hands the sums back: a sum that leaves thread 0's branch reaches the atomic as a per-lane value,
// and the compiler then adds the lanes' values up in a loop before the atomic instead of issuing it for the one lane.)
template <int N>
__device__ __forceinline__ void wave_partials(const float (&mine)[N], float (&red)[N][16]) {
  float v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = mine[j];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] += __shfl_down(v[j], o, 64);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int j = 0; j < N; ++j) red[j][threadIdx.x >> 6] = v[j];
  __syncthreads();
}
template <int N>
__device__ __forceinline__ void add_partials(const float (&red)[N][16], int n_waves, float (&sum)[N]) {
#pragma unroll
  for (int j = 0; j < N; ++j) sum[j] = red[j][0];
  for (int w = 1; w < n_waves; ++w)
#pragma unroll
    for (int j = 0; j < N; ++j) sum[j] += red[j][w];
}
