// What the row-walking input packs share (pack_input_rows_kernel in pointwise.hip, pack_aug_kernel in augment.hip): the walk's
// constant and grid, the normalisation-table entry and the packed-pixel store.  The augmented operand is bit for bit the plain pack
// of host-augmented frames because both kernels take the table entry from here.
#pragma once
#include "common.h"

// pairs of packed rows a block walks; 58 pairs cover the 115 packed rows of a frame
constexpr int kPackPairs = 4;
inline dim3 pack_rows_grid(int n_img) { return dim3((58 + kPackPairs - 1) / kPackPairs, n_img); }

// entry (c, t) of the per-block normalisation table: byte t of channel c as pack_input_kernel normalises it, element by element
template <typename T>
__device__ __forceinline__ T pack_norm_entry(int t, int c) {
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
  return from_f32<T>((((float)t / 255.0f) - mean[c]) / stdv[c]);
}

// the counter hash of every draw a pack makes (augment.hip's per-sample draws, attrib.hip's per-element noise)
__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the 16 elements of one packed pixel (12 values + 4 zero padding channels), as 16-byte vectors; v and d are 16-byte aligned
template <typename T>
__device__ __forceinline__ void pack_store16(T* d, const T* v) {
  constexpr int V16 = (int)(16 * sizeof(T) / 16);
#pragma unroll
  for (int q = 0; q < V16; ++q) reinterpret_cast<uint4*>(d)[q] = reinterpret_cast<const uint4*>(v)[q];
}
