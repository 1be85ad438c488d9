// Prioritized experience replay (Schaul et al., ICLR 2016) on the device: stratified sampling of a minibatch by priority,
// importance weights, and the priority update behind the TD loss.  No host round trip: the three launches are queued on the
// caller's stream next to the update's kernels.
//
// The priority table p[n] is f32 and holds (e + eps)^alpha (>= 0).  Every sum is f64 in a FIXED order, so a numpy restatement
// (tests/per_oracle.py) reproduces the draws bit for bit:
//
//   segments of kSeg = 32 entries, chunks of kSegsPerChunk = 64 segments (kChunk = 2048 entries); entries >= n count as 0
//   seg[s]   = (((0 + p[32s]) + p[32s+1]) + ...) + p[32s+31]              left to right      (per_blocksum, one lane per segment)
//   chunk[c] = (((0 + seg[64c]) + seg[64c+1]) + ...) + seg[64c+63]        left to right      (per_blocksum, lane 0 of the wave)
//   P[c]     = (((0 + chunk[0]) + chunk[1]) + ...) + chunk[c],  S = P[nchunk-1]            (per_sample, one thread)
//
// Draw j of the global batch G (per_sample, one thread per draw):
//   r_j = (h >> 11) * 2^-53,  h = splitmix64(splitmix64(seed) ^ (step * G + j))        (uint64 arithmetic, wrapping)
//   u_j = ((j + r_j) * S) / G
//   c   = smallest chunk with P[c] > u_j;   t = u_j - P[c-1]  (u_j when c = 0)
//         none (u_j rounded to >= S): c = the last chunk with chunk[c] > 0, t = +inf
//   s   = smallest segment of chunk c with (((0 + seg[64c]) + ...) + seg[s]) > t;   t2 = t - (((0 + seg[64c]) + ...) + seg[s-1])
//         none: s = the last segment of chunk c with seg[s] > 0, t2 = +inf
//   i_j = smallest entry of segment s with (((0 + p[32s]) + ...) + p[i]) > t2
//         none: the last entry of segment s with p > 0
//   An entry with p = 0 is never drawn (each level's running sum only grows at a non-zero entry, and t, t2 >= 0).
//   w_j = (n * p[i_j] / S)^-beta / max_k (n * p[i_k] / S)^-beta        (f64, stored as f32)
// The update (per_update) sets p[idx[j]] = (err[j] + eps)^alpha (f64 pow, stored as f32); an index drawn more than once takes
// the value of its LARGEST j (every other occurrence skips its store): no atomics, the same table on every run and rank.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSeg = 32;
constexpr int kSegsPerChunk = 64;
constexpr int64_t kChunk = (int64_t)kSeg * kSegsPerChunk;
constexpr int kMaxChunks = 4096;       // per_sample keeps the chunk prefix in LDS (32 KB): n <= 8,388,608
constexpr int kSampleThreads = 1024;
constexpr int kMaxDrawsPerThread = 4;  // G <= 4096
constexpr double kEps = 1e-6;

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ inline int64_t n_segs(int64_t n) { return (n + kSeg - 1) / kSeg; }
__host__ __device__ inline int64_t n_chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }
inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// ---- per_blocksum: one wave per chunk, one lane per segment ---------------------------------------------------------------
__global__ __launch_bounds__(256) void per_blocksum_kernel(const float* __restrict__ p, int64_t n, double* __restrict__ seg,
                                                           double* __restrict__ chunk, int64_t nchunk) {
  __shared__ double lane_sum[4][kSegsPerChunk];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + wave;
  const int64_t s = c * kSegsPerChunk + lane;
  const int64_t lo = s * kSeg;
  double acc = 0.0;
  if (lo + kSeg <= n) {
    const float4* q = reinterpret_cast<const float4*>(p + lo);
    float4 v[kSeg / 4];
#pragma unroll
    for (int k = 0; k < kSeg / 4; ++k) v[k] = q[k];
#pragma unroll
    for (int k = 0; k < kSeg / 4; ++k) {
      acc += (double)v[k].x;
      acc += (double)v[k].y;
      acc += (double)v[k].z;
      acc += (double)v[k].w;
    }
  } else {
    for (int64_t i = lo; i < n && i < lo + kSeg; ++i) acc += (double)p[i];
  }
  if (lo < n) seg[s] = acc;
  lane_sum[wave][lane] = acc;
  __syncthreads();
  if (lane == 0 && c < nchunk) {
    double t = 0.0;
    for (int k = 0; k < kSegsPerChunk; ++k) t += lane_sum[wave][k];
    chunk[c] = t;
  }
}

// ---- per_sample: ONE block; chunk prefix in LDS, then one thread per draw --------------------------------------------------
__global__ __launch_bounds__(kSampleThreads) void per_sample_kernel(const float* __restrict__ p, int64_t n, const double* __restrict__ seg,
                                                                    const double* __restrict__ chunk, int nchunk, int G, uint64_t seed,
                                                                    uint64_t step, double beta, int64_t* __restrict__ idx_out,
                                                                    float* __restrict__ w_out) {
  extern __shared__ double P[];  // [nchunk]
  __shared__ double red[kSampleThreads / 64];
  __shared__ int last_chunk;
  const int tid = threadIdx.x;
  for (int c = tid; c < nchunk; c += kSampleThreads) P[c] = chunk[c];
  __syncthreads();
  if (tid == 0) {
    double run = 0.0;
    int last = -1;
    for (int c = 0; c < nchunk; ++c) {
      if (P[c] > 0.0) last = c;
      run += P[c];
      P[c] = run;
    }
    last_chunk = last;
  }
  __syncthreads();
  const double S = P[nchunk - 1];
  const uint64_t key = splitmix64(seed);
  double wraw[kMaxDrawsPerThread];
  int64_t got[kMaxDrawsPerThread];
  double wmax = 0.0;
#pragma unroll
  for (int k = 0; k < kMaxDrawsPerThread; ++k) {
    const int j = tid + k * kSampleThreads;
    wraw[k] = 0.0;
    got[k] = 0;
    if (j >= G) continue;
    const uint64_t h = splitmix64(key ^ (step * (uint64_t)G + (uint64_t)j));
    const double r = (double)(h >> 11) * 0x1.0p-53;
    const double u = (((double)j + r) * S) / (double)G;
    // chunk: smallest c with P[c] > u (binary search over the non-decreasing prefix)
    int lo = 0, hi = nchunk;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (P[mid] > u) hi = mid;
      else lo = mid + 1;
    }
    int c = lo;
    double t;
    if (c < nchunk) {
      t = c > 0 ? u - P[c - 1] : u;
    } else {
      c = last_chunk;
      t = INFINITY;
    }
    int64_t i = 0;
    if (c >= 0) {
      // segment inside chunk c
      const int64_t s0 = (int64_t)c * kSegsPerChunk;
      const int64_t s_end = min(s0 + kSegsPerChunk, n_segs(n));
      double run = 0.0, before = 0.0;
      int64_t s_hit = -1, s_last = -1;
      for (int64_t s = s0; s < s_end; ++s) {
        const double v = seg[s];
        if (v > 0.0) s_last = s;
        if (s_hit < 0) {
          const double nr = run + v;
          if (nr > t) {
            s_hit = s;
            before = run;
          }
          run = nr;
        }
      }
      double t2 = t - before;
      if (s_hit < 0) {
        s_hit = s_last;
        t2 = INFINITY;
      }
      // entry inside segment s_hit (s_hit >= 0 whenever chunk[c] > 0, which the chunk search guarantees)
      const int64_t e0 = max(s_hit, (int64_t)0) * kSeg;
      const int64_t e_end = min(e0 + kSeg, n);
      double run2 = 0.0;
      int64_t e_hit = -1, e_last = e0;
      for (int64_t e = e0; e < e_end; ++e) {
        const float v = p[e];
        if (v > 0.f) e_last = e;
        if (e_hit < 0) {
          run2 += (double)v;
          if (run2 > t2) e_hit = e;
        }
      }
      i = e_hit >= 0 ? e_hit : e_last;
    }
    got[k] = i;
    wraw[k] = pow((double)n * (double)p[i] / S, -beta);
    wmax = fmax(wmax, wraw[k]);
  }
  // max over the global batch (exact: the order of a max does not matter)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, o, 64));
  if ((tid & 63) == 0) red[tid >> 6] = wmax;
  __syncthreads();
  wmax = red[0];
#pragma unroll
  for (int k = 1; k < kSampleThreads / 64; ++k) wmax = fmax(wmax, red[k]);
#pragma unroll
  for (int k = 0; k < kMaxDrawsPerThread; ++k) {
    const int j = tid + k * kSampleThreads;
    if (j >= G) continue;
    idx_out[j] = got[k];
    w_out[j] = (float)(wraw[k] / wmax);
  }
}

// ---- per_update: thread j writes p[idx[j]] unless a later draw holds the same index -----------------------------------------
__global__ __launch_bounds__(256) void per_update_kernel(float* __restrict__ p, int64_t n, const int64_t* __restrict__ idx,
                                                         const float* __restrict__ err, int G, double alpha) {
  extern __shared__ int64_t ids[];  // [G]
  for (int k = threadIdx.x; k < G; k += blockDim.x) ids[k] = idx[k];
  __syncthreads();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= G) return;
  const int64_t i = ids[j];
  if (i < 0 || i >= n) return;
  for (int k = j + 1; k < G; ++k)
    if (ids[k] == i) return;
  p[i] = (float)pow((double)err[j] + kEps, alpha);
}

}  // namespace

extern "C" int64_t vdqn_per_workspace_bytes(int64_t n) {
  if (n <= 0 || n_chunks(n) > kMaxChunks) return -1;
  return align256(n_segs(n) * 8) + align256(n_chunks(n) * 8);
}

extern "C" int vdqn_per_sample(const float* prio, int64_t n, int32_t global_batch, uint64_t seed, uint64_t step, double beta,
                               void* workspace, int64_t* idx_out, float* weight_out, void* stream) {
  VDQN_CHECK(prio && workspace && idx_out && weight_out, "vdqn_per_sample: null arg");
  VDQN_CHECK(vdqn_per_workspace_bytes(n) > 0, "vdqn_per_sample: n = %lld outside [1, %lld]", (long long)n, (long long)(kMaxChunks * kChunk));
  VDQN_CHECK(global_batch >= 1 && global_batch <= kSampleThreads * kMaxDrawsPerThread, "vdqn_per_sample: global_batch %d outside [1, %d]",
             global_batch, kSampleThreads * kMaxDrawsPerThread);
  VDQN_CHECK(beta >= 0.0 && beta <= 1.0, "vdqn_per_sample: beta %g outside [0, 1]", beta);
  VDQN_CHECK((((uintptr_t)prio | (uintptr_t)workspace) & 15) == 0, "vdqn_per_sample: prio and workspace must be 16-byte aligned");
  double* seg = (double*)workspace;
  double* chunk = (double*)((char*)workspace + align256(n_segs(n) * 8));
  const int64_t nc = n_chunks(n);
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope ps_("per_blocksum", (double)n, (double)n * 4.0 + (double)(n_segs(n) + nc) * 8.0, st);
    hipLaunchKernelGGL(per_blocksum_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, st, prio, n, seg, chunk, nc);
    VDQN_LAUNCH_CHECK();
  }
  {
    ProfScope ps_("per_sample", 0.0, (double)nc * 8.0 + (double)global_batch * (kSegsPerChunk * 8.0 + kSeg * 4.0 + 12.0), st);
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kSampleThreads), (size_t)nc * 8, st, prio, n, (const double*)seg, (const double*)chunk,
                       (int)nc, (int)global_batch, seed, step, beta, idx_out, weight_out);
    VDQN_LAUNCH_CHECK();
  }
  return VDQN_OK;
}

extern "C" int vdqn_per_update(float* prio, int64_t n, const int64_t* idx, const float* err, int32_t global_batch, double alpha,
                               void* stream) {
  VDQN_CHECK(prio && idx && err, "vdqn_per_update: null arg");
  VDQN_CHECK(n >= 1, "vdqn_per_update: n = %lld", (long long)n);
  VDQN_CHECK(global_batch >= 1 && global_batch <= kSampleThreads * kMaxDrawsPerThread, "vdqn_per_update: global_batch %d outside [1, %d]",
             global_batch, kSampleThreads * kMaxDrawsPerThread);
  VDQN_CHECK(alpha >= 0.0, "vdqn_per_update: alpha %g < 0", alpha);
  ProfScope ps_("per_update", 0.0, (double)global_batch * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(per_update_kernel, dim3((global_batch + 255) / 256), dim3(256), (size_t)global_batch * 8, (hipStream_t)stream, prio, n, idx,
                     err, (int)global_batch, alpha);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
