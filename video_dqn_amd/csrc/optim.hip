// Optimiser controls of the Q trainer on the device: global gradient-norm clipping (torch.nn.utils.clip_grad_norm_) and the
// AdamW update (torch.optim.AdamW) over the flat f32 master range.  No host round trip: the clip coefficient travels from the
// norm kernels to the Adam launch through device memory.
//
// The norm is an f64 sum of squares in a FIXED order, so it is bit-identical run to run, in every mode and on every rank
// (tests/test_gpu_optim.py restates it in numpy from the workspace):
//
//   workspace = kClipMaxSlots slots of kClipSlotDoubles doubles: slot s = { int64 count, double part[kClipMaxParts] }
//   vdqn_grad_sumsq(x, n, workspace, s): nb = clip_blocks(n) = min(kClipMaxParts, ceil(n / 4096)) blocks of 256 threads, count = nb.
//     head = the (0..3) elements in front of the first 16-byte boundary, tail = the (0..3) behind the last whole float4; thread t of
//     block 0 starts from x[t]^2 (t < head) plus tail[t]^2 (t < tail), every other thread from 0.  Thread t of block b then adds, for
//     i = b * 256 + t, i + nb * 256, ... < n4, the squares of body float4 i as (((acc + x^2) + y^2) + z^2) + w^2  (a square of an f32
//     is exact in f64).  Lanes are folded by shuffles at distances 32, 16, .. 1 (lane l += lane l + d), the four waves left to
//     right: part[b] = ((w0 + w1) + w2) + w3.
//   vdqn_clip_finalize(workspace, S, max_norm, out): sum = (((0 + part_0[0]) + part_0[1]) + ...) over slot 0, then slot 1, .. S-1;
//     norm = sqrt(sum), coef = max_norm / (norm + 1e-6) capped at 1 (a NaN stays a NaN, as in torch), both f64, each rounded once:
//     out = { (float)norm, (float)coef }.
#include <math.h>

#include "common.h"

namespace {

constexpr int kClipMaxSlots = 8;
constexpr int kClipMaxParts = 512;
constexpr int kClipSlotDoubles = 1 + kClipMaxParts;
constexpr int64_t kClipElemsPerBlock = 4096;

inline int clip_blocks(int64_t n) {
  int64_t b = (n + kClipElemsPerBlock - 1) / kClipElemsPerBlock;
  if (b > kClipMaxParts) b = kClipMaxParts;
  if (b < 1) b = 1;
  return (int)b;
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ x, long n, int head, double* __restrict__ slot) {
  const long n4 = (n - head) >> 2;
  const int tail = (int)(n - head - (n4 << 2));
  const float4* __restrict__ body = reinterpret_cast<const float4*>(x + head);
  double acc = 0.0;
  if (blockIdx.x == 0) {
    if ((int)threadIdx.x < head) acc = sq(x[threadIdx.x]);
    if ((int)threadIdx.x < tail) acc += sq(x[head + (n4 << 2) + threadIdx.x]);
  }
  const long stride = (long)gridDim.x * blockDim.x;
#pragma unroll 4
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const float4 v = body[i];
    acc += sq(v.x);
    acc += sq(v.y);
    acc += sq(v.z);
    acc += sq(v.w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    slot[1 + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    if (blockIdx.x == 0) reinterpret_cast<long*>(slot)[0] = (long)gridDim.x;
  }
}

__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ ws, int n_slots, double max_norm, float* __restrict__ out) {
  __shared__ double part[kClipMaxSlots * kClipMaxParts];
  __shared__ int first[kClipMaxSlots + 1];
  if (threadIdx.x == 0) {
    int pos = 0;
    for (int s = 0; s < n_slots; ++s) {
      first[s] = pos;
      long c = reinterpret_cast<const long*>(ws + (long)s * kClipSlotDoubles)[0];
      pos += c < 0 ? 0 : (c > kClipMaxParts ? kClipMaxParts : (int)c);  // (a workspace that was never written must not index past a slot)
    }
    first[n_slots] = pos;
  }
  __syncthreads();
  for (int s = 0; s < n_slots; ++s) {
    const int c = first[s + 1] - first[s];
    for (int i = threadIdx.x; i < c; i += blockDim.x) part[first[s] + i] = ws[(long)s * kClipSlotDoubles + 1 + i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = first[n_slots];
    double sum = 0.0;
    int i = 0;
    for (; i + 8 <= total; i += 8) {  // eight LDS reads in flight, the adds still one after the other in index order
      double t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = part[i + j];
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += t[j];
    }
    for (; i < total; ++i) sum += part[i];
    const double norm = sqrt(sum);
    const double c = max_norm / (norm + 1e-6);
    out[0] = (float)norm;
    out[1] = (float)(c > 1.0 ? 1.0 : c);
  }
}

// Soft (Polyak) target update of one element, theta- <- theta- + tau (theta - theta-), as torch.lerp's two-branch rule with every
// product rounded on its own (include/vdqn.h writes it out; tests/polyak_oracle.py restates it in numpy float32):
//   d = p - t;   tau < 0.5: t + tau_f * d;   otherwise: p - d * omt_f      (tau_f = (float)tau, omt_f = (float)(1.0 - tau))
// `lo` is tau < 0.5, decided on the host.  tau = 1 (omt_f = 0) returns p's bits, p == t (d = 0) returns t's.
__device__ __forceinline__ float lerp_rounded(float t, float p, float tau_f, float omt_f, bool lo) {
#pragma clang fp contract(off)
  const float d = p - t;
  const float a = tau_f * d;
  const float b = d * omt_f;
  return lo ? t + a : p - b;
}

// 256 threads, one float4 per thread and pass, 4096 blocks at the most (n / 4 + 1: a range shorter than 4 still gets its tail's block)
inline int flat_grid(int64_t n) {
  const int64_t b = ((n / 4 + 1) + 255) / 256;
  return (int)(b > 4096 ? 4096 : b);
}

__global__ __launch_bounds__(256) void polyak_kernel(float* __restrict__ t, const float* __restrict__ p, long n, float tau_f, float omt_f,
                                                     int lo) {
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 tt = reinterpret_cast<float4*>(t)[i];
    const float4 pp = reinterpret_cast<const float4*>(p)[i];
    tt.x = lerp_rounded(tt.x, pp.x, tau_f, omt_f, lo);
    tt.y = lerp_rounded(tt.y, pp.y, tau_f, omt_f, lo);
    tt.z = lerp_rounded(tt.z, pp.z, tau_f, omt_f, lo);
    tt.w = lerp_rounded(tt.w, pp.w, tau_f, omt_f, lo);
    reinterpret_cast<float4*>(t)[i] = tt;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) t[i] = lerp_rounded(t[i], p[i], tau_f, omt_f, lo);
}

// The Adam update of one element (torch.optim.Adam / AdamW; train_q_network.py:124,227), the only statement of it.  Contraction is
// off and every fused multiply-add is written out, so each fma below rounds once and every other product, sum and quotient rounds
// on its own, whichever loop, instance or compiler evaluates it:
//   SCALED:  g = g * coef;   p = p * decay                                  (coef = coef_ptr[0] or 1, decay = 1 - lr * weight_decay)
//   m = fma(omb1, g, beta1 * m)                v = fma(omb2 * g, g, beta2 * v)                          (omb = 1 - beta)
//   p = fma(-step_size, m / fma(sqrtf(v), inv_sqrt_bc2, eps), p)            (step_size = lr / bc1, inv_sqrt_bc2 = 1 / sqrt(bc2))
//   POLYAK:  t = lerp_rounded(t, p)            (the new p, still in registers: one more read and write of t, no second launch)
// A unit coef and decay multiply exactly, so the SCALED instances then write the plain one's bits.
struct adam_consts {
  float step_size, beta1, beta2, omb1, omb2, inv_sqrt_bc2, eps, decay, tau_f, omt_f;
  int lo;
};
template <bool SCALED, bool POLYAK>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float& t, float coef, const adam_consts& k) {
#pragma clang fp contract(off)
  if constexpr (SCALED) {
    g = g * coef;
    p = p * k.decay;
  }
  m = __builtin_fmaf(k.omb1, g, k.beta1 * m);
  v = __builtin_fmaf(k.omb2 * g, g, k.beta2 * v);
  p = __builtin_fmaf(-k.step_size, m / __builtin_fmaf(sqrtf(v), k.inv_sqrt_bc2, k.eps), p);
  if constexpr (POLYAK) t = lerp_rounded(t, p, k.tau_f, k.omt_f, k.lo);
}

// Three instances: plain (vdqn_adam), SCALED (vdqn_adam_scaled), SCALED + POLYAK (vdqn_adam_polyak).  Compile-time flags: a run-time
// one would put the target's loads and registers into every instance.  `t` and `coef_ptr` are read only by the instances that use them.
template <bool SCALED, bool POLYAK>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* __restrict__ t, const float* __restrict__ coef_ptr, long n,
                                                   const adam_consts k) {
  float coef = 1.0f;
  if constexpr (SCALED) coef = coef_ptr ? coef_ptr[0] : 1.0f;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 tt = {};
    if constexpr (POLYAK) tt = reinterpret_cast<float4*>(t)[i];
    adam_element<SCALED, POLYAK>(pp.x, gg.x, mm.x, vv.x, tt.x, coef, k);
    adam_element<SCALED, POLYAK>(pp.y, gg.y, mm.y, vv.y, tt.y, coef, k);
    adam_element<SCALED, POLYAK>(pp.z, gg.z, mm.z, vv.z, tt.z, coef, k);
    adam_element<SCALED, POLYAK>(pp.w, gg.w, mm.w, vv.w, tt.w, coef, k);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (POLYAK) reinterpret_cast<float4*>(t)[i] = tt;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float pp = p[i], mm = m[i], vv = v[i], tt = 0.f;
    if constexpr (POLYAK) tt = t[i];
    adam_element<SCALED, POLYAK>(pp, g[i], mm, vv, tt, coef, k);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
    if constexpr (POLYAK) t[i] = tt;
  }
}

// tau in (0, 1] and finite, written so that a NaN fails
inline bool tau_ok(double tau) { return isfinite(tau) && tau > 0.0 && tau <= 1.0; }

// [a, a + n) and [b, b + n) floats share no element (the kernels declare both __restrict__)
inline bool disjoint(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x + bytes <= y || y + bytes <= x;
}

}  // namespace

extern "C" int64_t vdqn_clip_workspace_bytes(int32_t n_ranges) {
  if (n_ranges < 1 || n_ranges > kClipMaxSlots) return -1;
  return (int64_t)n_ranges * kClipSlotDoubles * (int64_t)sizeof(double);
}

extern "C" int vdqn_grad_sumsq(const float* g, int64_t n, void* workspace, int32_t slot, void* stream) {
  VDQN_CHECK(g && workspace && n >= 1, "vdqn_grad_sumsq: bad args");
  VDQN_CHECK(slot >= 0 && slot < kClipMaxSlots, "vdqn_grad_sumsq: slot %d (0..%d)", slot, kClipMaxSlots - 1);
  VDQN_CHECK((((uintptr_t)g) & 3) == 0 && (((uintptr_t)workspace) & 7) == 0, "vdqn_grad_sumsq: g must be 4-byte, workspace 8-byte aligned");
  int64_t head = (int64_t)(((16 - (((uintptr_t)g) & 15)) & 15) >> 2);
  if (head > n) head = n;
  ProfScope ps_("grad_sumsq", 0.0, (double)n * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(clip_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, (long)n, (int)head,
                     (double*)workspace + (int64_t)slot * kClipSlotDoubles);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_clip_finalize(const void* workspace, int32_t n_ranges, double max_norm, float* out, void* stream) {
  VDQN_CHECK(workspace && out, "vdqn_clip_finalize: null arg");
  VDQN_CHECK(n_ranges >= 1 && n_ranges <= kClipMaxSlots, "vdqn_clip_finalize: n_ranges %d (1..%d)", n_ranges, kClipMaxSlots);
  VDQN_CHECK(max_norm > 0.0, "vdqn_clip_finalize: max_norm must be > 0");
  VDQN_CHECK((((uintptr_t)workspace) & 7) == 0 && (((uintptr_t)out) & 3) == 0, "vdqn_clip_finalize: workspace must be 8-byte, out 4-byte aligned");
  ProfScope ps_("clip_finalize", 0.0, (double)n_ranges * kClipSlotDoubles * 8.0, (hipStream_t)stream);
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, (int)n_ranges, max_norm, out);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_polyak(float* target, const float* p, int64_t n, double tau, void* stream) {
  VDQN_CHECK(target && p, "vdqn_polyak: null pointer");
  VDQN_CHECK(n >= 1, "vdqn_polyak: n must be >= 1");
  VDQN_CHECK((((uintptr_t)target | (uintptr_t)p) & 15) == 0, "vdqn_polyak: pointers must be 16-byte aligned");
  VDQN_CHECK(tau_ok(tau), "vdqn_polyak: tau must be finite and in (0, 1]");
  VDQN_CHECK(disjoint(target, p, n), "vdqn_polyak: target and p must not overlap");
  ProfScope ps_("polyak", 0.0, (double)n * 12.0, (hipStream_t)stream);
  hipLaunchKernelGGL(polyak_kernel, dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, target, p, (long)n, (float)tau, (float)(1.0 - tau),
                     (int)(tau < 0.5));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// The three Adam entries: every check (each fails by the entry's name before any HIP call), the host constants, then the one launch.
// Plain entries pass weight_decay 0 and coef NULL; only the POLYAK entry has a target and a tau.
template <bool SCALED, bool POLYAK>
static int adam_launch(const char* entry, const char* prof_name, float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr,
                       double beta1, double beta2, double eps, double weight_decay, const float* coef, float* target, double tau, void* stream) {
  VDQN_CHECK(p && g && m && v && (!POLYAK || target), "%s: null pointer", entry);
  VDQN_CHECK(n >= 1 && step >= 1, "%s: n and step must be >= 1", entry);
  VDQN_CHECK((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)target) & 15) == 0, "%s: pointers must be 16-byte aligned", entry);
  VDQN_CHECK((((uintptr_t)coef) & 3) == 0, "%s: coef must be 4-byte aligned", entry);
  VDQN_CHECK(weight_decay >= 0.0 && isfinite(weight_decay), "%s: weight_decay must be finite and >= 0", entry);
  if (POLYAK) {
    VDQN_CHECK(tau_ok(tau), "%s: tau must be finite and in (0, 1]", entry);
    VDQN_CHECK(disjoint(target, p, n) && disjoint(target, g, n) && disjoint(target, m, n) && disjoint(target, v, n),
               "%s: target must not overlap p, g, m or v", entry);
  }
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  adam_consts k;
  k.step_size = (float)(lr / bc1);
  k.beta1 = (float)beta1;
  k.beta2 = (float)beta2;
  k.omb1 = (float)(1.0 - beta1);
  k.omb2 = (float)(1.0 - beta2);
  k.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  k.eps = (float)eps;
  k.decay = (float)(1.0 - lr * weight_decay);
  k.tau_f = (float)tau;
  k.omt_f = (float)(1.0 - tau);
  k.lo = (int)(tau < 0.5);
  ProfScope ps_(prof_name, 0.0, (double)n * (POLYAK ? 36.0 : 28.0), (hipStream_t)stream);
  hipLaunchKernelGGL((adam_kernel<SCALED, POLYAK>), dim3(flat_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, target, coef, (long)n, k);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_adam(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2, double eps,
                         void* stream) {
  return adam_launch<false, false>("vdqn_adam", "adam", p, g, m, v, n, step, lr, beta1, beta2, eps, 0.0, nullptr, nullptr, 1.0, stream);
}

extern "C" int vdqn_adam_scaled(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2,
                                double eps, double weight_decay, const float* coef, void* stream) {
  return adam_launch<true, false>("vdqn_adam_scaled", "adam_scaled", p, g, m, v, n, step, lr, beta1, beta2, eps, weight_decay, coef, nullptr, 1.0,
                                  stream);
}

extern "C" int vdqn_adam_polyak(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2,
                                double eps, double weight_decay, const float* coef, float* target, double tau, void* stream) {
  return adam_launch<true, true>("vdqn_adam_polyak", "adam_polyak", p, g, m, v, n, step, lr, beta1, beta2, eps, weight_decay, coef, target, tau,
                                 stream);
}
