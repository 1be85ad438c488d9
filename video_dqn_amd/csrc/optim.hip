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

// The two multiplies AdamW and the clipping add in front of Adam's arithmetic, each rounded on its own: never contracted into the
// adds that follow, so a unit factor leaves every bit of the plain update as it is.
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// m = beta1 * m + omb1 * g of the scalar tail loops below, with the one fused multiply-add written out as adam_kernel's tail has it:
// fma(beta1, m, round(omb1 * g)).  Left to the compiler, the tail here contracted the other product (fma(omb1, g, round(beta1 * m))),
// and the up to three tail elements of a range then missed the plain kernel's bits at unit factors.
// What this pins is this file's side only.  adam_kernel (pointwise.hip) still leaves both of its loops to the compiler, and the float4
// bodies of adam_scaled_kernel and adam_polyak_kernel match its body because the compiler contracts the same expression the same
// way in all three: a toolchain that decides otherwise breaks the "vdqn_adam's bits" equality again, and tests/test_gpu_polyak.py
// (every size with a tail, moments that are not zero) is what notices.  Writing the fma out in adam_kernel too would settle it, at
// the price of that kernel's ISA.
__device__ __forceinline__ float tail_moment(float beta1, float m, float omb1, float g) {
  return __builtin_fmaf(beta1, m, mul_rounded(omb1, g));
}

// adam_kernel (pointwise.hip) with gs = g * coef in place of g and p * decay in place of p; the three expressions are that kernel's.
// A kernel of its own rather than a flag on adam_kernel, which keeps the ISA it has: coef = 1
// and decay = 1 give the plain kernel's bits.
__global__ __launch_bounds__(256) void adam_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, float step_size, float beta1, float beta2,
                                                          float omb1, float omb2, float inv_sqrt_bc2, float eps, float decay,
                                                          const float* __restrict__ coef_ptr) {
  const float coef = coef_ptr ? coef_ptr[0] : 1.0f;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
#define VDQN_ADAM1(c)                                              \
  gg.c = mul_rounded(gg.c, coef);                        \
  pp.c = mul_rounded(pp.c, decay);                       \
  mm.c = beta1 * mm.c + omb1 * gg.c;                     \
  vv.c = beta2 * vv.c + omb2 * gg.c * gg.c;              \
  pp.c = pp.c - step_size * (mm.c / (sqrtf(vv.c) * inv_sqrt_bc2 + eps));
    VDQN_ADAM1(x) VDQN_ADAM1(y) VDQN_ADAM1(z) VDQN_ADAM1(w)
#undef VDQN_ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = mul_rounded(g[i], coef);
    const float mm = tail_moment(beta1, m[i], omb1, gg);
    const float vv = beta2 * v[i] + omb2 * gg * gg;
    m[i] = mm;
    v[i] = vv;
    p[i] = mul_rounded(p[i], decay) - step_size * (mm / (sqrtf(vv) * inv_sqrt_bc2 + eps));
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

// adam_scaled_kernel, then the new p — still in registers — lerped into the target copy: one more read and one more write of `t`
// per element instead of a second launch that streams p again.  The p, m, v expressions are adam_scaled_kernel's, token for token.
__global__ __launch_bounds__(256) void adam_polyak_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, long n, float step_size, float beta1, float beta2,
                                                          float omb1, float omb2, float inv_sqrt_bc2, float eps, float decay,
                                                          const float* __restrict__ coef_ptr, float* __restrict__ t, float tau_f,
                                                          float omt_f, int lo) {
  const float coef = coef_ptr ? coef_ptr[0] : 1.0f;
  const long n4 = n >> 2;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 tt = reinterpret_cast<float4*>(t)[i];
#define VDQN_ADAM1(c)                                              \
  gg.c = mul_rounded(gg.c, coef);                        \
  pp.c = mul_rounded(pp.c, decay);                       \
  mm.c = beta1 * mm.c + omb1 * gg.c;                     \
  vv.c = beta2 * vv.c + omb2 * gg.c * gg.c;              \
  pp.c = pp.c - step_size * (mm.c / (sqrtf(vv.c) * inv_sqrt_bc2 + eps)); \
  tt.c = lerp_rounded(tt.c, pp.c, tau_f, omt_f, lo);
    VDQN_ADAM1(x) VDQN_ADAM1(y) VDQN_ADAM1(z) VDQN_ADAM1(w)
#undef VDQN_ADAM1
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(t)[i] = tt;
  }
  for (long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gg = mul_rounded(g[i], coef);
    const float mm = tail_moment(beta1, m[i], omb1, gg);
    const float vv = beta2 * v[i] + omb2 * gg * gg;
    m[i] = mm;
    v[i] = vv;
    const float pp = mul_rounded(p[i], decay) - step_size * (mm / (sqrtf(vv) * inv_sqrt_bc2 + eps));
    p[i] = pp;
    t[i] = lerp_rounded(t[i], pp, tau_f, omt_f, lo);
  }
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

extern "C" int vdqn_adam_scaled(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2,
                                double eps, double weight_decay, const float* coef, void* stream) {
  VDQN_CHECK(p && g && m && v && n > 0 && step >= 1, "vdqn_adam_scaled: bad args");
  VDQN_CHECK((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0, "vdqn_adam_scaled: pointers must be 16-byte aligned");
  VDQN_CHECK(weight_decay >= 0.0 && isfinite(weight_decay), "vdqn_adam_scaled: weight_decay must be finite and >= 0");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const float decay = (float)(1.0 - lr * weight_decay);
  int64_t grid = ((n / 4 + 1) + 255) / 256;  // vdqn_adam's grid
  if (grid > 4096) grid = 4096;
  ProfScope ps_("adam_scaled", 0.0, (double)n * 28.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_scaled_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, step_size, (float)beta1,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), inv_sqrt_bc2, (float)eps, decay, coef);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

namespace {

// tau in (0, 1] and finite, written so that a NaN fails
inline bool tau_ok(double tau) { return isfinite(tau) && tau > 0.0 && tau <= 1.0; }

// [a, a + n) and [b, b + n) floats share no element (the kernels declare both __restrict__)
inline bool disjoint(const float* a, const float* b, int64_t n) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
  return x + bytes <= y || y + bytes <= x;
}

}  // namespace

extern "C" int vdqn_polyak(float* target, const float* p, int64_t n, double tau, void* stream) {
  VDQN_CHECK(target && p, "vdqn_polyak: null pointer");
  VDQN_CHECK(n >= 1, "vdqn_polyak: n must be >= 1");
  VDQN_CHECK((((uintptr_t)target | (uintptr_t)p) & 15) == 0, "vdqn_polyak: pointers must be 16-byte aligned");
  VDQN_CHECK(tau_ok(tau), "vdqn_polyak: tau must be finite and in (0, 1]");
  VDQN_CHECK(disjoint(target, p, n), "vdqn_polyak: target and p must not overlap");
  int64_t grid = ((n / 4 + 1) + 255) / 256;
  if (grid > 4096) grid = 4096;
  ProfScope ps_("polyak", 0.0, (double)n * 12.0, (hipStream_t)stream);
  hipLaunchKernelGGL(polyak_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, target, p, (long)n, (float)tau, (float)(1.0 - tau),
                     (int)(tau < 0.5));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_adam_polyak(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1, double beta2,
                                double eps, double weight_decay, const float* coef, float* target, double tau, void* stream) {
  VDQN_CHECK(p && g && m && v && target, "vdqn_adam_polyak: null pointer");
  VDQN_CHECK(n >= 1 && step >= 1, "vdqn_adam_polyak: n and step must be >= 1");
  VDQN_CHECK((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)target) & 15) == 0,
             "vdqn_adam_polyak: pointers must be 16-byte aligned");
  VDQN_CHECK((((uintptr_t)coef) & 3) == 0, "vdqn_adam_polyak: coef must be 4-byte aligned");
  VDQN_CHECK(weight_decay >= 0.0 && isfinite(weight_decay), "vdqn_adam_polyak: weight_decay must be finite and >= 0");
  VDQN_CHECK(tau_ok(tau), "vdqn_adam_polyak: tau must be finite and in (0, 1]");
  VDQN_CHECK(disjoint(target, p, n) && disjoint(target, g, n) && disjoint(target, m, n) && disjoint(target, v, n),
             "vdqn_adam_polyak: target must not overlap p, g, m or v");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  const float decay = (float)(1.0 - lr * weight_decay);
  int64_t grid = ((n / 4 + 1) + 255) / 256;  // vdqn_adam's grid
  if (grid > 4096) grid = 4096;
  ProfScope ps_("adam_polyak", 0.0, (double)n * 36.0, (hipStream_t)stream);
  hipLaunchKernelGGL(adam_polyak_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, step_size, (float)beta1,
                     (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), inv_sqrt_bc2, (float)eps, decay, coef, target, (float)tau,
                     (float)(1.0 - tau), (int)(tau < 0.5));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
