// Attribution on the engine: perturbed copies of frames packed straight into the stem operand (integrated gradients' path points,
// SmoothGrad's noisy copies), the weighted sum of the per-copy frame gradients, and the two read-outs.  Three HBM-bound kernels;
// include/vdqn.h states the arithmetic, tests/attrib_oracle.py restates it in numpy float32.
//
// Rounding: every function below that states arithmetic compiles with contraction off, so each product and each sum written
// there rounds on its own, whichever loop or instance evaluates it.
//
//   x    the normalised f32 value of a pixel: the float source's, or pack_norm_entry<float> of a uint8 source's byte (pack_common.h:
//        the expression vdqn_pack_input normalises with)
//   b    base_const[c], or the same reading of the baseline image
//   path:   x_s = b + coef[s] * (x - b)
//   noise:  x_s = x + sigma[c] * z,  z = (float)(h0 + h1 + h2 + h3 - 131070) * kZ
//           h   = splitmix64(splitmix64(splitmix64(seed ^ "ATTRIB01") ^ (copy << 32 | image)) ^ element)
// The four 16-bit fields of h are uniform on 0 .. 65535: their sum has mean 131070 and variance 4 (2^32 - 1) / 12, so z has mean 0
// and variance 1 up to kZ's rounding, and |z| <= 131070 kZ = 3.46405.  The integer sum is below 2^24: its conversion is exact, and
// the one product is z's only rounding.
#include <math.h>

#include "engine_net.h"  // vdqn_stem_pixel_scale
#include "pack_common.h"

namespace {

constexpr uint64_t kAttribStream = 0x4154545249423031ull;  // "ATTRIB01"
constexpr float kZ = 0x1.bb67aep-16f;                       // (float)(1 / sqrt((2^32 - 1) / 3))
constexpr int kImgElems = 3 * 224 * 224;

__device__ __forceinline__ float noise_z(uint64_t key_ci, uint32_t e) {
#pragma clang fp contract(off)
  const uint64_t h = splitmix64(key_ci ^ (uint64_t)e);
  const int sum = (int)(h & 0xFFFFu) + (int)((h >> 16) & 0xFFFFu) + (int)((h >> 32) & 0xFFFFu) + (int)(h >> 48);
  return (float)(sum - 131070) * kZ;
}
__device__ __forceinline__ float path_point(float x, float b, float coef) {
#pragma clang fp contract(off)
  const float d = x - b;
  const float t = coef * d;
  return b + t;
}
__device__ __forceinline__ float noise_point(float x, float sigma, float z) {
#pragma clang fp contract(off)
  const float t = sigma * z;
  return x + t;
}

struct Source {
  const void* src;
  const void* baseline;
  int src_kind;
  float base_const[3];
};
// x and b of element (c, Y, X) of image i; lut: the 3 x 256 normalisation table of a uint8 source (LDS)
__device__ __forceinline__ void read_xb(const Source& s, const float (*lut)[256], int i, int c, int Y, int X, float& x, float& b) {
  b = s.base_const[c];
  if (s.src_kind == 0) {
    const size_t at = (((size_t)i * 224 + Y) * 224 + X) * 3 + c;
    x = lut[c][((const uint8_t*)s.src)[at]];
    if (s.baseline) b = lut[c][((const uint8_t*)s.baseline)[at]];
  } else {
    const size_t at = (((size_t)i * 3 + c) * 224 + Y) * 224 + X;
    x = ((const float*)s.src)[at];
    if (s.baseline) b = ((const float*)s.baseline)[at];
  }
}
__device__ __forceinline__ void fill_lut(float (*lut)[256], int src_kind) {
  if (src_kind != 0) return;  // (uniform over the grid)
  for (int t = threadIdx.x; t < 3 * 256; t += blockDim.x) lut[t >> 8][t & 255] = pack_norm_entry<float>(t & 255, t >> 8);
  __syncthreads();
}

// One thread per packed pixel of one copy: blockIdx.y = copy s, the x dimension walks the n_base * 115 * 115 packed pixels of the
// base images.  16 elements = 32 / 64 contiguous bytes per thread as 16-byte stores (pack_store16), consecutive threads consecutive
// pixels; the source of the other copies comes out of L2.
template <typename T>
__global__ __launch_bounds__(256) void attrib_pack_kernel(Source s, const float* __restrict__ coef, int mode, float sg0, float sg1, float sg2,
                                                          uint64_t key, int s0, int i0, int n_base, T* __restrict__ dst) {
  __shared__ float lut[3][256];
  fill_lut(lut, s.src_kind);
  const int cp = blockIdx.y;
  const int total = n_base * 115 * 115;
  const float cf = mode == 0 ? coef[cp] : 0.f;
  const float sigma[3] = {sg0, sg1, sg2};
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
    const int i = p / (115 * 115);
    const int rem = p - i * (115 * 115);
    const int y = rem / 115, x = rem - y * 115;
    const int ys = y - 2, xs = x - 2;
    __attribute__((aligned(16))) T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
    if ((unsigned)ys < 112u && (unsigned)xs < 112u) {
      const uint64_t key_ci = splitmix64(key ^ (((uint64_t)(uint32_t)(s0 + cp) << 32) | (uint64_t)(uint32_t)(i0 + i)));
#pragma unroll
      for (int bh = 0; bh < 2; ++bh)
#pragma unroll
        for (int bw = 0; bw < 2; ++bw) {
          const int Y = 2 * ys + bh, X = 2 * xs + bw;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float xv, bv;
            read_xb(s, lut, i, c, Y, X, xv, bv);
            const float r = mode == 0 ? path_point(xv, bv, cf) : noise_point(xv, sigma[c], noise_z(key_ci, (uint32_t)((c * 224 + Y) * 224 + X)));
            v[(bh * 2 + bw) * 3 + c] = from_f32<T>(r);
          }
        }
    }
    pack_store16(dst + ((size_t)cp * total + p) * 16, v);
  }
}

__device__ __forceinline__ float reduce_step(float run, float w, float g, int squared) {
#pragma clang fp contract(off)
  float t = w * g;
  if (squared) t = t * g;
  return run + t;
}
// one float4 of acc per thread and pass; the copies' float4s are n4 apart
__global__ __launch_bounds__(256) void attrib_reduce_kernel(const float4* __restrict__ g, const float* __restrict__ w, float4* __restrict__ acc,
                                                            long n4, int n_copies, int squared, int accumulate) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 r = accumulate ? acc[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = 0; s < n_copies; ++s) {
      const float4 v = g[(long)s * n4 + i];
      const float ws = w[s];
      r.x = reduce_step(r.x, ws, v.x, squared);
      r.y = reduce_step(r.y, ws, v.y, squared);
      r.z = reduce_step(r.z, ws, v.z, squared);
      r.w = reduce_step(r.w, ws, v.w, squared);
    }
    acc[i] = r;
  }
}

__device__ __forceinline__ float finish_product(float a, float x, float b, float scale, int scaled) {
#pragma clang fp contract(off)
  const float d = x - b;
  float r = a * d;
  if (scaled) r = r * scale;
  return r;
}
// mode 0: four consecutive X of one (image, channel, row) per thread and pass
__global__ __launch_bounds__(256) void attrib_finish_ig_kernel(const float4* __restrict__ acc, Source s, float sc0, float sc1, float sc2, int scaled,
                                                               long n4, float4* __restrict__ out) {
  __shared__ float lut[3][256];
  fill_lut(lut, s.src_kind);
  const float scale[3] = {sc0, sc1, sc2};
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
    const int X = (int)(q % 56) * 4;
    long t = q / 56;
    const int Y = (int)(t % 224);
    t /= 224;
    const int c = (int)(t % 3), i = (int)(t / 3);
    const float4 a = acc[q];
    const float av[4] = {a.x, a.y, a.z, a.w};
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float xv, bv;
      read_xb(s, lut, i, c, Y, X + k, xv, bv);
      r[k] = finish_product(av[k], xv, bv, scale[c], scaled);
    }
    out[q] = make_float4(r[0], r[1], r[2], r[3]);
  }
}
// the larger of m and |v|; a NaN stays one (torch.amax)
__device__ __forceinline__ float absmax(float m, float v) {
  const float a = fabsf(v);
  return (a > m || a != a) ? a : m;
}
// mode 1: one float4 of the [n][224][224] map per thread and pass
__global__ __launch_bounds__(256) void attrib_finish_max_kernel(const float4* __restrict__ acc, long n4, float4* __restrict__ out) {
  constexpr long kPlane4 = 224 * 224 / 4;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < n4; q += stride) {
    const long i = q / kPlane4, r = q - i * kPlane4;
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float4 v = acc[(i * 3 + c) * kPlane4 + r];
      m.x = absmax(m.x, v.x);
      m.y = absmax(m.y, v.y);
      m.z = absmax(m.z, v.z);
      m.w = absmax(m.w, v.w);
    }
    out[q] = m;
  }
}

// 256 threads, one 16-byte vector (or packed pixel) per thread and pass, 8 blocks per CU at the most
int flat_grid(long items) {
  const long b = (items + 255) / 256, cap = 8l * vdqn_num_cus();
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// what vdqn_attrib_pack and vdqn_attrib_finish (mode 0) both ask of the source; fills `s`
int check_source(const char* who, const void* src, int src_kind, const void* baseline, const float* base_const, int n_base, Source* s) {
  VDQN_CHECK(src, "%s: src is NULL", who);
  VDQN_CHECK(src_kind == 0 || src_kind == 1, "%s: src_kind %d (0: uint8 NHWC, 1: f32 NCHW)", who, src_kind);
  VDQN_CHECK(n_base >= 1, "%s: n_base %d must be >= 1", who, n_base);
  VDQN_CHECK(((uintptr_t)src & 15) == 0 && ((uintptr_t)baseline & 15) == 0, "%s: src and baseline must be 16-byte aligned", who);
  s->src = src; s->baseline = baseline; s->src_kind = src_kind;
  for (int c = 0; c < 3; ++c) {
    s->base_const[c] = base_const && !baseline ? base_const[c] : 0.f;
    VDQN_CHECK(isfinite(s->base_const[c]), "%s: base_const[%d] is not finite", who, c);
  }
  return VDQN_OK;
}

}  // namespace

extern "C" int vdqn_attrib_pack(const void* src, int32_t src_kind, const void* baseline, const float* base_const, int32_t n_base, int32_t n_copies,
                                int32_t mode, const float* coef, const float* sigma, uint64_t seed, int32_t s0, int32_t i0, void* dst, int32_t dtype,
                                void* stream) {
  VDQN_CHECK(dst, "vdqn_attrib_pack: dst is NULL");
  Source s;
  RC(check_source("vdqn_attrib_pack", src, src_kind, baseline, base_const, n_base, &s));
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_attrib_pack: bad dtype %d (the storage type: VDQN_F32 or VDQN_BF16)", dtype);
  VDQN_CHECK(((uintptr_t)dst & 15) == 0, "vdqn_attrib_pack: dst must be 16-byte aligned");
  VDQN_CHECK(mode == 0 || mode == 1, "vdqn_attrib_pack: mode %d (0: path, 1: noise)", mode);
  VDQN_CHECK(n_copies >= 1 && n_copies <= 65535, "vdqn_attrib_pack: n_copies %d must be in [1, 65535]", n_copies);
  VDQN_CHECK((int64_t)n_copies * n_base * 115 * 115 < (1ll << 31), "vdqn_attrib_pack: %d copies of %d images reach 2^31 packed pixels (split the copies)",
             n_copies, n_base);
  float sg[3] = {0.f, 0.f, 0.f};
  if (mode == 0) {
    VDQN_CHECK(coef, "vdqn_attrib_pack: mode 0 (path) needs coef");
    VDQN_CHECK(((uintptr_t)coef & 3) == 0, "vdqn_attrib_pack: coef must be 4-byte aligned");
  } else {
    VDQN_CHECK(sigma, "vdqn_attrib_pack: mode 1 (noise) needs sigma");
    VDQN_CHECK(s0 >= 0 && i0 >= 0, "vdqn_attrib_pack: s0 %d and i0 %d must be >= 0", s0, i0);
    VDQN_CHECK((int64_t)s0 + n_copies < (1ll << 31) && (int64_t)i0 + n_base < (1ll << 31), "vdqn_attrib_pack: s0 + n_copies or i0 + n_base reaches 2^31");
    for (int c = 0; c < 3; ++c) {
      sg[c] = sigma[c];
      VDQN_CHECK(isfinite(sg[c]) && sg[c] >= 0.f, "vdqn_attrib_pack: sigma[%d] = %g must be finite and >= 0", c, (double)sg[c]);
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const long pixels = (long)n_base * 115 * 115;
  const int esz = dtype == VDQN_BF16 ? 2 : 4;
  ProfScope ps_("attrib_pack", 0.0, (double)n_base * kImgElems * (src_kind == 0 ? 1 : 4) * (baseline ? 2 : 1) + (double)n_copies * pixels * 16 * esz, st);
  const dim3 grid(flat_grid(pixels), n_copies);
  const uint64_t key = splitmix64(seed ^ kAttribStream);
  if (dtype == VDQN_BF16)
    hipLaunchKernelGGL((attrib_pack_kernel<bf16raw>), grid, dim3(256), 0, st, s, coef, mode, sg[0], sg[1], sg[2], key, s0, i0, n_base, (bf16raw*)dst);
  else
    hipLaunchKernelGGL((attrib_pack_kernel<float>), grid, dim3(256), 0, st, s, coef, mode, sg[0], sg[1], sg[2], key, s0, i0, n_base, (float*)dst);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_attrib_reduce(const float* g, const float* w, float* acc, int32_t n_base, int32_t n_copies, int32_t squared, int32_t accumulate,
                                  void* stream) {
  VDQN_CHECK(g && w && acc, "vdqn_attrib_reduce: null arg");
  VDQN_CHECK(n_base >= 1 && n_copies >= 1, "vdqn_attrib_reduce: n_base %d and n_copies %d must be >= 1", n_base, n_copies);
  VDQN_CHECK(((uintptr_t)g & 15) == 0 && ((uintptr_t)acc & 15) == 0 && ((uintptr_t)w & 3) == 0, "vdqn_attrib_reduce: g and acc must be 16-byte aligned, w 4-byte");
  VDQN_CHECK((squared == 0 || squared == 1) && (accumulate == 0 || accumulate == 1), "vdqn_attrib_reduce: squared %d and accumulate %d are flags (0 / 1)", squared, accumulate);
  hipStream_t st = (hipStream_t)stream;
  const long n4 = (long)n_base * kImgElems / 4;
  ProfScope ps_("attrib_reduce", 0.0, (double)n4 * 16.0 * (n_copies + 1 + (accumulate ? 1 : 0)), st);
  hipLaunchKernelGGL(attrib_reduce_kernel, dim3(flat_grid(n4)), dim3(256), 0, st, (const float4*)g, w, (float4*)acc, n4, n_copies, squared, accumulate);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_attrib_finish(const float* acc, const void* src, int32_t src_kind, const void* baseline, const float* base_const, int32_t n_base,
                                  int32_t mode, int32_t scale_kind, float* out, void* stream) {
  VDQN_CHECK(acc && out, "vdqn_attrib_finish: null arg");
  VDQN_CHECK(mode == 0 || mode == 1, "vdqn_attrib_finish: mode %d (0: acc * (x - b), 1: max over colour of |acc|)", mode);
  VDQN_CHECK(n_base >= 1, "vdqn_attrib_finish: n_base %d must be >= 1", n_base);
  VDQN_CHECK(((uintptr_t)acc & 15) == 0 && ((uintptr_t)out & 15) == 0, "vdqn_attrib_finish: acc and out must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (mode == 1) {
    const long n4 = (long)n_base * 224 * 224 / 4;
    ProfScope ps_("attrib_finish<max>", 0.0, (double)n4 * 64.0, st);
    hipLaunchKernelGGL(attrib_finish_max_kernel, dim3(flat_grid(n4)), dim3(256), 0, st, (const float4*)acc, n4, (float4*)out);
    VDQN_LAUNCH_CHECK();
    return VDQN_OK;
  }
  Source s;
  RC(check_source("vdqn_attrib_finish", src, src_kind, baseline, base_const, n_base, &s));
  VDQN_CHECK(scale_kind == 0 || scale_kind == 1, "vdqn_attrib_finish: scale_kind %d (0: normalised frame, 1: uint8 pixel value)", scale_kind);
  float sc[3] = {1.f, 1.f, 1.f};
  if (scale_kind) vdqn_stem_pixel_scale(sc);
  const long n4 = (long)n_base * kImgElems / 4;
  ProfScope ps_("attrib_finish<ig>", 0.0, (double)n4 * 32.0 + (double)n_base * kImgElems * (src_kind == 0 ? 1 : 4) * (baseline ? 2 : 1), st);
  hipLaunchKernelGGL(attrib_finish_ig_kernel, dim3(flat_grid(n4)), dim3(256), 0, st, (const float4*)acc, s, sc[0], sc[1], sc[2], scale_kind, n4, (float4*)out);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
