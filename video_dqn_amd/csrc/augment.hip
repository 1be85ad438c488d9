// Random shift + left-right mirror augmentation (DrQ / RAD style), fused into the input pack: both transforms are index remaps of
// uint8 pixels, so the augmented stem operand is EXACTLY vdqn_pack_input of the augmented frames (tests/aug_oracle.py restates
// everything below in numpy; the tests are bit for bit).  No host round trip: the draw, the action swap and the pack are launches
// on the caller's stream.
//
// One triple (sx, sy, flip) per update and per SAMPLE, shared by the sample's F frames and by s and s' (the action label is the
// camera motion between s and s': a relative shift between the two would look like a small turn).
//
// Draw of sample j of the global batch G at update `step`, P = pad (uint64 arithmetic, wrapping):
//   key  = splitmix64(seed ^ 0x4155474D454E5431)          "AUGMENT1": a stream of its own, not prioritized replay's splitmix64(seed)
//   h    = splitmix64(key ^ (step * G + j))
//   sx   = (((h         & 0xFFFF) * (2P + 1)) >> 16) - P
//   sy   = ((((h >> 16) & 0xFFFF) * (2P + 1)) >> 16) - P
//   flip = flip_on ? (h >> 32) & 1 : 0
//   params[j] = int32 {sx, sy, flip, 0}
// Transform of one frame, output pixel (Y, X), 0 <= Y, X < 224:
//   Xs = clamp(X + sx, 0, 223);  Ys = clamp(Y + sy, 0, 223);  if flip: Xs = 223 - Xs;   out[Y][X][c] = in[Ys][Xs][c]
// i.e. mirror the source, pad it by edge replication, crop at the drawn offset.  The packed operand's zero border (the
// convolution's padding) stays zero.  The clamps hold for ANY int32 sx, sy and flip != 0 means 1: no parameter value makes the
// kernel read outside the frame.
//
// Colour jitter (brightness, contrast, saturation), a map from uint8 pixels to uint8 pixels in integer arithmetic, so the operand is
// still EXACTLY vdqn_pack_input of host-augmented frames (tests/aug_color_oracle.py restates it in numpy).  One int32 {f_b, f_c, f_s,
// 0} per update and per SAMPLE, shared by its F frames and by s and s' (one camera, a fraction of a second apart).  Factors are Q8:
// 256 = 1.0.  "/ 256" is floor division, i.e. an arithmetic shift.
// Draw of sample j of the global batch G at update `step`, Jq_k = int(J_k * 256 + 0.5) in 0 .. 256 the Q8 half-width of factor k:
//   key = splitmix64(seed ^ 0x415547434F4C5231)           "AUGCOLR1": a stream of its own, the shift / mirror draws do not move
//   h   = splitmix64(key ^ (step * G + j))
//   f_k = 256 - Jq_k + ((((h >> 16 k) & 0xFFFF) * (2 Jq_k + 1)) >> 16)     k = 0 brightness, 1 contrast, 2 saturation
//   color[j] = int32 {f_b, f_c, f_s, 0}
// Transform of one source pixel (R, G, B), in this order:
//   saturation:  g = (77 R + 150 G + 29 B + 128) / 256                                  (BT.601 weights, sum 256)
//                v = clamp(g + ((v - g) * f_s + 128) / 256, 0, 255)                     for v in R, G, B
//   brightness:  v = min(255, (v * f_b + 128) / 256)
//   contrast:    v = clamp(128 + ((v - 128) * f_c + 128) / 256, 0, 255)                 (pivot: mid-grey 128, no per-frame mean)
// then the normalisation of pack_input.  Saturation goes first because it is the only stage that mixes channels: what follows it,
// brightness then contrast, is a byte -> byte map bc(t) that folds into the per-block normalisation table, lut[c][t] = norm_c(bc(t)),
// so only saturation costs per-pixel work.  The shift / mirror remap only picks the source pixel: the two compose in either order.
// The kernel clamps every factor to [0, 512] first: no int32 value overflows a product or indexes outside a table; word 3 is ignored.
//
// Random zoom (a change of focal length: a window of [1 - J, 1] of the frame's side, resampled back to 224 x 224; never a zoom-out),
// bilinear with Q16 coordinates and Q8 weights in integer arithmetic, so the operand is still EXACTLY vdqn_pack_input of host-augmented
// frames (tests/aug_zoom_oracle.py restates it in numpy).  One int32 {ax, ay, bx, by} per update and per SAMPLE, shared by its F frames
// and by s and s': ax, ay the Q16 source step per output pixel (65536 = 1.0), bx, by the Q16 source coordinate of output pixel 0.
// ">>" is arithmetic.
// Draw of sample j of the global batch G at update `step`, Jz = int(J * 65536 + 0.5) in 0 .. 32768:
//   key = splitmix64(seed ^ 0x4155475A4F4F4D31)           "AUGZOOM1": a stream of its own, the shift / mirror / colour draws do not move
//   h   = splitmix64(key ^ (step * G + j));   h_k = (h >> 16 k) & 0xFFFF
//   ax  = 65536 - ((h_0 * (Jz + 1)) >> 16)                                in [65536 - Jz, 65536]
//   ay  = aspect ? 65536 - ((h_1 * (Jz + 1)) >> 16) : ax
//   origin(a, hk):  R = (224 * 65536 - 224 * a) >> 8                      the free range of the window's edge, in 1/256 pixel
//                   o = ((hk * (R + 1)) >> 16) << 8                       the window's edge, Q16, uniform over where it fits
//                   b = o + (a >> 1) - 32768                              pixel centres: output centre X + 1/2 maps to o + (X + 1/2) a
//   bx = origin(ax, h_2);  by = origin(ay, h_3);   zoom[j] = int32 {ax, ay, bx, by};   Jz = 0 gives {65536, 65536, 0, 0}, the identity
// Resample of one frame Z into the output pixel (Y, X), per channel:
//   u = bx + X * ax;  x0 = u >> 16;  wx = (u >> 8) & 255;     v = by + Y * ay;  y0 = v >> 16;  wy = (v >> 8) & 255
//   xa = clamp(x0, 0, 223), xb = clamp(x0 + 1, 0, 223), ya, yb likewise
//   top = Z[ya][xa] * (256 - wx) + Z[ya][xb] * wx;   bot = the same on row yb
//   out = (top * (256 - wy) + bot * wy + 32768) >> 16         (at most 255 * 65536 + 32768: fits int32; 0 .. 255)
// Z is the frame after shift and mirror, Z[y][x] = in[clamp(y + sy)][mirror(clamp(x + sx))]: the remap above applied to each tap.
// Colour jitter works on the resampled bytes: operand = pack(color(zoom(shift_mirror(frames)))).
// The kernel clamps ax, ay to [0, 65536] and bx, by to +-224 * 65536 first: |u|, |v| < 2^25, and every tap is clamped into the frame,
// whatever int32 the row holds.  A step of at most 1.0 is also what bounds the rows a pair of packed rows needs (below).
#include "common.h"

namespace {

constexpr uint64_t kAugStream = 0x4155474D454E5431ull;
constexpr uint64_t kColorStream = 0x415547434F4C5231ull;
constexpr int kMaxPad = 32;
constexpr int kMaxJq = 256;      // Q8 half-width of a colour factor: J in [0, 1]
constexpr int kMaxFactor = 512;  // 256 + kMaxJq
constexpr uint64_t kZoomStream = 0x4155475A4F4F4D31ull;
constexpr int kMaxJz = 32768;              // Q16 width of the zoom's side range: J in [0, 0.5]
constexpr int kZoomOne = 65536;            // Q16 1.0: the largest source step (no zoom-out)
constexpr int kZoomMaxOrigin = 224 << 16;  // |bx|, |by| beyond it already select an edge pixel everywhere

__host__ __device__ inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- aug_draw: one thread per sample ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_draw_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int pad, int flip_on,
                                                       int4* __restrict__ params) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = splitmix64(seed ^ kAugStream);
  const uint64_t h = splitmix64(key ^ (step * (uint64_t)G + (uint64_t)(first + i)));
  const uint32_t span = 2u * (uint32_t)pad + 1u;
  const int sx = (int)((((uint32_t)h & 0xFFFFu) * span) >> 16) - pad;
  const int sy = (int)((((uint32_t)(h >> 16) & 0xFFFFu) * span) >> 16) - pad;
  params[i] = make_int4(sx, sy, flip_on ? (int)((h >> 32) & 1) : 0, 0);
}

// ---- aug_draw_color: one thread per sample -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void aug_draw_color_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int jb, int jc, int js,
                                                             int4* __restrict__ color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = splitmix64(seed ^ kColorStream);
  const uint64_t h = splitmix64(key ^ (step * (uint64_t)G + (uint64_t)(first + i)));
  const int fb = 256 - jb + (int)((((uint32_t)h & 0xFFFFu) * (2u * (uint32_t)jb + 1u)) >> 16);
  const int fc = 256 - jc + (int)((((uint32_t)(h >> 16) & 0xFFFFu) * (2u * (uint32_t)jc + 1u)) >> 16);
  const int fs = 256 - js + (int)((((uint32_t)(h >> 32) & 0xFFFFu) * (2u * (uint32_t)js + 1u)) >> 16);
  color[i] = make_int4(fb, fc, fs, 0);
}

// ---- aug_draw_zoom: one thread per sample -------------------------------------------------------------------------------------
__device__ __forceinline__ int zoom_origin(int a, uint32_t hk) {
  const uint32_t R = (uint32_t)(224 * kZoomOne - 224 * a) >> 8;  // 0 .. 28672 for a in [32768, 65536]: hk * (R + 1) < 2^31
  return (int)(((hk * (R + 1u)) >> 16) << 8) + (a >> 1) - 32768;
}

__global__ __launch_bounds__(256) void aug_draw_zoom_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int jz, int aspect,
                                                            int4* __restrict__ zoom) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = splitmix64(seed ^ kZoomStream);
  const uint64_t h = splitmix64(key ^ (step * (uint64_t)G + (uint64_t)(first + i)));
  const uint32_t span = (uint32_t)jz + 1u;  // <= 32769: a 16-bit draw times it stays below 2^31
  const int ax = kZoomOne - (int)((((uint32_t)h & 0xFFFFu) * span) >> 16);
  const int ay = aspect ? kZoomOne - (int)((((uint32_t)(h >> 16) & 0xFFFFu) * span) >> 16) : ax;
  zoom[i] = make_int4(ax, ay, zoom_origin(ax, (uint32_t)(h >> 32) & 0xFFFFu), zoom_origin(ay, (uint32_t)(h >> 48) & 0xFFFFu));
}

// ---- aug_swap_actions: a0 <-> a1 for the flipped samples, a copy otherwise -------------------------------------------------------
__global__ __launch_bounds__(256) void aug_swap_actions_kernel(const int64_t* __restrict__ act, const int4* __restrict__ params, int n,
                                                               int64_t a0, int64_t a1, int64_t* __restrict__ act_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  int64_t a = act[b];
  if (params[b].z != 0) a = a == a0 ? a1 : a == a1 ? a0 : a;
  act_out[b] = a;
}

// ---- pack_input_aug: pack_input_rows_kernel (pointwise.hip) with the remap ------------------------------------------------------
// A block walks kPackPairs pairs of packed rows of one frame.  A pair covers the four output rows Y0 .. Y0 + 3 (Y0 a multiple of 4:
// a pair lies entirely inside the frame or entirely in the zero border); their source rows clamp(Y0 + r + sy) are non-decreasing in
// r and at most 3 apart, so the DISTINCT ones are Ys0 .. Ys3 and output row r reads LDS slot Ys_r - Ys0: every source row of the
// pair comes from HBM once, as 42 16-byte vectors.  The X remap and the mirror pick which 3 LDS bytes a pixel reads.  The
// normalisation table is built with the expression of pack_input_rows_kernel: same bits.
// COLOR: thread t writes table entry t at bc(t), brightness then contrast of byte t under the block's factors, and a pixel's three
// bytes go through the saturation stage between their LDS read and the table lookup.  COLOR = false is the kernel without any of it.
constexpr int kPackPairs = 4;
__device__ __forceinline__ int clamp223(int v) { return min(max(v, 0), 223); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

template <typename T, bool COLOR>
__global__ __launch_bounds__(256) void pack_input_aug_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, int frames_per_sample,
                                                             const int4* __restrict__ params, const int4* __restrict__ color, int n_params) {
  __shared__ uint4 rows[4][42];
  __shared__ T lut[3][256];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  int fs = 256;  // the saturation factor (COLOR only)
  {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    int t = tid;
    if constexpr (COLOR) {
      const int4 f = color[(n / frames_per_sample) % n_params];
      const int fb = min(max(f.x, 0), kMaxFactor), fc = min(max(f.y, 0), kMaxFactor);
      fs = min(max(f.z, 0), kMaxFactor);
      t = min(255, (t * fb + 128) >> 8);            // brightness
      t = clamp255(128 + (((t - 128) * fc + 128) >> 8));  // contrast about mid-grey (>> of a negative int: arithmetic, i.e. floor)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][tid] = from_f32<T>((((float)t / 255.0f) - mean[c]) / stdv[c]);
  }
  const int4 p = params[(n / frames_per_sample) % n_params];
  // |shift| > 223 already selects the edge pixel everywhere: clamping the shift first gives the same pixels without int overflow
  const int sx = min(max(p.x, -224), 224), sy = min(max(p.y, -224), 224);
  const bool flip = p.z != 0;
  const int yy = tid / 115, x = tid - yy * 115;
  // byte offsets of this thread's two source pixels inside a row (the same for every pair)
  int o0 = 0, o1 = 0;
  {
    const int xs = x - 2;
    int X0 = clamp223(2 * xs + sx), X1 = clamp223(2 * xs + 1 + sx);
    if (flip) {
      X0 = 223 - X0;
      X1 = 223 - X1;
    }
    o0 = 3 * X0;
    o1 = 3 * X1;
  }
  for (int pr = 0; pr < kPackPairs; ++pr) {
    const int y0 = 2 * ((int)blockIdx.x * kPackPairs + pr);  // packed rows y0, y0 + 1 -> output rows 2 (y0 - 2) .. + 3
    if (y0 >= 115) break;
    const int Y0 = 2 * (y0 - 2);
    const bool inside = (unsigned)Y0 < 224u;  // Y0 % 4 == 0: Y0 .. Y0 + 3 are all inside, or the pair is zero border
    const int Ys0 = clamp223(Y0 + sy), Ys3 = clamp223(Y0 + 3 + sy);
    __syncthreads();  // the previous pair's readers are done (first pass: the table is written)
    if (tid < 168 && inside) {
      const int s = tid / 42, c = tid - s * 42;
      if (Ys0 + s <= Ys3) rows[s][c] = reinterpret_cast<const uint4*>(src + ((size_t)n * 224 + (Ys0 + s)) * 672)[c];
    }
    __syncthreads();
    const int y = y0 + yy;
    if (tid >= 230 || y >= 115) continue;
    const int ys = y - 2, xs = x - 2;
    __attribute__((aligned(16))) T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
    if (inside && (unsigned)ys < 112u && (unsigned)xs < 112u) {
      const int r0 = clamp223(Y0 + 2 * yy + sy) - Ys0, r1 = clamp223(Y0 + 2 * yy + 1 + sy) - Ys0;  // LDS slots, 0 .. 3
      const uint8_t* b0 = reinterpret_cast<const uint8_t*>(rows[r0]);
      const uint8_t* b1 = reinterpret_cast<const uint8_t*>(rows[r1]);
      if constexpr (COLOR) {
        const uint8_t* px[4] = {b0 + o0, b0 + o1, b1 + o0, b1 + o1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int R = px[k][0], G = px[k][1], B = px[k][2];
          const int g = (77 * R + 150 * G + 29 * B + 128) >> 8;
          v[3 * k] = lut[0][clamp255(g + (((R - g) * fs + 128) >> 8))];
          v[3 * k + 1] = lut[1][clamp255(g + (((G - g) * fs + 128) >> 8))];
          v[3 * k + 2] = lut[2][clamp255(g + (((B - g) * fs + 128) >> 8))];
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] = lut[c][b0[o0 + c]];
          v[3 + c] = lut[c][b0[o1 + c]];
          v[6 + c] = lut[c][b1[o0 + c]];
          v[9 + c] = lut[c][b1[o1 + c]];
        }
      }
    }
    T* d = dst + ((size_t)n * 115 * 115 + (size_t)y * 115 + x) * 16;
    constexpr int V16 = (int)(16 * sizeof(T) / 16);
#pragma unroll
    for (int q = 0; q < V16; ++q) reinterpret_cast<uint4*>(d)[q] = reinterpret_cast<const uint4*>(v)[q];
  }
}

// ---- pack_input_zoom: pack_input_aug_kernel with four taps per output pixel ----------------------------------------------------------
// The same grid and the same walk over pairs of packed rows; a kernel of its own, so the four instances above keep their registers.
// A pair's output rows Y0 .. Y0 + 3 read the tap rows ya(Y0) .. yb(Y0 + 3) of Z.  The step ay is at most 1.0, so y0(Y0 + 3) <=
// y0(Y0) + 3 and the taps span at most y0(Y0) .. y0(Y0) + 4; the clamp into the frame and the shift clamp are non-decreasing and
// move neighbours by at most 1, so the DISTINCT source rows are at most five consecutive ones, first .. last, staged once per pair as
// 42 16-byte vectors each.  A tap reads slot clamp(y + sy) - first, which lies in 0 .. last - first for every row of the pair.
// A thread's four x-tap byte offsets and two wx do not depend on the pair: computed once per block, as o0 / o1 above.
struct ZoomRow {
  int ax, ay, bx, by;
};
__device__ __forceinline__ ZoomRow zoom_clamped(const int4 z) {
  return {min(max(z.x, 0), kZoomOne), min(max(z.y, 0), kZoomOne), min(max(z.z, -kZoomMaxOrigin), kZoomMaxOrigin),
          min(max(z.w, -kZoomMaxOrigin), kZoomMaxOrigin)};
}

template <typename T, bool COLOR>
__global__ __launch_bounds__(256) void pack_input_zoom_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, int frames_per_sample,
                                                              const int4* __restrict__ params, const int4* __restrict__ color,
                                                              const int4* __restrict__ zoom, int n_params) {
  __shared__ uint4 rows[5][42];
  __shared__ T lut[3][256];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int row = (n / frames_per_sample) % n_params;
  int fs = 256;  // the saturation factor (COLOR only)
  {
    const float mean[3] = {0.485f, 0.456f, 0.406f};
    const float stdv[3] = {0.229f, 0.224f, 0.225f};
    int t = tid;
    if constexpr (COLOR) {
      const int4 f = color[row];
      const int fb = min(max(f.x, 0), kMaxFactor), fc = min(max(f.y, 0), kMaxFactor);
      fs = min(max(f.z, 0), kMaxFactor);
      t = min(255, (t * fb + 128) >> 8);                  // brightness
      t = clamp255(128 + (((t - 128) * fc + 128) >> 8));  // contrast about mid-grey
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][tid] = from_f32<T>((((float)t / 255.0f) - mean[c]) / stdv[c]);
  }
  const int4 p = params[row];
  const int sx = min(max(p.x, -224), 224), sy = min(max(p.y, -224), 224);
  const bool flip = p.z != 0;
  const ZoomRow z = zoom_clamped(zoom[row]);
  const int yy = tid / 115, x = tid - yy * 115;
  // this thread's two output pixels X = 2 xs, 2 xs + 1: byte offsets of their taps xa, xb inside a staged row, and their weights
  int oa[2], ob[2], wx[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int u = z.bx + (2 * (x - 2) + k) * z.ax;
    const int x0 = u >> 16;
    int Xa = clamp223(clamp223(x0) + sx), Xb = clamp223(clamp223(x0 + 1) + sx);
    if (flip) {
      Xa = 223 - Xa;
      Xb = 223 - Xb;
    }
    oa[k] = 3 * Xa;
    ob[k] = 3 * Xb;
    wx[k] = (u >> 8) & 255;
  }
  for (int pr = 0; pr < kPackPairs; ++pr) {
    const int y0 = 2 * ((int)blockIdx.x * kPackPairs + pr);  // packed rows y0, y0 + 1 -> output rows 2 (y0 - 2) .. + 3
    if (y0 >= 115) break;
    const int Y0 = 2 * (y0 - 2);
    const bool inside = (unsigned)Y0 < 224u;
    // source rows of the pair's first and last tap row (Y0 in -4 .. 228: no overflow whether inside or not)
    const int first = clamp223(clamp223((z.by + Y0 * z.ay) >> 16) + sy);
    const int last = clamp223(clamp223(((z.by + (Y0 + 3) * z.ay) >> 16) + 1) + sy);
    __syncthreads();  // the previous pair's readers are done (first pass: the table is written)
    if (tid < 210 && inside) {
      const int s = tid / 42, c = tid - s * 42;
      if (first + s <= last) rows[s][c] = reinterpret_cast<const uint4*>(src + ((size_t)n * 224 + (first + s)) * 672)[c];
    }
    __syncthreads();
    const int y = y0 + yy;
    if (tid >= 230 || y >= 115) continue;
    const int ys = y - 2, xs = x - 2;
    __attribute__((aligned(16))) T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
    if (inside && (unsigned)ys < 112u && (unsigned)xs < 112u) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int vq = z.by + (Y0 + 2 * yy + r) * z.ay;
        const int yq = vq >> 16, wy = (vq >> 8) & 255;
        // LDS slots, 0 .. last - first <= 4 by the argument above; the clamp keeps a slot inside `rows` whatever happens
        const int sa = min(max(clamp223(clamp223(yq) + sy) - first, 0), 4), sb = min(max(clamp223(clamp223(yq + 1) + sy) - first, 0), 4);
        const uint8_t* ra = reinterpret_cast<const uint8_t*>(rows[sa]);
        const uint8_t* rb = reinterpret_cast<const uint8_t*>(rows[sb]);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int px[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int top = ra[oa[k] + c] * (256 - wx[k]) + ra[ob[k] + c] * wx[k];
            const int bot = rb[oa[k] + c] * (256 - wx[k]) + rb[ob[k] + c] * wx[k];
            px[c] = (top * (256 - wy) + bot * wy + 32768) >> 16;
          }
          T* o = v + 3 * (2 * r + k);
          if constexpr (COLOR) {
            const int g = (77 * px[0] + 150 * px[1] + 29 * px[2] + 128) >> 8;
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = lut[c][clamp255(g + (((px[c] - g) * fs + 128) >> 8))];
          } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = lut[c][px[c]];
          }
        }
      }
    }
    T* d = dst + ((size_t)n * 115 * 115 + (size_t)y * 115 + x) * 16;
    constexpr int V16 = (int)(16 * sizeof(T) / 16);
#pragma unroll
    for (int q = 0; q < V16; ++q) reinterpret_cast<uint4*>(d)[q] = reinterpret_cast<const uint4*>(v)[q];
  }
}

}  // namespace

extern "C" int vdqn_aug_draw(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t pad, int32_t flip,
                             int32_t* params, void* stream) {
  VDQN_CHECK(params, "vdqn_aug_draw: null params");
  VDQN_CHECK(n > 0, "vdqn_aug_draw: n = %d", n);
  VDQN_CHECK(global_batch >= 1 && first >= 0 && (int64_t)first + n <= (int64_t)global_batch,
             "vdqn_aug_draw: samples %d .. %lld outside the global batch of %d", first, (long long)first + n, global_batch);
  VDQN_CHECK(pad >= 0 && pad <= kMaxPad, "vdqn_aug_draw: pad %d outside [0, %d]", pad, kMaxPad);
  VDQN_CHECK(((uintptr_t)params & 15) == 0, "vdqn_aug_draw: params must be 16-byte aligned");
  ProfScope ps_("aug_draw", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first, (int)n,
                     (int)pad, (int)(flip != 0), (int4*)params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_aug_draw_color(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jb, int32_t jc,
                                   int32_t js, int32_t* color, void* stream) {
  VDQN_CHECK(color, "vdqn_aug_draw_color: null color");
  VDQN_CHECK(n > 0, "vdqn_aug_draw_color: n = %d", n);
  VDQN_CHECK(global_batch >= 1 && first >= 0 && (int64_t)first + n <= (int64_t)global_batch,
             "vdqn_aug_draw_color: samples %d .. %lld outside the global batch of %d", first, (long long)first + n, global_batch);
  VDQN_CHECK(jb >= 0 && jb <= kMaxJq && jc >= 0 && jc <= kMaxJq && js >= 0 && js <= kMaxJq,
             "vdqn_aug_draw_color: half-widths (%d, %d, %d) outside [0, %d] (Q8: int(J * 256 + 0.5), J in [0, 1])", jb, jc, js, kMaxJq);
  VDQN_CHECK(((uintptr_t)color & 15) == 0, "vdqn_aug_draw_color: color must be 16-byte aligned");
  ProfScope ps_("aug_draw_color", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_color_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first,
                     (int)n, (int)jb, (int)jc, (int)js, (int4*)color);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_aug_swap_actions(const int64_t* act, const int32_t* params, int32_t n, int32_t a0, int32_t a1, int64_t* act_out,
                                     void* stream) {
  VDQN_CHECK(act && params && act_out, "vdqn_aug_swap_actions: null arg");
  VDQN_CHECK(n > 0, "vdqn_aug_swap_actions: n = %d", n);
  VDQN_CHECK(a0 != a1 && a0 >= 0 && a0 <= 2 && a1 >= 0 && a1 <= 2, "vdqn_aug_swap_actions: actions (%d, %d) must be two different values of 0 .. 2",
             a0, a1);
  VDQN_CHECK(((uintptr_t)params & 15) == 0, "vdqn_aug_swap_actions: params must be 16-byte aligned");
  ProfScope ps_("aug_swap_actions", 0.0, (double)n * 32.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_swap_actions_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, act, (const int4*)params, (int)n,
                     (int64_t)a0, (int64_t)a1, act_out);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_pack_input_aug(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                   int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params, "vdqn_pack_input_aug: null arg");
  VDQN_CHECK(n_img > 0 && frames_per_sample > 0 && n_params > 0, "vdqn_pack_input_aug: n_img %d, frames_per_sample %d, n_params %d must be > 0",
             n_img, frames_per_sample, n_params);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_pack_input_aug: bad dtype");
  VDQN_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params) & 15) == 0, "vdqn_pack_input_aug: src, dst and params must be 16-byte aligned");
  ProfScope ps_("pack_input_aug", 0.0, (double)n_img * (224.0 * 224 * 3 + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  const dim3 grid((58 + kPackPairs - 1) / kPackPairs, n_img);
  if (dtype == VDQN_BF16)
    hipLaunchKernelGGL((pack_input_aug_kernel<bf16raw, false>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (bf16raw*)dst,
                       (int)frames_per_sample, (const int4*)params, (const int4*)nullptr, (int)n_params);
  else
    hipLaunchKernelGGL((pack_input_aug_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (float*)dst,
                       (int)frames_per_sample, (const int4*)params, (const int4*)nullptr, (int)n_params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_pack_input_aug_color(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                         const int32_t* color, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params && color, "vdqn_pack_input_aug_color: null arg");
  VDQN_CHECK(n_img > 0 && frames_per_sample > 0 && n_params > 0, "vdqn_pack_input_aug_color: n_img %d, frames_per_sample %d, n_params %d must be > 0",
             n_img, frames_per_sample, n_params);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_pack_input_aug_color: bad dtype");
  VDQN_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params | (uintptr_t)color) & 15) == 0,
             "vdqn_pack_input_aug_color: src, dst, params and color must be 16-byte aligned");
  ProfScope ps_("pack_input_aug_color", 0.0, (double)n_img * (224.0 * 224 * 3 + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  const dim3 grid((58 + kPackPairs - 1) / kPackPairs, n_img);
  if (dtype == VDQN_BF16)
    hipLaunchKernelGGL((pack_input_aug_kernel<bf16raw, true>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (bf16raw*)dst,
                       (int)frames_per_sample, (const int4*)params, (const int4*)color, (int)n_params);
  else
    hipLaunchKernelGGL((pack_input_aug_kernel<float, true>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (float*)dst,
                       (int)frames_per_sample, (const int4*)params, (const int4*)color, (int)n_params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_aug_draw_zoom(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jz, int32_t aspect,
                                  int32_t* zoom, void* stream) {
  VDQN_CHECK(zoom, "vdqn_aug_draw_zoom: null zoom");
  VDQN_CHECK(n > 0, "vdqn_aug_draw_zoom: n = %d", n);
  VDQN_CHECK(global_batch >= 1 && first >= 0 && (int64_t)first + n <= (int64_t)global_batch,
             "vdqn_aug_draw_zoom: samples %d .. %lld outside the global batch of %d", first, (long long)first + n, global_batch);
  VDQN_CHECK(jz >= 0 && jz <= kMaxJz, "vdqn_aug_draw_zoom: width %d outside [0, %d] (Q16: int(J * 65536 + 0.5), J in [0, 0.5])", jz, kMaxJz);
  VDQN_CHECK(((uintptr_t)zoom & 15) == 0, "vdqn_aug_draw_zoom: zoom must be 16-byte aligned");
  ProfScope ps_("aug_draw_zoom", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_zoom_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first,
                     (int)n, (int)jz, (int)(aspect != 0), (int4*)zoom);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_pack_input_aug_zoom(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                        const int32_t* color, const int32_t* zoom, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params && zoom, "vdqn_pack_input_aug_zoom: null arg");
  VDQN_CHECK(n_img > 0 && frames_per_sample > 0 && n_params > 0, "vdqn_pack_input_aug_zoom: n_img %d, frames_per_sample %d, n_params %d must be > 0",
             n_img, frames_per_sample, n_params);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_pack_input_aug_zoom: bad dtype");
  VDQN_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params | (uintptr_t)color | (uintptr_t)zoom) & 15) == 0,
             "vdqn_pack_input_aug_zoom: src, dst, params, color and zoom must be 16-byte aligned");
  ProfScope ps_("pack_input_aug_zoom", 0.0, (double)n_img * (224.0 * 224 * 3 + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  const dim3 grid((58 + kPackPairs - 1) / kPackPairs, n_img);
  const hipStream_t st = (hipStream_t)stream;
  const uint8_t* s = (const uint8_t*)src;
  const int F = (int)frames_per_sample, np = (int)n_params;
  const int4 *p = (const int4*)params, *c = (const int4*)color, *z = (const int4*)zoom;
  if (dtype == VDQN_BF16) {
    if (c) hipLaunchKernelGGL((pack_input_zoom_kernel<bf16raw, true>), grid, dim3(256), 0, st, s, (bf16raw*)dst, F, p, c, z, np);
    else hipLaunchKernelGGL((pack_input_zoom_kernel<bf16raw, false>), grid, dim3(256), 0, st, s, (bf16raw*)dst, F, p, c, z, np);
  } else {
    if (c) hipLaunchKernelGGL((pack_input_zoom_kernel<float, true>), grid, dim3(256), 0, st, s, (float*)dst, F, p, c, z, np);
    else hipLaunchKernelGGL((pack_input_zoom_kernel<float, false>), grid, dim3(256), 0, st, s, (float*)dst, F, p, c, z, np);
  }
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
