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
//
// Random rotation (camera roll) about the picture's centre, composed with the zoom into one affine map per SAMPLE, int32 [8] = {axx, axy,
// bx, 0, ayx, ayy, by, 0} in Q16, shared by its F frames and by s and s'.  All integers, ">>" arithmetic, "/" floors; the unit of angle
// is 1 / 64 degree.  tests/aug_rotate_oracle.py restates it in numpy; the operand is still EXACTLY vdqn_pack_input of host-augmented frames.
// Draw of sample j of the global batch G at update `step`, Jr = int(J * 64 + 0.5) in 0 .. 1920 (J <= 30 degrees):
//   key = splitmix64(seed ^ 0x415547524F544131)           "AUGROTA1": a stream of its own, the other draws do not move
//   h   = splitmix64(key ^ (step * G + j));   k = (((h & 0xFFFF) * (2 Jr + 1)) >> 16) - Jr          in [-Jr, Jr]
// Sine and cosine of k, Q16, in int64 (rot_sincos): Taylor polynomials in Q30, Horner form; no libm, so numpy gives the same bits
//   t = k * 292818 (Q30 radians, 292818 = round(pi / 11520 * 2^30), |t| < 2^30);   t2 = (t * t) >> 30;   ONE = 1 << 30
//   a = ONE - t2 / 42;  a = ONE - ((t2 * a) >> 30) / 20;  a = ONE - ((t2 * a) >> 30) / 6;   s = (t * a) >> 30
//   b = ONE - t2 / 56;  b = ONE - ((t2 * b) >> 30) / 30;  b = ONE - ((t2 * b) >> 30) / 12;  b = ONE - ((t2 * b) >> 30) / 2
//   S = (s + 8192) >> 14;   C = (b + 8192) >> 14          S(0) = 0, C(0) = 65536, S odd and C even in k, both within 0.53 * 2^-16 of float64
// The row, from the sample's zoom row {ax, ay, bxz, byz} (none: the identity {65536, 65536, 0, 0}), products in int64:
//   axx = (ax * C + 32768) >> 16      axy = -((ax * S + 32768) >> 16)     bx = bxz + ((223 * (ax - axx - axy)) >> 1)
//   ayx = (ay * S + 32768) >> 16      ayy = (ay * C + 32768) >> 16        by = byz + ((223 * (ay - ayx - ayy)) >> 1)
// i.e. rotate the output pixel centre about index (111.5, 111.5), then apply the zoom map; k = 0 gives {ax, 0, bxz, 0, 0, ay, byz, 0}.
// Resample of output pixel (Y, X): u = bx + X * axx + Y * axy, v = by + X * ayx + Y * ayy, then taps, weights and the bilinear exactly as
// the zoom's (above), on Z, the frame after shift and mirror; colour jitter works on the resampled bytes.  A row without cross terms
// gives the zoom entry's bits.  The kernel clamps axx, ayy to [0, 65536], axy, ayx to +-65536 and bx, by to +-448 * 65536 first: beyond
// that origin every tap of every output pixel already sits on one edge (a diagonal term adds at least 0 and a cross term at least
// -223 * 65536), |u|, |v| < 2^26, and a 32 x 32 tile of output pixels spans at most 62 source pixels per axis (pack_affine_kernel).
#include "pack_common.h"

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
constexpr uint64_t kRotateStream = 0x415547524F544131ull;
constexpr int kMaxJr = 1920;                  // 30 degrees in 1 / 64 degree
constexpr int kAffineMaxOrigin = 448 << 16;   // |bx|, |by| beyond it already select an edge pixel everywhere, whatever the cross term

// ---- the draws: one thread per sample --------------------------------------------------------------------------------------------
// the hash of sample j of the global batch G at update `step`, in the stream `stream` of the run's seed
__device__ __forceinline__ uint64_t sample_hash(uint64_t stream, uint64_t seed, uint64_t step, int G, int j) {
  return splitmix64(splitmix64(seed ^ stream) ^ (step * (uint64_t)G + (uint64_t)j));
}
// 16-bit field k of the hash, scaled to 0 .. span - 1 (span <= 2^15 + 1 everywhere: the product stays below 2^31)
__device__ __forceinline__ uint32_t draw16(uint64_t h, int k, uint32_t span) { return (((uint32_t)(h >> (16 * k)) & 0xFFFFu) * span) >> 16; }

__global__ __launch_bounds__(256) void aug_draw_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int pad, int flip_on,
                                                       int4* __restrict__ params) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = sample_hash(kAugStream, seed, step, G, first + i);
  const uint32_t span = 2u * (uint32_t)pad + 1u;
  params[i] = make_int4((int)draw16(h, 0, span) - pad, (int)draw16(h, 1, span) - pad, flip_on ? (int)((h >> 32) & 1) : 0, 0);
}

__global__ __launch_bounds__(256) void aug_draw_color_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int jb, int jc, int js,
                                                             int4* __restrict__ color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = sample_hash(kColorStream, seed, step, G, first + i);
  color[i] = make_int4(256 - jb + (int)draw16(h, 0, 2u * (uint32_t)jb + 1u), 256 - jc + (int)draw16(h, 1, 2u * (uint32_t)jc + 1u),
                       256 - js + (int)draw16(h, 2, 2u * (uint32_t)js + 1u), 0);
}

__device__ __forceinline__ int zoom_origin(int a, uint64_t h, int k) {
  const uint32_t R = (uint32_t)(224 * kZoomOne - 224 * a) >> 8;  // 0 .. 28672 for a in [32768, 65536]
  return (int)(draw16(h, k, R + 1u) << 8) + (a >> 1) - 32768;
}

__global__ __launch_bounds__(256) void aug_draw_zoom_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int jz, int aspect,
                                                            int4* __restrict__ zoom) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = sample_hash(kZoomStream, seed, step, G, first + i);
  const uint32_t span = (uint32_t)jz + 1u;  // <= 32769
  const int ax = kZoomOne - (int)draw16(h, 0, span), ay_own = kZoomOne - (int)draw16(h, 1, span);
  const int ay = aspect ? ay_own : ax;
  zoom[i] = make_int4(ax, ay, zoom_origin(ax, h, 2), zoom_origin(ay, h, 3));
}

// Q16 sine and cosine of k / 64 degrees, |k| <= 1920 (the arithmetic is written out at the top of this file)
__device__ __forceinline__ void rot_sincos(int k, int64_t& S, int64_t& C) {
  constexpr int64_t kOne = (int64_t)1 << 30;
  const int64_t t = (int64_t)k * 292818;
  const int64_t t2 = (t * t) >> 30;  // >= 0, as every dividend below: "/" floors
  int64_t a = kOne - t2 / 42;
  a = kOne - ((t2 * a) >> 30) / 20;
  a = kOne - ((t2 * a) >> 30) / 6;
  int64_t b = kOne - t2 / 56;
  b = kOne - ((t2 * b) >> 30) / 30;
  b = kOne - ((t2 * b) >> 30) / 12;
  b = kOne - ((t2 * b) >> 30) / 2;
  S = (((t * a) >> 30) + 8192) >> 14;
  C = (b + 8192) >> 14;
}

__global__ __launch_bounds__(256) void aug_draw_rotate_kernel(uint64_t seed, uint64_t step, int G, int first, int n, int jr,
                                                              const int4* __restrict__ zoom, int4* __restrict__ affine) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = sample_hash(kRotateStream, seed, step, G, first + i);
  const int k = (int)draw16(h, 0, 2u * (uint32_t)jr + 1u) - jr;
  const int4 z = zoom ? zoom[i] : make_int4(kZoomOne, kZoomOne, 0, 0);
  int64_t S, C;
  rot_sincos(k, S, C);
  const int64_t ax = z.x, ay = z.y;
  const int64_t axx = (ax * C + 32768) >> 16, axy = -((ax * S + 32768) >> 16);
  const int64_t ayx = (ay * S + 32768) >> 16, ayy = (ay * C + 32768) >> 16;
  affine[2 * i] = make_int4((int)axx, (int)axy, (int)(z.z + ((223 * (ax - axx - axy)) >> 1)), 0);
  affine[2 * i + 1] = make_int4((int)ayx, (int)ayy, (int)(z.w + ((223 * (ay - ayx - ayy)) >> 1)), 0);
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

// ---- the augmented pack: pack_input_rows_kernel (pointwise.hip) with the remap, the resample and the colour map -------------------
// One body, pack_aug_kernel<T, ZOOM, COLOR>.  Its eight instances are eight kernels, so each keeps the registers of its own work:
// ZOOM = false reads one tap per pixel and never pays for the four of the resample (which is why the shift is not run as a zoom
// with the identity row), COLOR = false is the kernel without any of the colour work.
// A block walks kPackPairs pairs of packed rows of one frame.  A pair covers the four output rows Y0 .. Y0 + 3 (Y0 a multiple of 4:
// a pair lies entirely inside the frame or entirely in the zero border).  The DISTINCT source rows they read are consecutive ones,
// first .. last, staged once per pair as 42 16-byte vectors each: every source row of the pair comes from HBM once, and a read of
// source row Ys takes LDS slot Ys - first.
//   shift: the source rows clamp(Y0 + r + sy) are non-decreasing in r and at most 3 apart: at most four rows, slots 0 .. 3.
//   ZOOM:  the output rows read the tap rows ya(Y0) .. yb(Y0 + 3) of Z.  The step ay is at most 1.0, so y0(Y0 + 3) <= y0(Y0) + 3 and
//          the taps span at most y0(Y0) .. y0(Y0) + 4; the clamp into the frame and the shift clamp are non-decreasing and move
//          neighbours by at most 1: at most five rows, and a tap's slot lies in 0 .. last - first for every row of the pair.
// What depends on the geometry is three small pieces: a thread's x taps (byte offsets inside a staged row, under ZOOM two per pixel
// and the weight between them; they do not depend on the pair and are computed once per block), a pair's first and last row, and the
// fetch of one output pixel's three bytes (one tap, or the four-tap bilinear).  The rest is shared.  The normalisation table takes
// its entries from pack_norm_entry, as pack_input_rows_kernel does: same bits.  COLOR: thread t writes table entry t at bc(t),
// brightness then contrast of byte t under the block's factors, and a pixel's three bytes go through the saturation stage between
// their fetch and the table lookup.
__device__ __forceinline__ int clamp223(int v) { return min(max(v, 0), 223); }
__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// Z[y][x] = in[src_y(y)][mirror(clamp(x + sx))]: the shifted and mirrored frame, as a source row and as a byte offset inside it
struct Shift {
  int sx, sy;
  bool flip;
};
// |shift| > 223 already selects the edge pixel everywhere: clamping the shift first gives the same pixels without int overflow
__device__ __forceinline__ Shift shift_clamped(const int4 p) { return {min(max(p.x, -224), 224), min(max(p.y, -224), 224), p.z != 0}; }
__device__ __forceinline__ int src_y(const Shift& s, int y) { return clamp223(y + s.sy); }
__device__ __forceinline__ int src_x3(const Shift& s, int x) {
  const int xs = clamp223(x + s.sx);
  return 3 * (s.flip ? 223 - xs : xs);
}

// pack_aug_kernel's table fill and saturation stage as functions, for pack_affine_kernel.  pack_aug_kernel keeps them written out in
// its body: calling these from it changed the code generated for its eight instances (register allocation and scheduling), and those
// instances stay as they were measured.
// Thread `tid` of a block of 256 writes entry `tid` of the block's normalisation table; COLOR: at bc(tid), brightness then contrast of
// byte `tid` under the factors of colour row `row`.  Returns the saturation factor (256 without COLOR).
template <typename T, bool COLOR>
__device__ __forceinline__ int pack_lut_fill(T (*lut)[256], int tid, const int4* __restrict__ color, int row) {
  int fs = 256;
  int t = tid;
  if constexpr (COLOR) {
    const int4 f = color[row];
    const int fb = min(max(f.x, 0), kMaxFactor), fc = min(max(f.y, 0), kMaxFactor);
    fs = min(max(f.z, 0), kMaxFactor);
    t = min(255, (t * fb + 128) >> 8);                  // brightness
    t = clamp255(128 + (((t - 128) * fc + 128) >> 8));  // contrast about mid-grey (>> of a negative int: arithmetic, i.e. floor)
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) lut[c][tid] = pack_norm_entry<T>(t, c);
  return fs;
}
// a pixel's three elements of the operand from its three bytes: the saturation stage (COLOR), then the table
template <typename T, bool COLOR>
__device__ __forceinline__ void pack_pixel(T* o, const int (&px)[3], const T (*lut)[256], int fs) {
  if constexpr (COLOR) {
    const int g = (77 * px[0] + 150 * px[1] + 29 * px[2] + 128) >> 8;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = lut[c][clamp255(g + (((px[c] - g) * fs + 128) >> 8))];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = lut[c][px[c]];
  }
}

struct ZoomRow {
  int ax, ay, bx, by;
};
__device__ __forceinline__ ZoomRow zoom_clamped(const int4 z) {
  return {min(max(z.x, 0), kZoomOne), min(max(z.y, 0), kZoomOne), min(max(z.z, -kZoomMaxOrigin), kZoomMaxOrigin),
          min(max(z.w, -kZoomMaxOrigin), kZoomMaxOrigin)};
}

template <typename T, bool ZOOM, bool COLOR>
__global__ __launch_bounds__(256) void pack_aug_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, int frames_per_sample,
                                                       const int4* __restrict__ params, const int4* __restrict__ color,
                                                       const int4* __restrict__ zoom, int n_params) {
  constexpr int kRows = ZOOM ? 5 : 4;
  __shared__ uint4 rows[kRows][42];
  __shared__ T lut[3][256];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int row = (n / frames_per_sample) % n_params;
  int fs = 256;  // the saturation factor (COLOR only)
  {
    int t = tid;
    if constexpr (COLOR) {
      const int4 f = color[row];
      const int fb = min(max(f.x, 0), kMaxFactor), fc = min(max(f.y, 0), kMaxFactor);
      fs = min(max(f.z, 0), kMaxFactor);
      t = min(255, (t * fb + 128) >> 8);                  // brightness
      t = clamp255(128 + (((t - 128) * fc + 128) >> 8));  // contrast about mid-grey (>> of a negative int: arithmetic, i.e. floor)
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c][tid] = pack_norm_entry<T>(t, c);
  }
  const Shift s = shift_clamped(params[row]);
  ZoomRow z = {};
  if constexpr (ZOOM) z = zoom_clamped(zoom[row]);
  const int yy = tid / 115, x = tid - yy * 115;
  // this thread's two output pixels X = 2 xs + k: byte offsets of their taps inside a staged row (ZOOM: taps xa and xb, and the
  // weight of xb), the same for every pair
  int oa[2], ob[2] = {0, 0}, wx[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int X = 2 * (x - 2) + k;
    if constexpr (ZOOM) {
      const int u = z.bx + X * z.ax;
      oa[k] = src_x3(s, clamp223(u >> 16));
      ob[k] = src_x3(s, clamp223((u >> 16) + 1));
      wx[k] = (u >> 8) & 255;
    } else {
      oa[k] = src_x3(s, X);
    }
  }
  for (int pr = 0; pr < kPackPairs; ++pr) {
    const int y0 = 2 * ((int)blockIdx.x * kPackPairs + pr);  // packed rows y0, y0 + 1 -> output rows 2 (y0 - 2) .. + 3
    if (y0 >= 115) break;
    const int Y0 = 2 * (y0 - 2);
    const bool inside = (unsigned)Y0 < 224u;  // Y0 % 4 == 0: Y0 .. Y0 + 3 are all inside, or the pair is zero border
    // the source rows of the pair's first and last read (Y0 in -4 .. 228: no overflow whether inside or not)
    int first, last;
    if constexpr (ZOOM) {
      first = src_y(s, clamp223((z.by + Y0 * z.ay) >> 16));
      last = src_y(s, clamp223(((z.by + (Y0 + 3) * z.ay) >> 16) + 1));
    } else {
      first = src_y(s, Y0);
      last = src_y(s, Y0 + 3);
    }
    __syncthreads();  // the previous pair's readers are done (first pass: the table is written)
    if (tid < 42 * kRows && inside) {
      const int r = tid / 42, c = tid - r * 42;
      if (first + r <= last) rows[r][c] = reinterpret_cast<const uint4*>(src + ((size_t)n * 224 + (first + r)) * 672)[c];
    }
    __syncthreads();
    const int y = y0 + yy;
    if (tid >= 230 || y >= 115) continue;
    const int ys = y - 2, xs = x - 2;
    __attribute__((aligned(16))) T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
    if (inside && (unsigned)ys < 112u && (unsigned)xs < 112u) {
      // One tap with COLOR: the four pixels' byte pointers are formed ahead of the pixel loops, the shape this instance had as a
      // kernel of its own.  Formed inside them (as the shift alone wants it), it costs about five more instructions per pair.
      const uint8_t* tap[4] = {};
      if constexpr (!ZOOM && COLOR) {
        const uint8_t* b0 = reinterpret_cast<const uint8_t*>(rows[src_y(s, Y0 + 2 * yy) - first]);
        const uint8_t* b1 = reinterpret_cast<const uint8_t*>(rows[src_y(s, Y0 + 2 * yy + 1) - first]);
        tap[0] = b0 + oa[0], tap[1] = b0 + oa[1], tap[2] = b1 + oa[0], tap[3] = b1 + oa[1];
      }
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int Y = Y0 + 2 * yy + r;
        const uint8_t *ra, *rb = nullptr;
        int wy = 0;
        if constexpr (ZOOM) {
          const int vq = z.by + Y * z.ay;
          const int yq = vq >> 16;
          wy = (vq >> 8) & 255;
          // LDS slots, 0 .. last - first <= 4 by the argument above; the clamp keeps a slot inside `rows` whatever happens
          ra = reinterpret_cast<const uint8_t*>(rows[min(max(src_y(s, clamp223(yq)) - first, 0), 4)]);
          rb = reinterpret_cast<const uint8_t*>(rows[min(max(src_y(s, clamp223(yq + 1)) - first, 0), 4)]);
        } else {
          ra = reinterpret_cast<const uint8_t*>(rows[src_y(s, Y) - first]);  // LDS slot, 0 .. 3
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int px[3];
          if constexpr (ZOOM) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int top = ra[oa[k] + c] * (256 - wx[k]) + ra[ob[k] + c] * wx[k];
              const int bot = rb[oa[k] + c] * (256 - wx[k]) + rb[ob[k] + c] * wx[k];
              px[c] = (top * (256 - wy) + bot * wy + 32768) >> 16;
            }
          } else {
            const uint8_t* p = COLOR ? tap[2 * r + k] : ra + oa[k];
            px[0] = p[0], px[1] = p[1], px[2] = p[2];  // named, not a loop over c: the compiler pairs the byte reads this way
          }
          // the pixel's three elements of the operand: the saturation stage (COLOR), then the table
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
    pack_store16(dst + ((size_t)n * 115 * 115 + (size_t)y * 115 + x) * 16, v);
  }
}

// the instance for (T, zoom rows given, colour rows given), launched over all frames
template <typename T>
void launch_pack_aug_kernel(hipStream_t st, const uint8_t* src, T* dst, int n_img, int F, const int4* params, const int4* color, const int4* zoom,
                            int n_params) {
  const auto kernel = zoom ? (color ? pack_aug_kernel<T, true, true> : pack_aug_kernel<T, true, false>)
                           : (color ? pack_aug_kernel<T, false, true> : pack_aug_kernel<T, false, false>);
  hipLaunchKernelGGL(kernel, pack_rows_grid(n_img), dim3(256), 0, st, src, dst, F, params, color, zoom, n_params);
}

// what the three draw entries share: the output `arg`, the count, the slice of the global batch and the output's alignment, with
// the entry's own check of its width (pad, half-widths, zoom width) in its place between the slice and the alignment
template <typename... W>
int check_draw(const char* name, const char* arg, const void* out, int32_t global_batch, int32_t first, int32_t n, bool width_ok,
               const char* width_text, W... width_args) {
  VDQN_CHECK(out, "%s: null %s", name, arg);
  VDQN_CHECK(n > 0, "%s: n = %d", name, n);
  VDQN_CHECK(global_batch >= 1 && first >= 0 && (int64_t)first + n <= (int64_t)global_batch,
             "%s: samples %d .. %lld outside the global batch of %d", name, first, (long long)first + n, global_batch);
  VDQN_CHECK(width_ok, width_text, width_args...);
  VDQN_CHECK(((uintptr_t)out & 15) == 0, "%s: %s must be 16-byte aligned", name, arg);
  return VDQN_OK;
}

// what the three pack entries share behind their null checks: the remaining checks (`aligned` lists the entry's pointers in its
// alignment message; a NULL colour or zoom array is aligned), the profiler scope named as the entry without "vdqn_", and the launch
int launch_pack_aug(const char* name, const char* aligned, const void* src, void* dst, int32_t n_img, int32_t frames_per_sample,
                    const int32_t* params, const int32_t* color, const int32_t* zoom, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(n_img > 0 && frames_per_sample > 0 && n_params > 0, "%s: n_img %d, frames_per_sample %d, n_params %d must be > 0", name, n_img,
             frames_per_sample, n_params);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "%s: bad dtype", name);
  VDQN_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params | (uintptr_t)color | (uintptr_t)zoom) & 15) == 0, "%s: %s must be 16-byte aligned",
             name, aligned);
  ProfScope ps_(name + 5, 0.0, (double)n_img * (224.0 * 224 * 3 + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  const int4 *p = (const int4*)params, *c = (const int4*)color, *z = (const int4*)zoom;
  if (dtype == VDQN_BF16)
    launch_pack_aug_kernel((hipStream_t)stream, (const uint8_t*)src, (bf16raw*)dst, (int)n_img, (int)frames_per_sample, p, c, z, (int)n_params);
  else
    launch_pack_aug_kernel((hipStream_t)stream, (const uint8_t*)src, (float*)dst, (int)n_img, (int)frames_per_sample, p, c, z, (int)n_params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// ---- the affine pack: rotation (and zoom) as one 2-D resample ----------------------------------------------------------------------
// Under a cross term an output row no longer reads one source row (at 30 degrees the four output rows of a pair of packed rows read
// 116 distinct source rows), so pack_aug_kernel's row staging does not carry over.  A block owns a TILE instead: kAffineTile x
// kAffineTile packed positions of one frame = 32 x 32 output pixels, one thread per packed position (its 2 x 2 pixels x 3 channels, stored
// with pack_store16: threads that are neighbours in x write contiguous 32 or 64 bytes); 8 x 8 tiles cover the 115 x 115 positions.
// u and v are affine in (X, Y), so over the tile's output pixels inside the frame they take their extremes at its four corners: the
// taps lie in the box [x0(umin), x0(umax) + 1] x [y0(vmin), y0(vmax) + 1] of Z, clamped into the frame as the taps are (the clamp is
// monotone: a clamped tap stays in the clamped box).  The block stages that box of Z — the shift / mirror remap is applied while
// staging, so the box is indexed in Z's coordinates — as one 32-bit word per pixel, and a tap is one LDS read.  With the clamped
// coefficients (|each| <= 1.0) 31 steps along X and 31 along Y move u by at most 62 pixels: x0 spans at most 63, the second tap one
// more, kAffineBox = 65 per axis always holds the box (at 30 degrees and step 1.0 it is at most 45 x 45).  Every LDS index is clamped into
// the array all the same.
constexpr int kAffineTile = 16;
constexpr int kAffineTiles = 8;  // per axis: 8 * 16 >= 115
constexpr int kAffineBox = 65;

struct AffineRow {
  int axx, axy, bx, ayx, ayy, by;
};
__device__ __forceinline__ AffineRow affine_clamped(const int4 x, const int4 y) {
  return {min(max(x.x, 0), kZoomOne),         min(max(x.y, -kZoomOne), kZoomOne), min(max(x.z, -kAffineMaxOrigin), kAffineMaxOrigin),
          min(max(y.x, -kZoomOne), kZoomOne), min(max(y.y, 0), kZoomOne),         min(max(y.z, -kAffineMaxOrigin), kAffineMaxOrigin)};
}

template <typename T, bool COLOR>
__global__ __launch_bounds__(256) void pack_affine_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst, int frames_per_sample,
                                                          const int4* __restrict__ params, const int4* __restrict__ color,
                                                          const int4* __restrict__ affine, int n_params) {
  __shared__ uint32_t box[kAffineBox * kAffineBox];
  __shared__ T lut[3][256];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
  const int row = (n / frames_per_sample) % n_params;
  const int fs = pack_lut_fill<T, COLOR>(lut, tid, color, row);
  const Shift s = shift_clamped(params[row]);
  const AffineRow a = affine_clamped(affine[2 * row], affine[2 * row + 1]);
  const int ty = (int)blockIdx.x / kAffineTiles, tx = (int)blockIdx.x - ty * kAffineTiles;
  const int ly = tid / kAffineTile, lx = tid - ly * kAffineTile;
  // the tile's output pixels inside the frame, X0 .. X1 by Y0 .. Y1 (never empty: packed 2 .. 113 hold pixels, every tile has some)
  const int X0 = max(2 * (tx * kAffineTile - 2), 0), X1 = min(2 * (tx * kAffineTile + kAffineTile - 3) + 1, 223);
  const int Y0 = max(2 * (ty * kAffineTile - 2), 0), Y1 = min(2 * (ty * kAffineTile + kAffineTile - 3) + 1, 223);
  const int u00 = a.bx + X0 * a.axx + Y0 * a.axy, u01 = a.bx + X1 * a.axx + Y0 * a.axy;
  const int u10 = a.bx + X0 * a.axx + Y1 * a.axy, u11 = a.bx + X1 * a.axx + Y1 * a.axy;
  const int v00 = a.by + X0 * a.ayx + Y0 * a.ayy, v01 = a.by + X1 * a.ayx + Y0 * a.ayy;
  const int v10 = a.by + X0 * a.ayx + Y1 * a.ayy, v11 = a.by + X1 * a.ayx + Y1 * a.ayy;
  const int zx0 = clamp223(min(min(u00, u01), min(u10, u11)) >> 16), zx1 = clamp223((max(max(u00, u01), max(u10, u11)) >> 16) + 1);
  const int zy0 = clamp223(min(min(v00, v01), min(v10, v11)) >> 16), zy1 = clamp223((max(max(v00, v01), max(v10, v11)) >> 16) + 1);
  const int bw = min(zx1 - zx0 + 1, kAffineBox), bh = min(zy1 - zy0 + 1, kAffineBox);
  const uint8_t* frame = src + (size_t)n * (224 * 672);
  // Staging: box pixel i = ry * bw + rx goes to thread i % 256, so a wave reads runs of neighbouring pixels of one source row, and
  // kAffineBatch pixels per thread are loaded before the first is stored: the loads of a batch are in flight together (one pixel per
  // trip of a loop over the box's rows exposed the full load latency nine times per block and measured 146 us over 512 frames).
  // i / bw as a multiply and shift: exact for bw <= 65 and i < 65 * bw, where i * m < 2^32.
  constexpr int kAffineBatch = 4;
  const int total = bw * bh;
  const uint32_t m = ((1u << 19) + (uint32_t)bw - 1u) / (uint32_t)bw;
  for (int i0 = tid; i0 < total; i0 += 256 * kAffineBatch) {
    uint32_t pix[kAffineBatch];
    int at[kAffineBatch];
#pragma unroll
    for (int j = 0; j < kAffineBatch; ++j) {
      const int i = min(i0 + 256 * j, total - 1);  // (past the end: the last pixel again, not stored)
      const int ry = (int)(((uint32_t)i * m) >> 19), rx = i - ry * bw;
      const uint8_t* p = frame + src_y(s, zy0 + ry) * 672 + src_x3(s, zx0 + rx);
      pix[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
      at[j] = ry * kAffineBox + rx;
    }
#pragma unroll
    for (int j = 0; j < kAffineBatch; ++j)
      if (i0 + 256 * j < total) box[at[j]] = pix[j];
  }
  __syncthreads();  // the box and the table are written
  const int y = ty * kAffineTile + ly, x = tx * kAffineTile + lx;
  if (y >= 115 || x >= 115) return;
  const int ys = y - 2, xs = x - 2;
  __attribute__((aligned(16))) T v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
  if ((unsigned)ys < 112u && (unsigned)xs < 112u) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int X = 2 * xs + k, Y = 2 * ys + r;
        const int uq = a.bx + X * a.axx + Y * a.axy, vq = a.by + X * a.ayx + Y * a.ayy;
        const int wx = (uq >> 8) & 255, wy = (vq >> 8) & 255;
        const int xa = min(max(clamp223(uq >> 16) - zx0, 0), kAffineBox - 1), xb = min(max(clamp223((uq >> 16) + 1) - zx0, 0), kAffineBox - 1);
        const int ya = min(max(clamp223(vq >> 16) - zy0, 0), kAffineBox - 1), yb = min(max(clamp223((vq >> 16) + 1) - zy0, 0), kAffineBox - 1);
        const uint32_t taa = box[ya * kAffineBox + xa], tab = box[ya * kAffineBox + xb];
        const uint32_t tba = box[yb * kAffineBox + xa], tbb = box[yb * kAffineBox + xb];
        int px[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int top = (int)((taa >> (8 * c)) & 255u) * (256 - wx) + (int)((tab >> (8 * c)) & 255u) * wx;
          const int bot = (int)((tba >> (8 * c)) & 255u) * (256 - wx) + (int)((tbb >> (8 * c)) & 255u) * wx;
          px[c] = (top * (256 - wy) + bot * wy + 32768) >> 16;
        }
        pack_pixel<T, COLOR>(v + 3 * (2 * r + k), px, lut, fs);
      }
    }
  }
  pack_store16(dst + ((size_t)n * 115 * 115 + (size_t)y * 115 + x) * 16, v);
}

// launch_pack_aug for the affine entry: the same checks, the same profiler scope naming, the instance for (T, colour rows given)
int launch_pack_affine(const char* name, const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                       const int32_t* color, const int32_t* affine, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(n_img > 0 && frames_per_sample > 0 && n_params > 0, "%s: n_img %d, frames_per_sample %d, n_params %d must be > 0", name, n_img,
             frames_per_sample, n_params);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "%s: bad dtype", name);
  VDQN_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)params | (uintptr_t)color | (uintptr_t)affine) & 15) == 0,
             "%s: src, dst, params, color and affine must be 16-byte aligned", name);
  ProfScope ps_(name + 5, 0.0, (double)n_img * (224.0 * 224 * 3 + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  const int4 *p = (const int4*)params, *c = (const int4*)color, *a = (const int4*)affine;
  const dim3 grid(kAffineTiles * kAffineTiles, n_img);
  if (dtype == VDQN_BF16)
    hipLaunchKernelGGL((c ? pack_affine_kernel<bf16raw, true> : pack_affine_kernel<bf16raw, false>), grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src, (bf16raw*)dst, (int)frames_per_sample, p, c, a, (int)n_params);
  else
    hipLaunchKernelGGL((c ? pack_affine_kernel<float, true> : pack_affine_kernel<float, false>), grid, dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t*)src, (float*)dst, (int)frames_per_sample, p, c, a, (int)n_params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

}  // namespace

extern "C" int vdqn_aug_draw(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t pad, int32_t flip,
                             int32_t* params, void* stream) {
  if (const int rc = check_draw("vdqn_aug_draw", "params", params, global_batch, first, n, pad >= 0 && pad <= kMaxPad,
                                "vdqn_aug_draw: pad %d outside [0, %d]", pad, kMaxPad))
    return rc;
  ProfScope ps_("aug_draw", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first, (int)n,
                     (int)pad, (int)(flip != 0), (int4*)params);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_aug_draw_color(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jb, int32_t jc,
                                   int32_t js, int32_t* color, void* stream) {
  if (const int rc = check_draw("vdqn_aug_draw_color", "color", color, global_batch, first, n,
                                jb >= 0 && jb <= kMaxJq && jc >= 0 && jc <= kMaxJq && js >= 0 && js <= kMaxJq,
                                "vdqn_aug_draw_color: half-widths (%d, %d, %d) outside [0, %d] (Q8: int(J * 256 + 0.5), J in [0, 1])", jb, jc, js,
                                kMaxJq))
    return rc;
  ProfScope ps_("aug_draw_color", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_color_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first,
                     (int)n, (int)jb, (int)jc, (int)js, (int4*)color);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_aug_draw_zoom(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jz, int32_t aspect,
                                  int32_t* zoom, void* stream) {
  if (const int rc = check_draw("vdqn_aug_draw_zoom", "zoom", zoom, global_batch, first, n, jz >= 0 && jz <= kMaxJz,
                                "vdqn_aug_draw_zoom: width %d outside [0, %d] (Q16: int(J * 65536 + 0.5), J in [0, 0.5])", jz, kMaxJz))
    return rc;
  ProfScope ps_("aug_draw_zoom", 0.0, (double)n * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_zoom_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first,
                     (int)n, (int)jz, (int)(aspect != 0), (int4*)zoom);
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
  return launch_pack_aug("vdqn_pack_input_aug", "src, dst and params", src, dst, n_img, frames_per_sample, params, nullptr, nullptr, n_params, dtype,
                         stream);
}

extern "C" int vdqn_pack_input_aug_color(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                         const int32_t* color, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params && color, "vdqn_pack_input_aug_color: null arg");
  return launch_pack_aug("vdqn_pack_input_aug_color", "src, dst, params and color", src, dst, n_img, frames_per_sample, params, color, nullptr,
                         n_params, dtype, stream);
}

// colour NULL: none
extern "C" int vdqn_pack_input_aug_zoom(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                        const int32_t* color, const int32_t* zoom, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params && zoom, "vdqn_pack_input_aug_zoom: null arg");
  return launch_pack_aug("vdqn_pack_input_aug_zoom", "src, dst, params, color and zoom", src, dst, n_img, frames_per_sample, params, color, zoom,
                         n_params, dtype, stream);
}

// zoom NULL: the identity zoom row for every sample
extern "C" int vdqn_aug_draw_rotate(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jr, const int32_t* zoom,
                                    int32_t* affine, void* stream) {
  if (const int rc = check_draw("vdqn_aug_draw_rotate", "affine", affine, global_batch, first, n, jr >= 0 && jr <= kMaxJr,
                                "vdqn_aug_draw_rotate: range %d outside [0, %d] (1 / 64 degree: int(J * 64 + 0.5), J in [0, 30])", jr, kMaxJr))
    return rc;
  VDQN_CHECK(((uintptr_t)zoom & 15) == 0, "vdqn_aug_draw_rotate: zoom must be 16-byte aligned");
  ProfScope ps_("aug_draw_rotate", 0.0, (double)n * (zoom ? 48.0 : 32.0), (hipStream_t)stream);
  hipLaunchKernelGGL(aug_draw_rotate_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, step, (int)global_batch, (int)first,
                     (int)n, (int)jr, (const int4*)zoom, (int4*)affine);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// colour NULL: none
extern "C" int vdqn_pack_input_aug_affine(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                                          const int32_t* color, const int32_t* affine, int32_t n_params, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && params && affine, "vdqn_pack_input_aug_affine: null arg");
  return launch_pack_affine("vdqn_pack_input_aug_affine", src, dst, n_img, frames_per_sample, params, color, affine, n_params, dtype, stream);
}
