// The stem's DATA gradient: dL/d(frame) from the pooled gradient — max-pool backward followed by the transposed 7x7 / stride-2
// convolution, 64 -> 3 channels, back to 224 x 224 (what torch.autograd runs for `x.grad` through resnet.maxpool, resnet.relu,
// resnet.bn1 and resnet.conv1 of archs/HabitatDQNMultiAction.py:30 when the frames require a gradient).
//
// The arithmetic is done in the packed space of vdqn_pack_input ([n][115][115][16]), where conv1 is a 4 x 4 / stride-1 convolution:
//   g_t[py][px][k] = sum over r, s in 0..3 and co in 0..63 of g_c1[py - r][px - s][co] * w[co][r][s * 16 + k]
// with g_c1 the max-pool backward of g_pool (rows / columns outside 0..111 are zero) and w the FORWARD operand [64][4][1][64] as
// fold.hip packs it (K index r * 64 + s * 16 + k: fold_src_index, K_CONV1_S2D).  pack_input_kernel (pointwise.hip) puts source pixel
// (2 (py - 2) + dy, 2 (px - 2) + dx), channel c at packed channel k = (dy * 2 + dx) * 3 + c, so g_t unpacks to the frame as
// y = 2 py - 4 + dy, x = 2 px - 4 + dx; packed rows / columns 0, 1 and 114 are border and the channels 12..15 are pad: dropped.
//
// bf16 (stem_dgrad_kernel): ONE kernel, nothing but the f32 NCHW result goes to HBM.  A workgroup walks pooled rows k of one image.
// Per step the two pooled rows k, k + 1 (gradient + arg-max codes, staged by LDS-DMA, one new row per step) give the gradient tiles
// of conv rows 2k and 2k + 1 in LDS, by the rule of stem_wgrad_pool_kernel (wgrad.hip, the twin of `build` below): f32 sum of the
// <= 4 windows whose arg-max is the pixel, pooled row then window column, one rounding — the bits of vdqn_maxpool_bwd.
// The GEMM is output-stationary in the packed ROW: conv row h feeds packed rows h .. h + 3 (kernel row r = py - h), so instead of
// a ring of conv rows in LDS the four packed rows in flight live as f32 ACCUMULATORS in registers (slot py & 3) and only the two
// conv rows of the step are in LDS: 33 KB instead of 74 KB, which is what lets two workgroups share a CU (measured, DESIGN 3t:
// the build, MFMA and epilogue phases still add up — one workgroup's VALU build does not yet hide behind the other's MFMAs).
// A packed row is complete when conv row h = py has been added; the sums of a packed row always
// arrive in the order r = 3, 2, 1, 0, inside a row s = 0..3, then the two channel halves: no atomics, two runs agree bit for bit.
//   M = the 112 live packed pixels px = 2 + m of a row (8 MFMA tiles of 16, two per wave; the last one is padding),
//   N = 16 packed channels (12 live), K = 4 x 4 x 64 = 1024 on v_mfma_f32_16x16x32_bf16.
// The weight operand (32 KB) lives in registers for the kernel's life: every wave holds all 32 K-step fragments (128 VGPRs),
// gathered once through LDS.  A pixel fragment does not depend on r and is read once per (s, channel half, tile): 32
// ds_read_b128 beside 128 MFMAs per wave and step; the tile image is XOR-swizzled by the pixel PAIR, (chunk ^ (pixel >> 1)) & 7,
// so the 16 lanes of a read group cover the 256-byte bank row.
// Epilogue: the finished accumulators go through LDS ([2 packed rows][16 ch][128 px] f32) and leave as contiguous float4 runs of
// the three colour planes (896-byte row segments), times the per-channel scale: one f32 product.
//
// f32 / bf16x3 (stem_dgrad_plain_kernel): a correctness path, not a hot one — vdqn_maxpool_bwd into caller workspace (the engine
// has already written g_c1 in these modes), then one thread per frame element with f32 FMAs over its <= 16 taps x 64 channels.
#include "engine_net.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kDgPoolG = 56 * 128;                 // a pooled gradient row: 56 pixels x 64 channels bf16 (7 DMA pieces)
constexpr int kDgPoolI = 4096;                     // its arg-max codes, 56 x 64 bytes, staged as 4 pieces (the last one half used)
constexpr int kDgPoolRow = kDgPoolG + kDgPoolI;
constexpr int kDgTilePix = 131;                    // conv columns -1 .. 129 at index column + 1; only 0..111 are ever non-zero
constexpr int kDgTile = kDgTilePix * 128;          // one conv row: 131 pixels x 64 channels bf16
constexpr int kDgOutPitch = 130;                  // floats per channel row of sOut (128 pixels + 2: the four channel groups of a store spread over the banks)
constexpr int kDgOut = 2 * 16 * kDgOutPitch * 4;   // two finished packed rows, f32 [2][16 ch][kDgOutPitch]
constexpr int kDgGyOff = 2 * kDgPoolRow;
constexpr int kDgOutOff = kDgGyOff + 2 * kDgTile;
constexpr int kDgSmem = kDgOutOff + kDgOut;        // 72704 bytes: two workgroups per CU
static_assert(kDgSmem >= 64 * 256 * 2, "the weight operand is gathered through this LDS");
static_assert(2 * kDgSmem <= 160 * 1024, "two workgroups per CU");

struct DgScale { float v[3]; };

// diagnostic builds only (-DVDQN_DGRAD_PROBE=bits, wrong results): bit 0 = no tile build, bit 1 = no MFMA phase, bit 2 = no frame
// stores inside the step loop — what a phase costs is the time that goes when it is left out
#ifndef VDQN_DGRAD_PROBE
#define VDQN_DGRAD_PROBE 0
#endif

// byte offset of 16-byte chunk `chunk` (8 channels) of tile pixel index `ci`
__device__ __forceinline__ int dg_tile_off(int ci, int chunk) { return ci * 128 + (((chunk ^ (ci >> 1)) & 7) << 4); }

__global__ __launch_bounds__(256, 2) void stem_dgrad_kernel(const bf16raw* __restrict__ g_pool, const uint8_t* __restrict__ idx,
                                                            const bf16raw* __restrict__ wt, float* __restrict__ out, int pairs_per_block,
                                                            int blocks_per_img, int gp_bytes, int idx_bytes, const DgScale scale) {
  using T = bf16raw;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* sPool = smem;               // [2][kDgPoolRow]: pooled row r lives in slot r & 1
  unsigned char* sGy = smem + kDgGyOff;      // [2][kDgTile]: conv rows 2k, 2k + 1
  float* sOut = reinterpret_cast<float*>(smem + kDgOutOff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const int i16 = lane & 15, q = lane >> 4;
  const int img = blockIdx.x / blocks_per_img;
  const int k0 = (blockIdx.x - img * blocks_per_img) * pairs_per_block;  // this block owns packed rows 2 k0 .. 2 k1 - 1 (+ 112, 113)
  const int k1 = min(56, k0 + pairs_per_block);
  if (k0 >= k1) return;
  const int kb = max(0, k0 - 2);  // conv rows 2 k0 - 3 .. 2 k0 - 1 feed packed row 2 k0: two steps of run-in whose rows are not stored

  // ---- weights: raw copy to LDS, then this lane's fragments.  Fragment (r, s, hh), element e = w[co][r][s * 16 + n] with
  // co = hh * 32 + q * 8 + e (the K order of the pixel fragments below), n = i16 ----
  for (int i = tid; i < 64 * 256 * 2 / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = reinterpret_cast<const uint4*>(wt)[i];
  __syncthreads();
  u32x4 fb[4][4][2];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const T* w0 = reinterpret_cast<const T*>(smem) + (hh * 32 + q * 8) * 256 + r * 64 + s * 16 + i16;
        uint32_t pk[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = (uint32_t)w0[(2 * e) * 256] | ((uint32_t)w0[(2 * e + 1) * 256] << 16);
        fb[r][s][hh] = (u32x4){pk[0], pk[1], pk[2], pk[3]};
      }
  __syncthreads();
  // what neither the DMA nor the builder ever writes stays zero: tile pixels 0 and 113..130 (conv columns -1, 112..129), and the
  // pooled-row slots, so that a slot no row was staged into (pooled row 56) holds arg-max codes of 0, not whatever LDS held
  for (int i = tid; i < kDgOutOff / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();  // before the first LDS-DMA lands in a slot

  const unsigned long long g_ptr = (unsigned long long)g_pool, i_ptr = (unsigned long long)idx;
  const i32x4 rs_g = {__builtin_amdgcn_readfirstlane((int)(unsigned)g_ptr), __builtin_amdgcn_readfirstlane((int)((g_ptr >> 32) & 0xffff)), gp_bytes, 0x00020000};
  const i32x4 rs_i = {__builtin_amdgcn_readfirstlane((int)(unsigned)i_ptr), __builtin_amdgcn_readfirstlane((int)((i_ptr >> 32) & 0xffff)), idx_bytes, 0x00020000};
  const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  const uint32_t lane16 = (uint32_t)lane * 16u;
#define VDQN_DG_DMA(VOFF, LDS, RSRC)                                                                                   \
  {                                                                                                                    \
    const uint32_t l_ = (uint32_t)__builtin_amdgcn_readfirstlane((int)(LDS));                                           \
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds" ::"v"(VOFF), "s"(l_), "s"(RSRC) : "memory"); \
  }
  // pooled row r of this image -> slot r & 1: 7 gradient pieces + 4 code pieces of 1 KiB, piece p by wave p & 3 (reads behind the
  // end of the last image's codes fall outside the descriptor's range: zeros)
  auto issue_pool = [&](int r) {
    if (r >= 56) return;
    const uint32_t px0 = (uint32_t)((img * 56 + r) * 56);
    const uint32_t slot = lds_base + (uint32_t)((r & 1) * kDgPoolRow);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int pc = wv + 4 * i;  // wave-uniform
      if (pc < 7) {
        VDQN_DG_DMA(px0 * 128u + (uint32_t)(pc * 1024) + lane16, slot + (uint32_t)(pc * 1024), rs_g)
      } else if (pc < 11) {
        VDQN_DG_DMA(px0 * 64u + (uint32_t)((pc - 7) * 1024) + lane16, slot + (uint32_t)(kDgPoolG + (pc - 7) * 1024), rs_i)
      }
    }
  };
#undef VDQN_DG_DMA
  // ---- the gradient tiles of conv rows 2k (hr = 0) and 2k + 1 (hr = 1): the twin of stem_wgrad_pool_kernel's `build` (wgrad.hip);
  // only the place an item is stored differs.  An item is (conv row, pixel w, 8-channel group); row 2k only receives from pooled
  // row k (window row kh = 1), row 2k + 1 from pooled rows k (kh = 2) and k + 1 (kh = 0); an even pixel w = 2 j lies in window
  // column j only (dx = 1), an odd one in columns j (dx = 2) and j + 1 (dx = 0).  Runs of 64 items of ONE (row, pixel parity)
  // class; sums in f32 in the order of maxpool_bwd_rows_kernel (pooled row, then window column), one rounding. ----
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  auto add8 = [&](float (&sacc)[8], const unsigned char* slot, int ow, int cg, uint32_t tap) {
    const uint4 gv = *reinterpret_cast<const uint4*>(slot + ow * 128 + cg * 16);
    const uint2 iv = *reinterpret_cast<const uint2*>(slot + kDgPoolG + ow * 64 + cg * 8);
    const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w};
    const uint32_t xw[2] = {iv.x ^ (tap * 0x01010101u), iv.y ^ (tap * 0x01010101u)};  // a zero byte = a channel whose arg-max is this tap
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
      const uint32_t t = __builtin_amdgcn_perm(0u, xw[pq >> 1], (pq & 1) ? 0x0c030c02u : 0x0c010c00u);
      const u16x2 m = __builtin_elementwise_min(__builtin_bit_cast(u16x2, t), (u16x2){1, 1}) - (u16x2){1, 1};
      const uint32_t mg = gw[pq] & __builtin_bit_cast(uint32_t, m);
      sacc[2 * pq] += __uint_as_float(mg << 16);
      sacc[2 * pq + 1] += __uint_as_float(mg & 0xffff0000u);
    }
  };
  auto build = [&](int k) {
    const bool two = k + 1 < 56;
    const unsigned char* s0 = sPool + (k & 1) * kDgPoolRow;        // pooled row k
    const unsigned char* s1 = sPool + ((k + 1) & 1) * kDgPoolRow;  // pooled row k + 1
#pragma unroll 1
    for (int i = 0; i < 7; ++i) {
      const int run = wv + 4 * i;   // wave-uniform, 0..27
      const int cls = run / 7;      // 0: row 2k, even w | 1: row 2k, odd w | 2: row 2k + 1, even w | 3: row 2k + 1, odd w
      const int j = (run - cls * 7) * 64 + lane;
      const int cg = j & 7, jp = j >> 3;
      const int jr = min(jp + 1, 55);  // a window that does not exist is read at a clamped address against a code no arg-max has
      const uint32_t no = 0xffu;
      const bool right = jp + 1 < 56;
      float sacc[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) sacc[e] = 0.f;
      if (cls == 0) {
        add8(sacc, s0, jp, cg, 4);
      } else if (cls == 1) {
        add8(sacc, s0, jp, cg, 5);
        add8(sacc, s0, jr, cg, right ? 3u : no);
      } else if (cls == 2) {
        add8(sacc, s0, jp, cg, 7);
        add8(sacc, s1, jp, cg, two ? 1u : no);
      } else {
        add8(sacc, s0, jp, cg, 8);
        add8(sacc, s0, jr, cg, right ? 6u : no);
        add8(sacc, s1, jp, cg, two ? 2u : no);
        add8(sacc, s1, jr, cg, (two && right) ? 0u : no);
      }
      const int w = 2 * jp + (cls & 1);
      T ov[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = from_f32<T>(sacc[e]);
      *reinterpret_cast<uint4*>(sGy + (cls >> 1) * kDgTile + dg_tile_off(w + 1, cg)) = *reinterpret_cast<const uint4*>(ov);
    }
  };

  // acc[slot][t]: packed row py with py & 3 == slot, pixels m = (2 wave + t) * 16 + i16, packed channels 4 q .. 4 q + 3
  f32x4 acc[4][2];
#pragma unroll
  for (int sl = 0; sl < 4; ++sl)
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[sl][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // a finished slot -> sOut[hr] (the pad channels 12..15 of q == 3 are not stored), then cleared for packed row py + 4
  auto retire = [&](f32x4 (&a)[2], int hr) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (q < 3) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sOut[(hr * 16 + q * 4 + reg) * kDgOutPitch + (2 * wv + t) * 16 + i16] = a[t][reg];
      }
      a[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  };
  // conv rows 2k, 2k + 1 of a step with k & 1 == P into the accumulators; packed rows 2k, 2k + 1 retire.  Pixel fragment of
  // tile t, shift s, half hh: the 8 channels hh * 32 + 8 q .. of conv column m + 2 - s, tile pixel index m + 3 - s.
  auto gemm = [&](auto par) {
    constexpr int P = decltype(par)::value;
#pragma unroll
    for (int hr = 0; hr < 2; ++hr) {
      constexpr int kBase = 2 * P;
      const unsigned char* a = sGy + hr * kDgTile;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        u32x4 fa[2][2];
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int t = 0; t < 2; ++t) fa[hh][t] = *reinterpret_cast<const u32x4*>(a + dg_tile_off((2 * wv + t) * 16 + i16 + 3 - s, hh * 4 + q));
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              acc[(kBase + hr + r) & 3][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fb[r][s][hh]), __builtin_bit_cast(bf16x8, fa[hh][t]),
                                                                                    acc[(kBase + hr + r) & 3][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);  // (one shift's fragments at a time: all sixteen up front do not fit beside the weights)
      }
      retire(acc[(kBase + hr) & 3], hr);
    }
  };
  // packed rows 2k, 2k + 1 from sOut to the frame: item = (packed row hr, source row dy, colour c, run of four x); element x of
  // source row 2 py - 4 + dy is packed pixel m = x / 2, channel (dy * 2 + (x & 1)) * 3 + c
  auto store_rows = [&](int k) {
    for (int it = tid; it < 2 * 2 * 3 * 56; it += 256) {
      const int x4 = it % 56, rest = it / 56;
      const int c = rest % 3, rr = rest / 3;
      const int hr = rr >> 1, dy = rr & 1;
      const int py = 2 * k + hr;
      if (py < 2 || py < 2 * k0) continue;  // border rows 0, 1; the run-in rows belong to the block before
      const float sc = c == 0 ? scale.v[0] : c == 1 ? scale.v[1] : scale.v[2];
      // channel-major sOut: the four elements are two neighbouring pixels of the channels of dx = 0 and dx = 1, and neighbouring
      // lanes read neighbouring 8 bytes (pixel-major, the lanes of a read met in ONE bank: 0.055 of 0.245 ms at 256 images)
      const float* src = sOut + (hr * 16 + dy * 6 + c) * kDgOutPitch + 2 * x4;
      const float2 e0 = *reinterpret_cast<const float2*>(src), e1 = *reinterpret_cast<const float2*>(src + 3 * kDgOutPitch);
      float4 v;
      v.x = e0.x * sc; v.y = e1.x * sc; v.z = e0.y * sc; v.w = e1.y * sc;
      const int y = 2 * py - 4 + dy;
      *reinterpret_cast<float4*>(out + (((size_t)img * 3 + c) * 224 + y) * 224 + 4 * x4) = v;
    }
  };

  issue_pool(kb);
  issue_pool(kb + 1);
  // two instances of the GEMM, by the parity of k, so that the accumulator slot of every (conv row, kernel row) pair is a
  // compile-time register
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  for (int k = kb; k < k1; ++k) {
    __builtin_amdgcn_s_barrier();  // [A] pooled rows k, k + 1 are in LDS; every wave is done with the tiles and sOut of step k - 1
#if !(VDQN_DGRAD_PROBE & 1)
    build(k);
#endif
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // [B] tiles built; pooled row k is no longer read
    if (k + 1 < k1) issue_pool(k + 2);
#if !(VDQN_DGRAD_PROBE & 2)
    if (k & 1) gemm(std::integral_constant<int, 1>{});
    else gemm(std::integral_constant<int, 0>{});
#else
    if ((fb[0][0][0][0] ^ fb[3][3][1][3]) == 0x12345678u) retire(acc[0], 0);  // (keeps the weight registers live)
#endif
    // the pooled row's DMA has had the MFMA phase to land: waited for HERE, in front of the frame stores, so that no step waits
    // for its predecessor's stores to be acknowledged
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // [C] packed rows 2k, 2k + 1 are in sOut; pooled row k + 2 is in LDS
#if !(VDQN_DGRAD_PROBE & 4)
    store_rows(k);
#endif
  }
  if (k1 == 56) {  // packed rows 112, 113 (slots 0, 1): conv rows 112.. do not exist, their sums are complete
    __syncthreads();
    retire(acc[0], 0);
    retire(acc[1], 1);
    __syncthreads();
    store_rows(56);
  }
}

// f32 / bf16x3: one thread per frame element, f32 FMAs in the order r, s, co
__global__ __launch_bounds__(256) void stem_dgrad_plain_kernel(const float* __restrict__ g_c1, const float* __restrict__ wt, float* __restrict__ out,
                                                               long long total, const DgScale scale) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % 224);
  long long t = i / 224;
  const int y = (int)(t % 224);
  t /= 224;
  const int c = (int)(t % 3);
  const long long n = t / 3;
  const int py = (y + 4) >> 1, px = (x + 4) >> 1;
  const int k = ((y & 1) * 2 + (x & 1)) * 3 + c;
  float acc = 0.f;
  for (int r = 0; r < 4; ++r) {
    const int h = py - r;
    if ((unsigned)h >= 112u) continue;
    for (int s = 0; s < 4; ++s) {
      const int w = px - s;
      if ((unsigned)w >= 112u) continue;
      const float4* g = reinterpret_cast<const float4*>(g_c1 + ((n * 112 + h) * 112 + w) * 64);
      const float* wp = wt + r * 64 + s * 16 + k;
#pragma unroll 4
      for (int c4 = 0; c4 < 16; ++c4) {
        const float4 gv = g[c4];
        acc = fmaf(gv.x, wp[(4 * c4) * 256], acc);
        acc = fmaf(gv.y, wp[(4 * c4 + 1) * 256], acc);
        acc = fmaf(gv.z, wp[(4 * c4 + 2) * 256], acc);
        acc = fmaf(gv.w, wp[(4 * c4 + 3) * 256], acc);
      }
    }
  }
  out[i] = acc * (c == 0 ? scale.v[0] : c == 1 ? scale.v[1] : scale.v[2]);
}

DgScale dg_scale(const float* scale) {
  DgScale s = {{1.f, 1.f, 1.f}};
  if (scale) for (int c = 0; c < 3; ++c) s.v[c] = scale[c];
  return s;
}

}  // namespace

// scale_kind 1: d(normalised value) / d(uint8 pixel value) = 1 / (255 std_c), the constants of pack_input_kernel
void vdqn_stem_pixel_scale(float* scale3) {
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int c = 0; c < 3; ++c) scale3[c] = 1.0f / (255.0f * stdv[c]);
}

// the f32 kernel on an existing g_c1 (engine, f32 / bf16x3 modes)
int vdqn_stem_dgrad_from_c1(const float* g_c1, const float* wt, const float* scale, float* out, int n_img, hipStream_t st) {
  const long long total = (long long)n_img * 3 * 224 * 224;
  ProfScope ps_("stem_input_grad<f32>", 2.0 * n_img * 112 * 112 * 64 * 147, (double)n_img * (112.0 * 112 * 64 * 4 + 3.0 * 224 * 224 * 4), st);
  hipLaunchKernelGGL(stem_dgrad_plain_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g_c1, wt, out, total, dg_scale(scale));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int64_t vdqn_stem_input_grad_workspace_bytes(int32_t n_img, int32_t dtype) {
  if (n_img <= 0 || (dtype != VDQN_BF16 && dtype != VDQN_F32 && dtype != VDQN_F32X3)) return -1;
  return dtype == VDQN_BF16 ? 0 : (int64_t)n_img * 112 * 112 * 64 * 4;
}

extern "C" int vdqn_stem_input_grad(const void* g_pool, const uint8_t* idx, const void* wt, const float* scale, float* out, int32_t n_img,
                                    int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  VDQN_CHECK(g_pool && idx && wt && out, "vdqn_stem_input_grad: null pointer");
  VDQN_CHECK(n_img > 0, "vdqn_stem_input_grad: n_img = %d", n_img);
  VDQN_CHECK(dtype == VDQN_BF16 || dtype == VDQN_F32 || dtype == VDQN_F32X3, "vdqn_stem_input_grad: bad dtype %d", dtype);
  VDQN_CHECK((((uintptr_t)g_pool | (uintptr_t)idx | (uintptr_t)wt | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0,
             "vdqn_stem_input_grad: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype != VDQN_BF16) {
    const int64_t need = vdqn_stem_input_grad_workspace_bytes(n_img, dtype);
    VDQN_CHECK(workspace && workspace_bytes >= need, "vdqn_stem_input_grad: workspace of %lld bytes, need %lld", (long long)workspace_bytes, (long long)need);
    RC(vdqn_maxpool_bwd(g_pool, idx, nullptr, workspace, n_img, 112, 112, 64, VDQN_F32, stream));
    return vdqn_stem_dgrad_from_c1((const float*)workspace, (const float*)wt, scale, out, n_img, st);
  }
  const long long gp_bytes = (long long)n_img * 56 * 56 * 128;
  VDQN_CHECK(gp_bytes < (1ll << 31), "vdqn_stem_input_grad: %d images exceed the 2 GiB range of the kernel's 32-bit buffer addressing (split the batch)", n_img);
  // blocks: ranges of an EVEN number of pooled rows of ONE image each, about two per CU in all; a range below the first costs two
  // steps of run-in, so at least 8 rows per block
  const int want = (2 * vdqn_num_cus() + n_img - 1) / n_img;
  const int bpi_max = want < 1 ? 1 : (want > 7 ? 7 : want);
  int ppb = (56 + bpi_max - 1) / bpi_max;
  ppb += ppb & 1;
  const int bpi = (56 + ppb - 1) / ppb;
  vdqn_ensure_dyn_smem(reinterpret_cast<const void*>(&stem_dgrad_kernel), (size_t)kDgSmem);
  ProfScope ps_("stem_input_grad<bf16>", 2.0 * n_img * 112 * 112 * 64 * 147, (double)n_img * (56.0 * 56 * 64 * 3 + 3.0 * 224 * 224 * 4) + 64.0 * 256 * 2, st);
  hipLaunchKernelGGL(stem_dgrad_kernel, dim3(n_img * bpi), dim3(256), kDgSmem, st, (const bf16raw*)g_pool, idx, (const bf16raw*)wt, out, ppb, bpi, (int)gp_bytes,
                     (int)(gp_bytes / 2), dg_scale(scale));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
