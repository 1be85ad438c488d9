// HBM-bound kernels of the hot path: input packing (normalise + space-to-depth), 3x3/2 max-pool forward and
// backward, and the fused Double-DQN target / TD-loss / dQ kernel.  (The optimiser, Adam included, is optim.hip.)
// All accesses are 16-byte vectors over the contiguous NHWC channel axis.
#include <math.h>

#include "block_sum.h"  // wave_partials / add_partials of the loss kernels (shared with iql.hip)
#include "common.h"
#include "pack_common.h"  // what pack_input_rows_kernel shares with the augmented pack (augment.hip)

namespace {

// ---------------------------------------------------------------------------------------------------------
// pack_input: 224x224x3 frame -> [115][115][16] space-to-depth operand of the 4x4/1 stem GEMM.
// dst pixel (y, x) holds source pixels (2(y-2)+bh, 2(x-2)+bw), channel (bh*2+bw)*3+c; channels 12..15 = 0.
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_input_kernel(const void* __restrict__ src, int src_kind, T* __restrict__ dst, int n_img) {
  const int total = n_img * 115 * 115;
  const float mean[3] = {0.485f, 0.456f, 0.406f};
  const float stdv[3] = {0.229f, 0.224f, 0.225f};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = i / (115 * 115);
    const int rem = i - n * (115 * 115);
    const int y = rem / 115, x = rem - y * 115;
    const int ys = y - 2, xs = x - 2;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
    if ((unsigned)ys < 112u && (unsigned)xs < 112u) {
#pragma unroll
      for (int bh = 0; bh < 2; ++bh)
#pragma unroll
        for (int bw = 0; bw < 2; ++bw) {
          const int Y = 2 * ys + bh, X = 2 * xs + bw;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float val;
            if (src_kind == 0) {
              const uint8_t u = ((const uint8_t*)src)[(((size_t)n * 224 + Y) * 224 + X) * 3 + c];
              val = (((float)u / 255.0f) - mean[c]) / stdv[c];
            } else {
              val = ((const float*)src)[(((size_t)n * 3 + c) * 224 + Y) * 224 + X];
            }
            v[(bh * 2 + bw) * 3 + c] = val;
          }
        }
    }
    T* d = dst + (size_t)i * 16;
    if constexpr (sizeof(T) == 2) {
      uint32_t w[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = (uint32_t)f32_to_bf16(v[2 * e]) | ((uint32_t)f32_to_bf16(v[2 * e + 1]) << 16);
      reinterpret_cast<uint4*>(d)[0] = make_uint4(w[0], w[1], w[2], w[3]);
      reinterpret_cast<uint4*>(d)[1] = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) reinterpret_cast<float4*>(d)[e] = make_float4(v[4 * e], v[4 * e + 1], v[4 * e + 2], v[4 * e + 3]);
    }
  }
}

// uint8 HWC source: a block walks kPackPairs pairs of packed rows; per pair the four source rows (672 bytes each) are read as 16-byte
// vectors into LDS and every thread builds one packed pixel from there.  The normalisation (u / 255 - mean) / std — two IEEE
// divisions per element, 24 per packed pixel: what bounded this kernel at 2.9 TB/s — is evaluated ONCE per block for the 3 x 256
// possible (channel, byte) pairs into an LDS table, with the same expression: same bits as the per-element arithmetic.
// (kPackPairs, the table entry and the store: pack_common.h, shared with the augmented pack of augment.hip.)
template <typename T>
__global__ __launch_bounds__(256) void pack_input_rows_kernel(const uint8_t* __restrict__ src, T* __restrict__ dst) {
  __shared__ uint4 rows[4][42];
  __shared__ T lut[3][256];
  const int n = blockIdx.y;
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < 3; ++c) lut[c][tid] = pack_norm_entry<T>(tid, c);
  const int yy = tid / 115, x = tid - yy * 115;
  for (int pr = 0; pr < kPackPairs; ++pr) {
    const int y0 = 2 * ((int)blockIdx.x * kPackPairs + pr);  // packed rows y0, y0 + 1 -> source rows 2 (y0 - 2) .. + 3
    if (y0 >= 115) break;
    const int Y0 = 2 * (y0 - 2);
    __syncthreads();  // the previous pair's readers are done (first pass: the table is written)
    if (tid < 168) {
      const int r = tid / 42, c = tid - r * 42, Y = Y0 + r;
      rows[r][c] = ((unsigned)Y < 224u) ? reinterpret_cast<const uint4*>(src + ((size_t)n * 224 + Y) * 672)[c] : make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const int y = y0 + yy;
    if (tid >= 230 || y >= 115) continue;
    const int ys = y - 2, xs = x - 2;
    __attribute__((aligned(16))) T v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = from_f32<T>(0.f);
    if ((unsigned)ys < 112u && (unsigned)xs < 112u) {
      const uint8_t* b0 = reinterpret_cast<const uint8_t*>(rows[2 * yy]) + 6 * xs;
      const uint8_t* b1 = reinterpret_cast<const uint8_t*>(rows[2 * yy + 1]) + 6 * xs;
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        v[e] = lut[e % 3][b0[e]];
        v[6 + e] = lut[e % 3][b1[e]];
      }
    }
    pack_store16(dst + ((size_t)n * 115 * 115 + (size_t)y * 115 + x) * 16, v);
  }
}

// ---------------------------------------------------------------------------------------------------------
// max-pool 3x3 / stride 2 / pad 1 (NHWC), first maximum wins (torch CPU semantics)
// ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ in, T* __restrict__ out, uint8_t* __restrict__ idx,
                                                          int n_img, int hi, int wi, int c) {
  constexpr int E16 = 16 / (int)sizeof(T);
  const int ho = (hi + 2 - 3) / 2 + 1, wo = (wi + 2 - 3) / 2 + 1;
  const int cg_n = c / E16;
  const long total = (long)n_img * ho * wo * cg_n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % cg_n);
    long t = i / cg_n;
    const int ow = (int)(t % wo);
    t /= wo;
    const int oh = (int)(t % ho);
    const int n = (int)(t / ho);
    float best[E16];
    uint8_t bi[E16];
#pragma unroll
    for (int e = 0; e < E16; ++e) {
      best[e] = -INFINITY;
      bi[e] = 0;
    }
    bool first = true;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int h = oh * 2 - 1 + kh;
      if ((unsigned)h >= (unsigned)hi) continue;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int w = ow * 2 - 1 + kw;
        if ((unsigned)w >= (unsigned)wi) continue;
        const uint4 v = *reinterpret_cast<const uint4*>(in + (((size_t)n * hi + h) * wi + w) * c + cg * E16);
        const T* pv = reinterpret_cast<const T*>(&v);
#pragma unroll
        for (int e = 0; e < E16; ++e) {
          const float f = to_f32<T>(pv[e]);
          if (first || f > best[e] || f != f) {
            best[e] = f;
            bi[e] = (uint8_t)(kh * 3 + kw);
          }
        }
        first = false;
      }
    }
    const size_t o = (((size_t)n * ho + oh) * wo + ow) * c + cg * E16;
    T ov[E16];
#pragma unroll
    for (int e = 0; e < E16; ++e) ov[e] = from_f32<T>(best[e]);
    *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<const uint4*>(ov);
    if constexpr (E16 == 8) *reinterpret_cast<uint2*>(idx + o) = *reinterpret_cast<const uint2*>(bi);
    else *reinterpret_cast<uint32_t*>(idx + o) = *reinterpret_cast<const uint32_t*>(bi);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const T* __restrict__ gy, const uint8_t* __restrict__ idx, const T* __restrict__ x,
                                                          T* __restrict__ gx, int n_img, int hi, int wi, int c) {
  constexpr int E16 = 16 / (int)sizeof(T);
  const int ho = (hi + 2 - 3) / 2 + 1, wo = (wi + 2 - 3) / 2 + 1;
  const int cg_n = c / E16;
  const long total = (long)n_img * hi * wi * cg_n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % cg_n);
    long t = i / cg_n;
    const int w = (int)(t % wi);
    t /= wi;
    const int h = (int)(t % hi);
    const int n = (int)(t / hi);
    float s[E16];
#pragma unroll
    for (int e = 0; e < E16; ++e) s[e] = 0.f;
    const int oh_lo = h / 2, oh_hi = min(ho - 1, (h + 1) / 2);
    const int ow_lo = w / 2, ow_hi = min(wo - 1, (w + 1) / 2);
    for (int oh = oh_lo; oh <= oh_hi; ++oh)
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int tap = (h - (2 * oh - 1)) * 3 + (w - (2 * ow - 1));
        const size_t o = (((size_t)n * ho + oh) * wo + ow) * c + cg * E16;
        const uint4 gv = *reinterpret_cast<const uint4*>(gy + o);
        const T* pg = reinterpret_cast<const T*>(&gv);
        uint8_t iv[E16];
        if constexpr (E16 == 8) *reinterpret_cast<uint2*>(iv) = *reinterpret_cast<const uint2*>(idx + o);
        else *reinterpret_cast<uint32_t*>(iv) = *reinterpret_cast<const uint32_t*>(idx + o);
#pragma unroll
        for (int e = 0; e < E16; ++e)
          if (iv[e] == tap) s[e] += to_f32<T>(pg[e]);
      }
    const size_t xo = (((size_t)n * hi + h) * wi + w) * c + cg * E16;
    T ov[E16];
    if (x) {
      const uint4 xv = *reinterpret_cast<const uint4*>(x + xo);
      const T* px = reinterpret_cast<const T*>(&xv);
#pragma unroll
      for (int e = 0; e < E16; ++e) ov[e] = from_f32<T>(to_f32<T>(px[e]) > 0.f ? s[e] : 0.f);
    } else {
#pragma unroll
      for (int e = 0; e < E16; ++e) ov[e] = from_f32<T>(s[e]);
    }
    *reinterpret_cast<uint4*>(gx + xo) = *reinterpret_cast<const uint4*>(ov);
  }
}

// Row-pair tiled variant (even input heights, c * sizeof(T) a multiple of 16): one block produces input rows 2k and 2k+1
// of one image.  Row 2k only receives from pooled row k (kh = 1), row 2k+1 from pooled rows k (kh = 2) and k+1 (kh = 0),
// so the block stages those two pooled rows of gy and idx in LDS once (each pooled element is then fetched from HBM/L2
// by two blocks instead of by 2.25 scattered gathers) and writes full 16-byte vectors of gx.
template <typename T>
__global__ __launch_bounds__(256) void maxpool_bwd_rows_kernel(const T* __restrict__ gy, const uint8_t* __restrict__ idx, const T* __restrict__ x,
                                                               T* __restrict__ gx, int hi, int wi, int c) {
  constexpr int E16 = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) unsigned char mp_smem[];
  const int ho = hi / 2, wo = wi / 2;
  const int cg_n = c / E16;
  const int n = blockIdx.y, k = blockIdx.x;
  const int rows = (k + 1 < ho) ? 2 : 1;          // pooled rows k (and k + 1)
  const int vec_row = wo * cg_n;                    // 16-byte gy vectors per pooled row
  uint4* sG = reinterpret_cast<uint4*>(mp_smem);    // [2][wo][cg_n] gy vectors
  uint8_t* sI = mp_smem + 2 * vec_row * 16;         // [2][wo][c] arg-max codes
  const size_t prow = ((size_t)n * ho + k) * wo;    // first pooled pixel of row k
  for (int i = threadIdx.x; i < rows * vec_row; i += 256) {
    sG[i] = reinterpret_cast<const uint4*>(gy + prow * c)[i];
    if constexpr (E16 == 8) reinterpret_cast<uint2*>(sI)[i] = reinterpret_cast<const uint2*>(idx + prow * c)[i];
    else reinterpret_cast<uint32_t*>(sI)[i] = reinterpret_cast<const uint32_t*>(idx + prow * c)[i];
  }
  __syncthreads();
  const int items = 2 * wi * cg_n;
  for (int it = threadIdx.x; it < items; it += 256) {
    const int cg = it % cg_n;
    const int t = it / cg_n;
    const int w = t % wi, hr = t / wi;              // hr = 0: row 2k, 1: row 2k + 1
    const int h = 2 * k + hr;
    float s[E16];
#pragma unroll
    for (int e = 0; e < E16; ++e) s[e] = 0.f;
    const int ow_lo = w / 2, ow_hi = min(wo - 1, (w + 1) / 2);
    const int pr_hi = hr == 0 ? 0 : rows - 1;       // pooled rows (relative to k) whose window holds h
    for (int pr = 0; pr <= pr_hi; ++pr) {
      const int kh = h - (2 * (k + pr) - 1);
      for (int ow = ow_lo; ow <= ow_hi; ++ow) {
        const int tap = kh * 3 + (w - (2 * ow - 1));
        const uint4 gv = sG[(pr * wo + ow) * cg_n + cg];
        const T* pg = reinterpret_cast<const T*>(&gv);
        const uint8_t* iv = sI + ((size_t)(pr * wo + ow) * cg_n + cg) * E16;
#pragma unroll
        for (int e = 0; e < E16; ++e)
          if (iv[e] == tap) s[e] += to_f32<T>(pg[e]);
      }
    }
    const size_t xo = (((size_t)n * hi + h) * wi + w) * c + cg * E16;
    T ov[E16];
    if (x) {
      const uint4 xv = *reinterpret_cast<const uint4*>(x + xo);
      const T* px = reinterpret_cast<const T*>(&xv);
#pragma unroll
      for (int e = 0; e < E16; ++e) ov[e] = from_f32<T>(to_f32<T>(px[e]) > 0.f ? s[e] : 0.f);
    } else {
#pragma unroll
      for (int e = 0; e < E16; ++e) ov[e] = from_f32<T>(s[e]);
    }
    *reinterpret_cast<uint4*>(gx + xo) = *reinterpret_cast<const uint4*>(ov);
  }
}

// ---------------------------------------------------------------------------------------------------------
// fused Double-DQN target + TD loss + dQ   (train_q_network.py:134-169,180)
// one thread per (sample, padded column); loss reduced per block, one atomic per block
// ---------------------------------------------------------------------------------------------------------
// d = Q(s)[b, col] - y for the taken action's column `col` of category c: the Double-DQN target (first arg-max of the online
// Q(s'), the target network's value there, terminal mask, LINEAR / gamma, rect clip).  The only statement of the target: the loss
// terms of every mode and the per-sample error take d from here.  `gamma` is the discount of sample b: a.gamma, or the sample's own
// (n-step returns: gamma^m of the m rows its chain walked, csrc/nstep.hip) in the instances with a per-sample discount.
// MC (the instances behind vdqn_td_loss_mc, 0 elsewhere: G is then not read): G is the Monte-Carlo return of (b, c)
// (csrc/mcreturn.hip); *raised = [G > y], taken before the floor, and with MC_FLOOR y = max(y, G) in front of the rect clip — the
// clip keeps the last word, so a floored target stays inside [0, 1] like every other.
enum { MC_FLOOR = 1, MC_CALIBRATED = 2 };
template <int MC = 0>
__device__ __forceinline__ float td_error_of(const vdqn_td_args& a, int b, int c, int col, float gamma, float G = 0.f, bool* raised = nullptr) {
  const float qb = a.q_before[(size_t)b * a.ldq + col];
  const float* qo = a.q_after_online + (size_t)b * a.ldq + c * a.n_act;
  int best = 0;
  float bv = qo[0];
  for (int k = 1; k < a.n_act; ++k) {
    const float v = qo[k];
    if (v > bv) {  // strict: first maximum wins (torch.argmax)
      bv = v;
      best = k;
    }
  }
  float qa = a.q_after_target[(size_t)b * a.ldq + c * a.n_act + best];
  qa = qa * (1.0f - a.term[b * a.n_cat + c]);
  const float r = a.rew[b * a.n_cat + c];
  float y = a.linear ? r + (qa - 0.1f) : r + gamma * qa;
  if constexpr (MC != 0) {
    if (raised) *raised = G > y;
    if constexpr ((MC & MC_FLOOR) != 0) y = fmaxf(y, G);
  }
  if (a.clip_rect) y = fminf(fmaxf(y, 0.f), 1.f);
  return qb - y;
}

// One kernel for the three entries, MODE chosen at compile time (a run-time flag would put the other modes' loads and registers
// into every instance).  For sample b and category c, with d = td_error_of, l(d) / dl(d) the half squared error and d, or Huber
// with beta 1 and its clamp (loss kinds 0 / 1), vm_bc = valid or 1, and a* = act[b]:
//   TD_PLAIN (vdqn_td_loss)             loss += l * vm                dq[b, c*A+a*] = dl * vm * inv_count
//   TD_WEIGHTED (vdqn_td_loss_weighted) loss += (l * w_b) * vm        dq[b, c*A+a*] = (dl * w_b) * vm * inv_count
//     w_b is applied before vm, so w = 1 leaves every rounding of TD_PLAIN as it is.  The thread of column 0 writes
//     err[b] = sum_c |d_bc| * vm_bc / n_cat (the raw TD error, whatever the loss kind).
//   TD_CQL (vdqn_td_loss_cql): the discrete conservative Q-learning penalty (Kumar et al., NeurIPS 2020) for training from logged
//     data only, on top of the loss of train_q_network.py:167,180.  With q = q_before[b, c*A .. c*A+A) in f32:
//       m      = max_a q_a          sum = sum_a expf(q_a - m)  (a = 0 .. A-1, in that order)          p_a = expf(q_a - m) / sum
//       pen_bc = logf(sum) + (m - q_{a*})    == logsumexp_a q_a - q_{a*}; the max is subtracted before anything is exponentiated, and
//                m - q_{a*} is taken before the logarithm is added, so a row such as [1e4, -1e4, 0] loses nothing to the size of m
//       s_bc   = w_b * vm_bc                                  (w_b = 1 without weights)
//       loss    += s_bc * (l(d_bc) + alpha * pen_bc)          penalty += s_bc * pen_bc           (not scaled by alpha)
//       dq[b, c*A+a] = (([a == a*] ? dl(d_bc) : 0) + alpha * (p_a - [a == a*])) * s_bc * inv_count
//     so dq is dense over the actions of every category, where the other two modes write one column per category.  Each thread of
//     a category recomputes that category's m and sum from A loads (A is 3 here; the row is in cache), and the thread of the taken
//     action adds the loss terms.  err[b] stays the raw mean |d| (priorities follow the TD error, not the penalty).
// The block's sums are multiplied by inv_count and added to a.loss (a.penalty) with one atomic each; padding columns of dq are 0.
// SG (vdqn_td_loss_nstep), also chosen at compile time: the discount of sample b is a.sg[b] where the other instances take a.gamma —
// one more load per taken-action thread, nothing else; with sg[b] == gamma for every b the instance writes the bits of its SG = false
// twin, and a row depends on its own sample's discount only.
// MC (vdqn_td_loss_mc), chosen at compile time like MODE and SG; 0 in every instance behind the other entries, which read neither
// a.mc nor a.mc_stats.  G_bc = a.mc[b][c] is the discounted return the logged data obtained from the sampled row (csrc/mcreturn.hip):
//   MC_FLOOR       y = max(y, G_bc) inside td_error_of, before the rect clip; err[b] follows the floored error.
//   MC_CALIBRATED  (TD_CQL only; Cal-QL, Nakamoto et al., NeurIPS 2023) the penalty's logsumexp runs over qc_a = max(q_a, G_bc):
//                  m = max_a qc_a, sum = sum_a expf(qc_a - m), p_a = expf(qc_a - m) / sum, pen_bc = logf(sum) + (m - q_{a*}) with the
//                  RAW q_{a*}, and the penalty's part of dq is alpha * (p_a * [q_a >= G_bc] - [a == a*]): where G_bc is the larger
//                  the term is a constant and carries no gradient; at a tie q_a == G_bc the Q value takes it.
//   a.mc_stats (f32[2] or NULL), summed and added like the loss, vm_bc = valid or 1 (no importance weight):
//                  [0] += vm_bc * [G_bc > y before the floor]      [1] += vm_bc * (q_{a*} - G_bc)
// With G = -inf max(x, G) == x, [q >= G] holds and [G > y] does not: every MC instance then writes the bits of its MC = 0 twin.
// Launch shapes: 256 threads and one element per thread.  A deterministic launch is ONE block that walks all elements (thread t
// takes t, t + blockDim.x, ..; the block sum's fixed order): 256 threads for TD_PLAIN and TD_WEIGHTED, 1024 for TD_CQL — a quarter of
// the serial passes.  __launch_bounds__(1024) is there for that launch alone, and it budgets the TD_CQL instances' 256-thread
// launches too: 128 VGPRs per thread.  They take 38 (the MC instances: DESIGN.md 3o); should they grow, they have to stay under that.
enum { TD_PLAIN = 0, TD_WEIGHTED = 1, TD_CQL = 2 };
struct td_kernel_args : vdqn_td_args {
  const float* w;  // [batch]; TD_CQL: or NULL (= 1)
  float* err;      // [batch] or NULL
  float* penalty;  // TD_CQL: f32 scalar or NULL
  float alpha;     // TD_CQL
  const float* sg;  // SG: [batch] per-sample discount
  const float* mc;  // MC: [batch][n_cat] Monte-Carlo returns
  float* mc_stats;  // MC: f32[2] or NULL
};
template <typename T, int MODE, bool SG, int MC>
__global__ __launch_bounds__(MODE == TD_CQL ? 1024 : 256) void td_loss_kernel(const td_kernel_args a) {
  static_assert(MC >= 0 && MC <= 3 && (MODE == TD_CQL || (MC & MC_CALIBRATED) == 0), "MC_CALIBRATED belongs to TD_CQL");
  const int total = a.batch * a.ldq;
  constexpr int N_LOSS = MODE == TD_CQL ? 2 : 1;
  constexpr int N_SUMS = N_LOSS + (MC != 0 ? 2 : 0);
  float sums[N_SUMS] = {};  // this thread's loss terms (TD_CQL: and penalty terms; MC: and the two mc_stats terms)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / a.ldq, col = i - b * a.ldq;
    float g = 0.f;
    if (col < a.n_cat * a.n_act) {
      const int c = col / a.n_act, ac = col - c * a.n_act;
      const int act = (int)a.act[b];
      const float* q = a.q_before + (size_t)b * a.ldq + c * a.n_act;
      if (a.q_copy) a.q_copy[(size_t)b * (a.n_cat * a.n_act) + col] = q[ac];
      float m = 0.f, sum = 0.f, p = 0.f, s = 0.f;  // TD_CQL only
      float G = 0.f;                               // MC only
      if constexpr (MC != 0) G = a.mc[b * a.n_cat + c];
      if constexpr (MODE == TD_CQL) {
        if constexpr ((MC & MC_CALIBRATED) != 0) {
          m = fmaxf(q[0], G);
          for (int k = 1; k < a.n_act; ++k) m = fmaxf(m, fmaxf(q[k], G));
          for (int k = 0; k < a.n_act; ++k) sum += expf(fmaxf(q[k], G) - m);
          p = expf(fmaxf(q[ac], G) - m) / sum;
          if (!(q[ac] >= G)) p = 0.f;  // (p is from here on the gradient's share alone: the penalty itself is logf(sum) + ...)
        } else {
          m = q[0];
          for (int k = 1; k < a.n_act; ++k) m = fmaxf(m, q[k]);
          for (int k = 0; k < a.n_act; ++k) sum += expf(q[k] - m);
          p = expf(q[ac] - m) / sum;
        }
        s = (a.w ? a.w[b] : 1.0f) * (a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f);
        g = a.alpha * p;
      }
      if (ac == act) {
        bool raised = false;
        const float d = td_error_of<MC>(a, b, c, col, SG ? a.sg[b] : a.gamma, G, &raised);
        if constexpr (MC != 0) {
          const float vs = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
          sums[N_LOSS] += raised ? vs : 0.f;
          sums[N_LOSS + 1] += vs * (q[ac] - G);
        }
        float l, dl;
        if (a.loss_kind == 1) {  // Huber, beta = 1 (torch.nn.functional.smooth_l1_loss)
          const float ad = fabsf(d);
          l = ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
          dl = fminf(fmaxf(d, -1.0f), 1.0f);
        } else {
          l = 0.5f * d * d;
          dl = d;
        }
        if constexpr (MODE == TD_CQL) {
          const float pen = logf(sum) + (m - q[ac]);
          sums[0] += s * (l + a.alpha * pen);
          sums[1] += s * pen;
          g = dl + a.alpha * (p - 1.0f);
        } else {
          const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
          if constexpr (MODE == TD_WEIGHTED) {
            l *= a.w[b];
            dl *= a.w[b];
          }
          sums[0] += l * vm;
          g = dl * vm * a.inv_count;
        }
      }
      if constexpr (MODE == TD_CQL) g = g * s * a.inv_count;
    }
    if constexpr (MODE != TD_PLAIN) {
      if (col == 0 && a.err) {
        float e = 0.f;
        for (int c = 0; c < a.n_cat; ++c)
          e += fabsf(td_error_of<MC>(a, b, c, c * a.n_act + (int)a.act[b], SG ? a.sg[b] : a.gamma, MC != 0 ? a.mc[b * a.n_cat + c] : 0.f)) *
               (a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f);
        a.err[b] = e / (float)a.n_cat;
      }
    }
    if (a.dq) ((T*)a.dq)[i] = from_f32<T>(g);
    if (a.dq_f32) a.dq_f32[i] = g;
  }
  __shared__ float red[N_SUMS][16];
  wave_partials(sums, red);
  if (threadIdx.x == 0) {
    add_partials(red, MODE == TD_CQL ? (int)(blockDim.x >> 6) : 4, sums);
    if (sums[0] != 0.f) atomicAdd(a.loss, sums[0] * a.inv_count);
    if constexpr (MODE == TD_CQL) {
      if (a.penalty && sums[1] != 0.f) atomicAdd(a.penalty, sums[1] * a.inv_count);
    }
    if constexpr (MC != 0) {
      if (a.mc_stats && sums[N_LOSS] != 0.f) atomicAdd(a.mc_stats, sums[N_LOSS] * a.inv_count);
      if (a.mc_stats && sums[N_LOSS + 1] != 0.f) atomicAdd(a.mc_stats + 1, sums[N_LOSS + 1] * a.inv_count);
    }
  }
}

// ground-truth branch (train_q_network.py:170-178)
template <typename T>
__global__ __launch_bounds__(256) void gt_loss_kernel(const float* __restrict__ q_before, const int64_t* __restrict__ act,
                                                      const float* __restrict__ gt, float* loss, T* dq, float* dq_f32, int batch,
                                                      int n_cat, int n_act, int ldq, float inv_count, int value_learning) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = batch * ldq;
  float my_loss = 0.f;
  if (i < total) {
    const int b = i / ldq, col = i - b * ldq;
    float g = 0.f;
    if (col < n_cat * n_act) {
      const int c = col / n_act, ac = col - c * n_act;
      if (ac == (int)act[b]) {
        const float qb = q_before[(size_t)b * ldq + col];
        const float t = gt[b * n_cat + c];
        if (value_learning) {
          const bool nan = t != t;
          const float mask = nan ? 0.f : 1.f;
          const float d = qb * mask - (nan ? 0.f : t);
          my_loss = 0.5f * d * d;
          g = d * mask * inv_count;
        } else {
          const float d = qb - t;
          my_loss = 0.5f * d * d;
          g = d * inv_count;
        }
      }
    }
    if (dq) dq[i] = from_f32<T>(g);
    if (dq_f32) dq_f32[i] = g;
  }
  __shared__ float red[1][16];
  float sum[1] = {my_loss};
  wave_partials(sum, red);
  if (threadIdx.x == 0) {
    add_partials(red, 4, sum);
    atomicAdd(loss, sum[0] * inv_count);
  }
}

inline int grid_for(long total, int cap = 8192) {
  long b = (total + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" int vdqn_pack_input(const void* src, int32_t src_kind, void* dst, int32_t n_img, int32_t dtype, void* stream) {
  VDQN_CHECK(src && dst && n_img > 0, "vdqn_pack_input: bad args");
  VDQN_CHECK(src_kind == 0 || src_kind == 1, "vdqn_pack_input: src_kind %d", src_kind);
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_pack_input: bad dtype");
  const int g = grid_for((long)n_img * 115 * 115);
  ProfScope ps_("pack_input", 0.0, (double)n_img * (224.0 * 224 * 3 * (src_kind == 0 ? 1 : 4) + 115.0 * 115 * 16 * (dtype == VDQN_BF16 ? 2 : 4)), (hipStream_t)stream);
  if (src_kind == 0 && n_img <= 65535 && (((uintptr_t)src) & 15) == 0) {  // frames are 150528 = 16 * 9408 bytes: every source row is 16-byte aligned
    if (dtype == VDQN_BF16) hipLaunchKernelGGL((pack_input_rows_kernel<bf16raw>), pack_rows_grid(n_img), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (bf16raw*)dst);
    else hipLaunchKernelGGL((pack_input_rows_kernel<float>), pack_rows_grid(n_img), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src, (float*)dst);
    VDQN_LAUNCH_CHECK();
    return VDQN_OK;
  }
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((pack_input_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, src, src_kind, (bf16raw*)dst, n_img);
  else hipLaunchKernelGGL((pack_input_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, src, src_kind, (float*)dst, n_img);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_maxpool_fwd(const void* in, void* out, uint8_t* idx, int32_t n_img, int32_t hi, int32_t wi, int32_t c, int32_t dtype,
                                void* stream) {
  VDQN_CHECK(in && out && idx && n_img > 0, "vdqn_maxpool_fwd: bad args");
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_maxpool_fwd: bad dtype");
  VDQN_CHECK(c % 8 == 0, "vdqn_maxpool_fwd: channels must be a multiple of 8");
  const int ho = (hi - 1) / 2 + 1, wo = (wi - 1) / 2 + 1;
  const int e16 = dtype == VDQN_BF16 ? 8 : 4;
  const int g = grid_for((long)n_img * ho * wo * (c / e16), 65536);
  ProfScope ps_("maxpool_fwd", 0.0, (double)n_img * c * ((double)hi * wi * (16 / e16) + (double)ho * wo * (16 / e16 + 1)), (hipStream_t)stream);
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((maxpool_fwd_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16raw*)in, (bf16raw*)out, idx, n_img, hi, wi, c);
  else hipLaunchKernelGGL((maxpool_fwd_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)in, (float*)out, idx, n_img, hi, wi, c);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_maxpool_bwd(const void* gy, const uint8_t* idx, const void* x, void* gx, int32_t n_img, int32_t hi, int32_t wi,
                                int32_t c, int32_t dtype, void* stream) {
  VDQN_CHECK(gy && idx && gx && n_img > 0, "vdqn_maxpool_bwd: bad args");
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_maxpool_bwd: bad dtype");
  VDQN_CHECK(c % 8 == 0, "vdqn_maxpool_bwd: channels must be a multiple of 8");
  const int e16 = dtype == VDQN_BF16 ? 8 : 4;
  const int g = grid_for((long)n_img * hi * wi * (c / e16), 65536);
  ProfScope ps_("maxpool_bwd", 0.0, (double)n_img * c * ((x ? 2.0 : 1.0) * hi * wi * (16 / e16) + (double)(hi / 2) * (wi / 2) * (16 / e16 + 1)), (hipStream_t)stream);
  const size_t rows_smem = (size_t)2 * (wi / 2) * c * ((dtype == VDQN_BF16 ? 2 : 4) + 1);
  if (hi % 2 == 0 && wi % 2 == 0 && n_img <= 65535 && rows_smem <= 64 * 1024) {  // row-pair tiles (the 112 x 112 x 64 stem gradient)
    if (dtype == VDQN_BF16)
      hipLaunchKernelGGL((maxpool_bwd_rows_kernel<bf16raw>), dim3(hi / 2, n_img), dim3(256), rows_smem, (hipStream_t)stream, (const bf16raw*)gy, idx, (const bf16raw*)x, (bf16raw*)gx, hi, wi, c);
    else
      hipLaunchKernelGGL((maxpool_bwd_rows_kernel<float>), dim3(hi / 2, n_img), dim3(256), rows_smem, (hipStream_t)stream, (const float*)gy, idx, (const float*)x, (float*)gx, hi, wi, c);
    VDQN_LAUNCH_CHECK();
    return VDQN_OK;
  }
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((maxpool_bwd_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16raw*)gy, idx, (const bf16raw*)x, (bf16raw*)gx, n_img, hi, wi, c);
  else hipLaunchKernelGGL((maxpool_bwd_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)gy, idx, (const float*)x, (float*)gx, n_img, hi, wi, c);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

__global__ void softmax_rows_kernel(const float* __restrict__ x, float* __restrict__ y, int rows, int ld, int n_valid) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float m = -INFINITY;
  for (int j = 0; j < n_valid; ++j) m = fmaxf(m, x[(size_t)r * ld + j]);
  float sum = 0.f;
  for (int j = 0; j < n_valid; ++j) sum += expf(x[(size_t)r * ld + j] - m);
  for (int j = 0; j < ld; ++j) y[(size_t)r * ld + j] = j < n_valid ? expf(x[(size_t)r * ld + j] - m) / sum : 0.f;
}

extern "C" int vdqn_softmax_rows(const float* x, float* y, int32_t rows, int32_t ld, int32_t n_valid, void* stream) {
  VDQN_CHECK(x && y && rows > 0 && ld > 0 && n_valid > 0 && n_valid <= ld && n_valid <= 64, "vdqn_softmax_rows: bad args");
  hipLaunchKernelGGL(softmax_rows_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, x, y, rows, ld, n_valid);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// mean cross-entropy over rows of logits[rows][ld] (first n_cls columns) against int64 labels, and its gradient
// (softmax - onehot) * inv_count written as T into dlogits[rows][ld] (columns >= n_cls zero): nn.CrossEntropyLoss()
// of train_inverse_model.py:103-104 and its backward
template <typename T>
__global__ void softmax_ce_kernel(const float* __restrict__ x, const int64_t* __restrict__ label, float* __restrict__ loss, T* __restrict__ dx,
                                  int rows, int ld, int n_cls, float inv_count) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  float my = 0.f;
  if (r < rows) {
    float m = -INFINITY;
    for (int j = 0; j < n_cls; ++j) m = fmaxf(m, x[(size_t)r * ld + j]);
    float sum = 0.f;
    for (int j = 0; j < n_cls; ++j) sum += expf(x[(size_t)r * ld + j] - m);
    const int lab = (int)label[r];
    my = (logf(sum) + m - x[(size_t)r * ld + lab]) * inv_count;
    for (int j = 0; j < ld; ++j) {
      float g = 0.f;
      if (j < n_cls) g = (expf(x[(size_t)r * ld + j] - m) / sum - (j == lab ? 1.f : 0.f)) * inv_count;
      dx[(size_t)r * ld + j] = from_f32<T>(g);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) my += __shfl_down(my, o, 64);
  if ((threadIdx.x & 63) == 0 && my != 0.f) atomicAdd(loss, my);
}

// out = x * mask * scale (dropout forward and backward with a caller-supplied 0/1 mask of the same dtype)
template <typename T>
__global__ void mask_scale_kernel(const T* __restrict__ x, const T* __restrict__ mask, T* __restrict__ out, long n, float scale) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = from_f32<T>(to_f32<T>(x[i]) * to_f32<T>(mask[i]) * scale);
}

__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float alpha, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] += alpha * x[i];
}

extern "C" int vdqn_softmax_ce(const float* logits, const int64_t* labels, float* loss, void* dlogits, int32_t rows, int32_t ld, int32_t n_cls,
                               float inv_count, int32_t dtype, void* stream) {
  VDQN_CHECK(logits && labels && loss && dlogits && rows > 0 && n_cls > 0 && n_cls <= ld, "vdqn_softmax_ce: bad args");
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_softmax_ce: bad dtype");
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((softmax_ce_kernel<bf16raw>), dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, logits, labels, loss, (bf16raw*)dlogits, rows, ld, n_cls, inv_count);
  else hipLaunchKernelGGL((softmax_ce_kernel<float>), dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, logits, labels, loss, (float*)dlogits, rows, ld, n_cls, inv_count);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_mask_scale(const void* x, const void* mask, void* out, int64_t n, float scale, int32_t dtype, void* stream) {
  VDQN_CHECK(x && mask && out && n > 0, "vdqn_mask_scale: bad args");
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_mask_scale: bad dtype");
  const int g = grid_for(n, 4096);
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((mask_scale_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const bf16raw*)x, (const bf16raw*)mask, (bf16raw*)out, (long)n, scale);
  else hipLaunchKernelGGL((mask_scale_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, (const float*)x, (const float*)mask, (float*)out, (long)n, scale);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_axpy(float* y, const float* x, float alpha, int64_t n, void* stream) {
  VDQN_CHECK(y && x && n > 0, "vdqn_axpy: bad args");
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n, 4096)), dim3(256), 0, (hipStream_t)stream, y, x, alpha, (long)n);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// The TD-loss entries: every check (each fails by the entry's name before any HIP call), then the one launch.  sample_gamma != NULL
// (vdqn_td_loss_nstep, vdqn_td_loss_mc) selects the instances with a per-sample discount, mc_flags != 0 (vdqn_td_loss_mc only)
// those with the Monte-Carlo return: MC_CALIBRATED is instantiated for TD_CQL alone.
template <int MODE, int MC>
static void td_loss_launch_instance(int dtype, bool sg, int g, int threads, hipStream_t st, const td_kernel_args& k) {
  if (sg) {
    if (dtype == VDQN_BF16) hipLaunchKernelGGL((td_loss_kernel<bf16raw, MODE, true, MC>), dim3(g), dim3(threads), 0, st, k);
    else hipLaunchKernelGGL((td_loss_kernel<float, MODE, true, MC>), dim3(g), dim3(threads), 0, st, k);
  } else {
    if (dtype == VDQN_BF16) hipLaunchKernelGGL((td_loss_kernel<bf16raw, MODE, false, MC>), dim3(g), dim3(threads), 0, st, k);
    else hipLaunchKernelGGL((td_loss_kernel<float, MODE, false, MC>), dim3(g), dim3(threads), 0, st, k);
  }
}
template <int MODE>
static int td_loss_launch(const char* entry, const char* prof_name, const vdqn_td_args* a, const float* weight, float* err_out, float cql_alpha,
                          float* penalty, const float* sample_gamma, void* stream, const float* mc_return = nullptr, int mc_flags = 0,
                          float* mc_stats = nullptr) {
  VDQN_CHECK(a && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term && a->loss && (MODE != TD_WEIGHTED || weight),
             "%s: null arg", entry);
  VDQN_CHECK(!a->use_valid || a->valid, "%s: use_valid without valid mask", entry);
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq >= a->n_cat * a->n_act, "%s: bad dims", entry);
  if (MODE == TD_CQL) VDQN_CHECK(a->n_act >= 2, "%s: n_act is 1: with one action logsumexp_a Q - Q(a) is identically zero; use vdqn_td_loss", entry);
  VDQN_CHECK(a->dtype == VDQN_F32 || a->dtype == VDQN_BF16, "%s: bad dtype", entry);
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "%s: loss_kind %d (0 = half squared error, 1 = Huber)", entry, a->loss_kind);
  VDQN_CHECK(!sample_gamma || !a->linear, "%s: linear with a per-sample discount: y = r + (Qa - 0.1) has no discount and no n-step form", entry);
  if (MODE == TD_CQL)
    VDQN_CHECK(isfinite(cql_alpha) && cql_alpha > 0.f, "%s: cql_alpha %g must be finite and > 0 (without the penalty: vdqn_td_loss)", entry, (double)cql_alpha);
  VDQN_CHECK(MODE == TD_CQL || !(mc_flags & MC_CALIBRATED), "%s: mc_flags %d: the calibrated penalty needs cql_alpha > 0", entry, mc_flags);
  const int threads = MODE == TD_CQL && a->deterministic ? 1024 : 256;
  const int g = a->deterministic ? 1 : (a->batch * a->ldq + 255) / 256;
  ProfScope ps_(prof_name, 0.0, (double)a->batch * a->ldq * 16.0 + (MODE == TD_PLAIN ? 0.0 : (double)a->batch * 8.0), (hipStream_t)stream);
  td_kernel_args k;
  static_cast<vdqn_td_args&>(k) = *a;
  k.w = weight;
  k.err = err_out;
  k.penalty = penalty;
  k.alpha = cql_alpha;
  k.sg = sample_gamma;
  k.mc = mc_return;
  k.mc_stats = mc_stats;
  const bool sg = sample_gamma != nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (mc_flags == 0) td_loss_launch_instance<MODE, 0>(a->dtype, sg, g, threads, st, k);
  else if (mc_flags == MC_FLOOR) td_loss_launch_instance<MODE, MC_FLOOR>(a->dtype, sg, g, threads, st, k);
  else if constexpr (MODE == TD_CQL) {
    if (mc_flags == MC_CALIBRATED) td_loss_launch_instance<MODE, MC_CALIBRATED>(a->dtype, sg, g, threads, st, k);
    else td_loss_launch_instance<MODE, MC_FLOOR | MC_CALIBRATED>(a->dtype, sg, g, threads, st, k);
  }
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_td_loss(const vdqn_td_args* a, void* stream) {
  return td_loss_launch<TD_PLAIN>("vdqn_td_loss", "td_loss", a, nullptr, nullptr, 0.f, nullptr, nullptr, stream);
}

extern "C" int vdqn_td_loss_weighted(const vdqn_td_args* a, const float* weight, float* err_out, void* stream) {
  return td_loss_launch<TD_WEIGHTED>("vdqn_td_loss_weighted", "td_loss_w", a, weight, err_out, 0.f, nullptr, nullptr, stream);
}

extern "C" int vdqn_td_loss_cql(const vdqn_td_args* a, const float* weight, float* err_out, float cql_alpha, float* penalty, void* stream) {
  return td_loss_launch<TD_CQL>("vdqn_td_loss_cql", "td_loss_cql", a, weight, err_out, cql_alpha, penalty, nullptr, stream);
}

// The three modes with a per-sample discount (n-step returns): cql_alpha > 0 is vdqn_td_loss_cql, else weight != NULL is
// vdqn_td_loss_weighted, else vdqn_td_loss — each with sample_gamma[b] where it takes a->gamma, which is not read.
extern "C" int vdqn_td_loss_nstep(const vdqn_td_args* a, const float* weight, float* err_out, float cql_alpha, float* penalty,
                                  const float* sample_gamma, void* stream) {
  VDQN_CHECK(sample_gamma, "vdqn_td_loss_nstep: sample_gamma is NULL (the scalar discount: vdqn_td_loss, vdqn_td_loss_weighted, vdqn_td_loss_cql)");
  VDQN_CHECK(isfinite(cql_alpha) && cql_alpha >= 0.f, "vdqn_td_loss_nstep: cql_alpha %g must be finite and >= 0 (0 = no penalty)", (double)cql_alpha);
  if (cql_alpha > 0.f) return td_loss_launch<TD_CQL>("vdqn_td_loss_nstep", "td_loss_cql", a, weight, err_out, cql_alpha, penalty, sample_gamma, stream);
  VDQN_CHECK(!penalty, "vdqn_td_loss_nstep: penalty is given, but cql_alpha is 0");
  VDQN_CHECK(weight || !err_out, "vdqn_td_loss_nstep: err_out without weight (the unweighted launch writes no per-sample errors)");
  if (weight) return td_loss_launch<TD_WEIGHTED>("vdqn_td_loss_nstep", "td_loss_w", a, weight, err_out, 0.f, nullptr, sample_gamma, stream);
  return td_loss_launch<TD_PLAIN>("vdqn_td_loss_nstep", "td_loss", a, nullptr, nullptr, 0.f, nullptr, sample_gamma, stream);
}

// The entries above with the Monte-Carlo return of every sampled row (csrc/mcreturn.hip): the mode is chosen as vdqn_td_loss_nstep
// chooses it, sample_gamma may be NULL (the scalar a->gamma).
extern "C" int vdqn_td_loss_mc(const vdqn_td_args* a, const float* weight, float* err_out, float cql_alpha, float* penalty, const float* sample_gamma,
                               const float* mc_return, int32_t mc_flags, float* mc_stats, void* stream) {
  VDQN_CHECK(a, "vdqn_td_loss_mc: null arg");
  VDQN_CHECK(mc_return, "vdqn_td_loss_mc: mc_return is NULL (without the return table: vdqn_td_loss, _weighted, _cql, _nstep)");
  VDQN_CHECK((mc_flags & ~(MC_FLOOR | MC_CALIBRATED)) == 0, "vdqn_td_loss_mc: mc_flags 0x%x has unknown bits (bit 0 = floor, bit 1 = calibrated)", (unsigned)mc_flags);
  VDQN_CHECK(mc_flags != 0, "vdqn_td_loss_mc: mc_flags is 0: at least one of bit 0 (floor) and bit 1 (calibrated) must be set");
  VDQN_CHECK(isfinite(cql_alpha) && cql_alpha >= 0.f, "vdqn_td_loss_mc: cql_alpha %g must be finite and >= 0 (0 = no penalty)", (double)cql_alpha);
  VDQN_CHECK(!(mc_flags & MC_CALIBRATED) || cql_alpha > 0.f, "vdqn_td_loss_mc: mc_flags bit 1 (calibrated) needs cql_alpha > 0: there is no penalty to calibrate");
  VDQN_CHECK(!a->linear, "vdqn_td_loss_mc: linear: y = r + (Qa - 0.1) has no discount, and a discounted return bounds nothing of it");
  if (cql_alpha > 0.f)
    return td_loss_launch<TD_CQL>("vdqn_td_loss_mc", "td_loss_cql_mc", a, weight, err_out, cql_alpha, penalty, sample_gamma, stream, mc_return, mc_flags, mc_stats);
  VDQN_CHECK(!penalty, "vdqn_td_loss_mc: penalty is given, but cql_alpha is 0");
  VDQN_CHECK(weight || !err_out, "vdqn_td_loss_mc: err_out without weight (the unweighted launch writes no per-sample errors)");
  if (weight) return td_loss_launch<TD_WEIGHTED>("vdqn_td_loss_mc", "td_loss_w_mc", a, weight, err_out, 0.f, nullptr, sample_gamma, stream, mc_return, mc_flags, mc_stats);
  return td_loss_launch<TD_PLAIN>("vdqn_td_loss_mc", "td_loss_mc", a, nullptr, nullptr, 0.f, nullptr, sample_gamma, stream, mc_return, mc_flags, mc_stats);
}

extern "C" int vdqn_gt_loss(const float* q_before, const int64_t* act, const float* gt, float* loss, void* dq, float* dq_f32, int32_t batch,
                            int32_t n_cat, int32_t n_act, int32_t ldq, float inv_count, int32_t value_learning, int32_t dtype, void* stream) {
  VDQN_CHECK(q_before && act && gt && loss, "vdqn_gt_loss: null arg");
  VDQN_CHECK(batch > 0 && ldq >= n_cat * n_act, "vdqn_gt_loss: bad dims");
  VDQN_CHECK(dtype == VDQN_F32 || dtype == VDQN_BF16, "vdqn_gt_loss: bad dtype");
  const int g = (batch * ldq + 255) / 256;
  ProfScope ps_("gt_loss", 0.0, (double)batch * ldq * 8.0, (hipStream_t)stream);
  if (dtype == VDQN_BF16) hipLaunchKernelGGL((gt_loss_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, q_before, act, gt, loss, (bf16raw*)dq, dq_f32, batch, n_cat, n_act, ldq, inv_count, value_learning);
  else hipLaunchKernelGGL((gt_loss_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, q_before, act, gt, loss, (float*)dq, dq_f32, batch, n_cat, n_act, ldq, inv_count, value_learning);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
