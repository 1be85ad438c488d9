// BatchNorm-eval fold / weight packing, the gradient unfold, and the dL/dQ pad: the kernels that move between the master
// (OIHW, f32) parameters and the packed operands of the convolution kernels, and their launchers.
//
// BatchNorm-eval is folded into the packed weights:  y = conv(x, W * s) + (beta - mean * s),  s = gamma * rstd.
// Its parameter gradients need no saved conv output:  with dW' = dL/d(W*s) (what the wgrad kernel produces)
//   dL/dW = dW' * s,   dL/dbeta = sum(gy),   dL/dgamma = rstd * ( <dW'[co,:], W[co,:]> - mean * dL/dbeta ).
#include "engine_net.h"

namespace {

// ---------------------------------------------------------------------------------------------------------
// fold / unfold kernels
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long fold_src_index(const FoldDesc& d, int co, int k) {
  if (d.kind == K_CONV1_S2D) {
    const int a = k >> 6, j = (k >> 4) & 3, ch = k & 15;
    if (ch >= 12) return -1;
    const int bh = ch / 6, bw = (ch / 3) & 1, c = ch % 3;
    const int r7 = 2 * a + bh - 1, s7 = 2 * j + bw - 1;
    if (r7 < 0 || s7 < 0) return -1;
    return ((long)(co * 3 + c) * 7 + r7) * 7 + s7;
  } else if (d.kind == K_LINEAR_PERM) {
    const int f = k / 1600, rem = k - f * 1600;
    const int hw = rem >> 6, c = rem & 63;
    return (long)co * d.ci + f * 1600 + c * 25 + hw;
  } else {
    const int tap = k / d.k_ci, c = k - tap * d.k_ci;
    const int kr = tap / d.k_s, ks = tap - kr * d.k_s;
    return (((long)co * d.ci + c) * d.r + kr) * d.s + ks;
  }
}

__device__ __forceinline__ float fold_scale(const FoldDesc& d, const float* params, const float* bnstats, int co, int raw) {
  if (!d.has_bn || raw) return 1.0f;
  return params[d.g_off + co] / sqrtf(bnstats[d.var_off + co] + kBnEps);
}

// grid: (blocks, layers, 2): z = 0 packs Wf (+bias, scale), z = 1 packs Wd.  raw = 1: BatchNorm is NOT folded
// (train-mode BatchNorm of ARCHITECTURE='basic': the convs produce the raw output, bias 0)
template <typename T>
__global__ __launch_bounds__(256) void fold_kernel(const FoldTable tab, const float* __restrict__ params, const float* __restrict__ bnstats,
                                                   unsigned char* __restrict__ packed, int with_dgrad, int raw, int first_layer) {
  const FoldDesc& d = tab.d[first_layer + blockIdx.y];
  const int which = blockIdx.z;
  if (d.tiled) return;  // fold_tile_kernel's layers
  if (which == 1 && (!with_dgrad || d.wd_off < 0)) return;
  const long stride = (long)gridDim.x * blockDim.x;
  if (which == 0) {
    T* wf = reinterpret_cast<T*>(packed + d.wf_off);
    float* bias = reinterpret_cast<float*>(packed + d.bias_off);
    float* scale = reinterpret_cast<float*>(packed + d.scale_off);
    const long total = (long)d.co_pad * d.kf;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int row = (int)(i / d.kf), k = (int)(i - (long)row * d.kf);
      float v = 0.f;
      if (row < d.co) {
        const float sc = fold_scale(d, params, bnstats, row, raw);
        const long src = fold_src_index(d, row, k);
        if (src >= 0) v = params[d.w_off + src] * sc;
        if (k == 0) {
          scale[row] = sc;
          float b = 0.f;
          if (d.has_bn) b = raw ? 0.f : params[d.b_off + row] - bnstats[d.mean_off + row] * sc;
          else if (d.has_bias) b = params[d.b_off + row];
          bias[row] = b;
        }
      } else if (k == 0) {
        scale[row] = 0.f;
        bias[row] = 0.f;
      }
      wf[i] = from_f32<T>(v);
    }
  } else {
    T* wd = reinterpret_cast<T*>(packed + d.wd_off);
    const long total = (long)d.cd_rows * d.kd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int n = (int)(i / d.kd), kk = (int)(i - (long)n * d.kd);
      const int tap = kk / d.co_pad, co = kk - tap * d.co_pad;
      float v = 0.f;
      if (co < d.co) {
        const long src = fold_src_index(d, co, tap * d.k_ci + n);
        if (src >= 0) v = params[d.w_off + src] * fold_scale(d, params, bnstats, co, raw);
      }
      wd[i] = from_f32<T>(v);
    }
  }
}

// Plain convolutions (3x3 / 1x1, ci % 64 == 0): one block packs a tile of 32 output channels x 64 input channels x all
// taps.  The OIHW source of such a tile is 32 contiguous runs of 64*taps floats (coalesced 16-byte reads, each master
// weight fetched once); the tile is transposed through LDS and written as contiguous runs into BOTH packed operands
// (Wf rows [co][tap][c], Wd rows [c][tap][co]).  The element-wise kernel above read the master weights with a stride of `taps`
// floats for Wf and of ci*taps floats for Wd: 706 MB of HBM traffic per launch for ~150 MB of algorithmic bytes (PMC).
// grid: (64x64-channel tiles over all tiled layers, 2 halves of 32 output channels)
#ifndef VDQN_FOLD_COT
#define VDQN_FOLD_COT 32
#endif
constexpr int kFoldCot = VDQN_FOLD_COT;  // output channels per fold_tile block (a build-time choice: 64 / kFoldCot blocks per 64 x 64 tile)

template <typename T, int TAPS>
__device__ __forceinline__ void fold_tile_body(const FoldDesc& d, const float* __restrict__ params, const float* __restrict__ bnstats,
                                               unsigned char* __restrict__ packed, int with_dgrad, int raw, float* sW, float* s_scale, int t, int cot_sub) {
  constexpr int COT = kFoldCot;        // output channels per block
  constexpr int RUN = 64 * TAPS;       // floats per output channel in this tile (contiguous in OIHW)
  constexpr int PITCH = RUN + 1;       // LDS row pitch: odd, so the column walk of the Wd pass spreads over the banks
  const int ci_tiles = d.ci / 64;
  const int cot = t / ci_tiles, cit = t - cot * ci_tiles;
  const int co0 = cot * 64 + cot_sub * COT, c0 = cit * 64;
  if (threadIdx.x < COT) {
    const int co = co0 + threadIdx.x;
    const float sc = co < d.co ? fold_scale(d, params, bnstats, co, raw) : 0.f;
    s_scale[threadIdx.x] = sc;
    if (cit == 0) {
      float b = 0.f;
      if (co < d.co) {
        if (d.has_bn) b = raw ? 0.f : params[d.b_off + co] - bnstats[d.mean_off + co] * sc;
        else if (d.has_bias) b = params[d.b_off + co];
      }
      reinterpret_cast<float*>(packed + d.bias_off)[co] = b;
      reinterpret_cast<float*>(packed + d.scale_off)[co] = sc;
    }
  }
  __syncthreads();
  // master weights -> LDS in source order, scaled: 16-byte loads of the contiguous [c][tap] run of every output channel
#pragma unroll 6
  for (int i = threadIdx.x; i < COT * RUN / 4; i += 256) {
    const int co_l = i / (RUN / 4), q = i - co_l * (RUN / 4);
    const int co = co0 + co_l;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (co < d.co) v = *reinterpret_cast<const float4*>(params + d.w_off + ((long)co * d.ci + c0) * TAPS + 4 * q);
    const float sc = s_scale[co_l];
    float* dst = sW + co_l * PITCH + 4 * q;
    dst[0] = v.x * sc; dst[1] = v.y * sc; dst[2] = v.z * sc; dst[3] = v.w * sc;
  }
  __syncthreads();
  // Wf rows [co][tap][c]: a thread writes EIGHT consecutive channels (16 bytes of bf16; eight lanes = the 64-channel run of one tap)
  T* wf = reinterpret_cast<T*>(packed + d.wf_off);
  constexpr int V16 = (int)(8 * sizeof(T) / 16);  // 16-byte stores per eight elements
#pragma unroll 3
  for (int i = threadIdx.x; i < COT * TAPS * 8; i += 256) {
    const int co_l = i / (TAPS * 8), rem = i - co_l * (TAPS * 8);
    const int tap = rem >> 3, c_l = (rem & 7) * 8;
    const float* src = sW + co_l * PITCH + c_l * TAPS + tap;
    T o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = from_f32<T>(src[e * TAPS]);
    T* dst = wf + (long)(co0 + co_l) * d.kf + tap * d.ci + c0 + c_l;
#pragma unroll
    for (int v = 0; v < V16; ++v) reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(o8)[v];
  }
  if (with_dgrad && d.wd_off >= 0) {
    // Wd rows [c][tap][co]: a thread writes eight consecutive output channels (four lanes = this block's 32 of them)
    T* wd = reinterpret_cast<T*>(packed + d.wd_off);
#pragma unroll 3
    for (int i = threadIdx.x; i < 64 * TAPS * (COT / 8); i += 256) {
      const int co_l = (i % (COT / 8)) * 8, rem = i / (COT / 8);
      const int tap = rem % TAPS, c_l = rem / TAPS;
      const float* src = sW + co_l * PITCH + c_l * TAPS + tap;
      T o8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = from_f32<T>(src[e * PITCH]);
      T* dst = wd + (long)(c0 + c_l) * d.kd + tap * d.co_pad + co0 + co_l;
#pragma unroll
      for (int v = 0; v < V16; ++v) reinterpret_cast<uint4*>(dst)[v] = reinterpret_cast<const uint4*>(o8)[v];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fold_tile_kernel(const FoldTable tab, const float* __restrict__ params, const float* __restrict__ bnstats,
                                                        unsigned char* __restrict__ packed, int with_dgrad, int raw, int tile_first) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
  float* sW = reinterpret_cast<float*>(fold_smem);  // [32][64 * taps + 1] f32, source order
  __shared__ float s_scale[32];
  int li = 0;
  for (int i = 0; i < tab.n; ++i)
    if (tab.d[i].tiled && tile_first + (int)blockIdx.x >= tab.d[i].tile_begin) li = i;
  const FoldDesc& d = tab.d[li];
  const int t = tile_first + (int)blockIdx.x - d.tile_begin;
  if (d.r * d.s == 9) fold_tile_body<T, 9>(d, params, bnstats, packed, with_dgrad, raw, sW, s_scale, t, (int)blockIdx.y);
  else fold_tile_body<T, 1>(d, params, bnstats, packed, with_dgrad, raw, sW, s_scale, t, (int)blockIdx.y);
}

// grid: (max co, layers of the stage): one block per output channel
// raw = 1: the weights were packed without BatchNorm folding; the BatchNorm parameter gradients were already written
// by the train-mode BatchNorm backward
__global__ __launch_bounds__(256) void unfold_kernel(const FoldTable tab, const PartTable pt, int first_layer, const float* __restrict__ params,
                                                     const float* __restrict__ bnstats, const unsigned char* __restrict__ bwd,
                                                     float* __restrict__ grads, int raw) {
  const FoldDesc& d = tab.d[first_layer + blockIdx.y];
  const int co = blockIdx.x;
  if (co >= d.co) return;
  const float* dw = reinterpret_cast<const float*>(bwd + d.dw_off) + (long)co * d.kf;
  const float* db = reinterpret_cast<const float*>(bwd + d.db_off);
  const int li = first_layer + blockIdx.y;
  float dbsum = 0.f;
  if (pt.tiles[li] > 0) {
    const float* part = reinterpret_cast<const float*>(bwd + pt.off[li]);
    const int per_tile = pt.groups[li];
    const int total = pt.tiles[li] * per_tile;
    for (int i = threadIdx.x; i < total; i += 256) {
      const int t = i / per_tile, g = i - t * per_tile;
      dbsum += part[(long)t * pt.ld[li] + g * pt.gstride[li] + co];
    }
  }
  float rstd = 1.f, sc = 1.f;
  if (d.has_bn && !raw) {
    rstd = 1.0f / sqrtf(bnstats[d.var_off + co] + kBnEps);
    sc = params[d.g_off + co] * rstd;
  }
  float dot = 0.f;
  __shared__ __attribute__((aligned(16))) float s_row[4608];  // one packed-layout dW' row of a plain convolution (<= 9 taps x 512 channels)
  if (d.tiled && d.kf <= 4608) {
    // packed row -> LDS (coalesced), then the OIHW row of the gradient and of the master weights is walked in ITS order
    // (coalesced global accesses; the [tap][c] -> [c][tap] permutation happens on the LDS read)
    const int taps = d.r * d.s;
    const long base = d.w_off + (long)co * d.kf;
    if ((((uintptr_t)dw | (uintptr_t)(params + base) | (uintptr_t)(grads + base)) & 15) == 0 && (d.kf & 3) == 0) {
      // 16-byte accesses on both sides of the permutation (a stage's unfold moves up to 100 MB)
      for (int k = threadIdx.x; k < d.kf / 4; k += 256) reinterpret_cast<float4*>(s_row)[k] = reinterpret_cast<const float4*>(dw)[k];
      __syncthreads();
      for (int i4 = threadIdx.x; i4 < d.kf / 4; i4 += 256) {
        float g[4];
        int c = (4 * i4) / taps, tap = 4 * i4 - c * taps;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          g[e] = s_row[tap * d.ci + c];
          if (++tap == taps) { tap = 0; ++c; }
        }
        const float4 w = reinterpret_cast<const float4*>(params + base)[i4];
        reinterpret_cast<float4*>(grads + base)[i4] = make_float4(g[0] * sc, g[1] * sc, g[2] * sc, g[3] * sc);
        dot += g[0] * w.x + g[1] * w.y + g[2] * w.z + g[3] * w.w;
      }
    } else {
      for (int k = threadIdx.x; k < d.kf; k += 256) s_row[k] = dw[k];
      __syncthreads();
      for (int i = threadIdx.x; i < d.kf; i += 256) {
        const int c = i / taps, tap = i - c * taps;
        const float g = s_row[tap * d.ci + c];
        grads[base + i] = g * sc;
        dot += g * params[base + i];
      }
    }
  } else {
    for (int k = threadIdx.x; k < d.kf; k += 256) {
      const long src = fold_src_index(d, co, k);
      if (src >= 0) {
        const float g = dw[k];
        grads[d.w_off + src] = g * sc;
        dot += g * params[d.w_off + src];
      }
    }
  }
  __shared__ float red[8];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dot += __shfl_down(dot, o, 64);
    dbsum += __shfl_down(dbsum, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = dot;
    red[4 + (threadIdx.x >> 6)] = dbsum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = red[0] + red[1] + red[2] + red[3];
    const float dbp = pt.tiles[li] > 0 ? (red[4] + red[5] + red[6] + red[7]) : db[co];
    if (d.has_bn) {
      if (!raw) {
        grads[d.g_off + co] = rstd * (tot - bnstats[d.mean_off + co] * dbp);
        grads[d.b_off + co] = dbp;
      }
    } else if (d.has_bias) {
      grads[d.b_off + co] = dbp;
    }
  }
}

}  // namespace

// dL/dQ f32 [B][nq] -> the engine's [B][64] operand of the head's backward (zero padded)
template <typename T>
__global__ __launch_bounds__(256) void dq_pad_kernel(const float* __restrict__ src, T* __restrict__ dst, int rows, int nq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * 64) return;
  const int b = i >> 6, c = i & 63;
  dst[i] = from_f32<T>(c < nq ? src[(long)b * nq + c] : 0.f);
}

// BatchNorm fold + layout packs of layers [first_layer, first_layer + n_layers) of the table (stored by backward stage: head +
// layer4, layer3, then stem + layer1 + layer2)
static int pack_weights_layers(vdqn_net* net, const float* params, const float* bnstats, void* packed, int32_t with_dgrad, int first_layer,
                               int n_layers, hipStream_t stream) {
  if (n_layers <= 0) return VDQN_OK;
  dim3 grid(256, (unsigned)n_layers, 2);
  const int dgrad = with_dgrad & 1, raw = (with_dgrad >> 1) & 1;
  int tile_first = -1, tile_end = 0;
  for (int i = first_layer; i < first_layer + n_layers; ++i) {
    const FoldDesc& d = net->fold.d[i];
    if (!d.tiled) continue;
    if (tile_first < 0) tile_first = d.tile_begin;
    tile_end = d.tile_begin + (d.co_pad / 64) * (d.ci / 64);
  }
  const double share = (double)n_layers / (double)net->layers.size();
  ProfScope ps_("fold_weights", 0.0, ((double)net->trainable_numel * 4.0 + (double)net->packed_bytes * (dgrad ? 1.0 : 0.5)) * share, stream);
  const size_t tile_smem = kFoldCot * (64 * 9 + 1) * 4;  // [kFoldCot output channels][64 * taps + 1] f32
  vdqn_ensure_dyn_smem(reinterpret_cast<const void*>(&fold_tile_kernel<bf16raw>), (size_t)tile_smem);
  vdqn_ensure_dyn_smem(reinterpret_cast<const void*>(&fold_tile_kernel<float>), (size_t)tile_smem);
  if (net->cfg.dtype == VDQN_BF16) {
    hipLaunchKernelGGL((fold_kernel<bf16raw>), grid, dim3(256), 0, stream, net->fold, params, bnstats, (unsigned char*)packed, dgrad, raw, first_layer);
    if (tile_first >= 0)
      hipLaunchKernelGGL((fold_tile_kernel<bf16raw>), dim3(tile_end - tile_first, 64 / kFoldCot), dim3(256), tile_smem, stream, net->fold, params, bnstats,
                         (unsigned char*)packed, dgrad, raw, tile_first);
  } else {
    hipLaunchKernelGGL((fold_kernel<float>), grid, dim3(256), 0, stream, net->fold, params, bnstats, (unsigned char*)packed, dgrad, raw, first_layer);
    if (tile_first >= 0)
      hipLaunchKernelGGL((fold_tile_kernel<float>), dim3(tile_end - tile_first, 64 / kFoldCot), dim3(256), tile_smem, stream, net->fold, params, bnstats,
                         (unsigned char*)packed, dgrad, raw, tile_first);
  }
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_net_pack_weights(vdqn_net* net, const float* params, const float* bnstats, void* packed, int32_t with_dgrad, void* stream) {
  VDQN_CHECK(net && params && bnstats && packed, "vdqn_net_pack_weights: null arg");
  return pack_weights_layers(net, params, bnstats, packed, with_dgrad, 0, (int)net->layers.size(), (hipStream_t)stream);
}

// dL/dQ of a per-call backward (vdqn_net_backward_begin) into the head's [rows][64] operand at `dst`
void launch_dq_pad(const vdqn_net* net, const float* dq_f32, void* dst, int rows, hipStream_t stream) {
  const int nq = net->cfg.action_dim * net->cfg.num_classes;
  const int blocks = (rows * 64 + 255) / 256;
  if (net->cfg.dtype == VDQN_BF16)
    hipLaunchKernelGGL((dq_pad_kernel<bf16raw>), dim3(blocks), dim3(256), 0, stream, dq_f32, reinterpret_cast<bf16raw*>(dst), rows, nq);
  else
    hipLaunchKernelGGL((dq_pad_kernel<float>), dim3(blocks), dim3(256), 0, stream, dq_f32, reinterpret_cast<float*>(dst), rows, nq);
}

// the gradients of layers [first_layer, first_layer + n_layers) of the table, from the f32 accumulators and the partials `pt` names
// in a->bwd into a->grads; `bytes` is the launch profiler's traffic figure
void launch_unfold(const vdqn_net* net, const PartTable& pt, int first_layer, int n_layers, int max_co, int raw, const vdqn_step_args* a,
                   hipStream_t stream, double bytes) {
  ProfScope ps_("unfold_grads", 0.0, bytes, stream);
  hipLaunchKernelGGL(unfold_kernel, dim3(max_co, n_layers), dim3(256), 0, stream, net->fold, pt, first_layer, a->params, a->bnstats,
                     (const unsigned char*)a->bwd, a->grads, raw);
}
