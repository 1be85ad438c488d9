// What the engine's translation units share: the layer table, the two workspace layouts and the engine object
// (engine_table.hip builds them, fold.hip and engine.hip read them).
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"

#pragma GCC visibility push(hidden)  // internal to the library: nothing here joins its exported symbols

constexpr int kMaxLayers = 24;
constexpr float kBnEps = 1e-5f;
constexpr float kBnMomentum = 0.1f;

enum LayerKind { K_CONV = 0, K_CONV1_S2D = 1, K_LINEAR = 2, K_LINEAR_PERM = 3 };

struct Layer {
  std::string name, bn_name;
  int kind;
  int co, ci, r, s, stride, pad;  // master weight dims [co][ci][r][s] and conv geometry
  int has_bn, has_bias;
  int k_ci, k_r, k_s, pix_stride;  // kernel view
  int co_pad;
  int hi, wi, ho, wo;
  int per_sample;
  int stage, has_dgrad;
  int64_t w_off, g_off, b_off, mean_off, var_off;
  int64_t wf_off, wd_off, bias_off, scale_off;  // bytes in packed
  int64_t dw_off, db_off;                        // bytes in bwd workspace
  int kf() const { return k_r * k_s * k_ci; }
  int kd() const { return k_r * k_s * co_pad; }
};

struct FoldDesc {
  int64_t w_off, g_off, b_off, mean_off, var_off;
  int64_t wf_off, wd_off, bias_off, scale_off, dw_off, db_off;
  int co, ci, r, s, kind, co_pad, kf, k_ci, k_s, cd_rows, kd, has_bn, has_bias;
  int tiled;       // packed by fold_tile_kernel (plain convs with ci % 64 == 0): 64 x 64-channel tiles through LDS
  int tile_begin;  // first tile of this layer in fold_tile_kernel's grid
};
struct FoldTable {
  int n, n_tiles;
  FoldDesc d[kMaxLayers];
};
// where unfold finds dL/dbias of layer i: tiles > 0 -> sum of dgrad-epilogue partials
//   sum_t sum_g part[t * ld + g * gstride + co]   (g < groups), else the colsum kernel's db[co]
struct PartTable {
  int64_t off[kMaxLayers];
  int tiles[kMaxLayers], ld[kMaxLayers], groups[kMaxLayers], gstride[kMaxLayers];
};

// The buffers of BwdLayout that hold those partials, in the order bwd_layout reserves them: the column sums of g_l1, g_l0, g_f8
// and g_pool, then of g_o[b], g_h[b] per BasicBlock.
enum PartBuf { kPartL1 = 0, kPartL0, kPartF8, kPartPool, kPartBlocks, kPartBufs = kPartBlocks + 16 };
inline int part_o(int b) { return kPartBlocks + 2 * b; }
inline int part_h(int b) { return kPartBlocks + 2 * b + 1; }
constexpr int kTileRows = 128;  // rows per entry of the tiled kernels (igemm_common.h; a 256-row tile writes two entries)
struct PartInfo {
  int entries, ld, groups, gstride;  // what the producing data gradient wrote (PartTable's tiles / ld / groups / gstride)
  int64_t capacity;                  // entries bwd_layout reserved
};

struct ActLayout {
  int64_t t_in, c1, pool, idx;
  int64_t h[8], o[8], ds[8];
  int64_t f8, l0, l1, q, qf;
  // ARCHITECTURE='basic' only: pooled features, raw (pre-BatchNorm) conv outputs, per-layer BatchNorm work areas
  int64_t avg, r_c1, r_h[8], r_o[8], r_ds[8], bnw[kMaxLayers], bnw_begin, bnw_bytes, bn_sync;
  int64_t bn_det = -1, bn_det_bytes = 0;  // deterministic mode ('basic'): per-block partial sums of the train-mode BatchNorm kernels
  int64_t total;
};
struct BwdLayout {
  int64_t zero_begin, zero_bytes;  // region cleared every step: dW', dbias', loss scratch
  int64_t dq, g_l1, g_l0, g_f8, g_o[8], g_h[8], dsg[8], g_pool, g_c1;
  int64_t part[kPartBufs];  // per-tile column sums written by the dgrad epilogues (part_info() owns their shape)
  int64_t g_avg, g_or[8], g_dsr[8];  // 'basic' only: gradient of the pooled features / of the raw conv2, downsample outputs
  int64_t det_ws, det_ws_bytes;      // deterministic mode: the weight-gradient kernels' partial copies (one layer at a time)
  int64_t total;
};

inline int64_t align_up(int64_t v, int64_t a = 256) { return (v + a - 1) / a * a; }

enum Head { HEAD_NONE = 0, HEAD_VALUE, HEAD_SPREAD, HEAD_POLICY };

#pragma GCC visibility pop

struct vdqn_net {
  vdqn_net_config cfg;  // cfg.dtype is the STORAGE dtype: VDQN_F32 for a VDQN_F32X3 engine (every pointwise entry takes that)
  // The one extra head the Q layer may carry behind its Q columns.  HEAD_VALUE: num_classes state values, V(c) at column n_q() + c
  // (vdqn_net_create_v); HEAD_SPREAD: one spread rho(c, a) per Q column, at column n_q() + c * action_dim + a (vdqn_net_create_d);
  // HEAD_POLICY: one behaviour logit i(a) per action, at column n_q() + a (vdqn_net_create_p).
  Head head = HEAD_NONE;
  int gemm_dtype;  // dtype of the GEMM calls (convolutions, linear layers, weight gradients, stem): the requested one
  int esz;  // bytes per activation element
  std::vector<Layer> layers;
  std::vector<vdqn_param_info> params;
  int64_t trainable_numel, params_numel, bnstats_numel, packed_bytes;
  int64_t stage_begin[3], stage_end[3];
  int layer_stage_first[3], layer_stage_count[3];
  int64_t dw_bytes;  // total f32 dW' + dbias' bytes
  FoldTable fold;
  // layer indices
  int l_conv1, l_f8, l_top0, l_top2, l_top4;  // 'basic': l_top4 is the single `top` Linear, the other head layers are -1
  bool basic() const { return cfg.extra_capacity == 0; }
  int n_q() const { return cfg.action_dim * cfg.num_classes; }  // the Q columns; with the value head, V(c) is column n_q() + c
  int l_b_conv1[8], l_b_conv2[8], l_b_ds[8];
  // A second HIP stream for work that is independent of the main dependency chain: the weight gradients (they only
  // need gy, the data-gradient chain does not wait for them) and the target-network forward.  Blocks of the side
  // kernels fill the tail rounds of the main kernels (784..3136-block grids on 512 resident blocks).
  BnSync bn_sync = {nullptr, nullptr, nullptr, 1};  // SyncBN hook ('basic' under data parallelism)
  int wgrad_rr = 0;                                  // VDQN_WGRAD_STREAMS=2: which side stream took the last weight gradient
  int overlap = 1;
  hipStream_t side = nullptr;
  hipStream_t side2 = nullptr;  // the second half of the online forward pass
  std::vector<hipEvent_t> events;
  size_t ev_next = 0;
};

#pragma GCC visibility push(hidden)

#define RC(x)                     \
  do {                            \
    int rc_ = (x);                \
    if (rc_ != VDQN_OK) return rc_; \
  } while (0)

inline int64_t frame_bytes(const vdqn_net* net) { return (int64_t)115 * 115 * 16 * net->esz; }  // one packed space-to-depth frame
inline int block_planes(int b) { return 64 << (b / 2); }  // channels and side of BasicBlock b's output
inline int block_side(int b) { return 56 >> (b / 2); }

// engine_table.hip
ActLayout act_layout(const vdqn_net* net, int n_samples);
BwdLayout bwd_layout(const vdqn_net* net, int n_samples);
vdqn_wgrad_args wgrad_shape_args(const vdqn_net* net, const Layer& L, int n_units);
int64_t wgrad_max_imgs(const vdqn_net* net, const Layer& L);
int part_buf(const vdqn_net* net, int li);
PartInfo part_info(const vdqn_net* net, int buf, int n_samples, int rows_per_entry);
// engine.hip
bool wgrad_two_stage();
// fold.hip
void launch_unfold(const vdqn_net* net, const PartTable& pt, int first_layer, int n_layers, int max_co, int raw, const vdqn_step_args* a,
                   hipStream_t stream, double bytes);
void launch_dq_pad(const vdqn_net* net, const float* dq_f32, void* dst, int rows, hipStream_t stream);
// stem_dgrad.hip
void vdqn_stem_pixel_scale(float* scale3);  // 1 / (255 std_c): d(normalised value) / d(uint8 pixel value)
int vdqn_stem_dgrad_from_c1(const float* g_c1, const float* wt, const float* scale, float* out, int n_img, hipStream_t st);

#pragma GCC visibility pop
