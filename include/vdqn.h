/*
 * vdqn.h — C ABI of libvdqn.so, the MI355X (gfx950) implementation of the Q-learning hot path of
 * uiuc-robovision/video-dqn (train_q_network.py's inner loop).
 *
 * The reference is pure Python on PyTorch: it has no FFI of its own.  Every entry point below names the
 * reference call site (file:line under the reference tree) whose arithmetic it replaces; the reference-side
 * binding a maintainer would add is the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers unless a name ends in _host;
 *   - the caller owns every buffer (the library allocates nothing on the device except inside an explicit
 *     vdqn_net_create/vdqn_net_destroy pair, which holds host-side descriptors only);
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no host sync;
 *   - return value 0 = ok, negative = error (vdqn_last_error() gives the text); no exceptions cross the ABI;
 *   - activations are NHWC; `dtype` selects the storage/compute type of activations and packed weights:
 *       VDQN_F32  : f32 storage, exact-f32 MFMA (v_mfma_f32_16x16x4_f32)   — the parity mode
 *       VDQN_BF16 : bf16 storage, v_mfma_f32_16x16x32_bf16, f32 accumulate — the throughput mode
 *       VDQN_F32X3: f32 storage (everything as VDQN_F32), the GEMMs as split bf16 x 3: each f32 operand is split into
 *                   hi = bf16(x), lo = bf16(x - hi) and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16
 *                   (~2^-16 relative per product, f32 accumulate) — f32-grade results at bf16 MFMA rates.  Accepted by
 *                   vdqn_conv2d, vdqn_conv2d_wgrad, vdqn_stem_conv_pool(_n) and vdqn_net_config; every other entry takes
 *                   VDQN_F32 for the same tensors (the engine calls them so) and rejects it.
 *     master parameters, gradients, Adam state and Q-values are always f32.
 */
#ifndef VDQN_H_
#define VDQN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VDQN_F32 0
#define VDQN_BF16 1
#define VDQN_F32X3 2 /* f32 tensors, GEMMs computed as split bf16 x 3 (see above) */

#define VDQN_OK 0
#define VDQN_ERR_INVALID (-1)
#define VDQN_ERR_LAUNCH (-2)

/* thread-local text of the last error returned on this host thread */
const char* vdqn_last_error(void);
/* ABI version; bumped on any signature change */
int vdqn_abi_version(void);
/* sizeof() of the argument structs as THIS library was compiled (which: 0 vdqn_conv_args, 1 vdqn_wgrad_args, 2 vdqn_td_args,
 * 3 vdqn_net_config, 4 vdqn_param_info, 5 vdqn_prof_entry, 6 vdqn_step_args; -1 for any other value): a foreign-function binding
 * (ctypes / cgo / JNI) compares them with its own struct definitions at load time instead of finding a drifted field at run time */
int32_t vdqn_abi_struct_size(int32_t which);

/* Launch profiler (off by default).  While enabled, every kernel launch of the library is bracketed by HIP
 * events on its launch stream; collect() synchronises those events and returns one entry per kernel symbol:
 * launches, summed device milliseconds, summed algorithmic FLOPs and algorithmic bytes.  Resets on collect. */
typedef struct vdqn_prof_entry {
  char name[48];
  int64_t launches;
  double ms;
  double flops;
  double bytes;
} vdqn_prof_entry;
int vdqn_profile_enable(int on);
int vdqn_profile_collect(vdqn_prof_entry* out, int max_entries);

/* ------------------------------------------------------------------------------------------------
 * Operator level (each is also what the engine below launches).
 * ------------------------------------------------------------------------------------------------ */

/* Implicit-GEMM convolution / linear layer, forward or data-gradient.
 *   out[m, n] = epilogue( sum_{r,s,c} in[pix(m,r,s), c] * wt[n][r][s][c] )
 *   mode 0 (forward gather):  hi = ho*stride - pad + r,           wi likewise
 *   mode 1 (dgrad gather):    hi = (ho + pad - r) / stride if divisible and in range (transposed conv)
 *   epilogue: v += bias[n]; v += resid[m,n]; relu; v = mask[m,n] > 0 ? v : 0   (each optional);
 *             optional per-tile column sums of the stored values (colsum_part)
 * Replaces: torch conv2d/linear (+ folded eval BatchNorm, ReLU, residual add) reached from
 * archs/HabitatDQNMultiAction.py:30-31,49-53 and their autograd backward (train_q_network.py:226).
 * `ci` must be a multiple of 128 bytes / sizeof(elem); `wt` holds co_pad = roundup(co, 64 or 128) rows. */
typedef struct vdqn_conv_args {
  const void* in;      /* [n_img][hi][wi] pixels of pix_stride elems */
  const void* wt;      /* [co_pad][r][s][ci], K-contiguous */
  const float* bias;   /* [co_pad] or NULL */
  const void* resid;   /* [m][ldo] or NULL */
  const void* mask;    /* [m][ldo] or NULL */
  void* out;           /* [m][ldo], dtype; may be NULL if out_f32 is given */
  float* out_f32;      /* optional f32 copy of the result [m][ldo] */
  float* colsum_part;  /* optional [T][ldo] f32, T = ceil(m/R) with R = vdqn_conv2d_colsum_rows(a) = 128 for the tiled kernels
                          (stride-2 dgrad: 4*ceil(m/4/128), one run of tiles per output parity class) and 32 for the Q-head's
                          skinny GEMMs: per R-row tile, column sums of the stored `out` values
                          (summed over tiles they are the bias / BatchNorm-shift gradient of the layer that `out`
                          is the output-gradient of) */
  int32_t n_img, hi, wi, ci, pix_stride;
  int32_t ho, wo, co, ldo;
  int32_t r, s, stride, pad;
  int32_t mode, relu, dtype; /* dtype: VDQN_F32 | VDQN_BF16 | VDQN_F32X3 */
  /* Optional sibling 1x1 / stride-2 / pad-0 convolution fused into a 3x3 / stride-2 / pad-1 call: the downsample branch of a
   * ResNet BasicBlock (torchvision resnet.py `downsample`; archs/HabitatDQNMultiAction.py:30), whose input pixel is the 3x3's
   * centre tap.  All NULL / 0 = no sibling.
   *   mode 0: out2[m, :co2] = relu2?( sum_c in[pix(m, centre), c] * wt2[n][c] + bias2[n] ), wt2 = [co2_pad][1][1][ci];
   *           one launch, the input rows are fetched once for both convolutions.
   *   mode 1: out += dgrad_1x1_stride2(in2, wt2) before the epilogue (residual / mask / column sums then see the sum):
   *           in2 = gradient of the sibling's output, [n_img][hi][wi] pixels of pix_stride elems holding ci2 channels,
   *           wt2 = [co_pad][1][1][ci2] (the sibling's data-gradient operand); bias2 / out2 / relu2 unused. */
  const void* in2;
  const void* wt2;
  const float* bias2;
  void* out2;
  int32_t co2, ldo2, relu2, ci2;
} vdqn_conv_args;
int vdqn_conv2d(const vdqn_conv_args* a, void* stream);
/* rows of `out` covered by one entry of colsum_part for this call (what sizes that buffer): 128, or the row tile of the skinny
 * GEMM kernels that take the Q-head's bf16 linear layers (archs/HabitatDQNMultiAction.py:31; csrc/skinny.hip) */
int32_t vdqn_conv2d_colsum_rows(const vdqn_conv_args* a);

/* Weight gradient of the same layer:  dw[n][r][s][c] += sum_m gy[m, n] * x[pix(m,r,s), c]
 * (split over `splitk` pixel ranges whose partial tiles are added into dw with f32 atomics).  If dbias != NULL it also
 * accumulates dbias[n] += sum_m gy[m, n].
 * Deterministic mode (the reference pins cudnn.deterministic = True, train_q_network.py:88-89): with `workspace` set
 * (vdqn_conv2d_wgrad_workspace_bytes gives the size) every split stores its partial tile into its own copy of dw with plain
 * stores and a second kernel adds the copies to dw in split order — the result no longer depends on the order in which the
 * blocks finish, two runs are bit-identical.
 * Replaces: the convolution_backward/addmm weight-gradient kernels behind loss.backward(),
 * train_q_network.py:226. */
typedef struct vdqn_wgrad_args {
  const void* gy;   /* [m][ldg] gradient w.r.t. the layer output (already ReLU-masked) */
  const void* x;    /* layer input, as vdqn_conv_args.in */
  float* dw;        /* [co_pad][r][s][ci] f32, pre-zeroed */
  float* dbias;     /* [co_pad] f32, pre-zeroed, or NULL */
  int32_t n_img, hi, wi, ci, pix_stride;
  int32_t ho, wo, co, ldg;
  int32_t r, s, stride, pad;
  int32_t splitk, dtype;  /* VDQN_F32 | VDQN_BF16 | VDQN_F32X3 */
  void* workspace;          /* NULL: atomics; else >= vdqn_conv2d_wgrad_workspace_bytes(a) bytes, 16-byte aligned */
  int64_t workspace_bytes;
} vdqn_wgrad_args;
int vdqn_conv2d_wgrad(const vdqn_wgrad_args* a, void* stream);
int64_t vdqn_conv2d_wgrad_workspace_bytes(const vdqn_wgrad_args* a);  /* -1 on invalid arguments */

/* Host side of the streaming input path (decoded-frame shards that do not fit in HBM): gather n records of bytes_each bytes —
 * record i from src[i], e.g. a frame inside a memory-mapped shard — into dst + i * bytes_each (a pinned staging buffer) on
 * `threads` host threads; returns when all are in place.  One copy per frame where the reference's loader makes three
 * (worker decode + stack, collate, pin: dataloaders/q_learning_real.py:55-73 under torch's DataLoader, train_q_network.py:98,114).
 * No GPU involved. */
int vdqn_host_gather(void* dst, const void* const* src, int64_t n, int64_t bytes_each, int32_t threads);

/* Input packing: normalise + space-to-depth the 224x224 RGB frames into the conv1 operand
 * [n][115][115][16] (2x2x3 -> 12 channels + 4 zero, 2-pixel zero border top/left, 1 bottom/right), so the
 * 7x7/2 stem is a 4x4/1 implicit GEMM with 128-byte contiguous K rows.
 *   src_kind 0: uint8 NHWC [n][224][224][3]  -> (x/255 - mean)/std   (util/torch.py:5-12, :26-36)
 *   src_kind 1: f32 NCHW [n][3][224][224] already normalised (the tensor process_batch moves to the
 *               device, train_q_network.py:127-129) */
int vdqn_pack_input(const void* src, int32_t src_kind, void* dst, int32_t n_img, int32_t dtype, void* stream);

/* 3x3/2 pad 1 max-pool, NHWC (torchvision resnet stem; archs/HabitatDQNMultiAction.py:30). idx[m][c] stores
 * the arg-max tap (kh*3+kw, first maximum wins as in torch). */
int vdqn_maxpool_fwd(const void* in, void* out, uint8_t* idx, int32_t n_img, int32_t hi, int32_t wi, int32_t c,
                     int32_t dtype, void* stream);
/* gx[n,h,w,c] = (x[n,h,w,c] > 0) * sum over windows whose arg-max is (h,w) of gy  (pool + ReLU backward).
 * x may be NULL when gy is already zero wherever the pooled value is <= 0 (the engine's case: the producing dgrad
 * masks with the pooled activation; the arg-max of a window holds exactly that value), which saves the read of x. */
int vdqn_maxpool_bwd(const void* gy, const uint8_t* idx, const void* x, void* gx, int32_t n_img, int32_t hi,
                     int32_t wi, int32_t c, int32_t dtype, void* stream);

/* Fused Double-DQN target + TD loss + dLoss/dQ  (train_q_network.py:134-169,180).
 *   Qb = q_before[b,c,act[b]]; a* = argmax_a q_after_online[b,c,:] (first max); Qa = q_after_target[b,c,a*]
 *   Qa *= (1 - term); y = linear ? rew + (Qa - 0.1) : rew + gamma*Qa; rect clip -> clamp(y,0,1)
 *   d = Qb - y;  loss_kind 0 (the reference, :167): l = 0.5 d^2, dl = d
 *                loss_kind 1 (Huber / smooth-L1 with beta 1, the option archs/HabitatDQNMultiAction.py:25 leaves as a
 *                TODO): l = |d| < 1 ? 0.5 d^2 : |d| - 0.5, dl = clamp(d, -1, 1)
 *   l *= valid if use_valid; loss += inv_count * sum l;
 *   dq[b, c*A+a] = (a == act[b]) ? dl * (valid) * inv_count : 0   (rows of ldq elems, zero padded)
 * q_* are f32 [batch][ldq]; act i64; rew/term/valid f32 [batch][n_cat]; loss is a pre-zeroed f32 scalar. */
typedef struct vdqn_td_args {
  const float* q_before;
  const float* q_after_online;
  const float* q_after_target;
  const int64_t* act;
  const float* rew;
  const float* term;
  const float* valid;
  float* loss;
  void* dq;         /* [batch][ldq] dtype */
  float* dq_f32;    /* optional [batch][ldq] */
  int32_t batch, n_cat, n_act, ldq;
  float gamma, inv_count;
  int32_t clip_rect, linear, use_valid, dtype;
  int32_t loss_kind;      /* 0 = half squared error (reference), 1 = Huber */
  int32_t deterministic;  /* 1: the loss is summed by ONE block in a fixed order (no cross-block atomics) */
  float* q_copy;          /* optional [batch][n_cat * n_act] f32: a compact copy of q_before's first n_cat * n_act columns (what the
                             training loop reads back as Q(s)), written by the same launch */
} vdqn_td_args;
int vdqn_td_loss(const vdqn_td_args* a, void* stream);
/* The same loss with per-sample importance weights (prioritized replay): sample b's loss terms and its dq row are scaled by
 * weight[b] (f32 [batch]; inv_count is unchanged), and err_out[b] (f32 [batch], optional) receives the sample's mean absolute
 * TD error sum_c |d_bc| * valid_bc / n_cat, from the raw d under either loss kind.  No atomics for err_out; `deterministic` keeps
 * its one-block loss sum.  With weight == 1 the loss and dq are bit-identical to vdqn_td_loss. */
int vdqn_td_loss_weighted(const vdqn_td_args* a, const float* weight, float* err_out, void* stream);
/* The same loss with the discrete conservative Q-learning penalty (CQL; Kumar et al., NeurIPS 2020) for training from logged
 * data only, added to the loss of train_q_network.py:167,180 in the same launch:
 *   pen_bc = logsumexp_a q_before[b,c,:] - q_before[b,c,act[b]]   (the maximum is subtracted before anything is exponentiated)
 *   s_bc = weight[b] * valid_bc;  loss += inv_count * sum s_bc * (l(d_bc) + cql_alpha * pen_bc)
 *   penalty += inv_count * sum s_bc * pen_bc                      (not scaled by cql_alpha)
 *   dq[b, c*A+a] = inv_count * s_bc * ([a == act[b]] * dl(d_bc) + cql_alpha * (softmax_a(q_before[b,c,:]) - [a == act[b]]))
 * so dq is dense over the actions of every category (padding columns 0).  d, l, dl, weight and err_out are those of
 * vdqn_td_loss_weighted (err_out is the raw TD error: priorities do not follow the penalty); weight may be NULL (= 1), err_out and
 * penalty (a pre-zeroed f32 scalar) may be NULL.  dtype VDQN_F32 or VDQN_BF16.  cql_alpha must be finite and > 0 and n_act >= 2
 * (with one action the penalty is identically zero): both fail by name, like every other check, before any launch.
 * `deterministic` sums loss and penalty in one block in a fixed order. */
int vdqn_td_loss_cql(const vdqn_td_args* a, const float* weight /* NULL = 1 */, float* err_out /* NULL ok */, float cql_alpha,
                     float* penalty /* pre-zeroed f32 scalar, NULL ok */, void* stream);
/* The three entries above with a per-sample discount (n-step returns, vdqn_nstep_walk below): sample_gamma (f32 [batch], required)
 * gives sample b's discount where they take a->gamma, which is not read.  cql_alpha > 0: vdqn_td_loss_cql's launch; else weight !=
 * NULL: vdqn_td_loss_weighted's; else vdqn_td_loss's (err_out then has to be NULL, as penalty has to be when cql_alpha is 0).  The
 * choice is made at compile time inside the one kernel template: the instances behind the three entries above keep their loads and
 * bits, and with sample_gamma[b] == gamma for every b this entry writes exactly their bits; a dq row and err_out[b] depend on their
 * own sample's discount alone.  Fails by name, before any launch, for everything those entries refuse and for linear != 0
 * (y = r + (Qa - 0.1) has no discount), a NULL sample_gamma and a negative or non-finite cql_alpha. */
int vdqn_td_loss_nstep(const vdqn_td_args* a, const float* weight /* NULL ok */, float* err_out /* NULL ok */, float cql_alpha /* 0 = none */,
                       float* penalty /* NULL ok */, const float* sample_gamma, void* stream);
/* The entries above with the Monte-Carlo return G_bc = mc_return[b][c] of every sampled row (vdqn_mc_returns below: the discounted
 * return the logged data itself obtained from that row, a lower bound of the optimal value when rewards are non-negative).  The
 * mode is chosen as vdqn_td_loss_nstep chooses it (cql_alpha > 0, else weight, else plain); sample_gamma may be NULL (a->gamma).
 *   mc_flags bit 0, the floor (lower-bound Q-learning, He et al. 2017; Oh et al. 2018): y = max(y, G_bc) in front of the rect clip,
 *     which keeps the last word; err_out follows the floored error.
 *   mc_flags bit 1, calibrated (Cal-QL, Nakamoto et al., NeurIPS 2023; needs cql_alpha > 0): with qc_a = max(q_a, G_bc),
 *     m = max_a qc_a, sum = sum_a expf(qc_a - m), p_a = expf(qc_a - m) / sum, pen_bc = logf(sum) + (m - q_{a*}) with the raw
 *     q_{a*}, and the penalty's part of dq is alpha * (p_a * [q_a >= G_bc] - [a == a*]); at a tie q_a == G_bc the Q value takes the
 *     gradient.
 *   mc_stats (f32[2], pre-zeroed, NULL ok), each inv_count times a sum that is formed like the loss's (`deterministic`: one block,
 *     a fixed order), vm_bc = valid or 1 and no importance weight:
 *     [0] += vm_bc * [G_bc > y before the floor]   the share of targets the floor raises (under either flag)
 *     [1] += vm_bc * (q_{a*} - G_bc)               by how far Q sits above the achieved return
 * A compile-time choice inside the one kernel template: the instances behind the entries above keep their loads and bits, and
 * with mc_return filled with -inf this entry writes exactly the bits of the matching entry above under any flags, mc_stats[0]
 * staying 0.  Fails by name, before any launch, for everything those entries refuse and for a NULL mc_return, mc_flags 0 or with
 * unknown bits, bit 1 with cql_alpha == 0, a negative or non-finite cql_alpha and linear != 0. */
int vdqn_td_loss_mc(const vdqn_td_args* a, const float* weight /* NULL ok */, float* err_out /* NULL ok */, float cql_alpha /* 0 = none */,
                    float* penalty /* NULL ok */, const float* sample_gamma /* NULL = a->gamma */,
                    const float* mc_return /* f32 [batch][n_cat], required */, int32_t mc_flags, float* mc_stats /* f32[2], pre-zeroed, NULL ok */,
                    void* stream);
/* Implicit Q-learning (IQL; Kostrikov et al., ICLR 2022) in one launch (video_dqn_amd/csrc/iql.hip): a row of ldq columns holds
 * Q(c, a) at column c * n_act + a and a state value V(c) at column n_cat * n_act + c, so n_cat * n_act + n_cat <= ldq.  With
 * a* = act[b], tau = expectile, w_b = weight[b] (NULL = 1), vm_bc = valid or 1 and gamma_b = sample_gamma[b] (NULL = a->gamma):
 *   v  = q_before[b][V(c)]     v' = q_after_online[b][V(c)]     qt = q_after_target[b][Q(c, a*)]
 *        (q_after_target is read as the TARGET network's Q(s), not Q(s'); no gradient flows through v' or qt)
 *   u  = qt - v;  omega = u > 0 ? tau : 1 - tau;  L_V = omega u^2;  dL_V/dv = -2 omega u        (expectile regression of V on qt)
 *   y  = rew + gamma_b * (v' * (1 - term)), rect clip as vdqn_td_loss;  d = q_before[b][Q(c, a*)] - y;  L_Q = l(d), dl(d) by loss_kind
 *   loss += inv_count * sum w_b vm_bc (L_Q + L_V)
 *   stats[0] += inv_count * sum w_b vm_bc L_V        stats[1] += inv_count * sum vm_bc u      (f32[2], pre-zeroed, NULL ok)
 *   dq[b][Q(c, a*)] = dl(d) w_b vm_bc inv_count      dq[b][V(c)] = -2 omega u w_b vm_bc inv_count      every other column 0
 *   err_out[b] = sum_c |d_bc| vm_bc / n_cat          (NULL ok; priorities follow the Q error)
 * y is formed in vdqn_td_loss's expression order: with a q_after_target row whose actions all hold v', vdqn_td_loss_weighted
 * writes the same bits into the taken-action columns of dq and into err_out.  `deterministic` sums in one block in a fixed order;
 * q_copy and dq_f32 as in vdqn_td_loss.  Fails by name, before any launch, for a null required pointer, bad dims, columns that do
 * not fit in ldq, linear != 0 and an expectile outside [0.5, 1). */
int vdqn_td_loss_iql(const vdqn_td_args* a, const float* weight /* NULL = 1 */, float* err_out /* NULL ok */,
                     const float* sample_gamma /* NULL = a->gamma */, float expectile, float* stats /* f32[2], pre-zeroed, NULL ok */,
                     void* stream);
/* Gaussian distributional Q-learning in one launch (video_dqn_amd/csrc/dist.hip; the reference's config keys DISTRIBUTIONAL,
 * KL_BACKWARDS, LOG_SIGMA): a row of ldq columns holds the mean of the return at column M(c, a) = c * n_act + a (the Q column) and a
 * spread parameter rho at column S(c, a) = n_cat * n_act + c * n_act + a, so 2 * n_cat * n_act <= ldq.  flags bit 0 = KL_BACKWARDS,
 * bit 1 = LOG_SIGMA.  With a* = act[b], smin2 = sigma_min^2, w_b = weight[b] (NULL = 1), vm_bc = valid or 1, gamma_b = sample_gamma[b]
 * (NULL = a->gamma):
 *   var(rho) = e(rho) + smin2;  LOG_SIGMA: e = exp(2 clamp(rho, -8, 4)), de/drho = 2 e inside the clamp and exactly 0 outside;
 *              otherwise e = softplus(rho)^2 (rho > 20: softplus = rho), de/drho = 2 softplus(rho) sigmoid(rho)
 *   a' = first arg-max of q_after_online[b][M(c, .)];  mt = q_after_target[b][M(c, a')];  vt = var(q_after_target[b][S(c, a')])
 *   m  = the y of vdqn_td_loss in its order: qa = mt * (1 - term); y = rew + gamma_b * qa; rect clip
 *   g  = gamma_b * (1 - term);  v = max((g * g) * vt, smin2);  mu = q_before[b][M(c, a*)];  s2 = var(q_before[b][S(c, a*)]);  d = mu - m
 *   bit 0 clear: L = KL(N(m, v) || N(mu, s2)) = 0.5 (log(s2 / v) + (v + d^2) / s2 - 1),  dL/dmu = d / s2,  dL/ds2 = 0.5 (s2 - v - d^2) / s2^2
 *   bit 0 set:   L = KL(N(mu, s2) || N(m, v)) = 0.5 (log(v / s2) + (s2 + d^2) / v - 1),  dL/dmu = d / v,   dL/ds2 = 0.5 (s2 - v) / (v s2)
 *   loss += inv_count * sum w_b vm_bc L       dq[b][M(c, a*)] = dL/dmu w_b vm_bc inv_count
 *   dq[b][S(c, a*)] = dL/ds2 de/drho w_b vm_bc inv_count      every other column 0      (no gradient through m, v, a')
 *   err_out[b] = sum_c |d_bc| vm_bc / n_cat                   (NULL ok; the bits vdqn_td_loss_weighted writes for the same mean columns)
 *   stats[0] += inv_count * sum vm_bc sqrt(s2)                stats[1] += inv_count * sum vm_bc d^2 / s2     (f32[2], pre-zeroed, NULL ok)
 * `deterministic` sums in one block in a fixed order; q_copy (the mean columns) and dq_f32 as in vdqn_td_loss.  A row whose action
 * is outside [0, n_act) writes zeros.  Fails by name, before any launch, for a null required pointer, bad dims,
 * 2 * n_cat * n_act > ldq, batch * ldq >= 2^31, linear != 0, loss_kind != 0 (a KL has no Huber form), unknown flag bits and a
 * sigma_min that is not finite or outside [1e-4, 10]. */
int vdqn_td_loss_dist(const vdqn_td_args* a, const float* weight /* NULL = 1 */, float* err_out /* NULL ok */,
                      const float* sample_gamma /* NULL = a->gamma */, int32_t flags, float sigma_min,
                      float* stats /* f32[2], pre-zeroed, NULL ok */, void* stream);
/* The two moments of every (category, action) from rows in vdqn_td_loss_dist's layout: out (f32 [batch][n_cat][n_act][2], 8-byte
 * aligned) [..][0] = the mean, [..][1] = var(rho), by the same device function as the loss.  Only bit 1 of flags is read. */
int vdqn_dist_moments(const float* q_rows, float* out, int32_t batch, int32_t n_cat, int32_t n_act, int32_t ldq, int32_t flags,
                      float sigma_min, void* stream);
/* Discrete batch-constrained Q-learning in one launch (BCQ, Fujimoto et al. 2019; video_dqn_amd/csrc/bcq.hip): a row of ldq columns
 * holds Q(c, a) at column c * n_act + a and the behaviour logit i(a) at column n_cat * n_act + a (one set per sample: the logged
 * action is shared by all categories), so n_cat * n_act + n_act <= ldq.  With a* = act[b], w_b = weight[b] (NULL = 1), vm_bc = valid
 * or 1, gamma_b = sample_gamma[b] (NULL = a->gamma), i = q_before[b][n_cat*n_act + .] (the logits at s) and
 * i' = q_after_online[b][n_cat*n_act + .] (the ONLINE logits at s'):
 *   allowed at s':  m' = max_a i'_a;  lt = (float)log((double)threshold) (threshold 0: -inf);  a is allowed iff (i'_a - m') > lt in f32
 *                   (the arg-max of i' always is, as threshold < 1: the set is never empty, and no exponential is taken)
 *   a' = first maximum of q_after_online[b][c*n_act + a] over the allowed a;  Qa = q_after_target[b][c*n_act + a']
 *   y, d as vdqn_td_loss in its order: Qa *= (1 - term); y = rew + gamma_b * Qa; rect clip; d = Qb - y;  l(d), dl(d) by loss_kind
 *   behaviour loss, per sample (not per category, no valid mask): m = max_a i_a;  S = sum_a expf(i_a - m)
 *     ce_b = logf(S) + (m - i_{a*});  reg_b = (sum_a i_a^2) / n_act;  L_B = bc_weight * (ce_b + logit_reg * reg_b)
 *     dL_B/di_a = bc_weight * (expf(i_a - m) / S - [a == a*] + logit_reg * 2 i_a / n_act)
 *   loss += inv_count * sum_bc w_b vm_bc l(d_bc) + n_cat * inv_count * sum_b w_b L_B      (the TD terms are means over B*C with
 *           inv_count = 1 / (n_cat * global batch); the behaviour terms are means over B, hence the factor n_cat * inv_count)
 *   dq[b][c*n_act + a*] = dl(d) w_b vm_bc inv_count      dq[b][n_cat*n_act + a] = dL_B/di_a w_b n_cat inv_count      every other column 0
 *   (no gradient through i', a' or y)             err_out[b] = sum_c |d_bc| vm_bc / n_cat   (priorities follow the TD error alone)
 *   stats[0] += n_cat * inv_count * sum_b ce_b                              (the unweighted mean cross-entropy)
 *   stats[1] += inv_count * sum_bc vm_bc [a' != the free arg-max]           (the share of targets the constraint changes)
 *   stats[2] += n_cat * inv_count * sum_b [first arg-max of i == a*]        (behaviour accuracy)
 * With threshold 0 every action is allowed: the taken-action columns of dq and err_out are then vdqn_td_loss_weighted's bits
 * (vdqn_td_loss_nstep's with sample_gamma).  `deterministic` sums in one block in a fixed order; q_copy and dq_f32 as in
 * vdqn_td_loss.  A row whose action is outside [0, n_act) writes zeros and adds nothing.  Fails by name, before any launch, for a
 * null required pointer, use_valid without valid, bad dims, n_act < 2, n_cat * n_act + n_act > ldq, batch * ldq >= 2^31, a dtype
 * other than F32 / BF16, loss_kind outside {0, 1}, linear != 0, a threshold that is not finite or outside [0, 1), a bc_weight that is
 * not finite or <= 0 and a logit_reg that is not finite or < 0. */
int vdqn_td_loss_bcq(const vdqn_td_args* a, const float* weight /* NULL = 1 */, float* err_out /* NULL ok */,
                     const float* sample_gamma /* NULL = a->gamma */, float threshold, float bc_weight, float logit_reg,
                     float* stats /* f32[3], pre-zeroed, NULL ok */, void* stream);
/* The constrained read-out of rows in vdqn_td_loss_bcq's layout, by the same allowed-set device function as the loss:
 * q_out[b][c][a] = q_rows[b][c*n_act + a], or -inf where action a is not allowed by the row's own logits (its arg-max over a is the
 * BCQ policy); prob_out[b][a] (NULL ok) = the softmax of the logits.  Fails by name for a null q_rows / q_out, bad dims, n_act < 2,
 * n_cat * n_act + n_act > ldq, batch * ldq >= 2^31 and a threshold that is not finite or outside [0, 1). */
int vdqn_bcq_constrain(const float* q_rows, float* q_out /* [batch][C][A] */, float* prob_out /* [batch][A], NULL ok */,
                       int32_t batch, int32_t n_cat, int32_t n_act, int32_t ldq, float threshold, void* stream);
/* Held-out validation metrics of the same loss, forward only: the `eval_losses` list the reference reserves and never fills
 * (train_q_network.py:183-186) and its `# checkpoint and eval` (:240).  One launch adds eight sums per category into
 * acc (device f64 [n_cat][8], 8-byte aligned, ACCUMULATED into: the caller zeroes it once per validation pass).  With d, y and l(d)
 * exactly vdqn_td_loss's f32 arithmetic, pen = vdqn_td_loss_cql's logsumexp_a q_before[b,c,:] - q_before[b,c,act[b]] (exactly 0 when
 * n_act == 1) and vm = use_valid ? valid[b,c] : 1, every term is formed in f32, multiplied by vm last, converted to f64 and summed
 * over b:
 *   acc[c][0] += sum vm                 acc[c][1] += sum l(d) vm             acc[c][2] += sum |d| vm
 *   acc[c][3] += sum Q(s,c,act[b]) vm   acc[c][4] += sum max_a Q(s,c,a) vm   acc[c][5] += sum y vm
 *   acc[c][6] += sum pen vm             acc[c][7] += sum [argmax_a Q(s,c,.) == act[b]] vm   (first maximum)
 * One block per category, no atomics, a fixed summation order that depends on batch, n_cat and n_act alone (written out in
 * video_dqn_amd/csrc/eval.hip): two runs agree bit for bit, and each table entry takes one f64 addition of the launch's sum.
 * Reads q_before, q_after_online, q_after_target, act, rew, term, valid (when use_valid), batch, n_cat, n_act, ldq, gamma,
 * clip_rect, linear, use_valid, loss_kind; ignores loss, dq, dq_f32, inv_count, dtype, deterministic, q_copy (NULL / 0 allowed).  Non-finite
 * Q values are not special-cased; a row whose action is outside [0, n_act) adds nothing.  Fails by name before any launch for a
 * null required pointer, batch / n_cat / n_act < 1, n_cat * n_act > ldq, loss_kind outside {0, 1}, acc not 8-byte aligned. */
int vdqn_td_eval(const vdqn_td_args* a, double* acc, void* stream);
/* What a head algorithm adds to the held-out metrics (the same unfilled `eval_losses`, train_q_network.py:183-186,240): one launch
 * adds eight sums per category and one row of per-sample sums into acc_head (device f64 [n_cat + 1][8], 8-byte aligned,
 * ACCUMULATED into), beside vdqn_td_eval's table, which it leaves alone.  Rows in the layout of the algorithm's loss entry; every
 * quantity is that loss launch's own f32 statement of it (the same device functions, contraction off) with the scalar gamma, no
 * importance weight and no per-sample discount; each term is multiplied by vm = use_valid ? valid[b,c] : 1 last and summed in f64 in
 * vdqn_td_eval's fixed order (n_cat + 1 blocks, no atomics: two runs agree bit for bit).  A row whose action is outside [0, n_act)
 * adds nothing.  Row c < n_cat, slots 0 .. 7 (symbols as in the loss entries' comments above):
 *   vdqn_td_eval_iql   q_after_target holds the TARGET network's rows AT S (as vdqn_td_loss_iql's), q_after_online the online rows at s':
 *                      vm | L_V = omega u^2 | u = Q_target(s, a*) - V(s) | l(d), d = Q(s, a*) - (rew + gamma (1 - term) V(s')), by loss_kind
 *                      | |d| | V(s) | y | [u > 0]
 *   vdqn_td_eval_dist  vm | L, the KL in the direction of flags bit 0, clamped at 0 | sqrt(s2) | d^2 / s2 | 0.5 (log s2 + d^2 / s2): the
 *                      Gaussian NLL of the backup's mean, constant dropped | [d^2 <= s2] (one-sigma coverage: 0.683 when calibrated)
 *                      | sqrt(v), the backup's sigma | sqrt(var(rho(c, k*))), k* = first arg-max of the means at s
 *   vdqn_td_eval_bcq   vm | l(d), d against the constrained target | |d| | y | [a' != the free arg-max] | [kc == a*], kc = first maximum
 *                      of Q(s, c, .) over the actions the logits AT S allow (the policy vdqn_bcq_constrain's read-out deploys)
 *                      | [kc != the free first arg-max of Q(s, c, .)] | Q(s, c, kc)
 * Row n_cat: untouched by _iql and _dist; _bcq adds per sample (unweighted, no valid mask, i = the logits at s):
 *   1 | ce_b | [first arg-max of i == a*] | reg_b | actions allowed at s | softmax(i)[a*] | actions allowed at s' (online logits) | 0
 * Each fails by name, before any launch, for what its loss entry refuses of the fields it reads: a null required pointer, use_valid
 * without valid, bad dims, columns that do not fit ldq, batch * ldq >= 2^31, linear != 0, loss_kind outside {0, 1} (_dist: != 0),
 * its scalars out of range (expectile outside [0.5, 1); unknown flag bits, sigma_min outside [1e-4, 10]; n_act < 2, threshold outside
 * [0, 1)) and an acc_head that is not 8-byte aligned.  loss, dq, dq_f32, inv_count, dtype, deterministic, q_copy are ignored. */
int vdqn_td_eval_iql(const vdqn_td_args* a, float expectile, double* acc_head, void* stream);
int vdqn_td_eval_dist(const vdqn_td_args* a, int32_t flags, float sigma_min, double* acc_head, void* stream);
int vdqn_td_eval_bcq(const vdqn_td_args* a, float threshold, double* acc_head, void* stream);

/* Ground-truth branch (train_q_network.py:170-178): l = 0.5 (Qb*mask - gt)^2, mask = !isnan(gt) when
 * value_learning, else l = 0.5 (Qb - gt)^2.  gt is f32 [batch][n_cat] (NaN allowed). */
int vdqn_gt_loss(const float* q_before, const int64_t* act, const float* gt, float* loss, void* dq, float* dq_f32,
                 int32_t batch, int32_t n_cat, int32_t n_act, int32_t ldq, float inv_count, int32_t value_learning,
                 int32_t dtype, void* stream);

/* The ResNet stem in one kernel: conv1 7x7/2 (as the 4x4/1 convolution over the packed operand of vdqn_pack_input,
 * weights [64][4][1][64] with BatchNorm folded, f32 bias[64]) + ReLU + MaxPool2d(3, 2, 1)
 * (torchvision resnet.py conv1/bn1/relu/maxpool; archs/HabitatDQNMultiAction.py:30).  Writes pool [n][56][56][64] and
 * the argmax codes idx (as vdqn_maxpool_fwd); the 112x112x64 convolution output is never stored.  Results are
 * bit-identical to vdqn_conv2d followed by vdqn_maxpool_fwd.  idx may be NULL for frames that never see a backward pass
 * (the target pass, whose result is `.detach()`ed, and the s' rows of the online pass, which only feed an argmax: train_q_network.py:140-142,148,155-156 — the reference builds their graphs and never back-propagates through them): pool is the same,
 * the arg-max bytes are not computed. */
int vdqn_stem_conv_pool(const void* t_in, const void* wt, const float* bias, void* pool, void* idx, int32_t n_img,
                        int32_t dtype, void* stream);
/* The same with arg-max bytes for the first n_idx_img images only (0 <= n_idx_img <= n_img; idx may be NULL when it is 0): one
 * launch over [s; s'] of the online pass, where only the s rows see loss.backward() (train_q_network.py:131,142,226). */
int vdqn_stem_conv_pool_n(const void* t_in, const void* wt, const float* bias, void* pool, void* idx, int32_t n_img,
                          int32_t n_idx_img, int32_t dtype, void* stream);

/* conv1's weight gradient straight from the POOLED gradient (the extra_capacity stem in bf16): what vdqn_maxpool_bwd(g_pool, idx)
 * followed by vdqn_conv2d_wgrad on the packed stem geometry computes, without the 112 x 112 x 64 gradient of conv1's output
 * ever being stored (autograd's max_pool2d backward + conv1 weight gradient behind loss.backward(), train_q_network.py:226;
 * torchvision resnet stem reached from archs/HabitatDQNMultiAction.py:30).  g_pool [n][56][56][64] bf16, idx as written by
 * vdqn_stem_conv_pool / vdqn_maxpool_fwd, t_in the packed frames of vdqn_pack_input; dw [64][4][64] f32 is ACCUMULATED into
 * (f32 atomics; with a workspace of vdqn_stem_wgrad_pool_workspace_bytes(n_img) bytes: per-block partial copies summed in
 * block order = deterministic).  The gradient tiles the kernel builds in LDS are bit-identical to vdqn_maxpool_bwd's output. */
int vdqn_stem_wgrad_pool(const void* g_pool, const uint8_t* idx, const void* t_in, float* dw, int32_t n_img, void* workspace,
                         int64_t workspace_bytes, void* stream);
int64_t vdqn_stem_wgrad_pool_workspace_bytes(int32_t n_img);

/* The stem's DATA gradient, dL/d(frame), from the pooled gradient: autograd's max_pool2d backward followed by conv1's input
 * gradient, `torch.autograd.grad(q, frames)` through resnet.maxpool / relu / bn1 / conv1 (torchvision resnet stem reached from
 * archs/HabitatDQNMultiAction.py:30; the reference itself never asks for it).  g_pool [n][56][56][64] (already masked by
 * pool > 0), idx as written by vdqn_stem_conv_pool / vdqn_maxpool_fwd, wt conv1's FORWARD operand [64][4][1][64] (BatchNorm
 * folded), in the dtype's storage type; out f32 NCHW [n][3][224][224], every element written.  scale: HOST pointer to three f32,
 * one per colour channel, multiplied into the result as one f32 product (NULL = 1).  dtype VDQN_BF16: one fused kernel, no
 * workspace, no atomics (run-to-run bit-identical).  VDQN_F32 / VDQN_F32X3: vdqn_maxpool_bwd into `workspace`
 * (vdqn_stem_input_grad_workspace_bytes) and an f32 kernel.  Refused with a message: NULL or not 16-byte aligned pointers,
 * n_img <= 0, an n_img whose g_pool exceeds the bf16 kernel's 2 GiB buffer addressing, a workspace that is too small.
 * Added without a change of vdqn_abi_version(). */
int vdqn_stem_input_grad(const void* g_pool, const uint8_t* idx, const void* wt, const float* scale, float* out, int32_t n_img,
                         int32_t dtype, void* workspace, int64_t workspace_bytes, void* stream);
/* Bytes of that workspace: 0 for VDQN_BF16; -1 for n_img <= 0 or an unknown dtype.  Host only. */
int64_t vdqn_stem_input_grad_workspace_bytes(int32_t n_img, int32_t dtype);

/* Row-wise softmax over the first n_valid columns of x[rows][ld] (f32), written to y[rows][ld] (other columns 0):
 * `torch.softmax(x, dim=1)` of the inverse-action model's 3-way output (archs/inverse_action2.py:95). n_valid <= 64. */
int vdqn_softmax_rows(const float* x, float* y, int32_t rows, int32_t ld, int32_t n_valid, void* stream);

/* Training of the inverse-action model (train_inverse_model.py:86-112): mean nn.CrossEntropyLoss over `rows` samples of
 * f32 logits[rows][ld] (first n_cls columns) and its gradient (softmax - onehot) * inv_count as `dtype` elements;
 * dropout with a caller-supplied 0/1 mask: out = x * mask * scale (forward and backward); y += alpha * x (Adam's
 * weight_decay term, train_inverse_model.py:190). */
int vdqn_softmax_ce(const float* logits, const int64_t* labels, float* loss, void* dlogits, int32_t rows, int32_t ld,
                    int32_t n_cls, float inv_count, int32_t dtype, void* stream);
int vdqn_mask_scale(const void* x, const void* mask, void* out, int64_t n, float scale, int32_t dtype, void* stream);
int vdqn_axpy(float* y, const float* x, float alpha, int64_t n, void* stream);

/* torch.optim.Adam step (train_q_network.py:124,227) over one flat f32 range.  vdqn_adam, vdqn_adam_scaled and vdqn_adam_polyak
 * (below) are three instances of one kernel and share one element update, in which every fma rounds once and every other
 * product, sum and quotient rounds on its own, in the float4 body and in the scalar tail (the n % 4 last elements) alike:
 *   m = fma(1-b1, g, b1 * m);   v = fma((1-b2) * g, g, b2 * v);
 *   p = fma(-(lr / (1-b1^t)), m / fma(sqrtf(v), 1 / sqrt(1-b2^t), eps), p)
 * so an element's result does not depend on its position in the range or on the entry.  Hyper-parameters are doubles like
 * torch's python scalars (1-b2 is formed in double before rounding to f32).  All three check alike and fail by their own name
 * before any launch: no null pointer, n >= 1, step >= 1, p / g / m / v (and target) 16-byte aligned. */
int vdqn_adam(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
              double beta2, double eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Gradient-norm clipping and AdamW on the device (video_dqn_amd/csrc/optim.hip): the clip coefficient goes from the norm kernels
 * to the Adam launch through device memory, nothing is read back.  The reference itself trains with plain Adam(lr=1e-3)
 * (train_q_network.py:124); these replace what a torch loop would add around it.
 * ------------------------------------------------------------------------------------------------ */
/* Bytes of the norm workspace for up to n_ranges (1..8) ranges; -1 outside that.  Host only. */
int64_t vdqn_clip_workspace_bytes(int32_t n_ranges);
/* torch.nn.utils.clip_grad_norm_, part 1: the f64 sum of squares of g[0, n) (any 4-byte aligned start, n >= 1) as per-block
 * partials into slot `slot` (0..7) of the workspace (8-byte aligned).  Fixed order, no atomics: the grid depends on n alone and
 * block b writes partial b, so the result is bit-identical run to run; the order is written out in optim.hip. */
int vdqn_grad_sumsq(const float* g, int64_t n, void* workspace, int32_t slot, void* stream);
/* torch.nn.utils.clip_grad_norm_, part 2: one block adds the partials of slots 0 .. n_ranges-1 (each written by a
 * vdqn_grad_sumsq ordered in front of this launch) in index order in f64 and writes out[0] = norm = sqrt(sum),
 * out[1] = coef = min(1, max_norm / (norm + 1e-6)), computed in f64 and rounded to f32 once.  max_norm > 0.  A non-finite norm
 * is not special-cased (a NaN norm gives a NaN coef, as torch's does). */
int vdqn_clip_finalize(const void* workspace, int32_t n_ranges, double max_norm, float* out, void* stream);
/* torch.optim.AdamW step on gradients scaled by a device-side coefficient (the multiply clip_grad_norm_ does in place):
 *   gs = g * coef[0] (coef == NULL: 1);  p = p * (1 - lr * weight_decay);  then vdqn_adam's update with gs for g,
 * both products rounded on their own: with coef[0] == 1 and weight_decay == 0 it writes vdqn_adam's bits.  g itself is left as it
 * is.  weight_decay finite and >= 0; coef 4-byte aligned (checked here as in vdqn_adam_polyak). */
int vdqn_adam_scaled(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
                     double beta2, double eps, double weight_decay, const float* coef, void* stream);

/* Soft (Polyak) target update over one flat f32 range, target <- target + tau (p - target): what a DQN loop does after every
 * optimiser step in place of the hard copy every TARGET_UPDATE_INTERVAL updates.  The arithmetic is torch.lerp's two-branch rule
 * with every product rounded to f32 on its own (nothing contracted into a fused multiply-add), per element:
 *   d = p - t                                     (rounded)
 *   tau <  0.5:  t' = t + tau_f * d               tau_f = (float)tau; the product is rounded, then the sum
 *   tau >= 0.5:  t' = p - d * omt_f               omt_f = (float)(1.0 - tau), the difference formed in double
 * so tau = 1 writes p's bits, p == t leaves t's bits, and three lines of numpy float32 reproduce it bit for bit
 * (tests/polyak_oracle.py lerp_f32).  n >= 1, both pointers 16-byte aligned (float4 body, scalar tail), the two ranges disjoint,
 * tau finite in (0, 1]; anything else fails by name before a launch. */
int vdqn_polyak(float* target, const float* p, int64_t n, double tau, void* stream);
/* vdqn_adam_scaled and vdqn_polyak in one launch: p, m, v are updated by vdqn_adam_scaled's element update (coef == NULL and
 * weight_decay == 0: vdqn_adam's bits), then the new p, still in registers, is lerped into target[0, n) by the rule above — one
 * more read and one more write of `target` per element, where a second launch would stream p a third time.  Arguments as
 * vdqn_adam_scaled's; target 16-byte aligned like the others, its range disjoint from theirs (refused by name otherwise); tau finite
 * in (0, 1]. */
int vdqn_adam_polyak(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, double lr, double beta1,
                     double beta2, double eps, double weight_decay, const float* coef /* NULL = 1 */,
                     float* target, double tau, void* stream);

/* torch.nn.BatchNorm2d in train mode over an NHWC conv output y[n_img][hw][c] (ARCHITECTURE='basic':
 * archs/HabitatDQNMultiAction.py:32-34,37-40 keeps the ResNet in train mode).  Images are sample-major, frame-minor;
 * image i belongs to statistic group (i / imgs_per_half) * num_frames + i % num_frames — one group per model call and
 * frame slot, the minibatches the reference normalises over (:49-51; train_q_network.py:131,142).
 *   z = relu?( (y - mean_g) * rstd_g * gamma + beta (+ resid) );   biased variance, eps inside the sqrt
 *   running_* (may be NULL): updated once per group, in group order, with `momentum` and the unbiased variance
 * work: f32 [groups][6][c] = mean, rstd, scale, shift and two sums; the forward fills it, the backward reads it. */
int vdqn_bn_train_fwd(const void* y, const void* resid, void* z, const float* gamma, const float* beta,
                      float* running_mean, float* running_var, float* work, int32_t n_img, int32_t hw, int32_t c,
                      int32_t num_frames, int32_t imgs_per_half, int32_t relu, float momentum, float eps, int32_t dtype,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* dy = gamma * rstd * (g - mean(g) - xhat * mean(g * xhat)) per group; dgamma/dbeta (may be NULL) = sums over all
 * groups of g*xhat / g.  dy may alias g.  `work` must be the array the forward of the same tensor filled. */
int vdqn_bn_train_bwd(const void* g, const void* y, void* dy, float* work, float* dgamma, float* dbeta, int32_t n_img,
                      int32_t hw, int32_t c, int32_t num_frames, int32_t imgs_per_half, int32_t dtype, void* workspace,
                      int64_t workspace_bytes, void* stream);
/* Deterministic mode of the two calls above (train_q_network.py:88-89 pins cudnn.deterministic): with `workspace` (>= this many
 * bytes, 16-byte aligned; NULL = f32 atomics) every block stores its partial statistic sums and a second kernel adds them in
 * block order — two runs are bit-identical.  -1 on invalid sizes. */
int64_t vdqn_bn_train_workspace_bytes(int32_t n_img, int32_t hw, int32_t c, int32_t num_frames, int32_t imgs_per_half);
/* AdaptiveAvgPool2d(1) of the ResNet (torchvision resnet.py avgpool) on NHWC x[n_img][hw][c] -> out[n_img][c], and its
 * backward fused with the mask of the ReLU that produced x: gx = (x > 0) * g / hw. */
int vdqn_avgpool_fwd(const void* x, void* out, int32_t n_img, int32_t hw, int32_t c, int32_t dtype, void* stream);
int vdqn_avgpool_bwd(const void* g, const void* x, void* gx, int32_t n_img, int32_t hw, int32_t c, int32_t dtype,
                     void* stream);

/* ------------------------------------------------------------------------------------------------
 * Engine level: the whole HabitatDQNMultiAction network and one TD update.
 * ------------------------------------------------------------------------------------------------ */
typedef struct vdqn_net_config {
  int32_t action_dim;      /* A: 3, or 1 for VALUE_LEARNING/ONE_ACTION (train_q_network.py:38-41) */
  int32_t num_classes;     /* 5 */
  int32_t num_frames;      /* F: 1, or 4 for PANORAMA/PREVIOUS_IMAGES (archs/...:16-19); any F >= 1 accepted */
  int32_t extra_capacity;  /* 1: ARCHITECTURE 'extra_capacity' (BatchNorm on running stats, conv+MLP head);
                              0: 'basic' (defaults.py:14 — train-mode BatchNorm, average pool + one Linear) */
  int32_t dtype;           /* VDQN_F32 | VDQN_BF16 | VDQN_F32X3 (sizes, layouts and tensors as VDQN_F32) */
  int32_t max_batch;       /* largest per-call sample count B the workspaces are sized for */
  int32_t deterministic;   /* 1: run-to-run bit-identical updates (the reference's cudnn.deterministic = True,
                              train_q_network.py:88-89): weight gradients through the two-stage ordered reduction of
                              vdqn_conv2d_wgrad (its workspace is part of `bwd`), the loss summed by one block,
                              ARCHITECTURE='basic': the train-mode BatchNorm statistics through the ordered two-stage sums
                              of vdqn_bn_train_fwd/bwd (workspace inside `acts`). */
} vdqn_net_config;

typedef struct vdqn_net vdqn_net;

int vdqn_net_create(const vdqn_net_config* cfg, vdqn_net** out);
/* vdqn_net_create with a state-value head behind the Q head (implicit Q-learning, vdqn_net_td_forward_iql).  value_head = 0 is
 * vdqn_net_create: the same tables, offsets and bits.  value_head = 1: the Q layer (`top.4`, or `top` in 'basic') computes
 * action_dim * num_classes + num_classes columns, Q(c, a) at c * action_dim + a and V(c) behind them; its extra rows are the
 * parameters `value.weight` [num_classes, in] and `value.bias` [num_classes], registered directly behind `<top>.weight` and
 * `<top>.bias` in the flat arrays (the layer's operand is one contiguous block) with param_ids after the reference's.  Every
 * entry that reads Q (vdqn_net_forward, vdqn_net_td_forward*, vdqn_net_td_eval, vdqn_net_backward_begin) keeps reading the
 * first action_dim * num_classes columns and leaves the V columns of dq at 0.  Needs action_dim >= 2 and
 * action_dim * num_classes + num_classes <= 64; value_head outside {0, 1} fails. */
int vdqn_net_create_v(const vdqn_net_config* cfg, int32_t value_head, vdqn_net** out);
int vdqn_net_value_head(const vdqn_net* net); /* 1 when the net was created with the value head, else 0 */
/* vdqn_net_create_v with a spread head behind the Q head (Gaussian distributional Q-learning, vdqn_net_td_forward_dist).
 * spread_head = 0 is vdqn_net_create_v(cfg, value_head, out).  spread_head = 1: the Q layer computes 2 * action_dim * num_classes
 * columns, the mean Q(c, a) at c * action_dim + a and the spread parameter rho(c, a) action_dim * num_classes columns behind it; the
 * extra rows are the parameters `spread.weight` [action_dim * num_classes, in] and `spread.bias` [action_dim * num_classes],
 * registered directly behind `<top>.weight` and `<top>.bias` with param_ids after the reference's, as `value.*` are.  Every entry
 * that reads Q keeps reading the first action_dim * num_classes columns and leaves the spread columns of dq at 0.  Fails by name
 * for value_head and spread_head together (out of scope), 2 * action_dim * num_classes > 64 and a flag outside {0, 1}. */
int vdqn_net_create_d(const vdqn_net_config* cfg, int32_t value_head, int32_t spread_head, vdqn_net** out);
int vdqn_net_spread_head(const vdqn_net* net); /* 1 when the net was created with the spread head, else 0 */
/* vdqn_net_create_d with a policy head behind the Q head (discrete batch-constrained Q-learning, vdqn_net_td_forward_bcq).
 * policy_head = 0 is vdqn_net_create_d(cfg, value_head, spread_head, out): the same tables and bits.  policy_head = 1: the Q layer
 * computes action_dim * num_classes + action_dim columns, Q(c, a) at c * action_dim + a as ever and the behaviour logit i(a) at
 * action_dim * num_classes + a; the extra rows are the parameters `policy.weight` [action_dim, in] and `policy.bias` [action_dim],
 * registered directly behind `<top>.weight` and `<top>.bias` with param_ids after the reference's, as `value.*` and `spread.*` are.
 * Every entry that reads Q keeps reading the first action_dim * num_classes columns and leaves the logit columns of dq at 0.
 * Fails by name for policy_head together with value_head or spread_head (out of scope), action_dim < 2,
 * action_dim * num_classes + action_dim > 64 and a flag outside {0, 1}. */
int vdqn_net_create_p(const vdqn_net_config* cfg, int32_t value_head, int32_t spread_head, int32_t policy_head, vdqn_net** out);
int vdqn_net_policy_head(const vdqn_net* net); /* 1 when the net was created with the policy head, else 0 */
/* The engine runs weight gradients and the target-network forward on a second, internal HIP stream (joined back
 * into the caller's stream before their results are consumed).  on = 0 serialises everything on the caller's
 * stream (used for per-kernel roofline timing, where each kernel must have the chip to itself).  Default: on
 * (or off when the environment has VDQN_NO_OVERLAP=1). */
int vdqn_net_set_overlap(vdqn_net* net, int on);
void vdqn_net_destroy(vdqn_net* net);

/* Parameter table: the reference's named_parameters()/buffers as slices of two flat f32 arrays.
 * kind: 0 trainable parameter (offset into `params`, gradient/Adam state at the same offset),
 *       1 frozen parameter (resnet.fc.*: never receives a gradient; stored after the trainable range),
 *       2 BatchNorm running_mean, 3 running_var (offsets into `bnstats`).
 * `param_id` is the index in the reference's model.parameters() order (Adam state_dict ids). */
typedef struct vdqn_param_info {
  char name[96];
  int64_t offset;
  int64_t numel;
  int32_t ndim;
  int32_t shape[4];
  int32_t kind;
  int32_t param_id;
  int32_t stage;     /* backward stage (0 head+layer4, 1 layer3, 2 layer2+layer1+stem) that completes its grad */
} vdqn_param_info;
int vdqn_net_num_params(const vdqn_net* net);
int vdqn_net_param_info(const vdqn_net* net, int index, vdqn_param_info* out);
int64_t vdqn_net_params_numel(const vdqn_net* net);     /* total flat params (trainable + frozen) */
int64_t vdqn_net_trainable_numel(const vdqn_net* net);  /* prefix that has gradients / Adam state */
int64_t vdqn_net_bnstats_numel(const vdqn_net* net);
/* [begin,end) of the flat gradient completed by backward stage s (for bucketed all-reduce) */
int vdqn_net_stage_range(const vdqn_net* net, int stage, int64_t* begin, int64_t* end);

/* Workspace sizes in bytes.  packed = folded/packed weights of ONE network instance (online or target);
 * acts = activations of one forward over `n_samples` samples; bwd = gradient workspaces of one backward. */
int64_t vdqn_net_packed_bytes(const vdqn_net* net);
int64_t vdqn_net_acts_bytes(const vdqn_net* net, int32_t n_samples);
int64_t vdqn_net_bwd_bytes(const vdqn_net* net, int32_t n_samples);

/* Byte offset of a named tensor inside the `acts` / `bwd` workspaces (for layer-by-layer parity tests and
 * debuggers); -1 if the name is unknown.  acts names: t_in c1 pool idx h0..h7 o0..o7 ds2 ds4 ds6 f8 l0 l1 q qf;
 * bwd names: dq g_l1 g_l0 g_f8 g_o0..g_o7 g_h0..g_h7 dsg2 dsg4 dsg6 g_pool g_c1, and dw:<layer> / db:<layer>
 * (f32 packed-layout weight-gradient accumulators, e.g. "dw:resnet.layer1.0.conv1"). */
int64_t vdqn_net_act_offset(const vdqn_net* net, int32_t n_samples, const char* name);
int64_t vdqn_net_bwd_offset(const vdqn_net* net, int32_t n_samples, const char* name);

/* Byte offset of one layer's region inside a `packed` workspace (vdqn_net_packed_bytes), for element-by-element tests of the
 * weight fold.  names: wf:<layer> (forward operand), wd:<layer> (data-gradient operand), bias:<layer> and scale:<layer> (f32
 * [co_pad] each), e.g. "wf:resnet.layer1.0.conv1".  -1 if the region or the layer is unknown, -2 for the wd region of a
 * layer that has no data-gradient operand (resnet.conv1).  Read only; added without a change of vdqn_abi_version(). */
int64_t vdqn_net_packed_offset(const vdqn_net* net, const char* name);

/* Fold eval-mode BatchNorm into the convolutions and pack the master weights (OIHW f32) into the K-contiguous
 * forward and data-gradient operands (set_train semantics: archs/HabitatDQNMultiAction.py:37-40 — in
 * extra_capacity all 20 BatchNorm layers run on running statistics). */
int vdqn_net_pack_weights(vdqn_net* net, const float* params, const float* bnstats, void* packed, int32_t with_dgrad,
                          void* stream);
/* with_dgrad is a flag word: bit 0 = also pack the data-gradient operands, bit 1 = do NOT fold BatchNorm (the
 * convolutions then produce the raw pre-BatchNorm output; used by the train-mode BatchNorm path of 'basic'). */

/* Forward of `n_samples` samples (n_samples * F frames).  frames: see vdqn_pack_input (src_kind).
 * q_out: f32 [n_samples][num_classes*action_dim] (HabitatDQNMultiAction.forward, archs/...:44-54). */
int vdqn_net_forward(vdqn_net* net, const void* packed, const void* frames, int32_t src_kind, int32_t n_samples,
                     void* acts, float* q_out, void* stream);

/* The frozen ResNet-18 trunk only (eval-mode BatchNorm folded): frames -> 512 x 7 x 7 features, left in the `acts`
 * workspace at vdqn_net_act_offset(net, n_samples, "o7") as NHWC [n_samples*F][7][7][512].  Serves the inverse-action
 * model (archs/inverse_action2.py:50-56,72-77: `self.resnet18(k)`, `self.resnet18(k_plus_one)`), whose head is built
 * from vdqn_conv2d calls by video_dqn_amd/inverse_model.py. */
int vdqn_net_trunk_forward(vdqn_net* net, const void* packed, const void* frames, int32_t src_kind, int32_t n_samples,
                           void* acts, void* stream);

/* SyncBN for ARCHITECTURE='basic' under data parallelism (without it N ranks are not one big batch).
 * `fn` must SUM-all-reduce `count` f32 at `buf` (device memory inside the `acts` workspace passed to the forward/step
 * call) across the ranks, in place, ordered on `stream`; it is called twice per BatchNorm layer and update (forward
 * statistics, backward sums).  world_size <= 1 or fn == NULL switches it off (per-rank statistics, torch DDP's default). */
typedef void (*vdqn_allreduce_fn)(void* user, float* buf, int64_t count, void* stream);
int vdqn_net_set_bn_sync(vdqn_net* net, vdqn_allreduce_fn fn, void* user, int32_t world_size);

/* ARCHITECTURE='basic' with the module in train mode (model.train(); archs/HabitatDQNMultiAction.py:37-40 leaves the
 * ResNet's BatchNorm layers in train mode): one model call over n_samples samples with batch statistics per frame
 * slot (features is applied slot by slot, :49-51); updates `bnstats` (momentum 0.1, unbiased variance) F times per
 * BatchNorm layer.  `packed` is a workspace of vdqn_net_packed_bytes that receives the un-folded weights. */
int vdqn_net_forward_train(vdqn_net* net, const float* params, float* bnstats, void* packed, const void* frames,
                           int32_t src_kind, int32_t n_samples, void* acts, float* q_out, void* stream);

/* One TD update's device work up to the flat gradient (train_q_network.py:222-226):
 *   online forward over [before; after] (2B samples, one pass — legal because BatchNorm is in eval mode),
 *   target forward over after, fused TD loss, full backward of the `before` half.
 * Split in calls so the host can overlap the gradient all-reduce of stage s with backward stage s+1:
 *   vdqn_net_td_forward -> vdqn_net_backward_stage(0..2)  (-> all-reduce) -> vdqn_adam on the flat range. */
typedef struct vdqn_step_args {
  const float* params;        /* online master parameters (flat) */
  float* bnstats;             /* running statistics; updated in place by every update when ARCHITECTURE='basic' */
  void* packed_online;        /* workspace: vdqn_net_packed_bytes */
  const void* packed_target;  /* packed target-network weights (refreshed by the caller on target sync) */
  const void* before;         /* frames of s  : [B][F] frames, src_kind layout */
  const void* after;          /* frames of s' */
  int32_t src_kind;
  int32_t batch;              /* B (per rank) */
  const int64_t* act;
  const float* rew;
  const float* term;
  const float* valid;
  const float* gt;            /* ground-truth targets [B][5] when train_on_ground_truth, else NULL */
  float gamma;
  float inv_count;            /* 1 / (num_classes * global_batch) */
  int32_t clip_rect, linear, use_valid, train_on_ground_truth, value_learning;
  void* acts_online;          /* vdqn_net_acts_bytes(2B) (B on the ground-truth branch) */
  void* acts_target;          /* vdqn_net_acts_bytes(B); NULL on the ground-truth branch */
  void* bwd;                  /* vdqn_net_bwd_bytes(B)   */
  float* grads;               /* flat f32 [trainable_numel] */
  float* loss;                /* f32 scalar (device) */
  float* q_before;            /* optional f32 [B][15] copy of Q(s) */
  int32_t loss_kind;          /* vdqn_td_args.loss_kind (TD branch only) */
  const void* packed_frames;  /* optional: the update's frames ALREADY packed by the caller — vdqn_pack_input's output for `before`
                                 ([B*F][115][115][16]) followed by the one for `after` (TD branch), in the network's dtype, complete
                                 on `stream` when vdqn_net_td_forward is called and untouched until the update's last
                                 vdqn_net_backward_stage has run.  `before` / `after` are then not read.  For loops whose frames
                                 arrive packed (or that pack the NEXT minibatch during this update: the loader of
                                 train_q_network.py:213 has it a step ahead — measured slower on one GPU).
                                 NULL: the update packs them itself. */
  int32_t acts_samples;       /* 0: `acts_online` is laid out as vdqn_net_td_forward leaves it (2B samples, B on the
                                 ground-truth branch).  > 0: `acts_online` is the workspace of ONE vdqn_net_forward call over that
                                 many samples (== batch) — the backward of a single model call, vdqn_net_backward_begin below. */
  const float* sample_weight; /* optional [batch] importance weights (prioritized replay): vdqn_net_td_forward launches
                                 vdqn_td_loss_weighted with them instead of vdqn_td_loss (TD branch only: the ground-truth branch
                                 then fails).  NULL: the reference loss. */
  float* sample_err;          /* optional [batch] per-sample error output of that launch; must be NULL when sample_weight is */
  const int32_t* aug_params;  /* optional device int32 [batch][4], 16-byte aligned: vdqn_net_td_forward packs `before` and `after`
                                 with vdqn_pack_input_aug (the same params for both) where it calls vdqn_pack_input otherwise; it
                                 then fails for src_kind != 0 and for packed_frames.  NULL: the plain pack. */
  const int32_t* aug_color;   /* optional device int32 [batch][4] {f_b, f_c, f_s, 0}, 16-byte aligned, indexed like aug_params (which must
                                 be given as well): vdqn_net_td_forward packs `before` and `after` with vdqn_pack_input_aug_color (the
                                 same factors for both).  NULL: no colour jitter.  vdqn_net_td_eval refuses it.  Added beside aug_params without a change
                                 of vdqn_abi_version(), as sample_gamma was: a binding that predates it fails the
                                 vdqn_abi_struct_size(6) comparison at load time. */
  const int32_t* aug_zoom;    /* optional device int32 [batch][4] {ax, ay, bx, by}, 16-byte aligned, indexed like aug_params (which must
                                 be given as well): vdqn_net_td_forward packs `before` and `after` with vdqn_pack_input_aug_zoom (the
                                 same window for both; aug_color, when given, goes through the same launch).  NULL: no zoom.
                                 vdqn_net_td_eval refuses it.  Added directly behind aug_color without a change of vdqn_abi_version(),
                                 as aug_color was. */
  const float* sample_gamma;  /* optional [batch] per-sample discount (n-step returns: `after`, rew, term are then those vdqn_nstep_walk
                                 folded along each sample's chain): the loss launch is vdqn_td_loss_nstep with it, and `gamma` is not
                                 read.  TD branch without `linear` only: vdqn_net_td_forward(_cql) fail by name otherwise, and
                                 vdqn_net_td_eval refuses it (validation stays one-step).  NULL: the scalar `gamma`.  Added at the end of
                                 the struct without a change of vdqn_abi_version(): a binding that predates it fails the
                                 vdqn_abi_struct_size(6) comparison at load time. */
} vdqn_step_args;
int vdqn_net_td_forward(vdqn_net* net, const vdqn_step_args* a, void* stream);
/* vdqn_net_td_forward with the conservative penalty (train_q_network.py:167,180): with cql_alpha > 0 the loss launch is
 * vdqn_td_loss_cql (sample_weight / sample_err passed through, NULL = unweighted) and cql_penalty (device f32 scalar, may be
 * NULL) is cleared beside `loss` and receives this call's share of the penalty; `loss` is then the full objective.  cql_alpha
 * == 0 is vdqn_net_td_forward: the same launches and bits.  Fails by name for a negative or non-finite cql_alpha, and with
 * cql_alpha > 0 for train_on_ground_truth and for action_dim == 1.  Either architecture, every compute mode. */
int vdqn_net_td_forward_cql(vdqn_net* net, const vdqn_step_args* a, float cql_alpha, float* cql_penalty, void* stream);
/* vdqn_net_td_forward_cql whose loss launch is vdqn_td_loss_mc(.., mc_return, mc_flags, mc_stats): mc_return is f32 [batch]
 * [num_classes] on the device, this update's alone (plain arguments: nothing is kept in the engine and no argument struct changes).
 * mc_stats (device f32[2], NULL ok) is cleared beside `loss`.  mc_return == NULL: vdqn_net_td_forward_cql, the same launches and
 * bits (mc_flags and mc_stats are then not looked at).  Otherwise fails by name, before any launch, for train_on_ground_truth,
 * linear, mc_flags 0 or with unknown bits, and bit 1 with cql_alpha == 0. */
int vdqn_net_td_forward_mc(vdqn_net* net, const vdqn_step_args* a, float cql_alpha, float* cql_penalty, const float* mc_return,
                           int32_t mc_flags, float* mc_stats, void* stream);
/* vdqn_net_td_forward for implicit Q-learning on a net with the value head (vdqn_net_create_v): the same update with two
 * differences.  The target pass runs over the `before` half of the packed frames (Q_target(s), where the others need Q_target(s')):
 * the same 3 * batch forward samples.  The loss launch is vdqn_td_loss_iql on the online pass's Q(s), V(s), V(s') and the target's
 * Q(s); iql_stats (device f32[2], NULL ok) is cleared beside `loss`.  sample_weight, sample_err, sample_gamma, aug_params,
 * aug_color, aug_zoom, packed_frames and the engine's `deterministic` behave as in vdqn_net_td_forward.  Fails by name, before
 * any launch, for a net without the value head, train_on_ground_truth, linear and an expectile outside [0.5, 1). */
int vdqn_net_td_forward_iql(vdqn_net* net, const vdqn_step_args* a, float expectile, float* iql_stats, void* stream);
/* vdqn_net_td_forward for Gaussian distributional Q-learning on a net with the spread head (vdqn_net_create_d): the same update —
 * the online pass over [s; s'], the target pass over s' — with vdqn_td_loss_dist as the loss launch on the three Q tensors;
 * dist_stats (device f32[2], NULL ok) is cleared beside `loss`.  sample_weight, sample_err, sample_gamma, aug_*, packed_frames and the
 * engine's `deterministic` behave as in vdqn_net_td_forward.  Fails by name, before any launch, for a net without the spread head,
 * train_on_ground_truth, linear, loss_kind != 0, unknown flag bits and a sigma_min outside [1e-4, 10]. */
int vdqn_net_td_forward_dist(vdqn_net* net, const vdqn_step_args* a, int32_t flags, float sigma_min, float* dist_stats, void* stream);
/* vdqn_net_td_forward for discrete batch-constrained Q-learning on a net with the policy head (vdqn_net_create_p): the same update —
 * the online pass over [s; s'], the target pass over s' — with vdqn_td_loss_bcq as the loss launch on the three Q tensors (the
 * logits it reads are the online pass's, at s and at s'); bcq_stats (device f32[3], NULL ok) is cleared beside `loss`.
 * sample_weight, sample_err, sample_gamma, aug_*, packed_frames and the engine's `deterministic` behave as in vdqn_net_td_forward.
 * Fails by name, before any launch, for a net without the policy head, train_on_ground_truth, linear, a threshold outside [0, 1), a
 * bc_weight that is not finite or <= 0 and a logit_reg that is not finite or < 0. */
int vdqn_net_td_forward_bcq(vdqn_net* net, const vdqn_step_args* a, float threshold, float bc_weight, float logit_reg, float* bcq_stats,
                            void* stream);
/* One held-out batch of a validation pass (the reference's unfilled `eval_losses`, train_q_network.py:183-186, and `# checkpoint
 * and eval`, :240): the online network over [before; after] (2 * batch samples), the target network over after on the side stream,
 * then vdqn_td_eval on the two f32 Q tensors (ldq 64) into acc (device f64 [num_classes][8], accumulated into).  Forward only, both
 * passes through the eval-mode path of either architecture ('basic' runs on its running statistics), no arg-max bytes, no backward
 * workspace; nothing of the training state is written and no host synchronisation happens.
 * Reads packed_online AS IT STANDS (the caller folds it once per validation pass with vdqn_net_pack_weights, flag word 0),
 * packed_target, before, after, src_kind, batch, act, rew, term, valid, gamma, clip_rect, linear, use_valid, loss_kind, acts_online,
 * acts_target; reads neither params, bnstats, bwd, grads, loss nor q_before.  1 <= batch and 2 * batch <= max_batch: the activation
 * layouts are those of 2 * batch and batch samples, which fit the workspaces of any larger batch, so a short last batch needs no
 * workspace of its own.  Refuses by name train_on_ground_truth, sample_weight, sample_err, aug_params, aug_color, aug_zoom, packed_frames,
 * sample_gamma (validation is one-step whatever the training target, so runs with different N_STEP are judged alike) and
 * acts_samples != 0. */
int vdqn_net_td_eval(vdqn_net* net, const vdqn_step_args* a, double* acc, void* stream);
/* vdqn_net_td_eval under a head algorithm (train_q_network.py:183-186,240): everything that entry does into acc, its refusals
 * included, then the algorithm's head metrics launch (vdqn_td_eval_iql / _dist / _bcq above) into acc_head (device f64
 * [num_classes + 1][8], accumulated into) behind it on `stream`.  _dist and _bcq read the two Q tensors the first launch read.  _iql
 * needs Q_target(s, a_data), and acts_target holds `batch` samples: a second target pass runs over the `before` half of the packed
 * frames into the same workspace, on the side stream BEHIND the first metrics launch (which reads Q_target(s') there), and the head
 * launch waits for it; the next entry on `stream` opens by making the side stream wait for `stream`, the head launch included.
 * One more batch-sample forward per validation batch.  Each fails by name, before any launch, for a net without the algorithm's head,
 * train_on_ground_truth, linear, its scalars out of range as the update's entry (vdqn_net_td_forward_iql / _dist / _bcq) refuses
 * them, a NULL or misaligned acc_head, and everything vdqn_net_td_eval refuses.  Added without a change of vdqn_abi_version(). */
int vdqn_net_td_eval_iql(vdqn_net* net, const vdqn_step_args* a, float expectile, double* acc, double* acc_head, void* stream);
int vdqn_net_td_eval_dist(vdqn_net* net, const vdqn_step_args* a, int32_t flags, float sigma_min, double* acc, double* acc_head, void* stream);
int vdqn_net_td_eval_bcq(vdqn_net* net, const vdqn_step_args* a, float threshold, double* acc, double* acc_head, void* stream);
/* Stage s of the backward pass (0: head + layer4, 1: layer3, 2: layer2, layer1, stem).  With the overlap on, the stage's weight
 * gradients and the kernel that writes its range of `grads` run on the engine's side stream: after the call returns that range is
 * complete on vdqn_net_grad_stream(net), NOT on `stream`, which goes straight on to the next stage's data gradients.  The call
 * for stage 2 makes `stream` wait for the side stream, so vdqn_adam on `stream` sees every gradient.  A consumer of one stage's
 * gradients (the data-parallel all-reduce) orders itself behind vdqn_net_grad_stream. */
int vdqn_net_backward_stage(vdqn_net* net, const vdqn_step_args* a, int32_t stage, void* stream);
/* Backward of ONE earlier vdqn_net_forward(net, packed, frames, .., B, acts, ..) call from a caller-supplied dL/dQ: what
 * torch.autograd runs for `before_values = model(before)` when the reference's own loop calls loss.backward()
 * (train_q_network.py:131,226) on the HIP-backed module (video_dqn_amd/model.py).  `a` carries params, bnstats, packed_online
 * (the SAME packed weights the forward used, packed with the data-gradient operands: vdqn_net_pack_weights bit 0),
 * acts_online = that call's `acts`, batch = acts_samples = B, bwd, grads; the loss fields are not read.  dq_f32 is
 * f32 [B][num_classes*action_dim].  This call clears the weight-gradient accumulators and converts dq; the caller then runs
 * vdqn_net_backward_stage(net, a, 0..2) as after vdqn_net_td_forward.  extra_capacity only (eval-mode BatchNorm: the three
 * model calls of process_batch are independent, so each has its own backward). */
int vdqn_net_backward_begin(vdqn_net* net, const vdqn_step_args* a, const float* dq_f32, void* stream);
/* The HIP stream (hipStream_t) on which a stage's gradients become complete; NULL when the overlap is off (then it is the
 * stream passed to vdqn_net_backward_stage). */
void* vdqn_net_grad_stream(vdqn_net* net);
/* dL/d(frames) of the same call: `frames.grad` after loss.backward() when the frames passed to `model(frames)` require a gradient
 * (torch.autograd through archs/HabitatDQNMultiAction.py:44-54 down to resnet.conv1's input).  Valid after
 * vdqn_net_backward_stage(net, a, 2, stream) of the same `a`, on the same stream: reads the pooled gradient (bf16) or conv1's
 * output gradient (f32 / bf16x3) from a->bwd, the arg-max codes from a->acts_online and conv1's forward operand from
 * a->packed_online.  out f32 NCHW [batch * num_frames][3][224][224].  scale_kind 0: with respect to the normalised frame;
 * 1: with respect to the uint8 pixel value, i.e. times 1 / (255 std_c).  extra_capacity only: ARCHITECTURE='basic' is refused.
 * Added without a change of vdqn_abi_version(). */
int vdqn_net_input_grad(vdqn_net* net, const vdqn_step_args* a, float* out, int32_t scale_kind, void* stream);
/* The same dL/d(frames), from a backward that computes nothing else: vdqn_net_backward_begin + vdqn_net_backward_stage(0..2) +
 * vdqn_net_input_grad of ONE earlier vdqn_net_forward (or vdqn_net_forward_attrib) call, without the weight gradients.  It launches
 * the dL/dQ conversion and the data-gradient chain (the head's four links, features.8, the eight BasicBlocks' data gradients, then
 * the stem's: vdqn_stem_input_grad for bf16, vdqn_maxpool_bwd + an f32 kernel for f32 / bf16x3), every launch with the arguments the
 * training walk gives it, the column-sum partial buffers included (the choice of kernel depends on them), so `out` holds the bits
 * the three-call sequence writes.  No weight gradient, no unfold, no clear of the accumulators, no side stream: everything is
 * queued on `stream`.  `a` carries packed_online (packed with the data-gradient operands), acts_online, batch = acts_samples, bwd;
 * grads may be NULL, params and bnstats are not read.  extra_capacity only: ARCHITECTURE='basic' is refused.
 * Added without a change of vdqn_abi_version(). */
int vdqn_net_backward_data(vdqn_net* net, const vdqn_step_args* a, const float* dq_f32, float* out, int32_t scale_kind, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attribution: perturbed copies of frames packed straight into the stem operand, and the sums over them (csrc/attrib.hip).
 * Integrated gradients (Sundararajan et al., ICML 2017) walks a straight path from a baseline to the frame; SmoothGrad (Smilkov
 * et al., 2017) averages the gradient over noisy copies.  Neither is in the reference.  In all three kernels every product and
 * every sum rounds on its own (no contraction into a fused multiply-add): tests/attrib_oracle.py restates them in numpy float32.
 *
 * x is the normalised f32 value of a pixel: the float source's value, or ((float)u / 255 - mean_c) / std_c of a uint8 source
 * (vdqn_pack_input's expression).  b is the baseline: base_const[c] (normalised units), or, with `baseline` given, the value of a
 * second image tensor of the source's kind and shape.  Copy s of image i is image s * n_base + i of the output.
 *   mode 0 (path):   x_s = b + coef[s] * (x - b)                           coef: DEVICE f32 [n_copies]
 *   mode 1 (noise):  x_s = x + sigma[c] * z                                sigma: normalised units
 *     h = splitmix64(splitmix64(splitmix64(seed ^ 0x4154545249423031) ^ ((uint64)(s0 + s) << 32 | (uint32)(i0 + i))) ^ e)
 *     z = (float)(h0 + h1 + h2 + h3 - 131070) * kZ,  h_k = (h >> 16 k) & 0xFFFF,  kZ = (float)(1 / sqrt((2^32 - 1) / 3))
 *   with e = (c * 224 + Y) * 224 + X the element's NCHW index inside its image ("ATTRIB01": a stream of its own).  z is
 *   Irwin-Hall of order 4 on integers: mean 0, variance 1, |z| <= 3.4641; s0 and i0 make a run's noise independent of how it
 *   is cut into calls.  x_s is rounded to the storage type once. */
/* The arguments the attribution entries share, in this order wherever they appear:
 *   src, src_kind   n_base images: uint8 NHWC [n_base][224][224][3] (src_kind 0) or f32 NCHW [n_base][3][224][224] (1)
 *   baseline        optional: the baseline images, same kind and shape as src; NULL: base_const
 *   base_const      HOST f32 [3], normalised units (NULL: zeros); not read when baseline is given
 *   n_base
 * and for the pack: n_copies, mode, coef (mode 0: DEVICE f32 [n_copies]), sigma (mode 1: HOST f32 [3], normalised units), seed,
 * s0, i0 (mode 1: global index of copy 0 and of image 0).
 * dst: [n_copies * n_base][115][115][16] in the dtype's storage type (VDQN_BF16 / VDQN_F32), borders and pad channels zero as
 * vdqn_pack_input writes them.  Refused with a message: null or misaligned (16 bytes; coef 4) pointers, src_kind or mode out of
 * range, n_base < 1, n_copies outside [1, 65535], 2^31 packed pixels or more, negative s0 / i0, a sigma that is negative or not
 * finite, a base_const that is not finite. */
int vdqn_attrib_pack(const void* src, int32_t src_kind, const void* baseline, const float* base_const, int32_t n_base, int32_t n_copies,
                     int32_t mode, const float* coef, const float* sigma, uint64_t seed, int32_t s0, int32_t i0, void* dst, int32_t dtype,
                     void* stream);
/* acc[i][e] = (accumulate ? acc[i][e] : 0) + w[0] * g[i][e] + w[1] * g[n_base + i][e] + ... in ascending s, one rounding per
 * product and per sum; squared: (w[s] * g) * g.  g f32 [n_copies * n_base][3][224][224], acc f32 [n_base][3][224][224], w DEVICE
 * f32 [n_copies].  No atomics: run-to-run bit-identical, and chunks of copies continued with `accumulate` give the bits of one call. */
int vdqn_attrib_reduce(const float* g, const float* w, float* acc, int32_t n_base, int32_t n_copies, int32_t squared,
                       int32_t accumulate, void* stream);
/* mode 0: out[i][c][y][x] = acc * (x - b) (then times 1 / (255 std_c) with scale_kind 1), x and b as vdqn_attrib_pack takes them;
 * out f32 [n_base][3][224][224].
 * mode 1: out[i][y][x] = max over c of |acc[i][c][y][x]| (a NaN stays one); the source arguments are not read and may be NULL;
 * out f32 [n_base][224][224]. */
int vdqn_attrib_finish(const float* acc, const void* src, int32_t src_kind, const void* baseline, const float* base_const, int32_t n_base,
                       int32_t mode, int32_t scale_kind, float* out, void* stream);
/* vdqn_net_forward over perturbed copies: vdqn_attrib_pack straight into the workspace's packed-input region, then the forward
 * pass; no float copy of the perturbed frames exists.  n_copies * n_base must equal n_samples * num_frames and n_base be a whole
 * number of samples (a sample's frames are consecutive base images); `acts` then feeds vdqn_net_backward_data like a
 * vdqn_net_forward workspace.  extra_capacity only. */
int vdqn_net_forward_attrib(vdqn_net* net, const void* packed, const void* src, int32_t src_kind, const void* baseline, const float* base_const,
                            int32_t n_base, int32_t n_copies, int32_t mode, const float* coef, const float* sigma, uint64_t seed, int32_t s0,
                            int32_t i0, int32_t n_samples, void* acts, float* q_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prioritized experience replay (Schaul et al., ICLR 2016), sampled and updated on the device: no host round trip.
 * The caller holds an f32 priority table prio[n] (>= 0, not all zero; (e + 1e-6)^alpha after an update, 1.0 to start) and a
 * workspace of vdqn_per_workspace_bytes(n).  The arithmetic is fixed and written out in video_dqn_amd/csrc/replay.hip:
 * f64 sums over 32-entry segments and 2048-entry chunks, left to right; draw j of the global batch G takes
 * u_j = ((j + r_j) * S) / G, S = sum(prio), r_j = top 53 bits of splitmix64(splitmix64(seed) ^ (step * G + j)) / 2^53, and the
 * smallest index whose inclusive prefix exceeds u_j (an entry with p = 0 is never drawn); its weight is
 * (n * p_i / S)^-beta over the largest such value of the batch.
 * ------------------------------------------------------------------------------------------------ */
/* Bytes of the sampling workspace for a table of n entries; -1 when n <= 0 or n > 8388608.  Host only. */
int64_t vdqn_per_workspace_bytes(int64_t n);
/* Draw a global batch of `global_batch` (<= 4096) indices: idx_out int64 [G], weight_out f32 [G] (beta in [0, 1]).  Two launches:
 * the segment / chunk sums into the workspace, then one block that scans the chunk sums and resolves every draw.
 * prio and workspace 16-byte aligned. */
int vdqn_per_sample(const float* prio, int64_t n, int32_t global_batch, uint64_t seed, uint64_t step, double beta, void* workspace,
                    int64_t* idx_out, float* weight_out, void* stream);
/* prio[idx[j]] = (err[j] + 1e-6)^alpha for j < global_batch (f64 pow, stored as f32); an index that appears more than once takes
 * the value of its largest j.  Indices outside [0, n) are skipped. */
int vdqn_per_update(float* prio, int64_t n, const int64_t* idx, const float* err, int32_t global_batch, double alpha, void* stream);

/* ------------------------------------------------------------------------------------------------
 * n-step returns (Sutton 1988; the multi-step target of Rainbow, Hessel et al., AAAI 2018) along a sampled row's chain in the logged
 * data: the n-fold composition of the one-step backup of train_q_network.py:134-169, evaluated per category,
 *   y = r(i0) + g (1 - t(i0)) [ r(i1) + g (1 - t(i1)) [ ... g (1 - t(i_{m-1})) Q_target(s^(m), argmax_a Q_online(s^(m), .)) ] ]
 * folded into rew_n, term_n and disc so that y = rew_n + disc * (1 - term_n) * Q(s^(m)) is what vdqn_td_loss_nstep forms.  i_{k+1} =
 * next_row[i_k] (int32 [n_rows]; a value outside [0, n_rows) means "no successor"), m <= n is the number of rows the chain provides,
 * s^(m) the `after` frames of the last row walked.  No importance correction: with non-negative rewards the target is a lower bound
 * of the optimal value.  The arithmetic, one thread per sample with every product and sum rounded on its own, is written out in
 * video_dqn_amd/csrc/nstep.hip (tests/nstep_oracle.py restates it in numpy float32, bit for bit).
 * ------------------------------------------------------------------------------------------------ */
/* idx int64 [batch] (clamped to [0, n_rows)); rew / term f32 [n_rows][n_cat], n_cat 1..8; n 1..16; gamma finite.  Outputs: rew_n,
 * term_n f32 [batch][n_cat], disc f32 [batch] (gamma^m), last_row int64 [batch], steps int32 [batch] (m).  No value of idx or
 * next_row makes the kernel read outside its tables; cycles are legal (the walk ends at n rows).  Every check fails by name before
 * any launch. */
int vdqn_nstep_walk(const int64_t* idx, int32_t batch, const int32_t* next_row, const float* rew, const float* term, int64_t n_rows,
                    int32_t n_cat, int32_t n, float gamma, float* rew_n, float* term_n, float* disc, int64_t* last_row, int32_t* steps,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Monte-Carlo return table: per row and category the discounted return the logged data obtained along the row's chain (the chain
 * vdqn_nstep_walk walks), over the chain's first 2^rounds rows:
 *   G(i) = sum_{k < 2^rounds} g^k prod_{j<k}(1 - t(i_j)) r(i_k),   i_0 = i, i_{k+1} = next_row[i_k], ending where the chain ends.
 * Built by pointer doubling, one launch per round and one thread per row, state (j, A[c], B[c]) per row:
 *   initial state:  j = next_row[i] (a value < 0 or >= n_rows becomes -1),  B = r,  A = g * (1 - t)   (the subtraction rounds, then
 *                   the product)
 *   one round, with j = j_old[i]:   j >= 0:  B' = B + (A * B_old[j]),  A' = A * A_old[j],  j' = j_old[j]
 *                                   j <  0:  B' = B,                   A' = 0,             j' = -1
 * every product and sum rounded on its own (tests/mc_oracle.py restates it in numpy float32, bit for bit); a round reads one
 * buffer set and writes the other; no atomics, no LDS, plain stores, so two builds are bit-identical.  After `rounds` rounds B is
 * G.  Self-loops and cycles are legal.  Against the exact sum, |G - exact| <= (3 * rounds + 3) * 2^-24 * S with S the same sum over
 * |r|.
 * ------------------------------------------------------------------------------------------------ */
/* Bytes of the caller's workspace (two j tables, two A tables and one B table; the other B table is G itself); -1 for n_rows
 * outside [1, 2^31 - 1] or n_cat outside [1, 8]. */
int64_t vdqn_mc_returns_workspace_bytes(int64_t n_rows, int32_t n_cat);
/* next_row int32 [n_rows], rew / term f32 [n_rows][n_cat] (read only), G f32 [n_rows][n_cat], all on the device; workspace 4-byte
 * aligned, its contents do not matter before and mean nothing after.  Every check fails by name before any launch: null pointers,
 * n_rows outside [1, 2^31 - 1], n_cat outside [1, 8], rounds outside [1, 31], a non-finite gamma, a workspace that is too small. */
int vdqn_mc_returns(const int32_t* next_row, const float* rew, const float* term, int64_t n_rows, int32_t n_cat, float gamma, int32_t rounds,
                    float* G, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Random shift + left-right mirror augmentation of the training minibatch (DrQ / RAD style), fused into the input pack.  The
 * reference's only transform is Resize + CenterCrop + Normalize (util/torch.py:5-12), which vdqn_pack_input fuses; these entries
 * extend that call site and the batch hand-over of train_q_network.py:127-131.  One int32 {sx, sy, flip, 0} per SAMPLE, shared by
 * its frames and by s and s'.  Output pixel (Y, X) of a frame reads source pixel
 *   Ys = clamp(Y + sy, 0, 223), Xs = clamp(X + sx, 0, 223), Xs = 223 - Xs if flip != 0
 * (mirror the source, pad by edge replication, crop at the offset): an index remap of uint8 pixels, so the packed operand equals
 * vdqn_pack_input of the augmented frames bit for bit.  Any int32 sx, sy is safe.  The arithmetic of the draw is written out in
 * video_dqn_amd/csrc/augment.hip.
 * ------------------------------------------------------------------------------------------------ */
/* params[i] (int32 [n][4], 16-byte aligned) = the draw of sample first + i of a global batch of `global_batch` samples at update
 * `step`: sx, sy uniform in [-pad, pad] (pad in 0 .. 32), flip a fair bit when `flip` != 0, else 0.  A rank of a data-parallel
 * job passes first = rank * B, n = B and gets its slice of the one-process draw. */
int vdqn_aug_draw(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t pad, int32_t flip,
                  int32_t* params, void* stream);
/* act_out[b] = act[b] with a0 <-> a1 exchanged where params[b].flip != 0 (a mirrored left turn is a right turn), a copy elsewhere.
 * int64 [n]; a0 != a1, both in 0 .. 2.  act_out may be act. */
int vdqn_aug_swap_actions(const int64_t* act, const int32_t* params, int32_t n, int32_t a0, int32_t a1, int64_t* act_out,
                          void* stream);
/* vdqn_pack_input for uint8 NHWC frames (src_kind 0) with the remap: frame i takes params[(i / frames_per_sample) % n_params].
 * src, dst and params 16-byte aligned.  All-zero params give vdqn_pack_input's output. */
int vdqn_pack_input_aug(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                        int32_t n_params, int32_t dtype, void* stream);

/* Colour jitter (brightness, contrast, saturation as torchvision's ColorJitter draws them: one uniform factor in [1 - J, 1 + J] each),
 * defined as a map from uint8 pixels to uint8 pixels in integer arithmetic, so the packed operand still equals vdqn_pack_input of
 * host-augmented frames bit for bit (tests/aug_color_oracle.py).  One int32 {f_b, f_c, f_s, 0} per SAMPLE, Q8 (256 = factor 1.0),
 * shared by its frames and by s and s'.  "/ 256" is floor division (an arithmetic shift).  One source pixel (R, G, B), in this order:
 *   saturation:  g = (77 R + 150 G + 29 B + 128) / 256;   v = clamp(g + ((v - g) * f_s + 128) / 256, 0, 255)   for v in R, G, B
 *   brightness:  v = min(255, (v * f_b + 128) / 256)
 *   contrast:    v = clamp(128 + ((v - 128) * f_c + 128) / 256, 0, 255)          (pivot: mid-grey 128, no per-frame mean)
 * then vdqn_pack_input's normalisation.  (256, 256, 256) is the identity on every byte.  Hue, white balance and blur are not
 * covered. */
/* color[i] (int32 [n][4], 16-byte aligned) = the draw of sample first + i of a global batch of `global_batch` samples at update `step`:
 *   h = splitmix64(splitmix64(seed ^ 0x415547434F4C5231 "AUGCOLR1") ^ (step * global_batch + first + i))
 *   f_k = 256 - j_k + ((((h >> 16 k) & 0xFFFF) * (2 j_k + 1)) >> 16)     k = 0 brightness (jb), 1 contrast (jc), 2 saturation (js)
 * uniform over the 2 j_k + 1 values of [256 - j_k, 256 + j_k]; word 3 is 0.  jb, jc, js are Q8 half-widths int(J * 256 + 0.5), 0 .. 256.
 * A stream of its own: vdqn_aug_draw's values at the same seed and update do not depend on it.  Slices as vdqn_aug_draw. */
int vdqn_aug_draw_color(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jb, int32_t jc,
                        int32_t js /* Q8 half-widths, 0 .. 256 */, int32_t* color, void* stream);
/* vdqn_pack_input_aug with the colour transform applied to every source pixel it reads: frame i takes params[(i / frames_per_sample)
 * % n_params] and color[(i / frames_per_sample) % n_params] (both int32 [n_params][4], 16-byte aligned).  Every factor is clamped to
 * [0, 512] before use and word 3 is ignored: any int32 content is safe.  Factors (256, 256, 256) give vdqn_pack_input_aug's output. */
int vdqn_pack_input_aug_color(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                              const int32_t* color, int32_t n_params, int32_t dtype, void* stream);

/* Random zoom (a change of focal length): a window of [1 - J, 1] of the frame's side, J <= 0.5, at a uniform position inside the frame,
 * resampled back to 224 x 224 — bilinear with Q16 coordinates and Q8 weights in integer arithmetic on the uint8 pixels, so the packed
 * operand still equals vdqn_pack_input of host-augmented frames bit for bit (tests/aug_zoom_oracle.py).  One int32 {ax, ay, bx, by} per
 * SAMPLE, shared by its frames and by s and s': ax, ay the Q16 source step per output pixel (65536 = 1.0, never more: no zoom-out), bx,
 * by the Q16 source coordinate of output pixel 0.  ">>" is arithmetic.  Output pixel (Y, X) of a frame Z, per channel:
 *   u = bx + X * ax;  x0 = u >> 16;  wx = (u >> 8) & 255;   v = by + Y * ay;  y0 = v >> 16;  wy = (v >> 8) & 255
 *   xa = clamp(x0, 0, 223), xb = clamp(x0 + 1, 0, 223), ya, yb likewise
 *   top = Z[ya][xa] * (256 - wx) + Z[ya][xb] * wx;   bot = the same on row yb;   out = (top * (256 - wy) + bot * wy + 32768) >> 16
 * Z is the frame after shift and mirror (vdqn_pack_input_aug's remap applied to each tap); the colour transform works on the
 * resampled bytes.  {65536, 65536, 0, 0} is the identity on every byte.  Zoom-out is not covered; rotation is vdqn_pack_input_aug_affine's
 * (below). */
/* zoom[i] (int32 [n][4], 16-byte aligned) = the draw of sample first + i of a global batch of `global_batch` samples at update `step`:
 *   h = splitmix64(splitmix64(seed ^ 0x4155475A4F4F4D31 "AUGZOOM1") ^ (step * global_batch + first + i));   h_k = (h >> 16 k) & 0xFFFF
 *   ax = 65536 - ((h_0 * (jz + 1)) >> 16);   ay = aspect ? 65536 - ((h_1 * (jz + 1)) >> 16) : ax
 *   origin(a, hk) = ((((hk * (((224 * 65536 - 224 * a) >> 8) + 1)) >> 16) << 8) + (a >> 1) - 32768;   bx = origin(ax, h_2), by = origin(ay, h_3)
 * jz is the Q16 width int(J * 65536 + 0.5), 0 .. 32768; jz = 0 gives the identity row.  The window always lies inside the frame:
 * bx + 223 ax < 224 * 65536.  A stream of its own: the other draws at the same seed and update do not depend on it.  Slices as
 * vdqn_aug_draw. */
int vdqn_aug_draw_zoom(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jz /* Q16 width, 0 .. 32768 */,
                       int32_t aspect, int32_t* zoom, void* stream);
/* vdqn_pack_input_aug(_color) of the resampled frames: frame i takes params, color and zoom row (i / frames_per_sample) % n_params (each
 * int32 [n_params][4], 16-byte aligned; color may be NULL: no colour transform).  ax, ay are clamped to [0, 65536] and bx, by to
 * +-224 * 65536 before use, and every tap is clamped into the frame: any int32 content is safe.  The identity row gives
 * vdqn_pack_input_aug's (vdqn_pack_input_aug_color's) output. */
int vdqn_pack_input_aug_zoom(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                             const int32_t* color /* NULL ok */, const int32_t* zoom, int32_t n_params, int32_t dtype, void* stream);

/* Random rotation (camera roll) about the picture's centre by an angle uniform in [-J, J], J <= 30 degrees, composed with the sample's
 * zoom row into ONE affine map and resampled with the zoom's integer bilinear, so the packed operand still equals vdqn_pack_input of
 * host-augmented frames bit for bit (tests/aug_rotate_oracle.py).  One int32 [8] = {axx, axy, bx, 0, ayx, ayy, by, 0} per SAMPLE (Q16, two
 * 16-byte vectors), shared by its frames and by s and s'.  ">>" is arithmetic, "/" floors, products are int64; the unit of angle is
 * 1 / 64 degree.  Output pixel (Y, X) of a frame Z, per channel:
 *   u = bx + X * axx + Y * axy;  x0 = u >> 16;  wx = (u >> 8) & 255;   v = by + X * ayx + Y * ayy;  y0 = v >> 16;  wy = (v >> 8) & 255
 *   taps, top, bot and out as vdqn_pack_input_aug_zoom's
 * Z is the frame after shift and mirror; the colour transform works on the resampled bytes.  Out-of-frame taps replicate the edge.
 * {65536, 0, 0, 0, 0, 65536, 0, 0} is the identity on every byte; a row with axy = ayx = 0 gives vdqn_pack_input_aug_zoom's output for
 * {axx, ayy, bx, by}.  Zoom-out is not covered. */
/* affine[i] (int32 [n][8], 16-byte aligned) = the draw of sample first + i of a global batch of `global_batch` samples at update `step`:
 *   h = splitmix64(splitmix64(seed ^ 0x415547524F544131 "AUGROTA1") ^ (step * global_batch + first + i))
 *   k = (((h & 0xFFFF) * (2 jr + 1)) >> 16) - jr                                     the angle, in [-jr, jr]
 *   t = k * 292818 (Q30 radians);  t2 = (t * t) >> 30;  ONE = 1 << 30
 *   a = ONE - t2 / 42;  a = ONE - ((t2 * a) >> 30) / 20;  a = ONE - ((t2 * a) >> 30) / 6;   s = (t * a) >> 30
 *   b = ONE - t2 / 56;  b = ONE - ((t2 * b) >> 30) / 30;  b = ONE - ((t2 * b) >> 30) / 12;  b = ONE - ((t2 * b) >> 30) / 2
 *   S = (s + 8192) >> 14;  C = (b + 8192) >> 14                                      Q16 sine and cosine, within 2^-16 of the exact ones
 *   {ax, ay, bxz, byz} = zoom[i] (int32 [n][4], the slice's zoom rows, 16-byte aligned), or {65536, 65536, 0, 0} when zoom is NULL
 *   axx = (ax * C + 32768) >> 16;  axy = -((ax * S + 32768) >> 16);  bx = bxz + ((223 * (ax - axx - axy)) >> 1)
 *   ayx = (ay * S + 32768) >> 16;  ayy = (ay * C + 32768) >> 16;     by = byz + ((223 * (ay - ayx - ayy)) >> 1)
 * i.e. rotate the output pixel centre about index (111.5, 111.5), then apply the zoom map.  jr is int(J * 64 + 0.5), 0 .. 1920; jr = 0
 * gives {ax, 0, bxz, 0, 0, ay, byz, 0}.  A stream of its own: the other draws at the same seed and update do not depend on it.  Slices
 * as vdqn_aug_draw. */
int vdqn_aug_draw_rotate(uint64_t seed, uint64_t step, int32_t global_batch, int32_t first, int32_t n, int32_t jr /* 0 .. 1920 */,
                         const int32_t* zoom /* NULL = identity */, int32_t* affine, void* stream);
/* vdqn_pack_input_aug(_color) of the affinely resampled frames: frame i takes params, color and affine row (i / frames_per_sample) %
 * n_params (params and color int32 [n_params][4], affine int32 [n_params][8], 16-byte aligned; color may be NULL: no colour transform).
 * axx, ayy are clamped to [0, 65536], axy, ayx to +-65536 and bx, by to +-448 * 65536 (where every tap already sits on an edge) before
 * use, words 3 and 7 are ignored and every tap is clamped into the frame: any int32 content is safe.  dtype VDQN_BF16 or VDQN_F32. */
int vdqn_pack_input_aug_affine(const void* src, void* dst, int32_t n_img, int32_t frames_per_sample, const int32_t* params,
                               const int32_t* color /* NULL ok */, const int32_t* affine, int32_t n_params, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel exchange: one process per GPU, the flat f32 gradient SUM-all-reduced over RCCL (xGMI)
 * in the three stage buckets of vdqn_net_stage_range, each issued on vdqn_net_grad_stream(net) when its stage's
 * vdqn_net_backward_stage call has returned; the caller's stream waits for the three collectives (hipStreamWaitEvent) before
 * vdqn_adam.  The fused TD kernel already divides by the GLOBAL batch (vdqn_step_args.inv_count), so the sum is the gradient of
 * the global-batch mean loss: N ranks == the reference's one big batch (the reference itself is single-GPU,
 * train_q_network.py:255-259,275; no reference call site is replaced).
 * RCCL is looked up at run time (an already-loaded librccl.so, e.g. PyTorch's, is reused; VDQN_RCCL_LIB names another):
 * single-GPU users of this library do not need it.  The Python host uses torch.distributed's "nccl" backend — the same
 * library — instead (video_dqn_amd/dist.py); these entries serve callers that bind this header directly.
 * ------------------------------------------------------------------------------------------------ */
#define VDQN_COMM_UID_BYTES 128
typedef struct vdqn_comm vdqn_comm;
/* Rank 0 creates the 128-byte rendezvous id (ncclGetUniqueId) and hands it to every rank by whatever channel the job has
 * (file, environment, socket); uid_host is HOST memory. */
int vdqn_comm_unique_id(void* uid_host);
/* Collective over all ranks: joins the communicator on the calling thread's current HIP device (ncclCommInitRank). */
int vdqn_comm_init(int32_t rank, int32_t nranks, const void* uid_host, vdqn_comm** out);
/* In-place SUM all-reduce of `count` elements (dtype VDQN_F32 | VDQN_BF16) at device pointer `ptr`, asynchronous on `stream`. */
int vdqn_allreduce_bucket(vdqn_comm* comm, void* ptr, int64_t count, int32_t dtype, void* stream);
int vdqn_comm_rank(const vdqn_comm* comm);
int vdqn_comm_size(const vdqn_comm* comm);
int vdqn_comm_destroy(vdqn_comm* comm);

#ifdef __cplusplus
}
#endif
#endif /* VDQN_H_ */
