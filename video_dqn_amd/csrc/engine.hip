// The network engine's orchestration: side streams, the launch helpers, both forward passes, and the staged backward of one
// TD update.  (Layer table and workspace layouts: engine_table.hip; fold / unfold kernels: fold.hip.)
//
// Follows: archs/HabitatDQNMultiAction.py:9-54 (wiring, set_train: trunk BatchNorm in eval mode),
// torchvision 0.4.2 resnet18 topology (third-party; restated in oracle/ref_cpu.py),
// train_q_network.py:126-181 (process_batch) and :222-227 (zero_grad / backward / step order).
#include "engine_net.h"

// VDQN_WGRAD_TWO_STAGE=1: the split-K weight-gradient partials as plain stores into per-split copies + one ordered reduce kernel
// per layer (the deterministic mode's path, include/vdqn.h vdqn_wgrad_args.workspace) also in the default mode — instead of
// ~25-50 MB of f32 atomics per launch at the ~1.3 TB/s the memory side sustains for them
bool wgrad_two_stage() {
  static const bool on = [] { const char* e = getenv("VDQN_WGRAD_TWO_STAGE"); return e && e[0] == '1'; }();
  return on;
}

namespace {

bool side_ready(vdqn_net* net) {
  if (!net->overlap) return false;
  if (!net->side) {
    // The side streams (target forward, weight gradients, unfold) run BELOW the caller's stream in the hardware queues' priority order:
    // the caller's stream carries the critical chain (online forward, data gradients), the side streams are what fills the chip around
    // it.  Measured on alternating runs of two boxes (profiles/r04i_*, r04j_*): low 5.766-5.781 against 5.832-5.842 ms per update on one
    // (+1.0 %, three rounds of three), 5.843-5.856 against 5.849-5.863 on the other (+0.1 %); HIGH priority for them: 5.911-5.916 against
    // 5.837-5.844 (-1.2 %).  VDQN_SIDE_PRIORITY=normal|high|low overrides.
    int prio = 0;
    {
      const char* e = getenv("VDQN_SIDE_PRIORITY");
      int lo = 0, hi = 0;  // (numerically lower = higher priority)
      if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess) prio = (!e || e[0] == 'l') ? lo : (e[0] == 'h' ? hi : 0);
    }
    if (hipStreamCreateWithPriority(&net->side, hipStreamNonBlocking, prio) != hipSuccess ||
        hipStreamCreateWithPriority(&net->side2, hipStreamNonBlocking, prio) != hipSuccess) {
      net->overlap = 0;
      net->side = nullptr;
      net->side2 = nullptr;
      return false;
    }
    net->events.resize(64);
    for (auto& e : net->events)
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
        net->overlap = 0;
        return false;
      }
  }
  return true;
}
hipEvent_t next_event(vdqn_net* net) {
  hipEvent_t e = net->events[net->ev_next];
  net->ev_next = (net->ev_next + 1) % net->events.size();
  return e;
}
// Side stream `which` (0: target forward, weight gradients, unfold; 1: the other half of the weight gradients) waits for everything
// queued on `from` so far.  Returns the stream to launch the side work on: `from` itself when the overlap is off.
hipStream_t fork(vdqn_net* net, hipStream_t from, int which = 0) {
  if (!side_ready(net)) return from;
  hipStream_t to = which ? net->side2 : net->side;
  hipEvent_t e = next_event(net);
  (void)hipEventRecord(e, from);
  (void)hipStreamWaitEvent(to, e, 0);
  return to;
}
// `into` waits for everything queued on the side stream `from` so far
void join(vdqn_net* net, hipStream_t from, hipStream_t into) {
  if (!net->overlap || !from) return;
  hipEvent_t e = next_event(net);
  (void)hipEventRecord(e, from);
  (void)hipStreamWaitEvent(into, e, 0);
}

// Stream of the next weight-gradient launch.  The launches alternate between the two side streams, so that one kernel's tail (a
// single round of split-K blocks that all end in f32 atomics) runs beside the next kernel's start; not in the deterministic /
// two-stage modes, whose partial copies share one workspace.  The stage's unfold kernel, on the first, waits for the second.
// Round 4: default ON now that the side streams run below the caller's stream in priority — seven alternating rounds on one box:
// better in five, equal in two, median 5.828 against 5.900 ms per update (profiles/r04n_ab_wgrad_two_low_priority_streams.txt;
// at equal priorities round 3 had measured no gain).  VDQN_WGRAD_STREAMS=1 keeps them on one stream.
int g_wgrad_streams_override = -1;  // tools/ab_inproc.py: vdqn_debug_set_wgrad_streams (1 / 2; -1 = VDQN_WGRAD_STREAMS)
bool wgrad_two_streams(const vdqn_net* net) {
  static const bool env_on = [] { const char* e = getenv("VDQN_WGRAD_STREAMS"); return !e || atoi(e) == 2; }();
  const bool on = g_wgrad_streams_override > 0 ? g_wgrad_streams_override == 2 : env_on;
  return on && !wgrad_two_stage() && !net->cfg.deterministic;
}
}  // namespace
extern "C" void vdqn_debug_set_wgrad_streams(int v) { g_wgrad_streams_override = v; }
static int g_stem_wgrad_main_override = -1;  // tools/ab_inproc.py (0 / 1; -1 = VDQN_STEM_WGRAD_MAIN)
extern "C" void vdqn_debug_set_stem_wgrad_main(int v) { g_stem_wgrad_main_override = v; }
namespace {
hipStream_t wgrad_stream(vdqn_net* net, hipStream_t main) {
  if (!wgrad_two_streams(net)) return fork(net, main);
  net->wgrad_rr ^= 1;
  return fork(net, main, net->wgrad_rr);
}

// ---------------------------------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------------------------------
// per-layer rows in the launch profiler (VDQN_PROFILE_LAYERS=1): "<kernel>|<layer> n<images>"
void prof_layer(const Layer& L, int n_units) {
  static const bool on = [] { const char* e = getenv("VDQN_PROFILE_LAYERS"); return e && e[0] == '1'; }();
  if (!on) return;
  static thread_local char buf[64];
  const char* nm = L.name.c_str();
  if (strncmp(nm, "resnet.", 7) == 0) nm += 7;
  snprintf(buf, sizeof(buf), "%s n%d", nm, n_units);
  g_prof_suffix = buf;
}

// VDQN_FUSE_DS: the 1x1 downsample of a stride-2 BasicBlock rides in its sibling 3x3's launches.  Bit 0 (default on): backward —
// extra K-steps of the 3x3's stride-2 data gradient, the shortcut gradient never exists (0.27 instead of 0.42 ms per update);
// bit 1 (default on since round 5, bf16 engines): forward — second output of one launch, three launches fewer per pass,
// bit-identical outputs: the persistent plane-window kernel (win9s.hip, win9sp_kernel) runs the 1x1 as extra K-steps on the P00
// window behind the 3x3's epilogue.  (On the generic kernel — f32 engines, odd-sized inputs — the short sibling tiles between the
// long ones cost more than their own launch did: bit 2 forces the fused form there too.)
int fuse_ds_mask() {
  static const int m = [] { const char* e = getenv("VDQN_FUSE_DS"); return e ? atoi(e) : 3; }();
  return m;
}
bool fuse_ds() { return (fuse_ds_mask() & 1) != 0; }
bool fuse_ds_fwd(int dtype) { return (fuse_ds_mask() & 2) != 0 && (dtype == VDQN_BF16 || (fuse_ds_mask() & 4) != 0); }

int run_conv(const vdqn_net* net, const Layer& L, const unsigned char* packed, const void* in, void* out, int n_units, const void* resid,
             int relu, float* out_f32, hipStream_t st, const Layer* sib = nullptr, void* sib_out = nullptr) {
  vdqn_conv_args a;
  memset(&a, 0, sizeof(a));
  a.in = in;
  a.wt = packed + L.wf_off;
  a.bias = reinterpret_cast<const float*>(packed + L.bias_off);
  a.resid = resid;
  a.mask = nullptr;
  a.out = out;
  a.out_f32 = out_f32;
  a.n_img = n_units; a.hi = L.hi; a.wi = L.wi; a.ci = L.k_ci; a.pix_stride = L.pix_stride;
  a.ho = L.ho; a.wo = L.wo; a.co = L.co_pad; a.ldo = L.co_pad;
  a.r = L.k_r; a.s = L.k_s;
  a.stride = L.kind == K_CONV1_S2D ? 1 : L.stride;
  a.pad = L.kind == K_CONV1_S2D ? 0 : L.pad;
  a.mode = 0; a.relu = relu; a.dtype = net->gemm_dtype;
  g_prof_alg_flops = 2.0 * n_units * L.ho * L.wo * (double)L.co * L.ci * L.r * L.s;
  if (sib) {  // the block's 1x1 / stride-2 downsample (BatchNorm folded, no ReLU): second output of the same launch
    a.wt2 = packed + sib->wf_off;
    a.bias2 = reinterpret_cast<const float*>(packed + sib->bias_off);
    a.out2 = sib_out;
    a.co2 = sib->co_pad; a.ldo2 = sib->co_pad; a.relu2 = 0;
    g_prof_alg_flops += 2.0 * n_units * sib->ho * sib->wo * (double)sib->co * sib->ci;
  }
  prof_layer(L, n_units);
  return vdqn_conv2d(&a, st);
}

// data gradient: gx = (dgrad(gy) + resid) masked by (mask > 0)
int run_dgrad(const vdqn_net* net, const Layer& L, const unsigned char* packed, const void* gy, void* gx, int n_units, const void* resid,
              const void* mask, hipStream_t st, void* colsum_part = nullptr, const Layer* sib = nullptr, const void* sib_gy = nullptr,
              int* part_rows = nullptr) {
  vdqn_conv_args a;
  memset(&a, 0, sizeof(a));
  a.in = gy;
  a.wt = packed + L.wd_off;
  a.bias = nullptr;
  a.resid = resid;
  a.mask = mask;
  a.out = gx;
  a.colsum_part = reinterpret_cast<float*>(colsum_part);
  a.n_img = n_units; a.hi = L.ho; a.wi = L.wo; a.ci = L.co_pad; a.pix_stride = L.co_pad;
  a.ho = L.hi; a.wo = L.wi; a.co = L.k_ci; a.ldo = L.k_ci;
  a.r = L.k_r; a.s = L.k_s; a.stride = L.stride; a.pad = L.pad;
  a.mode = 1; a.relu = 0; a.dtype = net->gemm_dtype;
  g_prof_alg_flops = 2.0 * n_units * L.ho * L.wo * (double)L.co * L.ci * L.r * L.s;
  if (sib) {  // + the data gradient of the block's 1x1 / stride-2 downsample, accumulated in the same tiles
    a.in2 = sib_gy;
    a.wt2 = packed + sib->wd_off;
    a.ci2 = sib->co_pad;
    g_prof_alg_flops += 2.0 * n_units * sib->ho * sib->wo * (double)sib->co * sib->ci;
  }
  if (part_rows) {  // rows of gx one entry of colsum_part covers: the kernel vdqn_conv2d picks for this call decides
    const int kind = vdqn_skinny_kind(&a);
    *part_rows = kind ? vdqn_skinny_part_rows(kind == 2) : 128;
  }
  prof_layer(L, n_units);
  return vdqn_conv2d(&a, st);
}

int run_wgrad(const vdqn_net* net, const Layer& L, unsigned char* bwd, const BwdLayout& W, const void* gy, const void* x, int n_units,
              hipStream_t st, bool colsum_kernel = false) {
  vdqn_wgrad_args a = wgrad_shape_args(net, L, n_units);
  a.gy = gy;
  a.x = x;
  a.dw = reinterpret_cast<float*>(bwd + L.dw_off);
  a.dbias = colsum_kernel ? reinterpret_cast<float*>(bwd + L.db_off) : nullptr;  // else: dgrad-epilogue partials
  if (net->cfg.deterministic || wgrad_two_stage()) {  // all weight gradients of an update run on ONE stream, so they can share the workspace
    a.workspace = bwd + W.det_ws;
    a.workspace_bytes = W.det_ws_bytes;
  }
  // vdqn_conv2d_wgrad addresses < 2^24 output pixels and < 2 GiB per operand (32-bit buffer offsets): larger batches
  // (conv1 at more than 1337 bf16 / 668 f32 frames, e.g. 12-view samples at batch 256) go through it in image ranges —
  // dw and dbias accumulate, so the ranges simply add up.
  const int64_t esz = net->esz;
  const int64_t pix = (int64_t)L.ho * L.wo, gy_img = pix * L.co_pad * esz, x_img = (int64_t)L.hi * L.wi * L.pix_stride * esz;
  const int64_t max_imgs = wgrad_max_imgs(net, L);
  if (max_imgs < 1) {
    vdqn_set_error("run_wgrad: one image of layer %s exceeds the weight-gradient kernel's addressing range", L.name.c_str());
    return VDQN_ERR_INVALID;
  }
  for (int64_t i0 = 0; i0 < n_units; i0 += max_imgs) {
    const int n_chunk = (int)std::min<int64_t>(max_imgs, n_units - i0);
    a.gy = (const unsigned char*)gy + i0 * gy_img;
    a.x = (const unsigned char*)x + i0 * x_img;
    a.n_img = n_chunk;
    g_prof_alg_flops = 2.0 * n_chunk * L.ho * L.wo * (double)L.co * L.ci * L.r * L.s;
    prof_layer(L, n_chunk);
    const int rc = vdqn_conv2d_wgrad(&a, st);
    if (rc != VDQN_OK) return rc;
  }
  return VDQN_OK;
}

// forward over n_samples samples whose packed input already sits at `t_in`
int forward_impl(const vdqn_net* net, const unsigned char* packed, const void* t_in, int n_samples, unsigned char* acts, const ActLayout& A,
                 hipStream_t st, bool trunk_only = false, int grad_samples = -1) {
  const int n = n_samples * net->cfg.num_frames;
  const int dt = net->cfg.dtype;
  // grad_samples >= 0: only the first grad_samples samples will see a backward pass — the stem skips the arg-max bytes of the
  // max-pool for the rest (the s' rows and the target pass of a TD update: 2/3 of its frames; VDQN_STEM_NOIDX=0 writes them all)
  static const bool stem_noidx = [] { const char* e = getenv("VDQN_STEM_NOIDX"); return !(e && e[0] == '0'); }();
  const int n_idx = (grad_samples >= 0 && stem_noidx) ? (grad_samples * net->cfg.num_frames < n ? grad_samples * net->cfg.num_frames : n) : n;
  if (A.c1 >= 0) {  // 'basic' eval path keeps the separate kernels (its train path needs the raw conv output anyway)
    RC(run_conv(net, net->layers[net->l_conv1], packed, t_in, acts + A.c1, n, nullptr, 1, nullptr, st));
    RC(vdqn_maxpool_fwd(acts + A.c1, acts + A.pool, acts + A.idx, n, 112, 112, 64, dt, st));
  } else {
    const Layer& L1 = net->layers[net->l_conv1];
    prof_layer(L1, n);
    RC(vdqn_stem_conv_pool_n(t_in, packed + L1.wf_off, reinterpret_cast<const float*>(packed + L1.bias_off), acts + A.pool, acts + A.idx, n, n_idx, net->gemm_dtype, st));
  }
  const unsigned char* x = acts + A.pool;
  for (int b = 0; b < 8; ++b) {
    const Layer& c1 = net->layers[net->l_b_conv1[b]];
    const Layer& c2 = net->layers[net->l_b_conv2[b]];
    const void* identity = x;
    if (net->l_b_ds[b] >= 0 && fuse_ds_fwd(dt)) {  // stride-2 block: conv1 and the downsample read the same pixels — one launch
      RC(run_conv(net, c1, packed, x, acts + A.h[b], n, nullptr, 1, nullptr, st, &net->layers[net->l_b_ds[b]], acts + A.ds[b]));
      identity = acts + A.ds[b];
    } else {
      RC(run_conv(net, c1, packed, x, acts + A.h[b], n, nullptr, 1, nullptr, st));
      if (net->l_b_ds[b] >= 0) {
        RC(run_conv(net, net->layers[net->l_b_ds[b]], packed, x, acts + A.ds[b], n, nullptr, 0, nullptr, st));
        identity = acts + A.ds[b];
      }
    }
    RC(run_conv(net, c2, packed, acts + A.h[b], acts + A.o[b], n, identity, 1, nullptr, st));
    x = acts + A.o[b];
  }
  if (trunk_only) return VDQN_OK;  // the 512 x 7 x 7 features are in o7
  if (net->basic()) {
    RC(vdqn_avgpool_fwd(x, acts + A.avg, n, 49, 512, dt, st));
    RC(run_conv(net, net->layers[net->l_top4], packed, acts + A.avg, acts + A.q, n_samples, nullptr, 0, reinterpret_cast<float*>(acts + A.qf), st));
    return VDQN_OK;
  }
  RC(run_conv(net, net->layers[net->l_f8], packed, x, acts + A.f8, n, nullptr, 1, nullptr, st));
  RC(run_conv(net, net->layers[net->l_top0], packed, acts + A.f8, acts + A.l0, n_samples, nullptr, 1, nullptr, st));
  RC(run_conv(net, net->layers[net->l_top2], packed, acts + A.l0, acts + A.l1, n_samples, nullptr, 1, nullptr, st));
  RC(run_conv(net, net->layers[net->l_top4], packed, acts + A.l1, acts + A.q, n_samples, nullptr, 0, reinterpret_cast<float*>(acts + A.qf), st));
  return VDQN_OK;
}

// train-mode BatchNorm of layer L over the raw conv output y: z = relu?(bn(y) (+ resid)); updates the running statistics
int run_bn(const vdqn_net* net, int li, const float* params, float* bnstats, unsigned char* acts, const ActLayout& A, const void* y,
           const void* resid, void* z, int n_img, int iph, int relu, hipStream_t st) {
  const Layer& L = net->layers[li];
  BnSync sy = net->bn_sync;
  sy.scratch = reinterpret_cast<float*>(acts + A.bn_sync);
  if (A.bn_det >= 0) {
    sy.det_ws = reinterpret_cast<float*>(acts + A.bn_det);
    sy.det_ws_bytes = A.bn_det_bytes;
  }
  return vdqn_bn_train_fwd_impl(y, resid, z, params + L.g_off, params + L.b_off, bnstats + L.mean_off, bnstats + L.var_off,
                                reinterpret_cast<float*>(acts + A.bnw[li]), n_img, L.ho * L.wo, L.co, net->cfg.num_frames, iph, relu, kBnMomentum,
                                kBnEps, net->cfg.dtype, st, &sy);
}

// ARCHITECTURE='basic' in train mode (archs/HabitatDQNMultiAction.py:37-40 leaves the ResNet in train mode): forward over
// n_samples samples = n_samples/halves per model call, batch statistics per (call, frame slot), raw conv outputs kept for
// the backward.  `packed` must hold the un-folded weights (vdqn_net_pack_weights flag 2).
int forward_train_impl(const vdqn_net* net, const unsigned char* packed, const float* params, float* bnstats, const void* t_in, int n_samples,
                       int halves, unsigned char* acts, const ActLayout& A, hipStream_t st) {
  const int F = net->cfg.num_frames, n = n_samples * F, iph = n / halves;
  const int dt = net->cfg.dtype;
  RC(run_conv(net, net->layers[net->l_conv1], packed, t_in, acts + A.r_c1, n, nullptr, 0, nullptr, st));
  RC(run_bn(net, net->l_conv1, params, bnstats, acts, A, acts + A.r_c1, nullptr, acts + A.c1, n, iph, 1, st));
  RC(vdqn_maxpool_fwd(acts + A.c1, acts + A.pool, acts + A.idx, n, 112, 112, 64, dt, st));
  const unsigned char* x = acts + A.pool;
  for (int b = 0; b < 8; ++b) {
    const int i1 = net->l_b_conv1[b], i2 = net->l_b_conv2[b], ids = net->l_b_ds[b];
    RC(run_conv(net, net->layers[i1], packed, x, acts + A.r_h[b], n, nullptr, 0, nullptr, st));
    RC(run_bn(net, i1, params, bnstats, acts, A, acts + A.r_h[b], nullptr, acts + A.h[b], n, iph, 1, st));
    RC(run_conv(net, net->layers[i2], packed, acts + A.h[b], acts + A.r_o[b], n, nullptr, 0, nullptr, st));
    const void* identity = x;
    if (ids >= 0) {
      RC(run_conv(net, net->layers[ids], packed, x, acts + A.r_ds[b], n, nullptr, 0, nullptr, st));
      RC(run_bn(net, ids, params, bnstats, acts, A, acts + A.r_ds[b], nullptr, acts + A.ds[b], n, iph, 0, st));
      identity = acts + A.ds[b];
    }
    RC(run_bn(net, i2, params, bnstats, acts, A, acts + A.r_o[b], identity, acts + A.o[b], n, iph, 1, st));
    x = acts + A.o[b];
  }
  RC(vdqn_avgpool_fwd(x, acts + A.avg, n, 49, 512, dt, st));
  RC(run_conv(net, net->layers[net->l_top4], packed, acts + A.avg, acts + A.q, n_samples, nullptr, 0, reinterpret_cast<float*>(acts + A.qf), st));
  return VDQN_OK;
}

}  // namespace

extern "C" int vdqn_net_forward(vdqn_net* net, const void* packed, const void* frames, int32_t src_kind, int32_t n_samples, void* acts,
                                float* q_out, void* stream) {
  VDQN_CHECK(net && packed && frames && acts && q_out, "vdqn_net_forward: null arg");
  VDQN_CHECK(n_samples >= 1 && n_samples <= net->cfg.max_batch, "vdqn_net_forward: n_samples %d exceeds max_batch %d", n_samples, net->cfg.max_batch);
  hipStream_t st = (hipStream_t)stream;
  const ActLayout A = act_layout(net, n_samples);
  unsigned char* ab = (unsigned char*)acts;
  RC(vdqn_pack_input(frames, src_kind, ab + A.t_in, n_samples * net->cfg.num_frames, net->cfg.dtype, st));
  RC(forward_impl(net, (const unsigned char*)packed, ab + A.t_in, n_samples, ab, A, st));
  const int nq = net->cfg.action_dim * net->cfg.num_classes;
  hipError_t e = hipMemcpy2DAsync(q_out, (size_t)nq * 4, ab + A.qf, 64 * 4, (size_t)nq * 4, (size_t)n_samples, hipMemcpyDeviceToDevice, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_forward: q copy failed: %s", hipGetErrorString(e));
  return VDQN_OK;
}

extern "C" int vdqn_net_trunk_forward(vdqn_net* net, const void* packed, const void* frames, int32_t src_kind, int32_t n_samples, void* acts,
                                      void* stream) {
  VDQN_CHECK(net && packed && frames && acts, "vdqn_net_trunk_forward: null arg");
  VDQN_CHECK(n_samples >= 1 && n_samples <= net->cfg.max_batch, "vdqn_net_trunk_forward: n_samples %d exceeds max_batch %d", n_samples, net->cfg.max_batch);
  hipStream_t st = (hipStream_t)stream;
  const ActLayout A = act_layout(net, n_samples);
  unsigned char* ab = (unsigned char*)acts;
  RC(vdqn_pack_input(frames, src_kind, ab + A.t_in, n_samples * net->cfg.num_frames, net->cfg.dtype, st));
  return forward_impl(net, (const unsigned char*)packed, ab + A.t_in, n_samples, ab, A, st, true);
}

extern "C" int vdqn_net_forward_train(vdqn_net* net, const float* params, float* bnstats, void* packed, const void* frames, int32_t src_kind,
                                      int32_t n_samples, void* acts, float* q_out, void* stream) {
  VDQN_CHECK(net && params && bnstats && packed && frames && acts && q_out, "vdqn_net_forward_train: null arg");
  VDQN_CHECK(net->basic(), "vdqn_net_forward_train: only ARCHITECTURE='basic' has train-mode BatchNorm (extra_capacity: use vdqn_net_forward)");
  VDQN_CHECK(n_samples >= 1 && n_samples <= net->cfg.max_batch, "vdqn_net_forward_train: n_samples %d exceeds max_batch %d", n_samples, net->cfg.max_batch);
  hipStream_t st = (hipStream_t)stream;
  const ActLayout A = act_layout(net, n_samples);
  unsigned char* ab = (unsigned char*)acts;
  RC(vdqn_net_pack_weights(net, params, bnstats, packed, 2, st));
  RC(vdqn_pack_input(frames, src_kind, ab + A.t_in, n_samples * net->cfg.num_frames, net->cfg.dtype, st));
  RC(forward_train_impl(net, (const unsigned char*)packed, params, bnstats, ab + A.t_in, n_samples, 1, ab, A, st));
  const int nq = net->cfg.action_dim * net->cfg.num_classes;
  hipError_t e = hipMemcpy2DAsync(q_out, (size_t)nq * 4, ab + A.qf, 64 * 4, (size_t)nq * 4, (size_t)n_samples, hipMemcpyDeviceToDevice, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_forward_train: q copy failed: %s", hipGetErrorString(e));
  return VDQN_OK;
}

// samples the `acts_online` workspace of this update is laid out for
static int step_layout_samples(const vdqn_net* net, const vdqn_step_args* a) {
  if (a->acts_samples > 0) return a->acts_samples;  // the workspace of one vdqn_net_forward call (vdqn_net_backward_begin)
  if (a->train_on_ground_truth) return a->batch;
  return 2 * a->batch;
}

// the frames of one update or validation batch into `dst`: s, then s' behind it (not in the ground-truth branch); nothing when the
// caller packed them ahead of time (vdqn_step_args.packed_frames)
static int pack_step_frames(const vdqn_net* net, const vdqn_step_args* a, unsigned char* dst, int B, hipStream_t st) {
  const int F = net->cfg.num_frames, dt = net->cfg.dtype;
  const bool gtb = a->train_on_ground_truth != 0;
  // one pack for s and s': the same [B][4] shift / mirror, zoom window and colour factors (NULL: none) for both
  const auto pack = [&](const void* src, void* to) {
    if (a->aug_zoom) return vdqn_pack_input_aug_zoom(src, to, B * F, F, a->aug_params, a->aug_color, a->aug_zoom, B, dt, st);
    if (a->aug_color) return vdqn_pack_input_aug_color(src, to, B * F, F, a->aug_params, a->aug_color, B, dt, st);
    if (a->aug_params) return vdqn_pack_input_aug(src, to, B * F, F, a->aug_params, B, dt, st);
    if (a->packed_frames) return (int)VDQN_OK;
    return vdqn_pack_input(src, a->src_kind, to, B * F, dt, st);
  };
  RC(pack(a->before, dst));
  if (!gtb) RC(pack(a->after, dst + (int64_t)B * F * frame_bytes(net)));
  return VDQN_OK;
}

// what the TD loss and the validation metrics both read: Q(s), Q(s') of the online pass over [s; s'], Q(s') of the target pass, and
// the step's inputs and loss options.  What only training has (loss, dq, inv_count, dtype, deterministic, q_copy) stays zero.
static vdqn_td_args fill_td_args(const vdqn_net* net, const vdqn_step_args* a, const float* qf_online, const float* qf_target, int B) {
  vdqn_td_args t;
  memset(&t, 0, sizeof(t));
  t.q_before = qf_online;
  t.q_after_online = qf_online + (size_t)B * 64;
  t.q_after_target = qf_target;
  t.act = a->act; t.rew = a->rew; t.term = a->term; t.valid = a->valid;
  t.batch = B; t.n_cat = net->cfg.num_classes; t.n_act = net->cfg.action_dim; t.ldq = 64;
  t.gamma = a->gamma;
  t.clip_rect = a->clip_rect; t.linear = a->linear; t.use_valid = a->use_valid;
  t.loss_kind = a->loss_kind;
  return t;
}

// What one TD update's loss is, filled by the exported vdqn_net_td_forward* entry that was called.  `algo` picks the loss launch
// and indexes kAlgos; the TD family (plain, weighted, n-step, CQL, Monte-Carlo floor / Cal-QL) reads the four fields marked so, each
// head algorithm its own scalars.  `stats` (n_stats floats, NULL ok) and cql_penalty (cql_alpha > 0) are cleared before the launch.
namespace {
enum LossAlgo { ALGO_TD = 0, ALGO_IQL, ALGO_DIST, ALGO_BCQ };
struct LossSpec {
  LossAlgo algo;
  float* stats;
  int n_stats;
  float cql_alpha; float* cql_penalty; const float* mc_return; int32_t mc_flags;  // the TD family
  float iql_expectile;
  int32_t dist_flags; float dist_sigma_min;
  float bcq_threshold, bcq_bc_weight, bcq_logit_reg;
};
// One row per LossAlgo; the TD family's is that of vdqn_net_td_forward_mc, its one entry with statistics and row refusals.
struct AlgoRow {
  const char* entry;
  const char* eval_entry;        // its validation batch: vdqn_net_td_eval plus the head metrics launch (NULL: the TD family's is vdqn_net_td_eval alone)
  Head head;                     // the head the net must carry
  const char *no_gt, *no_linear;  // why train_on_ground_truth and linear are refused
  int n_stats;
  bool target_over_before;  // the target pass reads s, not s'
};
const char kNoBootstrap[] = "the ground-truth branch regresses Q(s, a) on given targets and bootstraps nothing (train_on_ground_truth)";
const AlgoRow kAlgos[] = {
    {"vdqn_net_td_forward_mc", nullptr, HEAD_NONE, "mc_return is given, but the ground-truth branch has no target to floor and no penalty to calibrate (train_on_ground_truth)",
     "mc_return is given with linear: y = r + (Qa - 0.1) has no discount, and a discounted return bounds nothing of it", 2, false},
    {"vdqn_net_td_forward_iql", "vdqn_net_td_eval_iql", HEAD_VALUE, kNoBootstrap,
     "linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target and has no V(s') form", 2, true},
    {"vdqn_net_td_forward_dist", "vdqn_net_td_eval_dist", HEAD_SPREAD, kNoBootstrap,
     "linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; a variance has no backup without a discount", 2, false},
    {"vdqn_net_td_forward_bcq", "vdqn_net_td_eval_bcq", HEAD_POLICY, kNoBootstrap,
     "linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; the constrained target is not defined for it", 3, false},
};
LossSpec loss_spec(LossAlgo algo, float* stats) { return {algo, stats, kAlgos[algo].n_stats}; }  // (the rest zero)
// the refusals every row shares: the net lacks the row's head, the ground-truth branch, linear; in the name of `entry` (NULL: the
// row's update entry)
int refuse_by_row(const AlgoRow& r, const vdqn_net* net, const vdqn_step_args* a, const char* entry = nullptr) {
  if (!entry) entry = r.entry;
  static const char* const head_word[] = {"", "value", "spread", "policy"};
  static const char* const head_create[] = {"", "vdqn_net_create_v(cfg, 1, ..)", "vdqn_net_create_d(cfg, 0, 1, ..)", "vdqn_net_create_p(cfg, 0, 0, 1, ..)"};
  VDQN_CHECK(r.head == HEAD_NONE || net->head == r.head, "%s: the net has no %s head (create it with %s)", entry, head_word[r.head], head_create[r.head]);
  VDQN_CHECK(!a->train_on_ground_truth, "%s: %s", entry, r.no_gt);
  VDQN_CHECK(!a->linear, "%s: %s", entry, r.no_linear);
  return VDQN_OK;
}

int td_forward_impl(vdqn_net* net, const vdqn_step_args* a, const LossSpec& spec, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_forward: null arg");
  VDQN_CHECK(a->params && a->bnstats && a->packed_online && a->before && a->act && a->acts_online && a->bwd && a->loss, "vdqn_net_td_forward: null buffer");
  const int B = a->batch;
  const bool gtb = a->train_on_ground_truth != 0;
  VDQN_CHECK(B >= 1 && 2 * B <= net->cfg.max_batch, "vdqn_net_td_forward: batch %d needs max_batch >= %d", B, 2 * B);
  VDQN_CHECK(gtb ? (a->gt != nullptr) : (a->after && a->packed_target && a->rew && a->term), "vdqn_net_td_forward: missing inputs for this loss branch");
  VDQN_CHECK(gtb || a->acts_target, "vdqn_net_td_forward: acts_target is NULL");
  VDQN_CHECK(a->sample_weight || !a->sample_err, "vdqn_net_td_forward: sample_err without sample_weight");
  VDQN_CHECK(!a->sample_weight || !gtb, "vdqn_net_td_forward: sample_weight is given, but the ground-truth branch has no weighted loss");
  VDQN_CHECK(((uintptr_t)a->aug_params & 15) == 0, "vdqn_net_td_forward: aug_params must be 16-byte aligned");
  VDQN_CHECK(!a->aug_params || a->src_kind == 0, "vdqn_net_td_forward: aug_params take uint8 NHWC frames (src_kind 0), not src_kind %d", a->src_kind);
  VDQN_CHECK(!a->aug_params || !a->packed_frames, "vdqn_net_td_forward: aug_params are given, but packed_frames were packed without them");
  VDQN_CHECK(!a->aug_color || a->aug_params, "vdqn_net_td_forward: aug_color is given without aug_params (all-zero params are the plain geometry)");
  VDQN_CHECK(((uintptr_t)a->aug_color & 15) == 0, "vdqn_net_td_forward: aug_color must be 16-byte aligned");
  VDQN_CHECK(!a->aug_zoom || a->aug_params, "vdqn_net_td_forward: aug_zoom is given without aug_params (all-zero params are the plain geometry)");
  VDQN_CHECK(((uintptr_t)a->aug_zoom & 15) == 0, "vdqn_net_td_forward: aug_zoom must be 16-byte aligned");
  VDQN_CHECK(!a->sample_gamma || !gtb, "vdqn_net_td_forward: sample_gamma is given, but the ground-truth branch bootstraps nothing (train_on_ground_truth)");
  VDQN_CHECK(!a->sample_gamma || !a->linear, "vdqn_net_td_forward: sample_gamma is given with linear: y = r + (Qa - 0.1) has no discount and no n-step form");
  hipStream_t st = (hipStream_t)stream;
  const int F = net->cfg.num_frames, dt = net->cfg.dtype;
  const AlgoRow& row = kAlgos[spec.algo];
  const int ns_online = step_layout_samples(net, a);
  const ActLayout A = act_layout(net, ns_online);
  const BwdLayout W = bwd_layout(net, B);
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;

  // the frames are packed on the side stream while the main stream folds the weights (two small kernels each); the target
  // pass then simply continues on the side stream: it only reads the packed input and its own weights
  hipStream_t tst = fork(net, st);  // == st when the overlap is off
  // the packed frames of this update: the engine's own buffer, or the caller's (vdqn_step_args.packed_frames: packed ahead of time)
  const unsigned char* tin = a->packed_frames ? (const unsigned char*)a->packed_frames : ao + A.t_in;
  // (tried and measured slower, experiments/: the s' frames packed first with the target pass right behind them; the two packs
  // on two streams; a split weight fold with layer3+ beside the stem; stage folds behind their early Adam; online and target
  // forward as one chain of grouped launches; the online pass as two half-batch passes on two streams)
  RC(pack_step_frames(net, a, ao + A.t_in, B, tst));
  RC(vdqn_net_pack_weights(net, a->params, a->bnstats, a->packed_online, net->basic() ? 3 : 1, st));
  if (tst != st) join(net, net->side, st);  // packed input ready for the online pass
  if (!gtb) {
    const ActLayout T = act_layout(net, B);
    const unsigned char* tin_target = row.target_over_before ? tin : tin + (int64_t)B * F * frame_bytes(net);
    RC(forward_impl(net, (const unsigned char*)a->packed_target, tin_target, B, (unsigned char*)a->acts_target, T, tst, false, 0));  // (no backward: no arg-max bytes)
  }
  if (net->basic())  // two model calls (before, after), each with its own batch statistics; running stats updated in place
    RC(forward_train_impl(net, (const unsigned char*)a->packed_online, a->params, a->bnstats, tin, ns_online, gtb ? 1 : 2, ao, A, st));
  else
    RC(forward_impl(net, (const unsigned char*)a->packed_online, tin, ns_online, ao, A, st, false, B));
  if (tst != st) join(net, net->side, st);

  // (clearing the 47 MB of accumulators on a side stream beside the packs instead of here, between the forward pass and the loss,
  // measured no gain: profiles/r6_12_ab_inproc_fused_head_and_clear_placement.txt)
  hipError_t e = hipMemsetAsync(bw + W.zero_begin, 0, (size_t)W.zero_bytes, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_td_forward: memset failed: %s", hipGetErrorString(e));
  e = hipMemsetAsync(a->loss, 0, 4, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_td_forward: memset failed: %s", hipGetErrorString(e));
  if (spec.cql_alpha > 0.f && spec.cql_penalty) {
    e = hipMemsetAsync(spec.cql_penalty, 0, 4, st);
    VDQN_CHECK(e == hipSuccess, "vdqn_net_td_forward_cql: memset failed: %s", hipGetErrorString(e));
  }
  if (spec.stats) {
    e = hipMemsetAsync(spec.stats, 0, 4 * (size_t)spec.n_stats, st);
    VDQN_CHECK(e == hipSuccess, "%s: memset failed: %s", row.entry, hipGetErrorString(e));
  }

  const float* qf_online = reinterpret_cast<const float*>(ao + A.qf);
  if (!gtb) {
    const ActLayout T = act_layout(net, B);
    unsigned char* at = (unsigned char*)a->acts_target;
    vdqn_td_args t = fill_td_args(net, a, qf_online, reinterpret_cast<const float*>(at + T.qf), B);
    t.loss = a->loss;
    t.dq = bw + W.dq;
    t.inv_count = a->inv_count;
    t.dtype = dt;
    t.deterministic = net->cfg.deterministic;
    t.q_copy = a->q_before;  // (the compact copy of Q(s) rides in the loss launch: no 2-D copy between the loss and the first data gradient)
    float* pen = spec.cql_alpha > 0.f ? spec.cql_penalty : nullptr;
    const float *sw = a->sample_weight, *sg = a->sample_gamma;
    float* se = a->sample_err;
    switch (spec.algo) {
      case ALGO_BCQ: RC(vdqn_td_loss_bcq(&t, sw, se, sg, spec.bcq_threshold, spec.bcq_bc_weight, spec.bcq_logit_reg, spec.stats, st)); break;
      case ALGO_DIST: RC(vdqn_td_loss_dist(&t, sw, se, sg, spec.dist_flags, spec.dist_sigma_min, spec.stats, st)); break;
      case ALGO_IQL: RC(vdqn_td_loss_iql(&t, sw, se, sg, spec.iql_expectile, spec.stats, st)); break;
      case ALGO_TD:
        if (spec.mc_return) RC(vdqn_td_loss_mc(&t, sw, se, spec.cql_alpha, pen, sg, spec.mc_return, spec.mc_flags, spec.stats, st));
        else if (sg) RC(vdqn_td_loss_nstep(&t, sw, se, spec.cql_alpha, pen, sg, st));
        else if (spec.cql_alpha > 0.f) RC(vdqn_td_loss_cql(&t, sw, se, spec.cql_alpha, spec.cql_penalty, st));
        else if (sw) RC(vdqn_td_loss_weighted(&t, sw, se, st));
        else RC(vdqn_td_loss(&t, st));
        break;
    }
  } else {
    RC(vdqn_gt_loss(qf_online, a->act, a->gt, a->loss, bw + W.dq, nullptr, B, net->cfg.num_classes, net->cfg.action_dim, 64, a->inv_count,
                    a->value_learning, dt, st));
  }
  if (a->q_before && gtb) {
    const int nq = net->cfg.action_dim * net->cfg.num_classes;
    e = hipMemcpy2DAsync(a->q_before, (size_t)nq * 4, qf_online, 64 * 4, (size_t)nq * 4, (size_t)B, hipMemcpyDeviceToDevice, st);
    VDQN_CHECK(e == hipSuccess, "vdqn_net_td_forward: q copy failed: %s", hipGetErrorString(e));
  }
  return VDQN_OK;
}

}  // namespace

extern "C" int vdqn_net_td_forward(vdqn_net* net, const vdqn_step_args* a, void* stream) { return td_forward_impl(net, a, loss_spec(ALGO_TD, nullptr), stream); }

extern "C" int vdqn_net_td_forward_cql(vdqn_net* net, const vdqn_step_args* a, float cql_alpha, float* cql_penalty, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_forward_cql: null arg");
  VDQN_CHECK(isfinite(cql_alpha) && cql_alpha >= 0.f, "vdqn_net_td_forward_cql: cql_alpha %g must be finite and >= 0 (0 = vdqn_net_td_forward)", (double)cql_alpha);
  if (cql_alpha > 0.f) {
    VDQN_CHECK(!a->train_on_ground_truth, "vdqn_net_td_forward_cql: the ground-truth branch regresses Q(s, a) on given targets and has no conservative penalty (train_on_ground_truth with cql_alpha > 0)");
    VDQN_CHECK(net->cfg.action_dim >= 2, "vdqn_net_td_forward_cql: action_dim is 1: with one action the penalty is identically zero");
  }
  LossSpec spec = loss_spec(ALGO_TD, nullptr);
  spec.cql_alpha = cql_alpha; spec.cql_penalty = cql_penalty;
  return td_forward_impl(net, a, spec, stream);
}

// Each entry below refuses, before the forward, everything its loss launch would refuse; the order decides which message a call
// with several faults meets.
// vdqn_net_td_forward_cql with the Monte-Carlo return of every sampled row (csrc/mcreturn.hip) for the loss launch: per-update
// inputs, plain arguments, nothing kept in the engine.
extern "C" int vdqn_net_td_forward_mc(vdqn_net* net, const vdqn_step_args* a, float cql_alpha, float* cql_penalty, const float* mc_return,
                                      int32_t mc_flags, float* mc_stats, void* stream) {
  if (!mc_return) return vdqn_net_td_forward_cql(net, a, cql_alpha, cql_penalty, stream);
  VDQN_CHECK(net && a, "vdqn_net_td_forward_mc: null arg");
  VDQN_CHECK(isfinite(cql_alpha) && cql_alpha >= 0.f, "vdqn_net_td_forward_mc: cql_alpha %g must be finite and >= 0", (double)cql_alpha);
  RC(refuse_by_row(kAlgos[ALGO_TD], net, a));
  VDQN_CHECK((mc_flags & ~3) == 0, "vdqn_net_td_forward_mc: mc_flags 0x%x has unknown bits (bit 0 = floor, bit 1 = calibrated)", (unsigned)mc_flags);
  VDQN_CHECK(mc_flags != 0, "vdqn_net_td_forward_mc: mc_flags is 0: at least one of bit 0 (floor) and bit 1 (calibrated) must be set");
  VDQN_CHECK(!(mc_flags & 2) || cql_alpha > 0.f, "vdqn_net_td_forward_mc: mc_flags bit 1 (calibrated) needs cql_alpha > 0");
  if (cql_alpha > 0.f) VDQN_CHECK(net->cfg.action_dim >= 2, "vdqn_net_td_forward_mc: action_dim is 1: with one action the penalty is identically zero");
  LossSpec spec = loss_spec(ALGO_TD, mc_stats);
  spec.cql_alpha = cql_alpha; spec.cql_penalty = cql_penalty; spec.mc_return = mc_return; spec.mc_flags = mc_flags;
  return td_forward_impl(net, a, spec, stream);
}

// implicit Q-learning (csrc/iql.hip)
extern "C" int vdqn_net_td_forward_iql(vdqn_net* net, const vdqn_step_args* a, float expectile, float* iql_stats, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_forward_iql: null arg");
  RC(refuse_by_row(kAlgos[ALGO_IQL], net, a));
  VDQN_CHECK(isfinite(expectile) && expectile >= 0.5f && expectile < 1.0f, "vdqn_net_td_forward_iql: expectile %g must be in [0.5, 1)", (double)expectile);
  LossSpec spec = loss_spec(ALGO_IQL, iql_stats);
  spec.iql_expectile = expectile;
  return td_forward_impl(net, a, spec, stream);
}

// Gaussian distributional Q-learning (csrc/dist.hip)
extern "C" int vdqn_net_td_forward_dist(vdqn_net* net, const vdqn_step_args* a, int32_t flags, float sigma_min, float* dist_stats, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_forward_dist: null arg");
  RC(refuse_by_row(kAlgos[ALGO_DIST], net, a));
  VDQN_CHECK(a->loss_kind == 0, "vdqn_net_td_forward_dist: loss_kind %d: the loss is a KL divergence, which has no Huber form (loss_kind must be 0)", a->loss_kind);
  VDQN_CHECK((flags & ~3) == 0, "vdqn_net_td_forward_dist: flags 0x%x has unknown bits (bit 0 = KL_BACKWARDS, bit 1 = LOG_SIGMA)", (unsigned)flags);
  VDQN_CHECK(isfinite(sigma_min) && sigma_min >= 1e-4f && sigma_min <= 10.0f, "vdqn_net_td_forward_dist: sigma_min %g must be in [1e-4, 10]", (double)sigma_min);
  LossSpec spec = loss_spec(ALGO_DIST, dist_stats);
  spec.dist_flags = flags; spec.dist_sigma_min = sigma_min;
  return td_forward_impl(net, a, spec, stream);
}

// discrete batch-constrained Q-learning (csrc/bcq.hip)
extern "C" int vdqn_net_td_forward_bcq(vdqn_net* net, const vdqn_step_args* a, float threshold, float bc_weight, float logit_reg, float* bcq_stats,
                                       void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_forward_bcq: null arg");
  RC(refuse_by_row(kAlgos[ALGO_BCQ], net, a));
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_net_td_forward_bcq: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK(isfinite(threshold) && threshold >= 0.0f && threshold < 1.0f, "vdqn_net_td_forward_bcq: threshold %g must be in [0, 1)", (double)threshold);
  VDQN_CHECK(isfinite(bc_weight) && bc_weight > 0.0f, "vdqn_net_td_forward_bcq: bc_weight %g must be finite and > 0", (double)bc_weight);
  VDQN_CHECK(isfinite(logit_reg) && logit_reg >= 0.0f, "vdqn_net_td_forward_bcq: logit_reg %g must be finite and >= 0", (double)logit_reg);
  LossSpec spec = loss_spec(ALGO_BCQ, bcq_stats);
  spec.bcq_threshold = threshold; spec.bcq_bc_weight = bc_weight; spec.bcq_logit_reg = logit_reg;
  return td_forward_impl(net, a, spec, stream);
}

// One held-out batch of a validation pass (train_q_network.py:183-186 `eval_losses`, :240 `# checkpoint and eval`): the frames
// packed as td_forward_impl packs them, the target pass over s' on the side stream beside the online pass over [s; s'] — both
// through forward_impl, i.e. eval-mode BatchNorm in either architecture, with grad_samples = 0 (no arg-max bytes) — then the
// metrics launch on the two qf tensors.  `packed_online` is read as the caller folded it; nothing but the two activation
// workspaces and `acc` is written.  The layouts are those of 2 * batch and batch samples: prefixes of the workspaces of any larger batch.
extern "C" int vdqn_net_td_eval(vdqn_net* net, const vdqn_step_args* a, double* acc, void* stream) {
  VDQN_CHECK(net && a && acc, "vdqn_net_td_eval: null arg");
  VDQN_CHECK(!a->train_on_ground_truth, "vdqn_net_td_eval: train_on_ground_truth: the ground-truth branch has no target network and no TD error to validate");
  VDQN_CHECK(!a->sample_weight, "vdqn_net_td_eval: sample_weight is given: validation metrics are unweighted");
  VDQN_CHECK(!a->sample_err, "vdqn_net_td_eval: sample_err is given: the metrics launch writes no per-sample errors");
  VDQN_CHECK(!a->aug_params, "vdqn_net_td_eval: aug_params are given: validation frames are not augmented");
  VDQN_CHECK(!a->aug_color, "vdqn_net_td_eval: aug_color is given: validation frames are not augmented");
  VDQN_CHECK(!a->aug_zoom, "vdqn_net_td_eval: aug_zoom is given: validation frames are not augmented");
  VDQN_CHECK(!a->packed_frames, "vdqn_net_td_eval: packed_frames are given: the validation pass packs its own frames");
  VDQN_CHECK(!a->sample_gamma, "vdqn_net_td_eval: sample_gamma is given: validation is one-step (the scalar gamma), whatever the training target");
  VDQN_CHECK(a->acts_samples == 0, "vdqn_net_td_eval: acts_samples %d must be 0", a->acts_samples);
  VDQN_CHECK(a->packed_online && a->packed_target && a->before && a->after && a->act && a->rew && a->term && a->acts_online && a->acts_target,
             "vdqn_net_td_eval: null buffer");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_net_td_eval: use_valid without valid mask");
  const int B = a->batch;
  VDQN_CHECK(B >= 1 && 2 * (int64_t)B <= net->cfg.max_batch, "vdqn_net_td_eval: batch %d needs max_batch >= 2 * batch (max_batch %d)", B, net->cfg.max_batch);
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_net_td_eval: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK((((uintptr_t)acc) & 7) == 0, "vdqn_net_td_eval: acc must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int F = net->cfg.num_frames;
  const ActLayout A = act_layout(net, 2 * B), T = act_layout(net, B);
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* at = (unsigned char*)a->acts_target;
  hipStream_t tst = fork(net, st);  // == st when the overlap is off; ordered behind the previous batch's metrics launch
  RC(pack_step_frames(net, a, ao + A.t_in, B, tst));  // (plain: aug and packed_frames were refused above)
  if (tst != st) join(net, net->side, st);  // packed input ready for the online pass
  RC(forward_impl(net, (const unsigned char*)a->packed_target, ao + A.t_in + (int64_t)B * F * frame_bytes(net), B, at, T, tst, false, 0));
  RC(forward_impl(net, (const unsigned char*)a->packed_online, ao + A.t_in, 2 * B, ao, A, st, false, 0));
  if (tst != st) join(net, net->side, st);
  const float* qf_online = reinterpret_cast<const float*>(ao + A.qf);
  const vdqn_td_args t = fill_td_args(net, a, qf_online, reinterpret_cast<const float*>(at + T.qf), B);
  return vdqn_td_eval(&t, acc, st);
}

// One held-out batch under a head algorithm: everything vdqn_net_td_eval does, its refusals included, and behind its metrics launch
// the row's head metrics launch (csrc/eval.hip) into acc_head (device f64 [num_classes + 1][8], accumulated into).  Every refusal of
// the entry, the row (refuse_by_row) and the head operator's scalars comes before any launch.
namespace {
struct HeadEval {
  vdqn_td_args t;
  hipStream_t st;
  const unsigned char* t_in;  // the packed frames of [s; s'] in acts_online
  unsigned char* at;
  ActLayout T;
};
// vdqn_net_td_eval, then what the head launch needs: the operator's arguments on the two qf tensors, and where the target pass lives
int head_eval_begin(vdqn_net* net, const vdqn_step_args* a, double* acc, const double* acc_head, LossAlgo algo, HeadEval* h, void* stream) {
  const char* entry = kAlgos[algo].eval_entry;
  VDQN_CHECK(acc_head, "%s: null arg", entry);
  VDQN_CHECK((((uintptr_t)acc_head) & 7) == 0, "%s: acc_head must be 8-byte aligned", entry);
  RC(vdqn_net_td_eval(net, a, acc, stream));
  const int B = a->batch;
  const ActLayout A = act_layout(net, 2 * B);
  unsigned char* ao = (unsigned char*)a->acts_online;
  h->st = (hipStream_t)stream;
  h->t_in = ao + A.t_in;
  h->at = (unsigned char*)a->acts_target;
  h->T = act_layout(net, B);
  h->t = fill_td_args(net, a, reinterpret_cast<const float*>(ao + A.qf), reinterpret_cast<const float*>(h->at + h->T.qf), B);
  return VDQN_OK;
}
}  // namespace

// IQL's head metrics read Q_target(s, a_data), and acts_target holds one pass of `batch` samples, so a SECOND target pass runs over
// the `before` half of the packed frames into the same workspace.  The ordering, with the overlap on (off: one stream, program order):
//   1. vdqn_net_td_eval's metrics launch, on `stream`, reads Q_target(s') in acts_target.  fork() behind it makes the side stream
//      wait for everything queued on `stream` so far, that launch included, so the second pass overwrites acts_target only after it
//      was read.  (The side stream's own order puts the second pass behind the first.)
//   2. join() makes `stream` wait for the second pass; the head launch, on `stream`, then reads Q_target(s).
//   3. The next batch's entry (this one, vdqn_net_td_eval or an update's vdqn_net_td_forward*) opens with fork(net, stream): its
//      pack, which rewrites the packed frames the second pass read, and its target pass, which rewrites acts_target, wait for
//      everything on `stream`, the head launch included.  Its online pass follows the head launch on `stream` itself.
// The packed frames are written by nobody between the pack and step 3, and the online pass only reads them.
extern "C" int vdqn_net_td_eval_iql(vdqn_net* net, const vdqn_step_args* a, float expectile, double* acc, double* acc_head, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_eval_iql: null arg");
  RC(refuse_by_row(kAlgos[ALGO_IQL], net, a, kAlgos[ALGO_IQL].eval_entry));
  VDQN_CHECK(isfinite(expectile) && expectile >= 0.5f && expectile < 1.0f, "vdqn_net_td_eval_iql: expectile %g must be in [0.5, 1)", (double)expectile);
  HeadEval h;
  RC(head_eval_begin(net, a, acc, acc_head, ALGO_IQL, &h, stream));
  hipStream_t tst = fork(net, h.st);  // == st when the overlap is off; behind the metrics launch that read Q_target(s')
  RC(forward_impl(net, (const unsigned char*)a->packed_target, h.t_in, a->batch, h.at, h.T, tst, false, 0));  // the target over s
  if (tst != h.st) join(net, net->side, h.st);
  return vdqn_td_eval_iql(&h.t, expectile, acc_head, h.st);
}

// DIST and BCQ read the two qf tensors vdqn_net_td_eval's launch has just read: one more launch on `stream`, nothing to order.
extern "C" int vdqn_net_td_eval_dist(vdqn_net* net, const vdqn_step_args* a, int32_t flags, float sigma_min, double* acc, double* acc_head, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_eval_dist: null arg");
  RC(refuse_by_row(kAlgos[ALGO_DIST], net, a, kAlgos[ALGO_DIST].eval_entry));
  VDQN_CHECK(a->loss_kind == 0, "vdqn_net_td_eval_dist: loss_kind %d: the loss is a KL divergence, which has no Huber form (loss_kind must be 0)", a->loss_kind);
  VDQN_CHECK((flags & ~3) == 0, "vdqn_net_td_eval_dist: flags 0x%x has unknown bits (bit 0 = KL_BACKWARDS, bit 1 = LOG_SIGMA)", (unsigned)flags);
  VDQN_CHECK(isfinite(sigma_min) && sigma_min >= 1e-4f && sigma_min <= 10.0f, "vdqn_net_td_eval_dist: sigma_min %g must be in [1e-4, 10]", (double)sigma_min);
  HeadEval h;
  RC(head_eval_begin(net, a, acc, acc_head, ALGO_DIST, &h, stream));
  return vdqn_td_eval_dist(&h.t, flags, sigma_min, acc_head, h.st);
}

extern "C" int vdqn_net_td_eval_bcq(vdqn_net* net, const vdqn_step_args* a, float threshold, double* acc, double* acc_head, void* stream) {
  VDQN_CHECK(net && a, "vdqn_net_td_eval_bcq: null arg");
  RC(refuse_by_row(kAlgos[ALGO_BCQ], net, a, kAlgos[ALGO_BCQ].eval_entry));
  VDQN_CHECK(net->cfg.action_dim >= 2, "vdqn_net_td_eval_bcq: action_dim is 1: with one action there is nothing to constrain");
  VDQN_CHECK(isfinite(threshold) && threshold >= 0.0f && threshold < 1.0f, "vdqn_net_td_eval_bcq: threshold %g must be in [0, 1)", (double)threshold);
  HeadEval h;
  RC(head_eval_begin(net, a, acc, acc_head, ALGO_BCQ, &h, stream));
  return vdqn_td_eval_bcq(&h.t, threshold, acc_head, h.st);
}

namespace {

// backward of BasicBlock b (gradient of its output, already ReLU-masked, is in g_o[b]).  want_wgrad false (vdqn_net_backward_data):
// the data gradients alone, each launch with the arguments the training walk gives it, all on `st`.
int block_backward(vdqn_net* net, const vdqn_step_args* a, int b, const ActLayout& A, const BwdLayout& W, int n, hipStream_t st,
                   bool want_wgrad = true) {
  const unsigned char* pk = (const unsigned char*)a->packed_online;
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;
  const Layer& c1 = net->layers[net->l_b_conv1[b]];
  const Layer& c2 = net->layers[net->l_b_conv2[b]];
  const unsigned char* x = b == 0 ? ao + A.pool : ao + A.o[b - 1];
  unsigned char* gx = b == 0 ? bw + W.g_pool : bw + W.g_o[b - 1];
  const void* g_out = bw + W.g_o[b];
  // conv2: weight gradient, then data gradient into g_h masked by relu(h)
  if (want_wgrad) {
    hipStream_t ws = wgrad_stream(net, st);  // g_out is complete on `st`
    RC(run_wgrad(net, c2, bw, W, g_out, ao + A.h[b], n, ws));
    if (net->l_b_ds[b] >= 0) RC(run_wgrad(net, net->layers[net->l_b_ds[b]], bw, W, g_out, x, n, ws));
  }
  RC(run_dgrad(net, c2, pk, g_out, bw + W.g_h[b], n, nullptr, ao + A.h[b], st, bw + W.part[part_h(b)]));
  if (want_wgrad) RC(run_wgrad(net, c1, bw, W, bw + W.g_h[b], x, n, wgrad_stream(net, st)));  // g_h is complete
  const void* resid = g_out;  // identity shortcut
  if (net->l_b_ds[b] >= 0) {
    const Layer& ds = net->layers[net->l_b_ds[b]];
    if (fuse_ds()) {  // the shortcut's gradient is the downsample's data gradient: summed inside conv1's data-gradient launch
      RC(run_dgrad(net, c1, pk, bw + W.g_h[b], gx, n, nullptr, x, st, bw + W.part[b > 0 ? part_o(b - 1) : kPartPool], &ds, g_out));
      return VDQN_OK;
    }
    RC(run_dgrad(net, ds, pk, g_out, bw + W.dsg[b], n, nullptr, nullptr, st));
    resid = bw + W.dsg[b];
  }
  RC(run_dgrad(net, c1, pk, bw + W.g_h[b], gx, n, resid, x, st, bw + W.part[b > 0 ? part_o(b - 1) : kPartPool]));
  return VDQN_OK;
}

// extra_capacity, the head's four links and features.8: from dq down to g_o[7].  part_rows[i]: rows per entry of the column-sum
// partials that are layer i's bias gradient, as their producer reports them.
int head_backward(vdqn_net* net, const vdqn_step_args* a, const ActLayout& A, const BwdLayout& W, int B, int n, hipStream_t st, int* part_rows,
                  bool want_wgrad = true) {
  const unsigned char* pk = (const unsigned char*)a->packed_online;
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;
  const Layer& t4 = net->layers[net->l_top4];
  const Layer& t2 = net->layers[net->l_top2];
  const Layer& t0 = net->layers[net->l_top0];
  const Layer& f8 = net->layers[net->l_f8];
  if (want_wgrad) RC(run_wgrad(net, t4, bw, W, bw + W.dq, ao + A.l1, B, wgrad_stream(net, st), true));
  RC(run_dgrad(net, t4, pk, bw + W.dq, bw + W.g_l1, B, nullptr, ao + A.l1, st, bw + W.part[kPartL1], nullptr, nullptr, &part_rows[net->l_top2]));
  if (want_wgrad) RC(run_wgrad(net, t2, bw, W, bw + W.g_l1, ao + A.l0, B, wgrad_stream(net, st)));
  RC(run_dgrad(net, t2, pk, bw + W.g_l1, bw + W.g_l0, B, nullptr, ao + A.l0, st, bw + W.part[kPartL0], nullptr, nullptr, &part_rows[net->l_top0]));
  if (want_wgrad) RC(run_wgrad(net, t0, bw, W, bw + W.g_l0, ao + A.f8, B, wgrad_stream(net, st)));
  RC(run_dgrad(net, t0, pk, bw + W.g_l0, bw + W.g_f8, B, nullptr, ao + A.f8, st, bw + W.part[kPartF8], nullptr, nullptr, &part_rows[net->l_f8]));
  if (want_wgrad) RC(run_wgrad(net, f8, bw, W, bw + W.g_f8, ao + A.o[7], n, wgrad_stream(net, st)));
  RC(run_dgrad(net, f8, pk, bw + W.g_f8, bw + W.g_o[7], n, nullptr, ao + A.o[7], st, bw + W.part[part_o(7)]));
  return VDQN_OK;
}

// train-mode BatchNorm backward of layer li on the `before` half: dy = d/dy of bn(y), parameter gradients straight into `grads`
int run_bn_bwd(const vdqn_net* net, const vdqn_step_args* a, int li, const ActLayout& A, const void* g, const void* y, void* dy, int n,
               hipStream_t st) {
  const Layer& L = net->layers[li];
  BnSync sy = net->bn_sync;
  sy.scratch = reinterpret_cast<float*>((unsigned char*)a->acts_online + A.bn_sync);
  if (A.bn_det >= 0) {
    sy.det_ws = reinterpret_cast<float*>((unsigned char*)a->acts_online + A.bn_det);
    sy.det_ws_bytes = A.bn_det_bytes;
  }
  return vdqn_bn_train_bwd_impl(g, y, dy, reinterpret_cast<float*>((unsigned char*)a->acts_online + A.bnw[li]), a->grads + L.g_off, a->grads + L.b_off,
                                n, L.ho * L.wo, L.co, net->cfg.num_frames, n, net->cfg.dtype, st, &sy);
}

// 'basic': BasicBlock b with train-mode BatchNorm; g_o[b] holds the (ReLU-masked) gradient of the block output
int block_backward_train(vdqn_net* net, const vdqn_step_args* a, int b, const ActLayout& A, const BwdLayout& W, int n, hipStream_t st) {
  const unsigned char* pk = (const unsigned char*)a->packed_online;
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;
  const int i1 = net->l_b_conv1[b], i2 = net->l_b_conv2[b], ids = net->l_b_ds[b];
  const Layer& c1 = net->layers[i1];
  const Layer& c2 = net->layers[i2];
  const unsigned char* x = b == 0 ? ao + A.pool : ao + A.o[b - 1];
  unsigned char* gx = b == 0 ? bw + W.g_pool : bw + W.g_o[b - 1];
  const void* g_out = bw + W.g_o[b];
  RC(run_bn_bwd(net, a, i2, A, g_out, ao + A.r_o[b], bw + W.g_or[b], n, st));
  hipStream_t ws = fork(net, st);
  RC(run_wgrad(net, c2, bw, W, bw + W.g_or[b], ao + A.h[b], n, ws));
  if (ids >= 0) {
    RC(run_bn_bwd(net, a, ids, A, g_out, ao + A.r_ds[b], bw + W.g_dsr[b], n, st));
    ws = fork(net, st);
    RC(run_wgrad(net, net->layers[ids], bw, W, bw + W.g_dsr[b], x, n, ws));
  }
  RC(run_dgrad(net, c2, pk, bw + W.g_or[b], bw + W.g_h[b], n, nullptr, ao + A.h[b], st));
  RC(run_bn_bwd(net, a, i1, A, bw + W.g_h[b], ao + A.r_h[b], bw + W.g_h[b], n, st));
  ws = fork(net, st);
  RC(run_wgrad(net, c1, bw, W, bw + W.g_h[b], x, n, ws));
  const void* resid = g_out;
  if (ids >= 0) {
    RC(run_dgrad(net, net->layers[ids], pk, bw + W.g_dsr[b], bw + W.dsg[b], n, nullptr, nullptr, st));
    resid = bw + W.dsg[b];
  }
  RC(run_dgrad(net, c1, pk, bw + W.g_h[b], gx, n, resid, x, st));
  return VDQN_OK;
}

}  // namespace

extern "C" int vdqn_net_backward_begin(vdqn_net* net, const vdqn_step_args* a, const float* dq_f32, void* stream) {
  VDQN_CHECK(net && a && dq_f32, "vdqn_net_backward_begin: null arg");
  VDQN_CHECK(!net->basic(), "vdqn_net_backward_begin: only extra_capacity (eval-mode BatchNorm) has a per-call backward; ARCHITECTURE='basic' trains through vdqn_net_td_forward");
  VDQN_CHECK(a->params && a->bnstats && a->packed_online && a->acts_online && a->bwd && a->grads, "vdqn_net_backward_begin: null buffer");
  VDQN_CHECK(a->batch >= 1 && a->batch <= net->cfg.max_batch && a->acts_samples == a->batch,
             "vdqn_net_backward_begin: acts_samples (%d) must equal batch (%d) <= max_batch", a->acts_samples, a->batch);
  hipStream_t st = (hipStream_t)stream;
  const int B = a->batch;
  const BwdLayout W = bwd_layout(net, B);
  unsigned char* bw = (unsigned char*)a->bwd;
  hipError_t e = hipMemsetAsync(bw + W.zero_begin, 0, (size_t)W.zero_bytes, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_backward_begin: memset failed: %s", hipGetErrorString(e));
  launch_dq_pad(net, dq_f32, bw + W.dq, B, st);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" void* vdqn_net_grad_stream(vdqn_net* net) {
  if (!net || !side_ready(net)) return nullptr;
  return (void*)net->side;
}

extern "C" int vdqn_net_backward_stage(vdqn_net* net, const vdqn_step_args* a, int32_t stage, void* stream) {
  VDQN_CHECK(net && a && a->grads, "vdqn_net_backward_stage: null arg");
  VDQN_CHECK(stage >= 0 && stage < 3, "vdqn_net_backward_stage: stage %d", stage);
  hipStream_t st = (hipStream_t)stream;
  const int B = a->batch, F = net->cfg.num_frames, n = B * F, dt = net->cfg.dtype;
  const bool gtb = a->train_on_ground_truth != 0;
  const ActLayout A = act_layout(net, step_layout_samples(net, a));
  const BwdLayout W = bwd_layout(net, B);
  const unsigned char* pk = (const unsigned char*)a->packed_online;
  unsigned char* ao = (unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;
  bool split_conv1 = false;  // stage 2, extra_capacity: conv1's weight gradient is unfolded separately (see below)
  int part_rows[kMaxLayers];  // rows per entry of the column-sum partials that are layer i's bias gradient: what their producer reports
  std::fill(part_rows, part_rows + kMaxLayers, kTileRows);

  if (net->basic()) {
    if (stage == 0) {
      const Layer& top = net->layers[net->l_top4];
      RC(run_wgrad(net, top, bw, W, bw + W.dq, ao + A.avg, B, wgrad_stream(net, st), true));
      RC(run_dgrad(net, top, pk, bw + W.dq, bw + W.g_avg, B, nullptr, nullptr, st));
      RC(vdqn_avgpool_bwd(bw + W.g_avg, ao + A.o[7], bw + W.g_o[7], n, 49, 512, dt, st));
      RC(block_backward_train(net, a, 7, A, W, n, st));
      RC(block_backward_train(net, a, 6, A, W, n, st));
    } else if (stage == 1) {
      RC(block_backward_train(net, a, 5, A, W, n, st));
      RC(block_backward_train(net, a, 4, A, W, n, st));
    } else {
      for (int b = 3; b >= 0; --b) RC(block_backward_train(net, a, b, A, W, n, st));
      RC(vdqn_maxpool_bwd(bw + W.g_pool, ao + A.idx, nullptr, bw + W.g_c1, n, 112, 112, 64, dt, st));
      RC(run_bn_bwd(net, a, net->l_conv1, A, bw + W.g_c1, ao + A.r_c1, bw + W.g_c1, n, st));
      RC(run_wgrad(net, net->layers[net->l_conv1], bw, W, bw + W.g_c1, a->packed_frames ? a->packed_frames : ao + A.t_in, n, wgrad_stream(net, st)));
    }
  } else if (stage == 0) {
    RC(head_backward(net, a, A, W, B, n, st, part_rows));
    RC(block_backward(net, a, 7, A, W, n, st));
    RC(block_backward(net, a, 6, A, W, n, st));
  } else if (stage == 1) {
    RC(block_backward(net, a, 5, A, W, n, st));
    RC(block_backward(net, a, 4, A, W, n, st));
  } else {
    for (int b = 3; b >= 0; --b) RC(block_backward(net, a, b, A, W, n, st));
    // conv1's weight gradient is the last link of the chain (max-pool backward -> wgrad): the other layers of the stage are
    // unfolded ahead of it
    split_conv1 = net->overlap && net->side && net->l_conv1 == net->layer_stage_first[2] && net->layer_stage_count[2] > 1;
  }
  int max_co = 0;
  for (int i = net->layer_stage_first[stage]; i < net->layer_stage_first[stage] + net->layer_stage_count[stage]; ++i)
    max_co = net->layers[i].co > max_co ? net->layers[i].co : max_co;
  PartTable pt;
  memset(&pt, 0, sizeof(pt));
  for (int i = net->layer_stage_first[stage]; i < net->layer_stage_first[stage] + net->layer_stage_count[stage]; ++i) {
    const int buf = part_buf(net, i);
    if (buf < 0) continue;  // 'basic', top.4: tiles 0, db comes from the weight-gradient kernel's column sums
    const PartInfo pi = part_info(net, buf, B, part_rows[i]);
    VDQN_CHECK(pi.entries <= pi.capacity, "vdqn_net_backward_stage: layer %s has %d column-sum entries, its buffer holds %lld",
               net->layers[i].name.c_str(), pi.entries, (long long)pi.capacity);
    pt.off[i] = W.part[buf]; pt.tiles[i] = pi.entries; pt.ld[i] = pi.ld; pt.groups[i] = pi.groups; pt.gstride[i] = pi.gstride;
  }
  const bool stem_tail = stage == 2 && !net->basic();
  auto conv1_chain = [&]() -> int {  // conv1's weight gradient from the pooled gradient g_pool
    // g_pool is already masked by (pool > 0) in block 0's dgrad epilogue and c1[argmax] == pool, so the ReLU mask of c1 is implied.
    // bn1's shift gradient = column sums of g_c1 = column sums of g_pool (max-pool routes every pooled gradient element
    // to exactly one input position), which block 0's dgrad epilogue already produced as partials.
    const Layer& L1 = net->layers[net->l_conv1];
    // bf16: ONE kernel on the side stream builds the max-pool backward tiles in LDS (VDQN_FUSE_POOL_BWD=0: the two launches below)
    static const bool fuse_pool = [] { const char* e = getenv("VDQN_FUSE_POOL_BWD"); return !(e && e[0] == '0'); }();
    const int64_t det_need = net->cfg.deterministic ? vdqn_stem_wgrad_pool_workspace_bytes(n) : 0;
    if (fuse_pool && dt == VDQN_BF16 && (int64_t)n * 115 * 115 * 32 < (1ll << 31) && det_need <= W.det_ws_bytes) {
      prof_layer(L1, n);
      // Which stream: the side stream still holds block 0's last two weight gradients when the data-gradient chain ends, so in
      // the default mode this kernel runs on the CALLER's stream beside them (the update's tail on two streams instead of one;
      // its unfold below waits for it).  Deterministic mode keeps it on the side stream: the partial copies share one workspace.
      static const bool on_main_env = [] { const char* e = getenv("VDQN_STEM_WGRAD_MAIN"); return !(e && e[0] == '0'); }();
      const bool on_main = g_stem_wgrad_main_override >= 0 ? g_stem_wgrad_main_override != 0 : on_main_env;
      const bool main_st = on_main && split_conv1 && !net->cfg.deterministic;
      return vdqn_stem_wgrad_pool(bw + W.g_pool, ao + A.idx, a->packed_frames ? a->packed_frames : ao + A.t_in, reinterpret_cast<float*>(bw + L1.dw_off), n,
                                  net->cfg.deterministic ? bw + W.det_ws : nullptr, W.det_ws_bytes, main_st ? st : fork(net, st));
    }
    // max-pool backward on the caller's stream, the weight gradient behind it on the side stream
    RC(vdqn_maxpool_bwd(bw + W.g_pool, ao + A.idx, nullptr, bw + W.g_c1, n, 112, 112, 64, dt, st));
    RC(run_wgrad(net, L1, bw, W, bw + W.g_c1, a->packed_frames ? a->packed_frames : ao + A.t_in, n, wgrad_stream(net, st)));
    return VDQN_OK;
  };
  if (stem_tail && !split_conv1) RC(conv1_chain());
  // The unfold runs BEHIND the stage's weight gradients on the side stream (which first waits for the caller's stream: the
  // column-sum partials come from the data-gradient epilogues there), so the caller's stream goes straight on to the next stage's
  // data gradients; only stage 2 joins the side stream back (before Adam).  vdqn_net_grad_stream() is where a stage's range of
  // `grads` is complete.
  hipStream_t us = fork(net, st);  // == st when the overlap is off
  if (wgrad_two_streams(net)) join(net, net->side2, net->side);  // the unfold also needs the weight gradients queued on the second side stream
  const double unfold_bytes = (double)(net->stage_end[stage] - net->stage_begin[stage]) * 12.0;
  const int first = net->layer_stage_first[stage], count = net->layer_stage_count[stage];
  if (split_conv1) {
    launch_unfold(net, pt, first + 1, count - 1, max_co, 0, a, us, unfold_bytes);
    RC(conv1_chain());
    if (wgrad_two_streams(net)) join(net, net->side2, net->side);
    (void)fork(net, st);  // conv1's weight gradient may have run on the caller's stream
    launch_unfold(net, pt, net->l_conv1, 1, net->layers[net->l_conv1].co, 0, a, net->side, 0.0);
  } else {
    launch_unfold(net, pt, first, count, max_co, net->basic() ? 1 : 0, a, us, unfold_bytes);
  }
  if (stage == 2) join(net, net->side, st);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// The stem's link of the data-gradient chain: g_pool -> dL/d(frames).  bf16: from the pooled gradient in one launch.  f32 / bf16x3:
// the plain f32 kernel on g_c1 = vdqn_maxpool_bwd(g_pool), which `pool_bwd` launches first (the training walk's stage 2 already has).
static int stem_data_grad(vdqn_net* net, const vdqn_step_args* a, float* out, int scale_kind, bool pool_bwd, hipStream_t st) {
  const int n = a->batch * net->cfg.num_frames;
  const ActLayout A = act_layout(net, step_layout_samples(net, a));
  const BwdLayout W = bwd_layout(net, a->batch);
  const unsigned char* pk = (const unsigned char*)a->packed_online;
  const unsigned char* ao = (const unsigned char*)a->acts_online;
  unsigned char* bw = (unsigned char*)a->bwd;
  const Layer& L1 = net->layers[net->l_conv1];
  float sc[3];
  vdqn_stem_pixel_scale(sc);
  const float* scale = scale_kind ? sc : nullptr;
  if (net->cfg.dtype == VDQN_BF16) return vdqn_stem_input_grad(bw + W.g_pool, ao + A.idx, pk + L1.wf_off, scale, out, n, VDQN_BF16, nullptr, 0, st);
  if (pool_bwd) RC(vdqn_maxpool_bwd(bw + W.g_pool, ao + A.idx, nullptr, bw + W.g_c1, n, 112, 112, 64, net->cfg.dtype, st));
  return vdqn_stem_dgrad_from_c1(reinterpret_cast<const float*>(bw + W.g_c1), reinterpret_cast<const float*>(pk + L1.wf_off), scale, out, n, st);
}

extern "C" int vdqn_net_input_grad(vdqn_net* net, const vdqn_step_args* a, float* out, int32_t scale_kind, void* stream) {
  VDQN_CHECK(net && a && out, "vdqn_net_input_grad: null arg");
  VDQN_CHECK(!net->basic(), "vdqn_net_input_grad: ARCHITECTURE='basic' has no frame gradient (its backward runs through train-mode BatchNorm inside "
                            "vdqn_net_td_forward's update only); extra_capacity only");
  VDQN_CHECK(a->packed_online && a->acts_online && a->bwd, "vdqn_net_input_grad: null buffer");
  VDQN_CHECK(((uintptr_t)out & 15) == 0, "vdqn_net_input_grad: out must be 16-byte aligned");
  VDQN_CHECK(scale_kind == 0 || scale_kind == 1, "vdqn_net_input_grad: scale_kind %d (0: normalised frame, 1: uint8 pixel value)", scale_kind);
  VDQN_CHECK(a->batch >= 1 && a->batch <= net->cfg.max_batch, "vdqn_net_input_grad: batch %d", a->batch);
  // f32 / bf16x3: stage 2 has left g_c1 = vdqn_maxpool_bwd(g_pool) for conv1's weight gradient
  return stem_data_grad(net, a, out, scale_kind, false, (hipStream_t)stream);
}

// The data gradients of one forward call and nothing else: the walk of vdqn_net_backward_stage(0..2) with want_wgrad false, every
// data gradient with the partial buffer the training walk hands it (vdqn_conv2d's choice of kernel and epilogue depends on it), then
// the stem's link.  One stream, no fork, no join, no clear: nothing here accumulates.
extern "C" int vdqn_net_backward_data(vdqn_net* net, const vdqn_step_args* a, const float* dq_f32, float* out, int32_t scale_kind, void* stream) {
  VDQN_CHECK(net && a && dq_f32 && out, "vdqn_net_backward_data: null arg");
  VDQN_CHECK(!net->basic(), "vdqn_net_backward_data: ARCHITECTURE='basic' has no frame gradient (its backward runs through train-mode BatchNorm inside "
                            "vdqn_net_td_forward's update only); extra_capacity only");
  VDQN_CHECK(a->packed_online && a->acts_online && a->bwd, "vdqn_net_backward_data: null buffer");
  VDQN_CHECK(a->batch >= 1 && a->batch <= net->cfg.max_batch && a->acts_samples == a->batch,
             "vdqn_net_backward_data: acts_samples (%d) must equal batch (%d) <= max_batch", a->acts_samples, a->batch);
  VDQN_CHECK(((uintptr_t)out & 15) == 0, "vdqn_net_backward_data: out must be 16-byte aligned");
  VDQN_CHECK(scale_kind == 0 || scale_kind == 1, "vdqn_net_backward_data: scale_kind %d (0: normalised frame, 1: uint8 pixel value)", scale_kind);
  hipStream_t st = (hipStream_t)stream;
  const int B = a->batch, n = B * net->cfg.num_frames;
  const ActLayout A = act_layout(net, B);
  const BwdLayout W = bwd_layout(net, B);
  int part_rows[kMaxLayers];  // (what the unfold would read: nobody does here)
  launch_dq_pad(net, dq_f32, (unsigned char*)a->bwd + W.dq, B, st);
  VDQN_LAUNCH_CHECK();
  RC(head_backward(net, a, A, W, B, n, st, part_rows, false));
  for (int b = 7; b >= 0; --b) RC(block_backward(net, a, b, A, W, n, st, false));
  return stem_data_grad(net, a, out, scale_kind, true, st);
}

extern "C" int vdqn_net_forward_attrib(vdqn_net* net, const void* packed, const void* src, int32_t src_kind, const void* baseline, const float* base_const,
                                       int32_t n_base, int32_t n_copies, int32_t mode, const float* coef, const float* sigma, uint64_t seed, int32_t s0,
                                       int32_t i0, int32_t n_samples, void* acts, float* q_out, void* stream) {
  VDQN_CHECK(net && packed && acts && q_out, "vdqn_net_forward_attrib: null arg");
  VDQN_CHECK(!net->basic(), "vdqn_net_forward_attrib: ARCHITECTURE='basic' has no frame gradient to attribute with; extra_capacity only");
  VDQN_CHECK(n_samples >= 1 && n_samples <= net->cfg.max_batch, "vdqn_net_forward_attrib: n_samples %d exceeds max_batch %d", n_samples, net->cfg.max_batch);
  const int F = net->cfg.num_frames;
  VDQN_CHECK(n_base >= 1 && n_copies >= 1 && (int64_t)n_copies * n_base == (int64_t)n_samples * F,
             "vdqn_net_forward_attrib: %d copies of %d images are not %d samples of %d frames", n_copies, n_base, n_samples, F);
  VDQN_CHECK(n_base % F == 0, "vdqn_net_forward_attrib: n_base %d is not a whole number of %d-frame samples", n_base, F);
  hipStream_t st = (hipStream_t)stream;
  const ActLayout A = act_layout(net, n_samples);
  unsigned char* ab = (unsigned char*)acts;
  RC(vdqn_attrib_pack(src, src_kind, baseline, base_const, n_base, n_copies, mode, coef, sigma, seed, s0, i0, ab + A.t_in, net->cfg.dtype, st));
  RC(forward_impl(net, (const unsigned char*)packed, ab + A.t_in, n_samples, ab, A, st));
  const int nq = net->cfg.action_dim * net->cfg.num_classes;
  hipError_t e = hipMemcpy2DAsync(q_out, (size_t)nq * 4, ab + A.qf, 64 * 4, (size_t)nq * 4, (size_t)n_samples, hipMemcpyDeviceToDevice, st);
  VDQN_CHECK(e == hipSuccess, "vdqn_net_forward_attrib: q copy failed: %s", hipGetErrorString(e));
  return VDQN_OK;
}
