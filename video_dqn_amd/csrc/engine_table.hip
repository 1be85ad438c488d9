// The engine's host-side tables: error text and ABI entries, the static layer table of HabitatDQNMultiAction (ResNet-18 trunk +
// extra_capacity head), the activation / backward workspace layouts with their name -> offset tables, and the engine object.
// No kernels and no launches: every function here runs without a GPU.
//
// Follows: archs/HabitatDQNMultiAction.py:9-54 (wiring, set_train: trunk BatchNorm in eval mode),
// torchvision 0.4.2 resnet18 topology (third-party; restated in oracle/ref_cpu.py),
// train_q_network.py:126-181 (process_batch) and :222-227 (zero_grad / backward / step order).
#include "engine_net.h"

// ---------------------------------------------------------------------------------------------------------
// error text (thread local)
// ---------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void vdqn_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* vdqn_last_error(void) { return g_err; }
extern "C" int vdqn_abi_version(void) { return 16; }
extern "C" int32_t vdqn_abi_struct_size(int32_t which) {
  switch (which) {
    case 0: return (int32_t)sizeof(vdqn_conv_args);
    case 1: return (int32_t)sizeof(vdqn_wgrad_args);
    case 2: return (int32_t)sizeof(vdqn_td_args);
    case 3: return (int32_t)sizeof(vdqn_net_config);
    case 4: return (int32_t)sizeof(vdqn_param_info);
    case 5: return (int32_t)sizeof(vdqn_prof_entry);
    case 6: return (int32_t)sizeof(vdqn_step_args);
    default: return -1;
  }
}

// ---------------------------------------------------------------------------------------------------------
// table construction
// ---------------------------------------------------------------------------------------------------------
namespace {

void add_param(vdqn_net* net, const std::string& name, int64_t off, std::vector<int> shape, int kind, int stage) {
  vdqn_param_info pi;
  memset(&pi, 0, sizeof(pi));
  snprintf(pi.name, sizeof(pi.name), "%s", name.c_str());
  pi.offset = off;
  pi.ndim = (int)shape.size();
  int64_t n = 1;
  for (size_t i = 0; i < shape.size(); ++i) {
    pi.shape[i] = shape[i];
    n *= shape[i];
  }
  pi.numel = n;
  pi.kind = kind;
  pi.param_id = -1;
  pi.stage = stage;
  net->params.push_back(pi);
}

Layer make_conv(const std::string& name, const std::string& bn, int co, int ci, int k, int stride, int pad, int hi, int stage) {
  Layer L;
  L.name = name;
  L.bn_name = bn;
  L.kind = K_CONV;
  L.co = co; L.ci = ci; L.r = k; L.s = k; L.stride = stride; L.pad = pad;
  L.has_bn = !bn.empty();
  L.has_bias = bn.empty();
  L.k_ci = ci; L.k_r = k; L.k_s = k; L.pix_stride = ci;
  L.co_pad = (co + 63) / 64 * 64;
  L.hi = hi; L.wi = hi;
  L.ho = (hi + 2 * pad - k) / stride + 1;
  L.wo = L.ho;
  L.per_sample = 0;
  L.stage = stage;
  L.has_dgrad = 1;
  return L;
}

Layer make_linear(const std::string& name, int out_f, int in_f, int stage, bool perm) {
  Layer L;
  L.name = name;
  L.bn_name = "";
  L.kind = perm ? K_LINEAR_PERM : K_LINEAR;
  L.co = out_f; L.ci = in_f; L.r = 1; L.s = 1; L.stride = 1; L.pad = 0;
  L.has_bn = 0;
  L.has_bias = 1;
  L.k_ci = in_f; L.k_r = 1; L.k_s = 1; L.pix_stride = in_f;
  L.co_pad = (out_f + 63) / 64 * 64;
  L.hi = L.wi = L.ho = L.wo = 1;
  L.per_sample = 1;
  L.stage = stage;
  L.has_dgrad = 1;
  return L;
}

void build_layers(vdqn_net* net) {
  const int F = net->cfg.num_frames;
  std::vector<Layer> fwd;  // forward order
  // the extra head (rows indexed by Head): more rows of the Q layer, registered below as <head>.weight / <head>.bias.  The value
  // head: num_classes rows; the spread head: one row per Q column; the policy head: one behaviour logit per action.
  const struct {
    int rows;
    const char* name;
  } heads[] = {{0, ""}, {net->cfg.num_classes, "value"}, {net->n_q(), "spread"}, {net->cfg.action_dim, "policy"}};
  const int n_head = heads[net->head].rows;
  const std::string head = heads[net->head].name;
  {
    Layer L = make_conv("resnet.conv1", "resnet.bn1", 64, 3, 7, 2, 3, 224, 2);
    L.kind = K_CONV1_S2D;
    L.k_ci = 64; L.k_r = 4; L.k_s = 1; L.pix_stride = 16;
    L.hi = L.wi = 115;  // packed space-to-depth operand
    L.ho = L.wo = 112;
    L.has_dgrad = 0;
    fwd.push_back(L);
  }
  int inpl = 64, sp = 56;
  for (int li = 1; li <= 4; ++li) {
    const int planes = 64 << (li - 1);
    const int stage = li == 4 ? 0 : (li == 3 ? 1 : 2);
    for (int bi = 0; bi < 2; ++bi) {
      const int stride = (li > 1 && bi == 0) ? 2 : 1;
      char pfx[64];
      snprintf(pfx, sizeof(pfx), "resnet.layer%d.%d", li, bi);
      const std::string p(pfx);
      fwd.push_back(make_conv(p + ".conv1", p + ".bn1", planes, inpl, 3, stride, 1, sp, stage));
      const int sp_out = sp / stride;
      fwd.push_back(make_conv(p + ".conv2", p + ".bn2", planes, planes, 3, 1, 1, sp_out, stage));
      if (stride != 1 || inpl != planes) fwd.push_back(make_conv(p + ".downsample.0", p + ".downsample.1", planes, inpl, 1, stride, 0, sp, stage));
      inpl = planes;
      sp = sp_out;
    }
  }
  if (!net->basic()) {  // archs/HabitatDQNMultiAction.py:27-31
    fwd.push_back(make_conv("features.8", "", 64, 512, 3, 1, 0, 7, 0));
    fwd.push_back(make_linear("top.0", 512, 1600 * F, 0, true));
    fwd.push_back(make_linear("top.2", 256, 512, 0, false));
    fwd.push_back(make_linear("top.4", net->n_q() + n_head, 256, 0, false));
  } else {  // :32-34: global average pool, then one Linear over the F concatenated 512-vectors
    fwd.push_back(make_linear("top", net->n_q() + n_head, 512 * F, 0, false));
  }

  // store layers ordered by backward stage (stable), so each stage's gradients are one contiguous range
  net->layers.clear();
  for (int st = 0; st < 3; ++st) {
    net->layer_stage_first[st] = (int)net->layers.size();
    for (auto& L : fwd)
      if (L.stage == st) net->layers.push_back(L);
    net->layer_stage_count[st] = (int)net->layers.size() - net->layer_stage_first[st];
  }

  auto find = [&](const std::string& n) {
    for (size_t i = 0; i < net->layers.size(); ++i)
      if (net->layers[i].name == n) return (int)i;
    return -1;
  };
  net->l_conv1 = find("resnet.conv1");
  net->l_f8 = find("features.8");
  net->l_top0 = find("top.0");
  net->l_top2 = find("top.2");
  net->l_top4 = net->basic() ? find("top") : find("top.4");
  for (int b = 0; b < 8; ++b) {
    char pfx[64];
    snprintf(pfx, sizeof(pfx), "resnet.layer%d.%d", b / 2 + 1, b % 2);
    net->l_b_conv1[b] = find(std::string(pfx) + ".conv1");
    net->l_b_conv2[b] = find(std::string(pfx) + ".conv2");
    net->l_b_ds[b] = find(std::string(pfx) + ".downsample.0");
  }

  // flat offsets: trainable parameters grouped by stage, then the frozen resnet.fc
  int64_t poff = 0, soff = 0, pk = 0, dwoff = 0;
  const int esz = net->esz;
  for (int st = 0; st < 3; ++st) {
    net->stage_begin[st] = poff;
    for (int i = net->layer_stage_first[st]; i < net->layer_stage_first[st] + net->layer_stage_count[st]; ++i) {
      Layer& L = net->layers[i];
      L.w_off = poff;
      const bool q_layer = n_head > 0 && (L.name == "top.4" || L.name == "top");  // its last n_head rows are the extra head's
      if (q_layer) {  // <top>.weight {C*A, in} with <head>.weight {n_head, in} directly behind it: one contiguous [co, in] operand
        add_param(net, L.name + ".weight", poff, {L.co - n_head, L.ci}, 0, st);
        add_param(net, head + ".weight", poff + (int64_t)(L.co - n_head) * L.ci, {n_head, L.ci}, 0, st);
      } else if (L.kind == K_LINEAR || L.kind == K_LINEAR_PERM) add_param(net, L.name + ".weight", poff, {L.co, L.ci}, 0, st);
      else add_param(net, L.name + ".weight", poff, {L.co, L.ci, L.r, L.s}, 0, st);
      poff += (int64_t)L.co * L.ci * L.r * L.s;
      poff = (poff + 3) / 4 * 4;  // keep every tensor 16-byte aligned
      L.g_off = L.b_off = L.mean_off = L.var_off = -1;
      if (L.has_bn) {
        L.g_off = poff;
        add_param(net, L.bn_name + ".weight", poff, {L.co}, 0, st);
        poff += L.co;
        L.b_off = poff;
        add_param(net, L.bn_name + ".bias", poff, {L.co}, 0, st);
        poff += L.co;
        L.mean_off = soff;
        add_param(net, L.bn_name + ".running_mean", soff, {L.co}, 2, st);
        soff += L.co;
        L.var_off = soff;
        add_param(net, L.bn_name + ".running_var", soff, {L.co}, 3, st);
        soff += L.co;
      } else if (L.has_bias) {
        L.b_off = poff;
        add_param(net, L.name + ".bias", poff, {q_layer ? L.co - n_head : L.co}, 0, st);
        if (q_layer) add_param(net, head + ".bias", poff + L.co - n_head, {n_head}, 0, st);
        poff += L.co;
        poff = (poff + 3) / 4 * 4;
      }
      // packed weights
      L.wf_off = pk;
      pk = align_up(pk + (int64_t)L.co_pad * L.kf() * esz);
      if (L.has_dgrad) {
        L.wd_off = pk;
        pk = align_up(pk + (int64_t)L.k_ci * L.kd() * esz);
      } else {
        L.wd_off = -1;
      }
      L.bias_off = pk;
      pk = align_up(pk + (int64_t)L.co_pad * 4);
      L.scale_off = pk;
      pk = align_up(pk + (int64_t)L.co_pad * 4);
      // f32 gradient accumulators
      L.dw_off = dwoff;
      dwoff = align_up(dwoff + (int64_t)L.co_pad * L.kf() * 4);
      L.db_off = dwoff;
      dwoff = align_up(dwoff + (int64_t)L.co_pad * 4);
    }
    net->stage_end[st] = poff;
  }
  net->trainable_numel = poff;
  add_param(net, "resnet.fc.weight", poff, {1000, 512}, 1, -1);
  poff += 1000 * 512;
  add_param(net, "resnet.fc.bias", poff, {1000}, 1, -1);
  poff += 1000;
  net->params_numel = poff;
  net->bnstats_numel = soff;
  net->packed_bytes = pk;
  net->dw_bytes = dwoff;

  // reference model.parameters() order -> param_id (Adam state_dict ids)
  {
    std::vector<std::string> order;
    for (auto& L : fwd) {
      if (L.name.rfind("resnet.", 0) != 0) continue;
      order.push_back(L.name + ".weight");
      order.push_back(L.bn_name + ".weight");
      order.push_back(L.bn_name + ".bias");
    }
    order.push_back("resnet.fc.weight");
    order.push_back("resnet.fc.bias");
    if (!net->basic()) {
      for (const char* n : {"features.8", "top.0", "top.2", "top.4"}) {
        order.push_back(std::string(n) + ".weight");
        order.push_back(std::string(n) + ".bias");
      }
    } else {
      order.push_back("top.weight");
      order.push_back("top.bias");
    }
    if (n_head > 0) {  // behind the reference's ids: the reference's Adam state keeps its numbering
      order.push_back(head + ".weight");
      order.push_back(head + ".bias");
    }
    for (auto& pi : net->params)
      for (size_t i = 0; i < order.size(); ++i)
        if (order[i] == pi.name) pi.param_id = (int)i;
  }

  // device-side descriptors
  net->fold.n = (int)net->layers.size();
  for (size_t i = 0; i < net->layers.size(); ++i) {
    const Layer& L = net->layers[i];
    FoldDesc& d = net->fold.d[i];
    d.w_off = L.w_off; d.g_off = L.g_off; d.b_off = L.b_off; d.mean_off = L.mean_off; d.var_off = L.var_off;
    d.wf_off = L.wf_off; d.wd_off = L.wd_off; d.bias_off = L.bias_off; d.scale_off = L.scale_off;
    d.dw_off = L.dw_off; d.db_off = L.db_off;
    d.co = L.co; d.ci = L.ci; d.r = L.r; d.s = L.s; d.kind = L.kind; d.co_pad = L.co_pad; d.kf = L.kf();
    d.k_ci = L.k_ci; d.k_s = L.k_s; d.cd_rows = L.k_ci; d.kd = L.kd(); d.has_bn = L.has_bn; d.has_bias = L.has_bias;
    d.tiled = (L.kind == K_CONV && L.ci % 64 == 0 && (L.r * L.s == 9 || L.r * L.s == 1)) ? 1 : 0;
    d.tile_begin = 0;
  }
  net->fold.n_tiles = 0;
  for (int i = 0; i < net->fold.n; ++i) {
    FoldDesc& d = net->fold.d[i];
    if (!d.tiled) continue;
    d.tile_begin = net->fold.n_tiles;
    net->fold.n_tiles += (d.co_pad / 64) * (d.ci / 64);
  }
}

}  // namespace

ActLayout act_layout(const vdqn_net* net, int n_samples) {
  const int64_t F = net->cfg.num_frames, n = (int64_t)n_samples * F, e = net->esz;
  ActLayout L;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    const int64_t o = off;
    off = align_up(off + bytes);
    return o;
  };
  L.t_in = take(n * frame_bytes(net));
  L.c1 = net->basic() ? take(n * 112 * 112 * 64 * e) : -1;  // extra_capacity: conv1 + max-pool are one kernel, c1 never exists
  L.pool = take(n * 56 * 56 * 64 * e);
  L.idx = take(n * 56 * 56 * 64);
  for (int b = 0; b < 8; ++b) {
    const int li = b / 2;
    const int64_t planes = block_planes(b), sp = block_side(b);
    const int64_t sz = n * sp * sp * planes * e;
    L.h[b] = take(sz);
    L.o[b] = take(sz);
    L.ds[b] = (b % 2 == 0 && li > 0) ? take(sz) : -1;
  }
  L.f8 = take(n * 25 * 64 * e);
  L.l0 = take((int64_t)n_samples * 512 * e);
  L.l1 = take((int64_t)n_samples * 256 * e);
  L.q = take((int64_t)n_samples * 64 * e);
  L.qf = take((int64_t)n_samples * 64 * 4);
  L.avg = L.r_c1 = L.bnw_begin = L.bn_sync = -1;
  L.bnw_bytes = 0;
  for (int b = 0; b < 8; ++b) L.r_h[b] = L.r_o[b] = L.r_ds[b] = -1;
  for (int i = 0; i < kMaxLayers; ++i) L.bnw[i] = -1;
  if (net->basic()) {
    L.avg = take(n * 512 * e);
    L.r_c1 = take(n * 112 * 112 * 64 * e);
    for (int b = 0; b < 8; ++b) {
      const int li = b / 2;
      const int64_t planes = block_planes(b), sp = block_side(b);
      const int64_t sz = n * sp * sp * planes * e;
      L.r_h[b] = take(sz);
      L.r_o[b] = take(sz);
      L.r_ds[b] = (b % 2 == 0 && li > 0) ? take(sz) : -1;
    }
    L.bnw_begin = off;
    for (size_t i = 0; i < net->layers.size(); ++i)
      if (net->layers[i].has_bn) L.bnw[i] = take((int64_t)2 * F * 6 * net->layers[i].co * 4);
    L.bnw_bytes = off - L.bnw_begin;
    L.bn_sync = take((int64_t)2 * F * 2 * 512 * 4);  // packed sums of one layer (SyncBN scratch)
    if (net->cfg.deterministic) {  // ordered two-stage statistic sums: the largest per-block partial array of any layer and call shape
      for (const Layer& ly : net->layers) {
        if (!ly.has_bn) continue;
        for (int halves = 1; halves <= 2; ++halves) {
          if (n % halves || (n / halves) % F) continue;
          L.bn_det_bytes = std::max(L.bn_det_bytes, vdqn_bn_train_workspace_bytes((int32_t)n, ly.ho * ly.wo, ly.co, (int32_t)F, (int32_t)(n / halves)));
        }
      }
      L.bn_det = take(L.bn_det_bytes);
    }
  }
  L.total = off;
  return L;
}

// the geometry part of a layer's weight-gradient call (no pointers): what vdqn_conv2d_wgrad_workspace_bytes needs
vdqn_wgrad_args wgrad_shape_args(const vdqn_net* net, const Layer& L, int n_units) {
  vdqn_wgrad_args a;
  memset(&a, 0, sizeof(a));
  a.n_img = n_units; a.hi = L.hi; a.wi = L.wi; a.ci = L.k_ci; a.pix_stride = L.pix_stride;
  a.ho = L.ho; a.wo = L.wo; a.co = L.co_pad; a.ldg = L.co_pad;
  a.r = L.k_r; a.s = L.k_s;
  a.stride = L.kind == K_CONV1_S2D ? 1 : L.stride;
  a.pad = L.kind == K_CONV1_S2D ? 0 : L.pad;
  a.splitk = 0; a.dtype = net->gemm_dtype;
  return a;
}
// images one vdqn_conv2d_wgrad call can take for layer L (< 2^24 output pixels, < 2 GiB per operand: 32-bit buffer offsets)
int64_t wgrad_max_imgs(const vdqn_net* net, const Layer& L) {
  const int64_t esz = net->esz;
  const int64_t pix = (int64_t)L.ho * L.wo, gy_img = pix * L.co_pad * esz, x_img = (int64_t)L.hi * L.wi * L.pix_stride * esz;
  int64_t m = ((1ll << 24) - 1) / pix;
  m = std::min(m, (int64_t)0x7ffffffell / gy_img);
  m = std::min(m, (int64_t)0x7ffffffell / x_img);
  return m;
}

// ---------------------------------------------------------------------------------------------------------
// the bias-gradient partials
// ---------------------------------------------------------------------------------------------------------
// dL/dbias (dL/dbeta) of a layer is the column sum of the gradient of its output.  The data-gradient call that stores that
// gradient also writes its column sums per row tile (vdqn_conv_args.colsum_part), and the unfold kernel adds the entries up.
// This is the one place that says where a layer's entries are and how many: the producers' launches, bwd_layout's sizes and
// backward_stage's PartTable all take it from here.

// which partial buffer holds the column sums that are layer li's bias gradient (-1: none, the weight-gradient kernel sums them)
int part_buf(const vdqn_net* net, int li) {
  if (li < 0 || net->basic()) return -1;
  if (li == net->l_top2) return kPartL1;
  if (li == net->l_top0) return kPartL0;
  if (li == net->l_f8) return kPartF8;
  if (li == net->l_conv1) return kPartPool;  // max-pool routes every element of g_pool to one element of g_c1: the same sums
  for (int b = 0; b < 8; ++b) {
    if (li == net->l_b_conv2[b] || li == net->l_b_ds[b]) return part_o(b);
    if (li == net->l_b_conv1[b]) return part_h(b);
  }
  return -1;
}

// Partial buffer `buf` at batch n_samples when its producer wrote one entry per rows_per_entry rows (vdqn_conv2d_colsum_rows of
// that call).  `capacity` does not depend on rows_per_entry: it is what bwd_layout reserves, capacity * ld floats.
PartInfo part_info(const vdqn_net* net, int buf, int n_samples, int rows_per_entry) {
  const int64_t F = net->cfg.num_frames, n = (int64_t)n_samples * F;
  auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  PartInfo p;
  p.groups = 1;
  p.gstride = 0;
  if (buf < kPartPool) {  // the head: a row per sample
    p.ld = buf == kPartL1 ? 256 : (buf == kPartL0 ? 512 : (int)(1600 * F));
    if (buf == kPartF8) {  // g_f8 is [n_samples][25 * F pixels][64]: features.8's 64 columns recur 25 * F times in a row of top.0's input
      p.groups = (int)(25 * F);
      p.gstride = 64;
    }
    p.entries = (int)ceil_div(n_samples, rows_per_entry);
    p.capacity = ceil_div(n_samples, vdqn_skinny_part_rows(0));  // the smallest row tile of any kernel that takes these calls (skinny.hip)
    return p;
  }
  const bool pool = buf == kPartPool;  // the gradient of block 0's input
  const int b = pool ? 0 : (buf - kPartBlocks) / 2;
  const bool of_o = !pool && buf == part_o(b);
  const int64_t rows = pool ? n * 56 * 56 : n * block_side(b) * block_side(b);
  p.ld = pool ? 64 : block_planes(b);
  // g_o[b] below a stride-2 block comes from a stride-2 data gradient, laid out parity class by parity class: each class rounds up on its own
  const bool parity = of_o && b + 1 < 8 && net->l_b_ds[b + 1] >= 0;
  p.entries = parity ? (int)(4 * ceil_div(rows / 4, rows_per_entry)) : (int)ceil_div(rows, rows_per_entry);
  p.capacity = ceil_div(rows, kTileRows) + (of_o ? 4 : 0);  // + 4: the round-ups of the four parity classes (every g_o: one rule)
  return p;
}

BwdLayout bwd_layout(const vdqn_net* net, int n_samples) {
  const int64_t F = net->cfg.num_frames, n = (int64_t)n_samples * F, e = net->esz;
  BwdLayout L;
  int64_t off = 0;
  auto take = [&](int64_t bytes) {
    const int64_t o = off;
    off = align_up(off + bytes);
    return o;
  };
  L.zero_begin = 0;
  take(net->dw_bytes);
  L.zero_bytes = off;
  L.dq = take((int64_t)n_samples * 64 * e);
  L.g_l1 = take((int64_t)n_samples * 256 * e);
  L.g_l0 = take((int64_t)n_samples * 512 * e);
  L.g_f8 = take(n * 25 * 64 * e);
  for (int b = 0; b < 8; ++b) {
    const int li = b / 2;
    const int64_t planes = block_planes(b), sp = block_side(b);
    const int64_t sz = n * sp * sp * planes * e;
    L.g_o[b] = take(sz);
    L.g_h[b] = take(sz);
    // gradient of the downsample branch w.r.t. the block input (input geometry of the block)
    L.dsg[b] = (b % 2 == 0 && li > 0) ? take(n * (sp * 2) * (sp * 2) * (planes / 2) * e) : -1;
  }
  L.g_pool = take(n * 56 * 56 * 64 * e);
  L.g_c1 = take(n * 112 * 112 * 64 * e);
  for (int p = 0; p < kPartBufs; ++p) {
    const PartInfo pi = part_info(net, p, n_samples, kTileRows);
    L.part[p] = take(pi.capacity * pi.ld * 4);
  }
  L.det_ws = -1;
  L.det_ws_bytes = 0;
  if (net->cfg.deterministic || wgrad_two_stage()) {
    for (const Layer& ly : net->layers) {
      const int64_t units = ly.per_sample ? n_samples : n;
      const int64_t mx = wgrad_max_imgs(net, ly);
      if (mx < 1) continue;  // run_wgrad reports it
      const vdqn_wgrad_args wa = wgrad_shape_args(net, ly, (int)std::min(units, mx));
      L.det_ws_bytes = std::max(L.det_ws_bytes, vdqn_conv2d_wgrad_workspace_bytes(&wa));
    }
    L.det_ws = take(L.det_ws_bytes);
  }
  L.g_avg = -1;
  for (int b = 0; b < 8; ++b) L.g_or[b] = L.g_dsr[b] = -1;
  if (net->basic()) {
    L.g_avg = take(n * 512 * e);
    for (int b = 0; b < 8; ++b) {
      const int64_t planes = block_planes(b), sp = block_side(b);
      L.g_or[b] = take(n * sp * sp * planes * e);
      if (b % 2 == 0 && b > 0) L.g_dsr[b] = take(n * sp * sp * planes * e);
    }
  }
  L.total = off;
  return L;
}

// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
static int net_create(const vdqn_net_config* cfg, Head head, vdqn_net** out);
extern "C" int vdqn_net_create(const vdqn_net_config* cfg, vdqn_net** out) { return net_create(cfg, HEAD_NONE, out); }
// vdqn_net_create with num_classes state values V(c) behind the Q columns of the Q layer (implicit Q-learning, csrc/iql.hip)
extern "C" int vdqn_net_create_v(const vdqn_net_config* cfg, int32_t value_head, vdqn_net** out) {
  VDQN_CHECK(value_head == 0 || value_head == 1, "vdqn_net_create_v: value_head must be 0 or 1, not %d", value_head);
  if (value_head) {
    VDQN_CHECK(cfg && out, "vdqn_net_create_v: null arg");
    VDQN_CHECK(cfg->action_dim >= 2, "vdqn_net_create_v: action_dim is %d: with one action Q(s, a) is the state value already (value_head needs action_dim >= 2)", cfg->action_dim);
    VDQN_CHECK(cfg->num_classes >= 1 && (int64_t)cfg->action_dim * cfg->num_classes + cfg->num_classes <= 64,
               "vdqn_net_create_v: action_dim*num_classes + num_classes must be in 1..64 (the Q columns and one V per category share a 64-wide row)");
  }
  return net_create(cfg, value_head ? HEAD_VALUE : HEAD_NONE, out);
}
extern "C" int vdqn_net_value_head(const vdqn_net* net) { return net && net->head == HEAD_VALUE; }
// vdqn_net_create_v with one spread per Q column behind the Q columns (Gaussian distributional Q-learning, csrc/dist.hip)
extern "C" int vdqn_net_create_d(const vdqn_net_config* cfg, int32_t value_head, int32_t spread_head, vdqn_net** out) {
  VDQN_CHECK(spread_head == 0 || spread_head == 1, "vdqn_net_create_d: spread_head must be 0 or 1, not %d", spread_head);
  if (!spread_head) return vdqn_net_create_v(cfg, value_head, out);
  VDQN_CHECK(value_head == 0 || value_head == 1, "vdqn_net_create_d: value_head must be 0 or 1, not %d", value_head);
  VDQN_CHECK(!value_head, "vdqn_net_create_d: value_head and spread_head together are out of scope (one extra head behind the Q layer)");
  VDQN_CHECK(cfg && out, "vdqn_net_create_d: null arg");
  VDQN_CHECK(cfg->action_dim >= 1 && cfg->num_classes >= 1 && 2 * (int64_t)cfg->action_dim * cfg->num_classes <= 64,
             "vdqn_net_create_d: 2 * action_dim*num_classes must be in 2..64 (the means and one spread per mean share a 64-wide row)");
  return net_create(cfg, HEAD_SPREAD, out);
}
extern "C" int vdqn_net_spread_head(const vdqn_net* net) { return net && net->head == HEAD_SPREAD; }
// vdqn_net_create_d with one behaviour logit per action behind the Q columns (discrete batch-constrained Q-learning, csrc/bcq.hip)
extern "C" int vdqn_net_create_p(const vdqn_net_config* cfg, int32_t value_head, int32_t spread_head, int32_t policy_head, vdqn_net** out) {
  VDQN_CHECK(policy_head == 0 || policy_head == 1, "vdqn_net_create_p: policy_head must be 0 or 1, not %d", policy_head);
  if (!policy_head) return vdqn_net_create_d(cfg, value_head, spread_head, out);
  VDQN_CHECK((value_head == 0 || value_head == 1) && (spread_head == 0 || spread_head == 1),
             "vdqn_net_create_p: value_head and spread_head must be 0 or 1, not %d and %d", value_head, spread_head);
  VDQN_CHECK(!value_head && !spread_head, "vdqn_net_create_p: policy_head together with value_head or spread_head is out of scope (one extra head behind the Q layer)");
  VDQN_CHECK(cfg && out, "vdqn_net_create_p: null arg");
  VDQN_CHECK(cfg->action_dim >= 2, "vdqn_net_create_p: action_dim is %d: with one action there is nothing to constrain (policy_head needs action_dim >= 2)", cfg->action_dim);
  VDQN_CHECK(cfg->num_classes >= 1 && (int64_t)cfg->action_dim * cfg->num_classes + cfg->action_dim <= 64,
             "vdqn_net_create_p: action_dim*num_classes + action_dim must be in 1..64 (the Q columns and one behaviour logit per action share a 64-wide row)");
  return net_create(cfg, HEAD_POLICY, out);
}
extern "C" int vdqn_net_policy_head(const vdqn_net* net) { return net && net->head == HEAD_POLICY; }

static int net_create(const vdqn_net_config* cfg, Head head, vdqn_net** out) {
  VDQN_CHECK(cfg && out, "vdqn_net_create: null arg");
  VDQN_CHECK(cfg->extra_capacity == 0 || cfg->extra_capacity == 1, "vdqn_net_create: extra_capacity must be 0 or 1");
  VDQN_CHECK(cfg->dtype == VDQN_F32 || cfg->dtype == VDQN_BF16 || cfg->dtype == VDQN_F32X3, "vdqn_net_create: bad dtype %d", cfg->dtype);
  VDQN_CHECK(cfg->action_dim >= 1 && cfg->num_classes >= 1 && cfg->action_dim * cfg->num_classes <= 64, "vdqn_net_create: action_dim*num_classes must be in 1..64");
  VDQN_CHECK(cfg->num_frames >= 1 && cfg->num_frames <= 64, "vdqn_net_create: num_frames out of range");
  VDQN_CHECK(cfg->max_batch >= 1, "vdqn_net_create: max_batch");
  VDQN_CHECK(cfg->deterministic == 0 || cfg->deterministic == 1, "vdqn_net_create: deterministic must be 0 or 1");
  vdqn_net* net = new vdqn_net();
  net->cfg = *cfg;
  net->head = head;
  net->gemm_dtype = cfg->dtype;
  if (cfg->dtype == VDQN_F32X3) net->cfg.dtype = VDQN_F32;  // f32 layout, tensors and pointwise kernels; only the GEMMs differ
  net->esz = cfg->dtype == VDQN_BF16 ? 2 : 4;
  {
    const char* no = getenv("VDQN_NO_OVERLAP");
    net->overlap = (no && no[0] == '1') ? 0 : 1;
  }
  build_layers(net);
  if ((int)net->layers.size() > kMaxLayers) {
    delete net;
    vdqn_set_error("vdqn_net_create: layer table overflow");
    return VDQN_ERR_INVALID;
  }
  *out = net;
  return VDQN_OK;
}

extern "C" int vdqn_net_set_overlap(vdqn_net* net, int on) {
  VDQN_CHECK(net, "vdqn_net_set_overlap: null net");
  if (net->side) (void)hipStreamSynchronize(net->side);
  if (net->side2) (void)hipStreamSynchronize(net->side2);
  net->overlap = on ? 1 : 0;
  return VDQN_OK;
}

extern "C" int vdqn_net_set_bn_sync(vdqn_net* net, vdqn_allreduce_fn fn, void* user, int32_t world_size) {
  VDQN_CHECK(net, "vdqn_net_set_bn_sync: null net");
  VDQN_CHECK(net->basic() || fn == nullptr, "vdqn_net_set_bn_sync: only ARCHITECTURE='basic' has train-mode BatchNorm");
  net->bn_sync.fn = (fn && world_size > 1) ? fn : nullptr;
  net->bn_sync.user = user;
  net->bn_sync.world = world_size > 1 ? world_size : 1;
  return VDQN_OK;
}

extern "C" void vdqn_net_destroy(vdqn_net* net) {
  if (!net) return;
  if (net->side) {
    (void)hipStreamSynchronize(net->side);
    for (auto& e : net->events)
      if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(net->side);
    if (net->side2) {
      (void)hipStreamSynchronize(net->side2);
      (void)hipStreamDestroy(net->side2);
    }
  }
  delete net;
}

extern "C" int vdqn_net_num_params(const vdqn_net* net) { return net ? (int)net->params.size() : 0; }
extern "C" int vdqn_net_param_info(const vdqn_net* net, int index, vdqn_param_info* out) {
  VDQN_CHECK(net && out && index >= 0 && index < (int)net->params.size(), "vdqn_net_param_info: bad index");
  *out = net->params[index];
  return VDQN_OK;
}
extern "C" int64_t vdqn_net_params_numel(const vdqn_net* net) { return net->params_numel; }
extern "C" int64_t vdqn_net_trainable_numel(const vdqn_net* net) { return net->trainable_numel; }
extern "C" int64_t vdqn_net_bnstats_numel(const vdqn_net* net) { return net->bnstats_numel; }
extern "C" int vdqn_net_stage_range(const vdqn_net* net, int stage, int64_t* begin, int64_t* end) {
  VDQN_CHECK(net && stage >= 0 && stage < 3 && begin && end, "vdqn_net_stage_range: bad args");
  *begin = net->stage_begin[stage];
  *end = net->stage_end[stage];
  return VDQN_OK;
}
extern "C" int64_t vdqn_net_packed_bytes(const vdqn_net* net) { return net->packed_bytes; }
extern "C" int64_t vdqn_net_packed_offset(const vdqn_net* net, const char* name) {
  if (!net || !name) return -1;
  const char* colon = strchr(name, ':');
  if (!colon) return -1;
  const std::string region(name, colon - name);
  for (auto& L : net->layers) {
    if (L.name != colon + 1) continue;
    if (region == "wf") return L.wf_off;
    if (region == "wd") return L.has_dgrad ? L.wd_off : -2;
    if (region == "bias") return L.bias_off;
    if (region == "scale") return L.scale_off;
    return -1;
  }
  return -1;
}
extern "C" int64_t vdqn_net_acts_bytes(const vdqn_net* net, int32_t n_samples) { return act_layout(net, n_samples).total; }
extern "C" int64_t vdqn_net_bwd_bytes(const vdqn_net* net, int32_t n_samples) { return bwd_layout(net, n_samples).total; }

static int64_t indexed(const char* name, const char* prefix, const int64_t* arr) {
  const size_t n = strlen(prefix);
  if (strncmp(name, prefix, n) != 0 || name[n] < '0' || name[n] > '7' || name[n + 1] != 0) return -2;
  return arr[name[n] - '0'];
}
extern "C" int64_t vdqn_net_act_offset(const vdqn_net* net, int32_t n_samples, const char* name) {
  if (!net || !name) return -1;
  const ActLayout A = act_layout(net, n_samples);
  const struct { const char* n; int64_t v; } tab[] = {{"t_in", A.t_in}, {"c1", A.c1}, {"pool", A.pool}, {"idx", A.idx}, {"f8", A.f8},
                                                     {"l0", A.l0}, {"l1", A.l1}, {"q", A.q}, {"qf", A.qf}};
  for (auto& t : tab)
    if (strcmp(t.n, name) == 0) return t.v;
  int64_t v;
  if ((v = indexed(name, "h", A.h)) != -2) return v;
  if ((v = indexed(name, "o", A.o)) != -2) return v;
  if ((v = indexed(name, "ds", A.ds)) != -2) return v;
  if (strcmp(name, "avg") == 0) return A.avg;
  if (strcmp(name, "r_c1") == 0) return A.r_c1;
  if ((v = indexed(name, "r_h", A.r_h)) != -2) return v;
  if ((v = indexed(name, "r_o", A.r_o)) != -2) return v;
  if ((v = indexed(name, "r_ds", A.r_ds)) != -2) return v;
  return -1;
}
extern "C" int64_t vdqn_net_bwd_offset(const vdqn_net* net, int32_t n_samples, const char* name) {
  if (!net || !name) return -1;
  const BwdLayout W = bwd_layout(net, n_samples);
  const struct { const char* n; int64_t v; } tab[] = {{"dq", W.dq}, {"g_l1", W.g_l1}, {"g_l0", W.g_l0}, {"g_f8", W.g_f8},
                                                     {"g_pool", W.g_pool}, {"g_c1", W.g_c1}};
  for (auto& t : tab)
    if (strcmp(t.n, name) == 0) return t.v;
  int64_t v;
  if ((v = indexed(name, "g_o", W.g_o)) != -2) return v;
  if ((v = indexed(name, "g_h", W.g_h)) != -2) return v;
  if ((v = indexed(name, "dsg", W.dsg)) != -2) return v;
  if (strcmp(name, "g_avg") == 0) return W.g_avg;
  if ((v = indexed(name, "g_or", W.g_or)) != -2) return v;
  if ((v = indexed(name, "g_dsr", W.g_dsr)) != -2) return v;
  if (strncmp(name, "dw:", 3) == 0 || strncmp(name, "db:", 3) == 0)
    for (auto& L : net->layers)
      if (L.name == name + 3) return name[1] == 'w' ? L.dw_off : L.db_off;
  return -1;
}
