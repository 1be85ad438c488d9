// Held-out validation of the Q trainer: forward-only TD metrics summed on the device (the `eval_losses` list the reference
// reserves and never fills, train_q_network.py:183-186, and its `# checkpoint and eval` at :240).  One launch per validation batch
// turns Q(s), the online Q(s') and the target network's Q(s') into eight sums per category and adds them into a small f64 table
// in device memory; the host reads that table once per validation pass.  Nothing of the training state is read or written.
//
// Per sample b and category c, all in f32 (A = n_act, q = q_before[b, c*A .. c*A+A), a* = act[b]):
//   y, d   = the Double-DQN target and the TD error exactly as td_loss_kernel forms them (csrc/pointwise.hip td_error_of: first
//            arg-max of the online Q(s'), the target network's value there, (1 - term), LINEAR / gamma, rect clip; d = q[a*] - y)
//   l(d)   = 0.5 d^2, or Huber with beta 1 (loss_kind 1): |d| < 1 ? 0.5 d^2 : |d| - 0.5
//   m, k*  = max_a q[a] and its first index;  sum = sum_a expf(q[a] - m), a = 0 .. A-1 in that order
//   pen    = logf(sum) + (m - q[a*])          (TD_CQL's penalty: the maximum is subtracted first; exactly 0 when A == 1)
//   vm     = use_valid ? valid[b, c] : 1
// The eight terms, each multiplied by vm LAST, then converted to f64:
//   0: vm    1: l(d) * vm    2: |d| * vm    3: q[a*] * vm    4: m * vm    5: y * vm    6: pen * vm    7: [k* == a*] * vm
// A row whose action is outside [0, A) adds nothing (the loss launch has no term for it either: no column matches).
//
// The sums are f64 in a FIXED order that depends on batch, n_cat and n_act alone, so two runs agree bit for bit:
//   grid = n_cat blocks of 256 threads, block c owns category c and row c of the table.  Thread t starts from eight zeros and adds
//   the terms of samples b = t, t + 256, t + 512, .. < batch in that order.  Lanes are folded by shuffles at distances 32, 16, .. 1
//   (lane l += lane l + d), the four waves left to right: s_k = ((w0 + w1) + w2) + w3.  Thread k < 8 then performs the one f64
//   addition acc[c][k] = acc[c][k] + s_k.  No atomics: no other block touches row c.
//
// The head table (below the first launch): under a head algorithm (IQL, distributional, BCQ) a second launch per batch adds eight
// sums per category, and one row of per-sample sums, into a second f64 table [n_cat + 1][8].  Its slots are listed above its kernels.
#include <math.h>

#include "bcq_math.h"
#include "common.h"
#include "dist_math.h"
#include "iql_math.h"

namespace {

constexpr int kEvalSlots = 8;

__global__ __launch_bounds__(256) void td_eval_kernel(const vdqn_td_args a, double* __restrict__ acc) {
  const int c = blockIdx.x;
  const int A = a.n_act;
  double s[kEvalSlots];
#pragma unroll
  for (int k = 0; k < kEvalSlots; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < a.batch; b += 256) {
    const int act = (int)a.act[b];
    if (act < 0 || act >= A) continue;
    const float* q = a.q_before + (size_t)b * a.ldq + c * A;
    // the target, as td_error_of states it (the same expressions in the same order)
    const float* qo = a.q_after_online + (size_t)b * a.ldq + c * A;
    int best = 0;
    float bv = qo[0];
    for (int k = 1; k < A; ++k) {
      const float v = qo[k];
      if (v > bv) {  // strict: first maximum wins (torch.argmax)
        bv = v;
        best = k;
      }
    }
    float qa = a.q_after_target[(size_t)b * a.ldq + c * A + best];
    qa = qa * (1.0f - a.term[b * a.n_cat + c]);
    const float r = a.rew[b * a.n_cat + c];
    float y = a.linear ? r + (qa - 0.1f) : r + a.gamma * qa;
    if (a.clip_rect) y = fminf(fmaxf(y, 0.f), 1.f);
    const float qb = q[act];
    const float d = qb - y;
    const float ad = fabsf(d);
    const float l = (a.loss_kind == 1 && !(ad < 1.0f)) ? ad - 0.5f : 0.5f * d * d;
    // the greedy action of Q(s) and the conservative penalty
    int kmax = 0;
    float m = q[0];
    for (int k = 1; k < A; ++k) {
      const float v = q[k];
      if (v > m) {
        m = v;
        kmax = k;
      }
    }
    float pen = 0.f;
    if (A > 1) {
      float sum = 0.f;
      for (int k = 0; k < A; ++k) sum += expf(q[k] - m);
      pen = logf(sum) + (m - qb);
    }
    const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
    s[0] += (double)vm;
    s[1] += (double)(l * vm);
    s[2] += (double)(ad * vm);
    s[3] += (double)(qb * vm);
    s[4] += (double)(m * vm);
    s[5] += (double)(y * vm);
    s[6] += (double)(pen * vm);
    s[7] += (double)((kmax == act ? 1.0f : 0.0f) * vm);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < kEvalSlots; ++k) s[k] += __shfl_down(s[k], o, 64);
  __shared__ double red[kEvalSlots][4];
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < kEvalSlots; ++k) red[k][threadIdx.x >> 6] = s[k];
  __syncthreads();
  if (threadIdx.x < kEvalSlots) {
    const int k = threadIdx.x;
    const double sk = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    acc[c * kEvalSlots + k] = acc[c * kEvalSlots + k] + sk;
  }
}

}  // namespace

extern "C" int vdqn_td_eval(const vdqn_td_args* a, double* acc, void* stream) {
  VDQN_CHECK(a && acc && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term, "vdqn_td_eval: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_eval: use_valid without valid mask");
  VDQN_CHECK(a->batch >= 1 && a->n_cat >= 1 && a->n_act >= 1 && a->ldq >= 1 && (int64_t)a->n_cat * a->n_act <= a->ldq,
             "vdqn_td_eval: bad dims (batch %d, n_cat %d, n_act %d, ldq %d)", a->batch, a->n_cat, a->n_act, a->ldq);
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_td_eval: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK((((uintptr_t)acc) & 7) == 0, "vdqn_td_eval: acc must be 8-byte aligned");
  ProfScope ps_("td_eval", 0.0, (double)a->batch * a->n_cat * (3.0 * a->n_act + 3.0) * 4.0 + (double)a->n_cat * kEvalSlots * 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(td_eval_kernel, dim3(a->n_cat), dim3(256), 0, (hipStream_t)stream, *a, acc);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The head table: what a head algorithm adds to a validation pass.  acc_head is f64 [n_cat + 1][8]; one launch per validation batch
// of n_cat + 1 blocks of 256 threads.  Block c < n_cat owns category c and row c, block n_cat owns the per-sample row n_cat.  Every
// quantity is the loss kernel's own statement of it (iql_math.h, dist_math.h, bcq_math.h: the functions the loss launches call), with
// the scalar gamma, no importance weight and no per-sample discount: validation is one-step for every algorithm.  The summation is
// td_eval_kernel's: thread t adds the terms of samples t, t + 256, .. in that order, each formed in f32, multiplied by vm LAST and
// widened to f64; shuffle folds at 32 .. 1; the four waves left to right; one f64 addition per slot into the table.  No atomics: no
// other block touches the row, so two passes agree bit for bit.  A row whose action is outside [0, A) adds nothing to any row.
//
// Rows c < n_cat, per sample b (vm = valid or 1, a* = act[b], the symbols of the loss kernels' header comments):
//   slot  IQL (q_after_target = the TARGET at s)    DIST                                         BCQ
//   0     vm                                        vm                                           vm
//   1     L_V = omega * u * u                       L: the KL in the configured direction, >= 0   l(d), d against the constrained target
//   2     u = q_target[Q(c, a*)] - V(s)             sqrtf(s2)                                    |d|
//   3     l(d), d = iql_error_of (loss_kind)        (d * d) / s2                                 y
//   4     |d|                                       0.5 * (logf(s2) + (d * d) / s2): the NLL of   [a' != a0]
//                                                   the backup's mean, constant dropped
//   5     V(s)                                      [d * d <= s2]: one-sigma coverage             [kc == a*], kc = first maximum of Q(s, c, .) over
//                                                                                                the actions the logits AT S allow
//   6     y                                         sqrtf(v): the backup's sigma                  [kc != k*], k* = the free first arg-max of Q(s, c, .)
//   7     [u > 0]                                   sqrtf(var(rho(c, k*))), k* = first arg-max    Q(s, c, kc)
//                                                   of the means at s
// Row n_cat: zeros for IQL and DIST.  BCQ, per sample, unweighted, no valid mask, i = the logits at s, m = max i, S = sum expf(i - m):
//   0: 1    1: ce_b = logf(S) + (m - i_{a*})    2: [first arg-max of i == a*]    3: reg_b = (sum i * i) / A    4: actions allowed at s
//   5: expf(i_{a*} - m) / S    6: actions allowed at s' (the online logits)    7: 0
namespace {

// l(d) as td_eval_kernel writes it
__device__ __forceinline__ float head_loss_of(float d, float ad, int loss_kind) { return (loss_kind == 1 && !(ad < 1.0f)) ? ad - 0.5f : 0.5f * d * d; }

// td_eval_kernel's fold of the threads' eight f64 sums and the one addition per slot into `row`
__device__ __forceinline__ void head_fold(double (&s)[kEvalSlots], double* __restrict__ row) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int k = 0; k < kEvalSlots; ++k) s[k] += __shfl_down(s[k], o, 64);
  __shared__ double red[kEvalSlots][4];
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < kEvalSlots; ++k) red[k][threadIdx.x >> 6] = s[k];
  __syncthreads();
  if (threadIdx.x < kEvalSlots) {
    const int k = threadIdx.x;
    const double sk = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    row[k] = row[k] + sk;
  }
}

__global__ __launch_bounds__(256) void td_eval_iql_kernel(const iql_kernel_args a, double* __restrict__ acc) {
  const int c = blockIdx.x;
  if (c >= a.n_cat) return;  // (the per-sample row: nothing to add; the whole block leaves, no barrier is missed)
  const int nq = a.n_cat * a.n_act;
  double s[kEvalSlots];
#pragma unroll
  for (int k = 0; k < kEvalSlots; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < a.batch; b += 256) {
    const int act = (int)a.act[b];
    if (act < 0 || act >= a.n_act) continue;
    const float v = a.q_before[(size_t)b * a.ldq + nq + c];
    const float qt = a.q_after_target[(size_t)b * a.ldq + c * a.n_act + act];
    const float u = qt - v;
    const float lv = iql_omega(u, a.tau) * u * u;
    float y;
    const float d = iql_error_of(a, b, c, act, a.gamma, &y);
    const float ad = fabsf(d);
    const float l = head_loss_of(d, ad, a.loss_kind);
    const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
    s[0] += (double)vm;
    s[1] += (double)(lv * vm);
    s[2] += (double)(u * vm);
    s[3] += (double)(l * vm);
    s[4] += (double)(ad * vm);
    s[5] += (double)(v * vm);
    s[6] += (double)(y * vm);
    s[7] += (double)((u > 0.f ? 1.0f : 0.0f) * vm);
  }
  head_fold(s, acc + c * kEvalSlots);
}

// 0.5 * (logf(s2) + z2): the Gaussian negative log-likelihood of the backup's mean under the prediction, constant dropped
__device__ __forceinline__ float dist_nll(float s2, float z2) {
#pragma clang fp contract(off)
  return 0.5f * (logf(s2) + z2);
}

template <bool BACK, bool LOGS>
__global__ __launch_bounds__(256) void td_eval_dist_kernel(const dist_kernel_args a, double* __restrict__ acc) {
  const int c = blockIdx.x;
  if (c >= a.n_cat) return;  // (the per-sample row: nothing to add)
  const int nq = a.n_cat * a.n_act;
  double s[kEvalSlots];
#pragma unroll
  for (int k = 0; k < kEvalSlots; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < a.batch; b += 256) {
    const int act = (int)a.act[b];
    if (act < 0 || act >= a.n_act) continue;
    const float* row = a.q_before + (size_t)b * a.ldq;
    const int best = dist_choice(a, b, c);
    const float d = row[c * a.n_act + act] - dist_target_mean(a, b, c, best, a.gamma);
    const float v = dist_target_var<LOGS>(a, b, c, best, a.gamma);
    const float s2 = dist_var<LOGS>(row[nq + c * a.n_act + act], a.smin2);
    const float z2 = dist_z2(d, s2);
    const int kmax = dist_first_max(row + c * a.n_act, a.n_act);
    const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
    s[0] += (double)vm;
    s[1] += (double)(dist_kl<BACK>(d, v, s2) * vm);
    s[2] += (double)(sqrtf(s2) * vm);
    s[3] += (double)(z2 * vm);
    s[4] += (double)(dist_nll(s2, z2) * vm);
    s[5] += (double)((d * d <= s2 ? 1.0f : 0.0f) * vm);
    s[6] += (double)(sqrtf(v) * vm);
    s[7] += (double)(sqrtf(dist_var<LOGS>(row[nq + c * a.n_act + kmax], a.smin2)) * vm);
  }
  head_fold(s, acc + c * kEvalSlots);
}

__global__ __launch_bounds__(256) void td_eval_bcq_kernel(const bcq_kernel_args a, double* __restrict__ acc) {
  __builtin_assume(a.n_act >= 2 && a.n_cat >= 1);  // (the entry has checked both)
  const int c = blockIdx.x;
  const int nq = a.n_cat * a.n_act;
  double s[kEvalSlots];
#pragma unroll
  for (int k = 0; k < kEvalSlots; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < a.batch; b += 256) {
    const int act = (int)a.act[b];
    if (act < 0 || act >= a.n_act) continue;
    const float* q = a.q_before + (size_t)b * a.ldq + (c < a.n_cat ? c : 0) * a.n_act;
    const float* lg = a.q_before + (size_t)b * a.ldq + nq;               // the logits at s
    const float* lgo = a.q_after_online + (size_t)b * a.ldq + nq;        // the online logits at s'
    const float m = bcq_logit_max(lg, a.n_act), mo = bcq_logit_max(lgo, a.n_act);
    if (c < a.n_cat) {
      int fb, kfree;
      const int best = bcq_choice(a, b, c, mo, &fb);
      float y;
      const float d = bcq_error_of(a, b, c, act, a.gamma, best, &y);
      const float ad = fabsf(d);
      const float l = head_loss_of(d, ad, a.loss_kind);
      const int kc = bcq_choice_of(q, lg, a.n_act, m, a.lt, &kfree);
      const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
      s[0] += (double)vm;
      s[1] += (double)(l * vm);
      s[2] += (double)(ad * vm);
      s[3] += (double)(y * vm);
      s[4] += (double)((best != fb ? 1.0f : 0.0f) * vm);
      s[5] += (double)((kc == act ? 1.0f : 0.0f) * vm);
      s[6] += (double)((kc != kfree ? 1.0f : 0.0f) * vm);
      s[7] += (double)(q[kc] * vm);
    } else {
      float S, sq;
      int first;
      bcq_logit_walk(lg, a.n_act, m, &S, &sq, &first);
      const float x = lg[act];
      int n_s = 0, n_o = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
      for (int k = 0; k < a.n_act; ++k) {
        n_s += bcq_allowed(lg, k, m, a.lt) ? 1 : 0;
        n_o += bcq_allowed(lgo, k, mo, a.lt) ? 1 : 0;
      }
      s[0] += 1.0;
      s[1] += (double)(logf(S) + (m - x));
      s[2] += (double)(first == act ? 1.0f : 0.0f);
      s[3] += (double)(sq / (float)a.n_act);
      s[4] += (double)(float)n_s;
      s[5] += (double)(expf(x - m) / S);
      s[6] += (double)(float)n_o;
    }
  }
  head_fold(s, acc + c * kEvalSlots);
}

template <bool BACK>
void launch_eval_dist(bool log_sigma, int grid, hipStream_t st, const dist_kernel_args& k, double* acc) {
  if (log_sigma) hipLaunchKernelGGL((td_eval_dist_kernel<BACK, true>), dim3(grid), dim3(256), 0, st, k, acc);
  else hipLaunchKernelGGL((td_eval_dist_kernel<BACK, false>), dim3(grid), dim3(256), 0, st, k, acc);
}

double head_eval_bytes(const vdqn_td_args* a) { return (double)a->batch * a->n_cat * (3.0 * a->n_act + 3.0) * 4.0 + (double)(a->n_cat + 1) * kEvalSlots * 16.0; }

}  // namespace

// Every check its loss entry makes of what this launch reads (each fails by the entry's name before any HIP call), then the one launch.
extern "C" int vdqn_td_eval_iql(const vdqn_td_args* a, float expectile, double* acc_head, void* stream) {
  VDQN_CHECK(a && acc_head && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term, "vdqn_td_eval_iql: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_eval_iql: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_eval_iql: bad dims");
  VDQN_CHECK((int64_t)a->n_cat * a->n_act + a->n_cat <= a->ldq,
             "vdqn_td_eval_iql: n_cat * n_act + n_cat = %lld columns (Q, then one V per category) do not fit in ldq %d",
             (long long)a->n_cat * a->n_act + a->n_cat, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_eval_iql: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_td_eval_iql: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK(!a->linear, "vdqn_td_eval_iql: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target and has no V(s') form");
  VDQN_CHECK(isfinite(expectile) && expectile >= 0.5f && expectile < 1.0f, "vdqn_td_eval_iql: expectile %g must be in [0.5, 1)", (double)expectile);
  VDQN_CHECK((((uintptr_t)acc_head) & 7) == 0, "vdqn_td_eval_iql: acc_head must be 8-byte aligned");
  ProfScope ps_("td_eval_iql", 0.0, head_eval_bytes(a), (hipStream_t)stream);
  iql_kernel_args k;
  memset(&k, 0, sizeof(k));
  static_cast<vdqn_td_args&>(k) = *a;
  k.tau = expectile;
  hipLaunchKernelGGL(td_eval_iql_kernel, dim3(a->n_cat + 1), dim3(256), 0, (hipStream_t)stream, k, acc_head);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_td_eval_dist(const vdqn_td_args* a, int32_t flags, float sigma_min, double* acc_head, void* stream) {
  VDQN_CHECK(a && acc_head && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term, "vdqn_td_eval_dist: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_eval_dist: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_eval_dist: bad dims");
  VDQN_CHECK(2 * (int64_t)a->n_cat * a->n_act <= a->ldq, "vdqn_td_eval_dist: 2 * n_cat * n_act = %lld columns (the means, then one spread per mean) do not fit in ldq %d",
             2 * (long long)a->n_cat * a->n_act, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_eval_dist: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(!a->linear, "vdqn_td_eval_dist: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; a variance has no backup without a discount");
  VDQN_CHECK(a->loss_kind == 0, "vdqn_td_eval_dist: loss_kind %d: the loss is a KL divergence, which has no Huber form (loss_kind must be 0)", a->loss_kind);
  VDQN_CHECK((flags & ~3) == 0, "vdqn_td_eval_dist: flags 0x%x has unknown bits (bit 0 = KL_BACKWARDS, bit 1 = LOG_SIGMA)", (unsigned)flags);
  VDQN_CHECK(isfinite(sigma_min) && sigma_min >= 1e-4f && sigma_min <= 10.0f, "vdqn_td_eval_dist: sigma_min %g must be in [1e-4, 10]", (double)sigma_min);
  VDQN_CHECK((((uintptr_t)acc_head) & 7) == 0, "vdqn_td_eval_dist: acc_head must be 8-byte aligned");
  ProfScope ps_("td_eval_dist", 0.0, head_eval_bytes(a), (hipStream_t)stream);
  dist_kernel_args k;
  memset(&k, 0, sizeof(k));
  static_cast<vdqn_td_args&>(k) = *a;
  k.smin2 = sigma_min * sigma_min;
  if (flags & DIST_KL_BACKWARDS) launch_eval_dist<true>((flags & DIST_LOG_SIGMA) != 0, a->n_cat + 1, (hipStream_t)stream, k, acc_head);
  else launch_eval_dist<false>((flags & DIST_LOG_SIGMA) != 0, a->n_cat + 1, (hipStream_t)stream, k, acc_head);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_td_eval_bcq(const vdqn_td_args* a, float threshold, double* acc_head, void* stream) {
  VDQN_CHECK(a && acc_head && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term, "vdqn_td_eval_bcq: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_eval_bcq: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_eval_bcq: bad dims");
  VDQN_CHECK(a->n_act >= 2, "vdqn_td_eval_bcq: n_act is %d: with one action there is nothing to constrain (n_act >= 2)", a->n_act);
  VDQN_CHECK((int64_t)a->n_cat * a->n_act + a->n_act <= a->ldq,
             "vdqn_td_eval_bcq: n_cat * n_act + n_act = %lld columns (Q, then one behaviour logit per action) do not fit in ldq %d",
             (long long)a->n_cat * a->n_act + a->n_act, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_eval_bcq: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_td_eval_bcq: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK(!a->linear, "vdqn_td_eval_bcq: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; the constrained target is not defined for it");
  VDQN_CHECK(isfinite(threshold) && threshold >= 0.0f && threshold < 1.0f, "vdqn_td_eval_bcq: threshold %g must be in [0, 1)", (double)threshold);
  VDQN_CHECK((((uintptr_t)acc_head) & 7) == 0, "vdqn_td_eval_bcq: acc_head must be 8-byte aligned");
  ProfScope ps_("td_eval_bcq", 0.0, head_eval_bytes(a), (hipStream_t)stream);
  bcq_kernel_args k;
  memset(&k, 0, sizeof(k));
  static_cast<vdqn_td_args&>(k) = *a;
  k.lt = bcq_log_threshold(threshold);
  hipLaunchKernelGGL(td_eval_bcq_kernel, dim3(a->n_cat + 1), dim3(256), 0, (hipStream_t)stream, k, acc_head);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
