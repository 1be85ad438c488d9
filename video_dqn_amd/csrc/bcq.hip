// Discrete batch-constrained Q-learning (BCQ; Fujimoto, Conti, Ghavamzadeh, Pineau, 2019) on top of the TD loss of
// train_q_network.py:134-169,180: a behaviour head i(a) beside Q, fitted to the logged action by cross-entropy, and a Double-DQN
// target whose arg-max may only choose actions the behaviour head finds plausible at s'.
//
// A row of ldq columns holds Q(c, a) at column c * A + a and the behaviour logit i(a) at column C * A + a (one set of logits per
// sample: the logged action is shared by all categories), so C * A + A <= ldq.  With a* = act[b], w_b the importance weight (1
// without), vm_bc = valid or 1, gamma_b = sample_gamma[b] or gamma, i = q_before[b][C*A + .] (the logits at s) and
// i' = q_after_online[b][C*A + .] (the ONLINE logits at s'):
//   allowed set at s'   m' = max_a i'_a;  lt = (float)log((double)threshold), -inf for threshold 0, rounded once on the host;
//                       a is allowed iff (i'_a - m') > lt in f32.  The arg-max of i' is always allowed (0 > lt for threshold < 1),
//                       so the set is never empty, and no exponential is needed: pi(a) / max pi > threshold in the log domain.
//   a'  = first maximum of q_after_online[b][c*A + a] over the allowed a        a0 = first maximum over all a (the free arg-max)
//   qa  = q_after_target[b][c*A + a'] * (1 - term);  y = r + gamma_b * qa;  rect clip -> clamp(y, 0, 1)     (td_error_of's order)
//   d   = q_before[b][c*A + a*] - y       l(d), dl(d): half squared error and d, or Huber with beta 1 and its clamp (loss_kind)
//   behaviour loss, per sample, no valid mask:   m = max_a i_a;  S = sum_a expf(i_a - m)  (a = 0 .. A-1, in that order)
//     ce_b  = logf(S) + (m - i_{a*})          reg_b = (sum_a i_a * i_a) / A          L_B = bc_weight * (ce_b + logit_reg * reg_b)
//     dL_B/di_a = bc_weight * ((expf(i_a - m) / S - [a == a*]) + logit_reg * ((2 * i_a) / A))
//   The TD terms are means over B * C (inv_count = 1 / (C * global batch)); the behaviour terms are means over B, so they enter
//   with the factor kb = (float)C * inv_count.
//   loss     += inv_count * sum_bc (l * w_b) * vm_bc  +  kb * sum_b w_b * L_B
//   dq[b][c*A + a*] = ((dl * w_b) * vm_bc) * inv_count          dq[b][C*A + a] = (dL_B/di_a * w_b) * kb          every other column 0
//   err[b]    = sum_c |d_bc| * vm_bc / C                        (priorities follow the TD error alone)
//   stats[0] += kb * sum_b ce_b                                 (the unweighted mean cross-entropy)
//   stats[1] += inv_count * sum_bc vm_bc * [a' != a0]           (the share of targets the constraint changes)
//   stats[2] += kb * sum_b [first arg-max of i == a*]           (behaviour accuracy)
// No gradient flows through i', a' or y.  With threshold 0 every action is allowed, a' = a0, and bcq_error_of forms the bits of
// td_error_of: the taken-action columns of dq and err are then vdqn_td_loss_weighted's (vdqn_td_loss_nstep's with a per-sample
// discount) bit for bit (tests/test_gpu_bcq.py); that function compiles with contraction off, every product and sum rounds alone.
// One thread per (sample, padded column), 256 threads; the block's four sums are scaled and added to loss and stats[0..2] with one
// atomic each.  A deterministic launch is ONE block that walks all elements (thread t takes t, t + 256, ..; the block sum's fixed
// order), as td_loss_kernel's.  A row whose action is outside [0, A) writes zeros and adds nothing.
#include <math.h>

#include "block_sum.h"
#include "common.h"
#include "bcq_math.h"  // bcq_kernel_args, bcq_logit_max, bcq_allowed, bcq_choice, bcq_error_of, bcq_logit_walk: shared with eval.hip

namespace {

template <typename T>
__global__ __launch_bounds__(256) void bcq_loss_kernel(const bcq_kernel_args a) {
  __builtin_assume(a.n_act >= 2 && a.n_cat >= 1);  // (the entry has checked both: the short loops below need no guard of their own)
  const int total = a.batch * a.ldq;
  const int nq = a.n_cat * a.n_act;
  const float kb = (float)a.n_cat * a.inv_count;  // a mean over B inside sums that are scaled for means over B * C
  float sums[4] = {};  // this thread's share of the loss (scaled, set behind the walk), and its terms of the cross-entropy, of the changed targets, of the accuracy
  float tdl = 0.f, bcl = 0.f;  // its TD and behaviour loss terms, kept apart until the end: the first is scaled by inv_count, the second by kb
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / a.ldq, col = i - b * a.ldq;
    const int act = (int)a.act[b];
    const bool act_ok = act >= 0 && act < a.n_act;
    float g = 0.f;
    if (col < nq) {
      const int c = col / a.n_act, ac = col - c * a.n_act;
      if (a.q_copy) a.q_copy[(size_t)b * nq + col] = a.q_before[(size_t)b * a.ldq + col];
      if (ac == act) {
        int fb;
        const int best = bcq_choice(a, b, c, bcq_logit_max(a.q_after_online + (size_t)b * a.ldq + nq, a.n_act), &fb);
        const float d = bcq_error_of(a, b, c, act, a.sg ? a.sg[b] : a.gamma, best);
        float l, dl;
        if (a.loss_kind == 1) {  // Huber, beta = 1 (torch.nn.functional.smooth_l1_loss)
          const float ad = fabsf(d);
          l = ad < 1.0f ? 0.5f * d * d : ad - 0.5f;
          dl = fminf(fmaxf(d, -1.0f), 1.0f);
        } else {
          l = 0.5f * d * d;
          dl = d;
        }
        const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
        if (a.w) {
          l *= a.w[b];
          dl *= a.w[b];
        }
        tdl += l * vm;
        if (best != fb) sums[2] += vm;
        g = dl * vm * a.inv_count;
      }
    } else if (col < nq + a.n_act && act_ok) {
      const int ac = col - nq;
      const float* lg = a.q_before + (size_t)b * a.ldq + nq;
      const float m = bcq_logit_max(lg, a.n_act);
      float S, sq;
      int first;
      bcq_logit_walk(lg, a.n_act, m, &S, &sq, &first);  // the softmax's sum, the sum of squares and the first arg-max in one walk
      const float x = lg[ac];
      const float hit = ac == act ? 1.0f : 0.0f;
      float dl = a.bc_weight * ((expf(x - m) / S - hit) + a.logit_reg * ((2.0f * x) / (float)a.n_act));
      if (a.w) dl *= a.w[b];
      g = dl * kb;
      if (ac == act) {  // the one thread of the sample that adds its behaviour terms
        const float ce = logf(S) + (m - x);
        float lb = a.bc_weight * (ce + a.logit_reg * (sq / (float)a.n_act));
        if (a.w) lb *= a.w[b];
        bcl += lb;
        sums[1] += ce;
        if (first == act) sums[3] += 1.0f;
      }
    }
    if (col == 0 && a.err) {
      float e = 0.f;
      if (act_ok) {
        const float m = bcq_logit_max(a.q_after_online + (size_t)b * a.ldq + nq, a.n_act);
        const float gamma = a.sg ? a.sg[b] : a.gamma;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
        for (int c = 0; c < a.n_cat; ++c)
          e += fabsf(bcq_error_of(a, b, c, act, gamma, bcq_choice(a, b, c, m))) * (a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f);
      }
      a.err[b] = e / (float)a.n_cat;
    }
    if (a.dq) ((T*)a.dq)[i] = from_f32<T>(g);
    if (a.dq_f32) a.dq_f32[i] = g;
  }
  sums[0] = tdl * a.inv_count + bcl * kb;
  __shared__ float red[4][16];
  wave_partials(sums, red);
  if (threadIdx.x == 0) {
    add_partials(red, 4, sums);
    if (sums[0] != 0.f) atomicAdd(a.loss, sums[0]);
    if (a.stats && sums[1] != 0.f) atomicAdd(a.stats, sums[1] * kb);
    if (a.stats && sums[2] != 0.f) atomicAdd(a.stats + 1, sums[2] * a.inv_count);
    if (a.stats && sums[3] != 0.f) atomicAdd(a.stats + 2, sums[3] * kb);
  }
}

// One thread per (sample, j), j over the C*A Q columns and then the A logit columns: q_out = Q, or -inf where the action is not
// allowed; prob_out = the softmax of the logits.
__global__ __launch_bounds__(256) void bcq_constrain_kernel(const float* __restrict__ q, float* __restrict__ q_out, float* __restrict__ prob_out,
                                                            int batch, int nq, int n_act, int ldq, float lt) {
  const int per = nq + n_act;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * per) return;
  const int b = i / per, j = i - b * per;
  const float* row = q + (size_t)b * ldq;
  const float* lg = row + nq;
  const float m = bcq_logit_max(lg, n_act);
  if (j < nq) {
    const int ac = j % n_act;
    q_out[(size_t)b * nq + j] = bcq_allowed(lg, ac, m, lt) ? row[j] : -INFINITY;
  } else if (prob_out) {
    float S = 0.f;
    for (int k = 0; k < n_act; ++k) S += expf(lg[k] - m);
    prob_out[(size_t)b * n_act + (j - nq)] = expf(lg[j - nq] - m) / S;
  }
}

}  // namespace

// Every check (each fails by the entry's name before any HIP call), then the one launch.
extern "C" int vdqn_td_loss_bcq(const vdqn_td_args* a, const float* weight, float* err_out, const float* sample_gamma, float threshold, float bc_weight,
                                float logit_reg, float* stats, void* stream) {
  VDQN_CHECK(a && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term && a->loss, "vdqn_td_loss_bcq: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_loss_bcq: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_loss_bcq: bad dims");
  VDQN_CHECK(a->n_act >= 2, "vdqn_td_loss_bcq: n_act is %d: with one action there is nothing to constrain (n_act >= 2)", a->n_act);
  VDQN_CHECK((int64_t)a->n_cat * a->n_act + a->n_act <= a->ldq,
             "vdqn_td_loss_bcq: n_cat * n_act + n_act = %lld columns (Q, then one behaviour logit per action) do not fit in ldq %d",
             (long long)a->n_cat * a->n_act + a->n_act, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_loss_bcq: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(a->dtype == VDQN_F32 || a->dtype == VDQN_BF16, "vdqn_td_loss_bcq: bad dtype");
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_td_loss_bcq: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK(!a->linear, "vdqn_td_loss_bcq: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; the constrained target is not defined for it");
  VDQN_CHECK(isfinite(threshold) && threshold >= 0.0f && threshold < 1.0f, "vdqn_td_loss_bcq: threshold %g must be in [0, 1)", (double)threshold);
  VDQN_CHECK(isfinite(bc_weight) && bc_weight > 0.0f, "vdqn_td_loss_bcq: bc_weight %g must be finite and > 0", (double)bc_weight);
  VDQN_CHECK(isfinite(logit_reg) && logit_reg >= 0.0f, "vdqn_td_loss_bcq: logit_reg %g must be finite and >= 0", (double)logit_reg);
  const int g = a->deterministic ? 1 : (int)(((int64_t)a->batch * a->ldq + 255) / 256);
  ProfScope ps_("td_loss_bcq", 0.0, (double)a->batch * a->ldq * 16.0 + (double)a->batch * 8.0, (hipStream_t)stream);
  bcq_kernel_args k;
  static_cast<vdqn_td_args&>(k) = *a;
  k.w = weight;
  k.err = err_out;
  k.sg = sample_gamma;
  k.stats = stats;
  k.lt = bcq_log_threshold(threshold);
  k.bc_weight = bc_weight;
  k.logit_reg = logit_reg;
  if (a->dtype == VDQN_BF16) hipLaunchKernelGGL((bcq_loss_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL((bcq_loss_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, k);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_bcq_constrain(const float* q_rows, float* q_out, float* prob_out, int32_t batch, int32_t n_cat, int32_t n_act, int32_t ldq,
                                  float threshold, void* stream) {
  VDQN_CHECK(q_rows && q_out, "vdqn_bcq_constrain: null arg");
  VDQN_CHECK(batch > 0 && n_cat > 0 && n_act > 0 && ldq > 0, "vdqn_bcq_constrain: bad dims");
  VDQN_CHECK(n_act >= 2, "vdqn_bcq_constrain: n_act is %d: with one action there is nothing to constrain (n_act >= 2)", n_act);
  VDQN_CHECK((int64_t)n_cat * n_act + n_act <= ldq, "vdqn_bcq_constrain: n_cat * n_act + n_act = %lld columns (Q, then one behaviour logit per action) do not fit in ldq %d",
             (long long)n_cat * n_act + n_act, ldq);
  VDQN_CHECK((int64_t)batch * ldq < (1ll << 31), "vdqn_bcq_constrain: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(isfinite(threshold) && threshold >= 0.0f && threshold < 1.0f, "vdqn_bcq_constrain: threshold %g must be in [0, 1)", (double)threshold);
  const int nq = n_cat * n_act;
  const int g = (int)(((int64_t)batch * (nq + n_act) + 255) / 256);
  ProfScope ps_("bcq_constrain", 0.0, (double)batch * (nq + n_act) * 8.0, (hipStream_t)stream);
  hipLaunchKernelGGL(bcq_constrain_kernel, dim3(g), dim3(256), 0, (hipStream_t)stream, q_rows, q_out, prob_out, batch, nq, n_act, ldq,
                     bcq_log_threshold(threshold));
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
