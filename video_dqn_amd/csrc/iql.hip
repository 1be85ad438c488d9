// Implicit Q-learning (IQL; Kostrikov et al., ICLR 2022) on top of the TD loss of train_q_network.py:134-169,180: a state-value
// head V(s) fitted by expectile regression to the target network's Q(s, a_data), and the bootstrap r + gamma (1 - t) V(s') in
// place of the Double-DQN arg-max, so that no action outside the logged data is ever evaluated.
//
// A 64-wide row holds Q(c, a) at column c * A + a and V(c) at column C * A + c.  For sample b, category c, a* = act[b], tau the
// expectile, w_b the importance weight (1 without), vm_bc = valid or 1:
//   v  = q_before[b][V(c)]            v' = q_after_online[b][V(c)]            (no gradient through v')
//   qt = q_after_target[b][Q(c, a*)]  (the TARGET network at s: the engine runs the target pass over the `before` frames)
//   u  = qt - v      omega = u > 0 ? tau : 1 - tau      L_V = omega * u * u      dL_V/dv = -2 * omega * u
//   qa = v' * (1 - term);  y = r + gamma_b * qa;  rect clip -> clamp(y, 0, 1)    (td_error_of's expression order, pointwise.hip:
//        with a q_after_target row whose actions all hold v', vdqn_td_loss_weighted forms the same y, d, dq and err bits)
//   d  = q_before[b][Q(c, a*)] - y    L_Q = l(d), dl(d): half squared error or Huber with beta 1 (loss_kind), as td_loss_kernel
//   loss     += ((L_Q + L_V) * w_b) * vm_bc        (the thread of Q(c, a*) adds the L_Q term, the thread of V(c) the L_V term)
//   stats[0] += (L_V * w_b) * vm_bc                stats[1] += vm_bc * u        (unweighted, as mc_stats)
//   dq[b][Q(c, a*)] = (dl * w_b) * vm_bc * inv_count      dq[b][V(c)] = ((-2 * omega * u) * w_b) * vm_bc * inv_count      others 0
//   err[b] = sum_c |d_bc| * vm_bc / C              (priorities follow the Q error)
// One thread per (sample, padded column), 256 threads; the block's three sums are multiplied by inv_count and added to loss,
// stats[0] and stats[1] with one atomic each.  A deterministic launch is ONE block that walks all elements (thread t takes t,
// t + 256, ..; the block sum's fixed order), as td_loss_kernel's.  A row whose action is outside [0, A) writes zeros and adds nothing.
#include <math.h>

#include "block_sum.h"
#include "common.h"
#include "iql_math.h"  // iql_kernel_args, iql_error_of, iql_omega: shared with the held-out head metrics (eval.hip)

namespace {

template <typename T>
__global__ __launch_bounds__(256) void iql_loss_kernel(const iql_kernel_args a) {
  const int total = a.batch * a.ldq;
  const int nq = a.n_cat * a.n_act;
  float sums[3] = {};  // this thread's terms of the loss, of the V loss alone, of the advantage
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / a.ldq, col = i - b * a.ldq;
    const int act = (int)a.act[b];
    const bool act_ok = act >= 0 && act < a.n_act;
    float g = 0.f;
    if (col < nq) {
      const int c = col / a.n_act, ac = col - c * a.n_act;
      if (a.q_copy) a.q_copy[(size_t)b * nq + col] = a.q_before[(size_t)b * a.ldq + col];
      if (ac == act) {
        const float d = iql_error_of(a, b, c, act, a.sg ? a.sg[b] : a.gamma);
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
        sums[0] += l * vm;
        g = dl * vm * a.inv_count;
      }
    } else if (col < nq + a.n_cat && act_ok) {
      const int c = col - nq;
      const float v = a.q_before[(size_t)b * a.ldq + col];
      const float qt = a.q_after_target[(size_t)b * a.ldq + c * a.n_act + act];
      const float u = qt - v;
      const float om = iql_omega(u, a.tau);
      float lv = om * u * u;
      float dv = -2.0f * om * u;
      const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
      if (a.w) {
        lv *= a.w[b];
        dv *= a.w[b];
      }
      sums[0] += lv * vm;
      sums[1] += lv * vm;
      sums[2] += vm * u;
      g = dv * vm * a.inv_count;
    }
    if (col == 0 && a.err) {
      float e = 0.f;
      if (act_ok)
        for (int c = 0; c < a.n_cat; ++c)
          e += fabsf(iql_error_of(a, b, c, act, a.sg ? a.sg[b] : a.gamma)) * (a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f);
      a.err[b] = e / (float)a.n_cat;
    }
    if (a.dq) ((T*)a.dq)[i] = from_f32<T>(g);
    if (a.dq_f32) a.dq_f32[i] = g;
  }
  __shared__ float red[3][16];
  wave_partials(sums, red);
  if (threadIdx.x == 0) {
    add_partials(red, 4, sums);
    if (sums[0] != 0.f) atomicAdd(a.loss, sums[0] * a.inv_count);
    if (a.stats && sums[1] != 0.f) atomicAdd(a.stats, sums[1] * a.inv_count);
    if (a.stats && sums[2] != 0.f) atomicAdd(a.stats + 1, sums[2] * a.inv_count);
  }
}

}  // namespace

// Every check (each fails by the entry's name before any HIP call), then the one launch.
extern "C" int vdqn_td_loss_iql(const vdqn_td_args* a, const float* weight, float* err_out, const float* sample_gamma, float expectile, float* stats,
                                void* stream) {
  VDQN_CHECK(a && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term && a->loss, "vdqn_td_loss_iql: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_loss_iql: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_loss_iql: bad dims");
  VDQN_CHECK((int64_t)a->n_cat * a->n_act + a->n_cat <= a->ldq,
             "vdqn_td_loss_iql: n_cat * n_act + n_cat = %lld columns (Q, then one V per category) do not fit in ldq %d",
             (long long)a->n_cat * a->n_act + a->n_cat, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_loss_iql: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(a->dtype == VDQN_F32 || a->dtype == VDQN_BF16, "vdqn_td_loss_iql: bad dtype");
  VDQN_CHECK(a->loss_kind == 0 || a->loss_kind == 1, "vdqn_td_loss_iql: loss_kind %d (0 = half squared error, 1 = Huber)", a->loss_kind);
  VDQN_CHECK(!a->linear, "vdqn_td_loss_iql: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target and has no V(s') form");
  VDQN_CHECK(isfinite(expectile) && expectile >= 0.5f && expectile < 1.0f, "vdqn_td_loss_iql: expectile %g must be in [0.5, 1)", (double)expectile);
  const int g = a->deterministic ? 1 : (int)(((int64_t)a->batch * a->ldq + 255) / 256);
  ProfScope ps_("td_loss_iql", 0.0, (double)a->batch * a->ldq * 16.0 + (double)a->batch * 8.0, (hipStream_t)stream);
  iql_kernel_args k;
  static_cast<vdqn_td_args&>(k) = *a;
  k.w = weight;
  k.err = err_out;
  k.sg = sample_gamma;
  k.stats = stats;
  k.tau = expectile;
  if (a->dtype == VDQN_BF16) hipLaunchKernelGGL((iql_loss_kernel<bf16raw>), dim3(g), dim3(256), 0, (hipStream_t)stream, k);
  else hipLaunchKernelGGL((iql_loss_kernel<float>), dim3(g), dim3(256), 0, (hipStream_t)stream, k);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
