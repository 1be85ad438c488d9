// Gaussian distributional Q-learning on top of the TD loss of train_q_network.py:134-169,180 (config keys DISTRIBUTIONAL,
// KL_BACKWARDS, LOG_SIGMA of the reference's defaults.py:34-36; visualize_value.py:88-93 reads a mean and a variance per
// (category, action)): the return of every (category, action) is a Gaussian N(mean, var), the bootstrapped backup of the Double-DQN
// choice is another, and the loss is the KL divergence between the two.
//
// A row of ldq columns holds the mean at column M(c, a) = c * A + a (the Q column) and the spread parameter rho at column
// S(c, a) = C * A + c * A + a, so 2 * C * A <= ldq.  With a* = act[b], smin2 = sigma_min * sigma_min, w_b the importance weight
// (1 without), vm_bc = valid or 1, gamma_b = sample_gamma[b] or gamma:
//   var(rho) = e(rho) + smin2
//     LOG_SIGMA      rc = clamp(rho, -8, 4);  e = expf(2 * rc);  de/drho = 2 * e for -8 < rho < 4, else exactly 0
//     otherwise      sp = rho > 20 ? rho : log1pf(expf(rho));  e = sp * sp;  de/drho = (2 * sp) * (1 / (1 + expf(-rho)))
//   a'  = first arg-max of q_after_online[b][M(c, .)]              (the Double-DQN choice, on the means)
//   mt  = q_after_target[b][M(c, a')]         vt = var(q_after_target[b][S(c, a')])
//   m   = td_error_of's y (pointwise.hip):  qa = mt * (1 - term);  y = r + gamma_b * qa;  rect clip -> clamp(y, 0, 1)
//   g   = gamma_b * (1 - term)                v  = max((g * g) * vt, smin2)
//   mu  = q_before[b][M(c, a*)]               s2 = var(q_before[b][S(c, a*)])               d = mu - m
//   KL_BACKWARDS 0   L = KL(N(m, v) || N(mu, s2)) = 0.5 * (logf(s2 / v) + (v + d * d) / s2 - 1)
//                    dL/dmu = d / s2          dL/ds2 = 0.5 * ((s2 - (v + d * d)) / (s2 * s2))
//   KL_BACKWARDS 1   L = KL(N(mu, s2) || N(m, v)) = 0.5 * (logf(v / s2) + (s2 + d * d) / v - 1)
//                    dL/dmu = d / v           dL/ds2 = 0.5 * ((s2 - v) / (v * s2))
//   L is clamped at 0 from below (a KL divergence is; its f32 evaluation next to 0 may round to -1e-8).
//   loss     += (L * w_b) * vm_bc                                       (the thread of M(c, a*))
//   dq[b][M(c, a*)] = ((dL/dmu * w_b) * vm_bc) * inv_count              (the thread of M(c, a*))
//   dq[b][S(c, a*)] = (((dL/ds2 * de/drho) * w_b) * vm_bc) * inv_count  (the thread of S(c, a*));  every other column 0
//   stats[0] += vm_bc * sqrtf(s2)        stats[1] += vm_bc * ((d * d) / s2)                 (the thread of S(c, a*); unweighted)
//   err[b]    = sum_c |d_bc| * vm_bc / C                                (the thread of column 0; priorities follow the mean's error)
// No gradient flows through m, v or a'.  The floor smin2 keeps the KL finite at terminal rows, where g = 0, and bounds 1 / s2.
// Rounding: every function below that states arithmetic compiles with contraction off, so each product, quotient and sum written
// above rounds on its own (no fused multiply-add anywhere): gamma_b * qa, g * g, (g * g) * vt, d * d, 2 * rc, sp * sp, 2 * sp and
// s2 * s2 are separate roundings.  m and d are therefore the bits td_loss_kernel forms, and err[b] equals vdqn_td_loss_weighted's
// on the same mean columns bit for bit (tests/test_gpu_dist.py).
// One thread per (sample, padded column), 256 threads; the block's three sums are multiplied by inv_count and added to loss,
// stats[0] and stats[1] with one atomic each.  A deterministic launch is ONE block that walks all elements (thread t takes t,
// t + 256, ..; the block sum's fixed order), as td_loss_kernel's.  A row whose action is outside [0, A) writes zeros and adds nothing.
#include <math.h>

#include "block_sum.h"
#include "common.h"
#include "dist_math.h"  // dist_kernel_args, dist_var, dist_choice, dist_target_mean / _var, dist_error_of, dist_kl, dist_z2: shared with eval.hip

namespace {

// The four derivative forms, once (the two divergences: dist_math.h).
template <bool BACK>
__device__ __forceinline__ float dist_dmu(float d, float v, float s2) {
  return BACK ? d / v : d / s2;
}
template <bool BACK>
__device__ __forceinline__ float dist_ds2(float d, float v, float s2) {
#pragma clang fp contract(off)
  return BACK ? 0.5f * ((s2 - v) / (v * s2)) : 0.5f * ((s2 - (v + d * d)) / (s2 * s2));
}

template <typename T, bool BACK, bool LOGS>
__global__ __launch_bounds__(256) void dist_loss_kernel(const dist_kernel_args a) {
  const int total = a.batch * a.ldq;
  const int nq = a.n_cat * a.n_act;
  float sums[3] = {};  // this thread's terms of the loss, of the predicted sigma, of the squared standardised error
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / a.ldq, col = i - b * a.ldq;
    const int act = (int)a.act[b];
    const bool act_ok = act >= 0 && act < a.n_act;
    float g = 0.f;
    if (col < nq && a.q_copy) a.q_copy[(size_t)b * nq + col] = a.q_before[(size_t)b * a.ldq + col];
    if (col < 2 * nq && act_ok) {
      const bool spread = col >= nq;
      const int qcol = spread ? col - nq : col;
      const int c = qcol / a.n_act, ac = qcol - c * a.n_act;
      if (ac == act) {
        const float gamma = a.sg ? a.sg[b] : a.gamma;
        const int best = dist_choice(a, b, c);
        const float d = a.q_before[(size_t)b * a.ldq + qcol] - dist_target_mean(a, b, c, best, gamma);
        const float v = dist_target_var<LOGS>(a, b, c, best, gamma);
        float de;
        const float s2 = dist_var<LOGS>(a.q_before[(size_t)b * a.ldq + nq + qcol], a.smin2, &de);
        const float vm = a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f;
        if (!spread) {
          float l = dist_kl<BACK>(d, v, s2);
          float dl = dist_dmu<BACK>(d, v, s2);
          if (a.w) {
            l *= a.w[b];
            dl *= a.w[b];
          }
          sums[0] += l * vm;
          g = dl * vm * a.inv_count;
        } else {
          float dl = dist_ds2<BACK>(d, v, s2) * de;
          if (a.w) dl *= a.w[b];
          sums[1] += vm * sqrtf(s2);
          sums[2] += vm * dist_z2(d, s2);
          g = dl * vm * a.inv_count;
        }
      }
    }
    if (col == 0 && a.err) {
      float e = 0.f;
      if (act_ok)
        for (int c = 0; c < a.n_cat; ++c)
          e += fabsf(dist_error_of(a, b, c, act, a.sg ? a.sg[b] : a.gamma)) * (a.use_valid ? a.valid[b * a.n_cat + c] : 1.0f);
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

// out[b][c][a] = {mean, var(rho)}: one thread per (sample, Q column), the two floats as one 8-byte store
template <bool LOGS>
__global__ __launch_bounds__(256) void dist_moments_kernel(const float* __restrict__ q, float2* __restrict__ out, int batch, int nq, int ldq, float smin2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= batch * nq) return;
  const int b = i / nq, col = i - b * nq;
  const float* row = q + (size_t)b * ldq;
  out[i] = make_float2(row[col], dist_var<LOGS>(row[nq + col], smin2));
}

template <typename T, bool BACK, bool LOGS>
void launch_dist(int grid, hipStream_t st, const dist_kernel_args& k) {
  hipLaunchKernelGGL((dist_loss_kernel<T, BACK, LOGS>), dim3(grid), dim3(256), 0, st, k);
}
template <typename T>
void launch_dist_flags(int32_t flags, int grid, hipStream_t st, const dist_kernel_args& k) {
  switch (flags & 3) {
    case 0: launch_dist<T, false, false>(grid, st, k); break;
    case DIST_KL_BACKWARDS: launch_dist<T, true, false>(grid, st, k); break;
    case DIST_LOG_SIGMA: launch_dist<T, false, true>(grid, st, k); break;
    default: launch_dist<T, true, true>(grid, st, k); break;
  }
}

}  // namespace

// Every check (each fails by the entry's name before any HIP call), then the one launch.
extern "C" int vdqn_td_loss_dist(const vdqn_td_args* a, const float* weight, float* err_out, const float* sample_gamma, int32_t flags, float sigma_min,
                                 float* stats, void* stream) {
  VDQN_CHECK(a && a->q_before && a->q_after_online && a->q_after_target && a->act && a->rew && a->term && a->loss, "vdqn_td_loss_dist: null arg");
  VDQN_CHECK(!a->use_valid || a->valid, "vdqn_td_loss_dist: use_valid without valid mask");
  VDQN_CHECK(a->batch > 0 && a->n_cat > 0 && a->n_act > 0 && a->ldq > 0, "vdqn_td_loss_dist: bad dims");
  VDQN_CHECK(2 * (int64_t)a->n_cat * a->n_act <= a->ldq, "vdqn_td_loss_dist: 2 * n_cat * n_act = %lld columns (the means, then one spread per mean) do not fit in ldq %d",
             2 * (long long)a->n_cat * a->n_act, a->ldq);
  VDQN_CHECK((int64_t)a->batch * a->ldq < (1ll << 31), "vdqn_td_loss_dist: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(a->dtype == VDQN_F32 || a->dtype == VDQN_BF16, "vdqn_td_loss_dist: bad dtype");
  VDQN_CHECK(!a->linear, "vdqn_td_loss_dist: linear: y = r + (Qa - 0.1) is the reference's undiscounted Double-DQN target; a variance has no backup without a discount");
  VDQN_CHECK(a->loss_kind == 0, "vdqn_td_loss_dist: loss_kind %d: the loss is a KL divergence, which has no Huber form (loss_kind must be 0)", a->loss_kind);
  VDQN_CHECK((flags & ~3) == 0, "vdqn_td_loss_dist: flags 0x%x has unknown bits (bit 0 = KL_BACKWARDS, bit 1 = LOG_SIGMA)", (unsigned)flags);
  VDQN_CHECK(isfinite(sigma_min) && sigma_min >= 1e-4f && sigma_min <= 10.0f, "vdqn_td_loss_dist: sigma_min %g must be in [1e-4, 10]", (double)sigma_min);
  const int g = a->deterministic ? 1 : (int)(((int64_t)a->batch * a->ldq + 255) / 256);
  ProfScope ps_("td_loss_dist", 0.0, (double)a->batch * a->ldq * 16.0 + (double)a->batch * 8.0, (hipStream_t)stream);
  dist_kernel_args k;
  static_cast<vdqn_td_args&>(k) = *a;
  k.w = weight;
  k.err = err_out;
  k.sg = sample_gamma;
  k.stats = stats;
  k.smin2 = sigma_min * sigma_min;
  if (a->dtype == VDQN_BF16) launch_dist_flags<bf16raw>(flags, g, (hipStream_t)stream, k);
  else launch_dist_flags<float>(flags, g, (hipStream_t)stream, k);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}

extern "C" int vdqn_dist_moments(const float* q_rows, float* out, int32_t batch, int32_t n_cat, int32_t n_act, int32_t ldq, int32_t flags,
                                 float sigma_min, void* stream) {
  VDQN_CHECK(q_rows && out, "vdqn_dist_moments: null arg");
  VDQN_CHECK(batch > 0 && n_cat > 0 && n_act > 0 && ldq > 0, "vdqn_dist_moments: bad dims");
  VDQN_CHECK(2 * (int64_t)n_cat * n_act <= ldq, "vdqn_dist_moments: 2 * n_cat * n_act = %lld columns (the means, then one spread per mean) do not fit in ldq %d",
             2 * (long long)n_cat * n_act, ldq);
  VDQN_CHECK((int64_t)batch * ldq < (1ll << 31), "vdqn_dist_moments: batch * ldq exceeds the kernel's 32-bit element index");
  VDQN_CHECK(((uintptr_t)out & 7) == 0, "vdqn_dist_moments: out must be 8-byte aligned");
  VDQN_CHECK((flags & ~3) == 0, "vdqn_dist_moments: flags 0x%x has unknown bits (bit 0 = KL_BACKWARDS, unused here; bit 1 = LOG_SIGMA)", (unsigned)flags);
  VDQN_CHECK(isfinite(sigma_min) && sigma_min >= 1e-4f && sigma_min <= 10.0f, "vdqn_dist_moments: sigma_min %g must be in [1e-4, 10]", (double)sigma_min);
  const int nq = n_cat * n_act;
  const int g = (int)(((int64_t)batch * nq + 255) / 256);
  ProfScope ps_("dist_moments", 0.0, (double)batch * nq * 16.0, (hipStream_t)stream);
  if (flags & DIST_LOG_SIGMA) hipLaunchKernelGGL((dist_moments_kernel<true>), dim3(g), dim3(256), 0, (hipStream_t)stream, q_rows, (float2*)out, batch, nq, ldq, sigma_min * sigma_min);
  else hipLaunchKernelGGL((dist_moments_kernel<false>), dim3(g), dim3(256), 0, (hipStream_t)stream, q_rows, (float2*)out, batch, nq, ldq, sigma_min * sigma_min);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
