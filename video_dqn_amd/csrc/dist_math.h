// The arithmetic of Gaussian distributional Q-learning that more than one launch states: the loss and the moments read-out
// (csrc/dist.hip) and the held-out head metrics (csrc/eval.hip) take the spread's parametrisation, the Double-DQN choice, the
// backup's mean and variance and the divergence from here.  Every function that states arithmetic compiles with contraction off.
// Header-only, in an anonymous namespace: every including file gets its own inlined copy.
#pragma once

#include <math.h>

#include "common.h"

namespace {

enum { DIST_KL_BACKWARDS = 1, DIST_LOG_SIGMA = 2 };

struct dist_kernel_args : vdqn_td_args {
  const float* w;   // [batch] or NULL (= 1)
  float* err;       // [batch] or NULL
  const float* sg;  // [batch] per-sample discount or NULL (= gamma)
  float* stats;     // f32[2] or NULL
  float smin2;      // sigma_min * sigma_min, rounded once on the host
};

// var(rho) = e(rho) + smin2, and de/drho into *de when asked for: the only statement of the spread's parametrisation (the loss,
// the target's variance, vdqn_dist_moments and the head metrics all take it from here).
template <bool LOGS>
__device__ __forceinline__ float dist_var(float rho, float smin2, float* de = nullptr) {
#pragma clang fp contract(off)
  float e;
  if constexpr (LOGS) {
    const float rc = fminf(fmaxf(rho, -8.0f), 4.0f);
    e = expf(2.0f * rc);
    if (de) *de = (rho > -8.0f && rho < 4.0f) ? 2.0f * e : 0.0f;
  } else {
    const float sp = rho > 20.0f ? rho : log1pf(expf(rho));
    e = sp * sp;
    if (de) *de = (2.0f * sp) * (1.0f / (1.0f + expf(-rho)));
  }
  return e + smin2;
}

// the first maximum of n_act means (torch.argmax; td_error_of's loop)
__device__ __forceinline__ int dist_first_max(const float* qo, int n_act) {
  int best = 0;
  float bv = qo[0];
  for (int k = 1; k < n_act; ++k) {
    const float v = qo[k];
    if (v > bv) {
      bv = v;
      best = k;
    }
  }
  return best;
}

// a': the first maximum of the online means of s'
__device__ __forceinline__ int dist_choice(const dist_kernel_args& a, int b, int c) {
  return dist_first_max(a.q_after_online + (size_t)b * a.ldq + c * a.n_act, a.n_act);
}

// m: the y of td_error_of in its expression order
__device__ __forceinline__ float dist_target_mean(const dist_kernel_args& a, int b, int c, int best, float gamma) {
#pragma clang fp contract(off)
  float qa = a.q_after_target[(size_t)b * a.ldq + c * a.n_act + best];
  qa = qa * (1.0f - a.term[b * a.n_cat + c]);
  const float r = a.rew[b * a.n_cat + c];
  float y = r + gamma * qa;
  if (a.clip_rect) y = fminf(fmaxf(y, 0.f), 1.f);
  return y;
}

// v = max((g * g) * vt, smin2), g = gamma_b * (1 - term)
template <bool LOGS>
__device__ __forceinline__ float dist_target_var(const dist_kernel_args& a, int b, int c, int best, float gamma) {
#pragma clang fp contract(off)
  const float vt = dist_var<LOGS>(a.q_after_target[(size_t)b * a.ldq + a.n_cat * a.n_act + c * a.n_act + best], a.smin2);
  const float g = gamma * (1.0f - a.term[b * a.n_cat + c]);
  return fmaxf((g * g) * vt, a.smin2);
}

// d = mu - m for category c of sample b (the loss terms and the per-sample error take it from here)
__device__ __forceinline__ float dist_error_of(const dist_kernel_args& a, int b, int c, int act, float gamma) {
  return a.q_before[(size_t)b * a.ldq + c * a.n_act + act] - dist_target_mean(a, b, c, dist_choice(a, b, c), gamma);
}

// The two divergences, once.
template <bool BACK>
__device__ __forceinline__ float dist_kl(float d, float v, float s2) {
#pragma clang fp contract(off)
  const float l = BACK ? 0.5f * (logf(v / s2) + (s2 + d * d) / v - 1.0f) : 0.5f * (logf(s2 / v) + (v + d * d) / s2 - 1.0f);
  return fmaxf(l, 0.0f);
}

// z2 = (d * d) / s2: the squared standardised error of the backup's mean under the prediction
__device__ __forceinline__ float dist_z2(float d, float s2) {
#pragma clang fp contract(off)
  return (d * d) / s2;
}

}  // namespace
