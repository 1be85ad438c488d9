// The arithmetic of implicit Q-learning that more than one launch states: the loss (csrc/iql.hip) and the held-out head metrics
// (csrc/eval.hip) take the bootstrap's error and the expectile's weight from here, so that a validation pass reports the bits the
// loss launch trains on.  Header-only, in an anonymous namespace: every including file gets its own inlined copy.
#pragma once

#include "common.h"

namespace {

struct iql_kernel_args : vdqn_td_args {
  const float* w;   // [batch] or NULL (= 1)
  float* err;       // [batch] or NULL
  const float* sg;  // [batch] per-sample discount or NULL (= gamma)
  float* stats;     // f32[2] or NULL
  float tau;
};

// d = Q(s)[b, Q(c, a*)] - y with the bootstrap taken from V(s'); y into *y_out when asked for.  Every product and sum rounds on its
// own (no contraction into a fused multiply-add): that is what td_loss_kernel's instances evaluate, where the addition of r sits
// behind the select between the LINEAR and the discounted form, and what makes this launch's Q part the weighted TD loss bit for
// bit (tests/test_gpu_iql.py).
__device__ __forceinline__ float iql_error_of(const iql_kernel_args& a, int b, int c, int act, float gamma, float* y_out = nullptr) {
#pragma clang fp contract(off)
  const float qb = a.q_before[(size_t)b * a.ldq + c * a.n_act + act];
  float qa = a.q_after_online[(size_t)b * a.ldq + a.n_cat * a.n_act + c];
  qa = qa * (1.0f - a.term[b * a.n_cat + c]);
  const float r = a.rew[b * a.n_cat + c];
  float y = r + gamma * qa;
  if (a.clip_rect) y = fminf(fmaxf(y, 0.f), 1.f);
  if (y_out) *y_out = y;
  return qb - y;
}

// omega = u > 0 ? tau : 1 - tau: the expectile's weight of the advantage u = Q_target(s, a*) - V(s)
__device__ __forceinline__ float iql_omega(float u, float tau) { return u > 0.f ? tau : 1.0f - tau; }

}  // namespace
