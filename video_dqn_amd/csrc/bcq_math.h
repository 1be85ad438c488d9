// The arithmetic of discrete BCQ that more than one launch states: the loss and the constrained read-out (csrc/bcq.hip) and the
// held-out head metrics (csrc/eval.hip) take the allowed set, the constrained arg-max, the TD error and the walk over a row of
// behaviour logits from here.  Header-only, in an anonymous namespace: every including file gets its own inlined copy.
#pragma once

#include <math.h>

#include "common.h"

namespace {

struct bcq_kernel_args : vdqn_td_args {
  const float* w;   // [batch] or NULL (= 1)
  float* err;       // [batch] or NULL
  const float* sg;  // [batch] per-sample discount or NULL (= gamma)
  float* stats;     // f32[3] or NULL
  float lt;         // (float)log((double)threshold), -inf for 0
  float bc_weight, logit_reg;
};

// The allowed set: action a of a row of logits is allowed iff (logits[a] - max logits) > lt.  The only statement of the constraint
// (the loss's target, vdqn_bcq_constrain and the head metrics all take it from here).
__device__ __forceinline__ float bcq_logit_max(const float* logits, int n_act) {
  float m = logits[0];
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int k = 1; k < n_act; ++k) m = fmaxf(m, logits[k]);
  return m;
}
__device__ __forceinline__ bool bcq_allowed(const float* logits, int a, float m, float lt) { return (logits[a] - m) > lt; }
// lt of a threshold, rounded once on the host
inline float bcq_log_threshold(float threshold) { return threshold > 0.f ? (float)log((double)threshold) : -INFINITY; }

// The first maximum of the n_act values qo over the actions the logits lg allow (m = bcq_logit_max(lg)); *free_best: over all
// actions (torch.argmax; td_error_of's loop).  Should no action pass (logits that are not numbers), the free arg-max: the index
// stays inside the row.
__device__ __forceinline__ int bcq_choice_of(const float* qo, const float* lg, int n_act, float m, float lt, int* free_best = nullptr) {
  int best = -1, fb = 0;
  float bv = 0.f, fv = qo[0];
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int k = 0; k < n_act; ++k) {  // (selects, no branches: strict comparisons, the first maximum wins)
    const float v = qo[k];
    const bool up = k > 0 && v > fv;
    fv = up ? v : fv;
    fb = up ? k : fb;
    const bool take = bcq_allowed(lg, k, m, lt) && (best < 0 || v > bv);
    bv = take ? v : bv;
    best = take ? k : best;
  }
  if (free_best) *free_best = fb;
  return best < 0 ? fb : best;
}

// a': bcq_choice_of on the online Q(s') of category c under the online logits of s', m the largest of those logits (the same for
// every category of the sample).
__device__ __forceinline__ int bcq_choice(const bcq_kernel_args& a, int b, int c, float m, int* free_best = nullptr) {
  return bcq_choice_of(a.q_after_online + (size_t)b * a.ldq + c * a.n_act, a.q_after_online + (size_t)b * a.ldq + a.n_cat * a.n_act, a.n_act, m,
                       a.lt, free_best);
}

// d = Q(s)[b, c*A + a*] - y, y from the target network at a' in td_error_of's expression order (into *y_out when asked for).  Every
// product and sum rounds on its own (no contraction into a fused multiply-add): what td_loss_kernel's instances evaluate.
__device__ __forceinline__ float bcq_error_of(const bcq_kernel_args& a, int b, int c, int act, float gamma, int best, float* y_out = nullptr) {
#pragma clang fp contract(off)
  const float qb = a.q_before[(size_t)b * a.ldq + c * a.n_act + act];
  float qa = a.q_after_target[(size_t)b * a.ldq + c * a.n_act + best];
  qa = qa * (1.0f - a.term[b * a.n_cat + c]);
  const float r = a.rew[b * a.n_cat + c];
  float y = r + gamma * qa;
  if (a.clip_rect) y = fminf(fmaxf(y, 0.f), 1.f);
  if (y_out) *y_out = y;
  return qb - y;
}

// One walk over a row of behaviour logits lg (m = bcq_logit_max(lg)): the softmax's sum S = sum_a expf(lg_a - m), the sum of
// squares and the first arg-max, a = 0 .. n_act-1 in that order.
__device__ __forceinline__ void bcq_logit_walk(const float* lg, int n_act, float m, float* S_out, float* sq_out, int* first_out) {
  float S = 0.f, sq = 0.f, top = lg[0];
  int first = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  for (int k = 0; k < n_act; ++k) {
    const float v = lg[k];
    S += expf(v - m);
    sq += v * v;
    first = v > top ? k : first;
    top = v > top ? v : top;
  }
  *S_out = S;
  *sq_out = sq;
  *first_out = first;
}

}  // namespace
