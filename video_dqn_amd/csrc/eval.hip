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
#include <math.h>

#include "common.h"

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
