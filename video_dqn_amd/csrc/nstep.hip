// n-step returns along a sampled row's chain: the n-fold composition of the one-step backup of train_q_network.py:134-169, folded
// into one reward, one terminal mask and one discount per sample, so that the loss launch (pointwise.hip, td_error_of) still sees
// "r + discount * (1 - t) * Q_target(s', argmax_a Q_online(s', .))" — with s' the `after` frames of the LAST row walked:
//
//   y = r(i0) + g (1 - t(i0)) [ r(i1) + g (1 - t(i1)) [ ... g (1 - t(i_{m-1})) Q(s^(m)) ] ]            per category
//     = rew_n + disc * (1 - term_n) * Q(s^(m)),   rew_n = sum_k g^k prod_{j<k}(1 - t(i_j)) r(i_k),   1 - term_n = prod_{j<m}(1 - t(i_j)),
//       disc = g^m
//
// The chain is the successor table next_row[N] (video_dqn_amd/nstep.py: the row whose first `before` frame is this row's first
// `after` frame, -1 for none).  One thread per sample; a walk is a chain of dependent loads, bounded by n <= kMaxSteps.  Every
// product and sum rounds on its own (contraction off), in this order, so tests/nstep_oracle.py reproduces the bits in numpy float32:
//
//   row = clamp(idx[b], 0, N-1);  w_c = 1, g_c = 0 (c < n_cat), pw = 1, m = 0
//   repeat:
//     for c:  g_c = g_c + (pw * w_c) * rew[row][c];   w_c = w_c * (1 - term[row][c])
//     pw = pw * gamma;  m += 1;  last = row
//     if m == n: stop
//     nxt = next_row[row];  if nxt < 0 or nxt >= N: stop            (any int32 is safe: -7, N, 2^31-1 all mean "none")
//     if every w_c == 0: stop                                       (nothing further can reach the target)
//     row = nxt
//   rew_n[b][c] = g_c;  term_n[b][c] = 1 - w_c;  disc[b] = pw;  last_row[b] = last;  steps[b] = m
//
// Self-loops and cycles in next_row are legal: the walk ends at n rows whatever the table holds.  With n = 1 the outputs are the
// row's own rew, 1 - (1 - term) and gamma.  No atomics, no LDS, plain vector stores.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxCat = 8;     // categories kept in registers
constexpr int kMaxSteps = 16;  // rows per chain

__global__ __launch_bounds__(256) void nstep_walk_kernel(const int64_t* __restrict__ idx, int batch, const int32_t* __restrict__ next_row,
                                                         const float* __restrict__ rew, const float* __restrict__ term, int64_t N, int n_cat,
                                                         int n, float gamma, float* __restrict__ rew_n, float* __restrict__ term_n,
                                                         float* __restrict__ disc, int64_t* __restrict__ last_row, int32_t* __restrict__ steps) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  int64_t row = idx[b];
  row = row < 0 ? 0 : (row >= N ? N - 1 : row);
  float w[kMaxCat], g[kMaxCat];
#pragma unroll
  for (int c = 0; c < kMaxCat; ++c) {
    w[c] = 1.0f;
    g[c] = 0.0f;
  }
  float pw = 1.0f;
  int m = 0;
  int64_t last = row;
  for (;;) {
    const float* r = rew + row * n_cat;
    const float* t = term + row * n_cat;
    bool live = false;
#pragma unroll
    for (int c = 0; c < kMaxCat; ++c) {
      if (c < n_cat) {
        g[c] = g[c] + (pw * w[c]) * r[c];
        w[c] = w[c] * (1.0f - t[c]);
        live = live || w[c] != 0.0f;
      }
    }
    pw = pw * gamma;
    ++m;
    last = row;
    if (m == n) break;
    const int64_t nxt = next_row[row];
    if (nxt < 0 || nxt >= N) break;
    if (!live) break;
    row = nxt;
  }
#pragma unroll
  for (int c = 0; c < kMaxCat; ++c) {
    if (c < n_cat) {
      rew_n[(size_t)b * n_cat + c] = g[c];
      term_n[(size_t)b * n_cat + c] = 1.0f - w[c];
    }
  }
  disc[b] = pw;
  last_row[b] = last;
  steps[b] = m;
}

}  // namespace

extern "C" int vdqn_nstep_walk(const int64_t* idx, int32_t batch, const int32_t* next_row, const float* rew, const float* term, int64_t n_rows,
                               int32_t n_cat, int32_t n, float gamma, float* rew_n, float* term_n, float* disc, int64_t* last_row,
                               int32_t* steps, void* stream) {
  VDQN_CHECK(idx && next_row && rew && term && rew_n && term_n && disc && last_row && steps, "vdqn_nstep_walk: null arg");
  VDQN_CHECK(batch >= 1, "vdqn_nstep_walk: batch %d < 1", batch);
  VDQN_CHECK(n_rows >= 1 && n_rows <= 2147483647ll, "vdqn_nstep_walk: n_rows = %lld outside [1, 2^31 - 1] (next_row is int32)", (long long)n_rows);
  VDQN_CHECK(n_cat >= 1 && n_cat <= kMaxCat, "vdqn_nstep_walk: n_cat %d outside [1, %d]", n_cat, kMaxCat);
  VDQN_CHECK(n >= 1 && n <= kMaxSteps, "vdqn_nstep_walk: n %d outside [1, %d]", n, kMaxSteps);
  VDQN_CHECK(isfinite(gamma), "vdqn_nstep_walk: gamma %g is not finite", (double)gamma);
  ProfScope ps_("nstep_walk", 0.0, (double)batch * (8.0 + (double)n * (4.0 + 8.0 * n_cat) + 8.0 * n_cat + 16.0), (hipStream_t)stream);
  hipLaunchKernelGGL(nstep_walk_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, idx, (int)batch, next_row, rew, term, n_rows,
                     (int)n_cat, (int)n, gamma, rew_n, term_n, disc, last_row, steps);
  VDQN_LAUNCH_CHECK();
  return VDQN_OK;
}
