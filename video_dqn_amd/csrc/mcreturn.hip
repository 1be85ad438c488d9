// Monte-Carlo return table: the discounted return the logged data itself obtained from every row, folded along the chain that
// nstep.hip walks (next_row, video_dqn_amd/nstep.py: successors), per category:
//
//   G(i) = sum_{k < 2^R} g^k prod_{j<k}(1 - t(i_j)) r(i_k),   i_0 = i, i_{k+1} = next_row[i_k], ending where the chain ends
//
// With non-negative rewards G(i) is a lower bound of the optimal value of (s_i, a_i): the floor and the calibration of the TD-loss
// launch (pointwise.hip, vdqn_td_loss_mc).  A walk per row would be 2^R dependent loads for each of N rows; the table is built by
// pointer doubling instead, R rounds of one gather each.  State per row: (j, A[c], B[c]) — the row 2^k steps ahead, the product of
// g (1 - t) over the 2^k rows from this one, and the return over those rows.
//
//   initial state (one launch):  j = next_row[i] (any value < 0 or >= N becomes -1),  B[c] = r[i][c],  A[c] = g * (1 - t[i][c])
//                                (the subtraction rounds, then the product)
//   one round (one launch), j = j_old[i]:
//     j >= 0:  B'[c] = B[c] + (A[c] * B_old[j][c]),  A'[c] = A[c] * A_old[j][c],  j' = j_old[j]
//     j <  0:  B'[c] = B[c],                         A'[c] = 0,                   j' = -1
//
// Every product and every sum rounds on its own (contraction off), so tests/mc_oracle.py reproduces the bits in numpy float32.
// After R rounds B is G.  A round reads one buffer set and writes the other (a round that updated in place would read rows that
// other threads have already advanced): set 0 is (j0, A0, G), set 1 is (j1, A1, B1); the initial state goes to set R & 1, so that
// round R writes set 0 and with it G.  The last round writes B alone.  One thread per ROW: it loads j once, walks the n_cat <= 8
// categories of its row (contiguous floats, as are those of row j) and writes j' once.  No atomics, no LDS, plain vector stores;
// rew, term and next_row are only read.  Self-loops and cycles are legal: a cycle's rows keep adding their tail, which gamma < 1
// bounds (video_dqn_amd/mcreturn.py: rounds_for).  All offsets are 64-bit: N * n_cat may pass 2^31.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxCat = 8;
constexpr int kMaxRounds = 31;

struct mc_set {
  int32_t* j;
  float* A;
  float* B;
};

__global__ __launch_bounds__(256) void mc_init_kernel(const int32_t* __restrict__ next_row, const float* __restrict__ rew,
                                                      const float* __restrict__ term, int64_t N, int n_cat, float gamma, mc_set out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t nxt = next_row[i];
  out.j[i] = (nxt < 0 || (int64_t)nxt >= N) ? -1 : nxt;
  const size_t o = (size_t)i * n_cat;
  for (int c = 0; c < n_cat; ++c) {
    out.B[o + c] = rew[o + c];
    out.A[o + c] = gamma * (1.0f - term[o + c]);
  }
}

__global__ __launch_bounds__(256) void mc_round_kernel(const int32_t* __restrict__ j_old, const float* __restrict__ A_old,
                                                       const float* __restrict__ B_old, int64_t N, int n_cat, int last, mc_set out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t j = j_old[i];  // the initial state holds -1 or a row of the table: nothing else is ever stored
  const size_t o = (size_t)i * n_cat;
  if (j >= 0) {
    const size_t oj = (size_t)j * n_cat;
    for (int c = 0; c < n_cat; ++c) {
      const float a = A_old[o + c];
      out.B[o + c] = B_old[o + c] + (a * B_old[oj + c]);
      if (!last) out.A[o + c] = a * A_old[oj + c];
    }
    if (!last) out.j[i] = j_old[j];
  } else {
    for (int c = 0; c < n_cat; ++c) {
      out.B[o + c] = B_old[o + c];
      if (!last) out.A[o + c] = 0.0f;
    }
    if (!last) out.j[i] = -1;
  }
}

}  // namespace

// 2 x j (int32 [N]) + 2 x A + 1 x B (f32 [N][n_cat]): the other B is the output itself
extern "C" int64_t vdqn_mc_returns_workspace_bytes(int64_t n_rows, int32_t n_cat) {
  if (n_rows < 1 || n_rows > 2147483647ll || n_cat < 1 || n_cat > kMaxCat) return -1;
  return 4ll * (2ll * n_rows + 3ll * n_rows * n_cat);
}

extern "C" int vdqn_mc_returns(const int32_t* next_row, const float* rew, const float* term, int64_t n_rows, int32_t n_cat, float gamma,
                               int32_t rounds, float* G, void* workspace, int64_t workspace_bytes, void* stream) {
  VDQN_CHECK(next_row && rew && term && G && workspace, "vdqn_mc_returns: null arg");
  VDQN_CHECK(n_rows >= 1 && n_rows <= 2147483647ll, "vdqn_mc_returns: n_rows = %lld outside [1, 2^31 - 1] (next_row is int32)", (long long)n_rows);
  VDQN_CHECK(n_cat >= 1 && n_cat <= kMaxCat, "vdqn_mc_returns: n_cat %d outside [1, %d]", n_cat, kMaxCat);
  VDQN_CHECK(rounds >= 1 && rounds <= kMaxRounds, "vdqn_mc_returns: rounds %d outside [1, %d]", rounds, kMaxRounds);
  VDQN_CHECK(isfinite(gamma), "vdqn_mc_returns: gamma %g is not finite", (double)gamma);
  const int64_t need = vdqn_mc_returns_workspace_bytes(n_rows, n_cat);
  VDQN_CHECK(workspace_bytes >= need, "vdqn_mc_returns: workspace of %lld bytes, vdqn_mc_returns_workspace_bytes gives %lld", (long long)workspace_bytes,
             (long long)need);
  VDQN_CHECK(((uintptr_t)workspace & 3) == 0, "vdqn_mc_returns: workspace must be 4-byte aligned");
  const size_t nc = (size_t)n_rows * n_cat;
  int32_t* j0 = (int32_t*)workspace;
  float* f = (float*)(j0 + 2 * (size_t)n_rows);
  const mc_set set[2] = {{j0, f, G}, {j0 + n_rows, f + nc, f + 2 * nc}};
  const dim3 grid((unsigned)((n_rows + 255) / 256)), block(256);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps_("mc_returns", 0.0, (double)nc * (16.0 + 24.0 * rounds) + (double)n_rows * (8.0 + 12.0 * rounds), st);
  int cur = rounds & 1;
  hipLaunchKernelGGL(mc_init_kernel, grid, block, 0, st, next_row, rew, term, n_rows, (int)n_cat, gamma, set[cur]);
  VDQN_LAUNCH_CHECK();
  for (int k = 1; k <= rounds; ++k) {
    hipLaunchKernelGGL(mc_round_kernel, grid, block, 0, st, (const int32_t*)set[cur].j, (const float*)set[cur].A, (const float*)set[cur].B,
                       n_rows, (int)n_cat, (int)(k == rounds), set[cur ^ 1]);
    VDQN_LAUNCH_CHECK();
    cur ^= 1;
  }
  return VDQN_OK;
}
