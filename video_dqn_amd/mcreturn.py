"""Monte-Carlo returns over an HBM-resident dataset: per row and category the discounted return the logged video itself obtained
from that row on, folded along the chain that n-step returns walk (video_dqn_amd/nstep.py: successors),

    G(i) = sum_k g^k prod_{j<k}(1 - t(i_j)) r(i_k),       i_0 = i, i_{k+1} = next_row[i_k], ending where the chain ends.

G(i) is known exactly from the labels, and with non-negative rewards it is a lower bound of the optimal value of (s_i, a_i): the
argument nstep.py makes for m <= 16 rows, for the whole episode.  Two uses inside the one TD-loss launch (vdqn_td_loss_mc):

  * ``MC_RETURN_FLOOR``: y <- max(y, G) in front of the rect clip (lower-bound Q-learning / optimality tightening, He et al. 2017;
    Oh et al. 2018).  A row 200 frames before a detection gets a non-zero target in the first update, not after 200 target
    refreshes.
  * ``CQL_CALIBRATED`` (Cal-QL, Nakamoto et al., NeurIPS 2023): the conservative penalty's logsumexp runs over max(Q(s, a), G), so
    the penalty stops pushing values below what the data itself achieved.

The table is built once at start by pointer doubling on the device (video_dqn_amd/csrc/mcreturn.hip has the arithmetic): R rounds
cover the first 2^R rows of every chain.  Nothing of it goes into a checkpoint: a resume rebuilds it from the data, and with N ranks
every rank builds the same bits (no atomics), so no collective is needed.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_CAT = 8      # categories vdqn_mc_returns takes
MAX_ROUNDS = 31  # 2^31 rows per chain: more than an int32 successor table can hold


def rounds_for(gamma: float, n_rows: int) -> int:
    """Rounds of pointer doubling for an n_rows-row table at discount gamma, clamped to [1, MAX_ROUNDS]: the smaller of

      * ceil(log2(max(n_rows, 2))) — a chain without a cycle has fewer than n_rows + 1 rows, so 2^R >= n_rows covers it exactly;
      * for gamma < 1, the smallest R with gamma^(2^R) <= 2^-30 (float64) — what a cycle's tail beyond 2^R rows can still add is
        bounded by that factor times the tail's own return."""
    n = max(int(n_rows), 2)
    r = (n - 1).bit_length()  # ceil(log2(n)) for n >= 2
    gamma = float(gamma)
    if 0.0 <= gamma < 1.0:
        k = 0
        while k < MAX_ROUNDS and gamma ** float(2 ** k) > 2.0 ** -30:
            k += 1
        r = min(r, k)
    return min(max(r, 1), MAX_ROUNDS)


def check_tables(who: str, next_row, rew: torch.Tensor, term: torch.Tensor):
    """-> (rows, n_cat); ValueError naming `who` for tables vdqn_mc_returns does not take."""
    if rew.dtype != torch.float32 or term.dtype != torch.float32 or rew.dim() != 2 or rew.shape != term.shape \
            or not rew.is_contiguous() or not term.is_contiguous():
        raise ValueError(f"{who}: rew and term must be contiguous f32 [N][n_cat] tensors of one shape")
    rows, n_cat = int(rew.shape[0]), int(rew.shape[1])
    if not 1 <= n_cat <= MAX_CAT:
        raise ValueError(f"{who}: {n_cat} categories (vdqn_mc_returns takes 1 .. {MAX_CAT})")
    if next_row.dim() != 1 or next_row.numel() != rows:
        raise ValueError(f"{who}: the successor table has {next_row.numel()} entries, the dataset {rows} rows")
    return rows, n_cat


class ReturnTable:
    """``G`` f32 [N][n_cat] on `device`: the return table of an N-row dataset, built once (R + 1 launches on the current stream);
    the workspace is freed when the constructor returns.  next_row: `nstep.successors`' table (host or device, any integer type);
    rew / term: the store's device tables (f32 [N][n_cat], not written).  rounds: default `rounds_for(gamma, N)`."""

    def __init__(self, next_row, rew: torch.Tensor, term: torch.Tensor, gamma: float, device=None, rounds: int | None = None):
        lib = _lib.load()
        self.device = torch.device(device) if device is not None else rew.device
        nr = torch.as_tensor(np.asarray(next_row) if not torch.is_tensor(next_row) else next_row)
        self.rows, self.n_cat = check_tables("ReturnTable", nr, rew, term)
        self.gamma = float(gamma)
        self.rounds = rounds_for(self.gamma, self.rows) if rounds is None else int(rounds)
        with torch.cuda.device(self.device):
            nr = nr.to(torch.int32).to(self.device).contiguous()
            self.G = torch.empty((self.rows, self.n_cat), dtype=torch.float32, device=self.device)
            ws_bytes = int(lib.vdqn_mc_returns_workspace_bytes(self.rows, self.n_cat))
            ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=self.device)
            _lib.check(lib.vdqn_mc_returns(nr.data_ptr(), rew.data_ptr(), term.data_ptr(), self.rows, self.n_cat, self.gamma, self.rounds,
                                           self.G.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream),
                       "vdqn_mc_returns")
            torch.cuda.current_stream().synchronize()  # (once, at start: the workspace and the int32 table are released right here)
            del ws, nr

    def summary(self):
        """(max, mean) of the table: one read-back, for the trainer's start-up line."""
        return float(self.G.max().item()), float(self.G.double().mean().item())
