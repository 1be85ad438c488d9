"""n-step returns over an HBM-resident dataset: the chain of a sampled row is walked on the device and folded into one reward,
one terminal mask and one discount per sample (video_dqn_amd/csrc/nstep.hip has the arithmetic).

The reference backs a value up by one row per target refresh (train_q_network.py:134-169).  Its data is written one row per frame
i of an episode, (before = i, after = i + 3) (dataset/process_episodes_real.py:138-141), with the reward on the `after` frame and
terminal = reward (dataloaders/q_learning_real.py), so every reward before the first detection of an episode is 0 and a detection's
value moves back one row at a time.  With ``N_STEP: n`` the target of sampled row i0 is the n-fold composition of that backup
along the row's chain i0 -> i1 -> ...:

    y = r(i0) + g (1 - t(i0)) [ r(i1) + g (1 - t(i1)) [ ... g (1 - t(i_{m-1})) Q_target(s^(m), argmax_a Q_online(s^(m), .)) ] ]

per category, m <= n the rows the chain provides, s^(m) the `after` frames of the last row walked.  Every sample still costs one s'
forward.  There is no importance correction (the data carries no behaviour policy): with non-negative rewards "follow the video for
m steps, then act greedily" is a lower bound of the optimal value, so the bias points away from the max-operator's
over-estimation.  Nothing more is claimed.

The successor relation is already in the shard index: ``build_shards`` numbers frames by path, so the row that follows row r is
the row whose first `before` frame is r's first `after` frame (``successors``).  No shard format change.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib

MAX_N = 16  # rows per chain that vdqn_nstep_walk takes: the walk is a chain of dependent loads, one thread per sample
MAX_CAT = 8  # categories that vdqn_nstep_walk keeps in registers


def check_config(n) -> None:
    """Raise ValueError naming N_STEP for a value that is not an integer in 1 .. MAX_N (host only: no device work)."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= MAX_N:
        raise ValueError(f"N_STEP must be an integer in 1 .. {MAX_N} (1 = off, the reference's one-step target), not {n!r}")


def successors(before0, after0) -> np.ndarray:
    """int32 [N]: for every row r the SMALLEST row r' with before0[r'] == after0[r], or -1 when there is none.  before0 / after0 are
    the rows' first `before` / `after` frame numbers (index.npz `before[:, 0]`, `after[:, 0]`).  Sort-based: a stable argsort of
    before0 puts equal frames in row order, so the left insertion point of after0[r] is the smallest matching row.  Self-loops and
    cycles are legal results (the walk is bounded by n)."""
    before0 = np.ascontiguousarray(np.asarray(before0).reshape(-1), dtype=np.int64)
    after0 = np.ascontiguousarray(np.asarray(after0).reshape(-1), dtype=np.int64)
    if before0.shape != after0.shape:
        raise ValueError(f"successors: {before0.shape[0]} before frames, {after0.shape[0]} after frames")
    n = before0.shape[0]
    if n == 0:
        return np.empty(0, dtype=np.int32)
    if n > 2**31 - 1:
        raise ValueError(f"successors: {n} rows do not fit the int32 table")
    order = np.argsort(before0, kind="stable")
    keys = before0[order]
    pos = np.searchsorted(keys, after0, side="left")
    at = np.minimum(pos, n - 1)
    found = (pos < n) & (keys[at] == after0)
    return np.where(found, order[at], -1).astype(np.int32)


def chain_shares(next_row, n: int) -> list:
    """[share of rows whose chain provides exactly k rows, k = 1 .. n] (terminals ignored; a chain of n or more rows counts as n).
    Host arithmetic on the successor table."""
    next_row = np.asarray(next_row).astype(np.int64)
    rows = next_row.shape[0]
    if rows == 0:
        return [0.0] * n
    cur = np.arange(rows, dtype=np.int64)
    alive = np.ones(rows, dtype=bool)
    length = np.ones(rows, dtype=np.int64)
    for _ in range(1, n):
        nxt = next_row[cur]
        alive = alive & (nxt >= 0) & (nxt < rows)
        length += alive
        cur = np.where(alive, nxt, cur)
    counts = np.bincount(length, minlength=n + 1)[1:n + 1]
    return [float(c) / rows for c in counts]


class NStepWalker:
    """The successor table of an N-row dataset on `device` beside its reward / terminal tables, and the output buffers of one
    update's walk.

    ``walk(idx)`` queues one vdqn_nstep_walk launch on the current stream for the B sampled rows `idx` (device int64) and returns
    (rew_n [B, n_cat], term_n [B, n_cat], disc [B], last_row [B] int64, steps [B] int32): device tensors owned by the walker, valid
    until the next call."""

    def __init__(self, next_row, rew: torch.Tensor, term: torch.Tensor, batch: int, n: int, gamma: float, device=None):
        check_config(n)
        self.lib = _lib.load()
        self.device = torch.device(device) if device is not None else rew.device
        if rew.dtype != torch.float32 or term.dtype != torch.float32 or rew.dim() != 2 or rew.shape != term.shape \
                or not rew.is_contiguous() or not term.is_contiguous():
            raise ValueError("NStepWalker: rew and term must be contiguous f32 [N][n_cat] tensors of one shape")
        self.rows, self.n_cat = int(rew.shape[0]), int(rew.shape[1])
        if not 1 <= self.n_cat <= MAX_CAT:
            raise ValueError(f"NStepWalker: {self.n_cat} categories (vdqn_nstep_walk takes 1 .. {MAX_CAT})")
        nr = torch.as_tensor(np.asarray(next_row) if not torch.is_tensor(next_row) else next_row)
        if nr.dim() != 1 or nr.numel() != self.rows:
            raise ValueError(f"NStepWalker: the successor table has {nr.numel()} entries, the dataset {self.rows} rows")
        self.n, self.gamma, self.B = int(n), float(gamma), int(batch)
        self.rew, self.term = rew, term
        with torch.cuda.device(self.device):
            self.next_row = nr.to(torch.int32).to(self.device).contiguous()
            self.rew_n = torch.zeros((self.B, self.n_cat), dtype=torch.float32, device=self.device)
            self.term_n = torch.zeros((self.B, self.n_cat), dtype=torch.float32, device=self.device)
            self.disc = torch.zeros(self.B, dtype=torch.float32, device=self.device)
            self.last_row = torch.zeros(self.B, dtype=torch.int64, device=self.device)
            self.steps = torch.zeros(self.B, dtype=torch.int32, device=self.device)

    def walk(self, idx: torch.Tensor):
        if idx.dtype != torch.int64 or idx.numel() != self.B or not idx.is_contiguous() or idx.device != self.next_row.device:
            raise ValueError(f"NStepWalker.walk: idx must be a contiguous int64 [{self.B}] tensor on {self.next_row.device}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vdqn_nstep_walk(idx.data_ptr(), self.B, self.next_row.data_ptr(), self.rew.data_ptr(), self.term.data_ptr(),
                                                self.rows, self.n_cat, self.n, self.gamma, self.rew_n.data_ptr(), self.term_n.data_ptr(),
                                                self.disc.data_ptr(), self.last_row.data_ptr(), self.steps.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "vdqn_nstep_walk")
        return self.rew_n, self.term_n, self.disc, self.last_row, self.steps
