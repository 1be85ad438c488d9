"""Prioritized experience replay (Schaul et al., ICLR 2016) over an HBM-resident dataset, sampled and updated on the device.

The reference only samples shuffled epochs (``DataLoader(shuffle=True)``, train_q_network.py:98,114).  With
``PRIORITIZED_REPLAY`` the trainer draws every minibatch from a priority table instead: stratified over the global batch, with
importance weights, and the table is updated from the per-sample TD errors that the weighted loss kernel writes — three small
launches on the compute stream per update, no device-to-host read (video_dqn_amd/csrc/replay.hip has the arithmetic).

Data parallelism keeps N ranks == one process on the big batch: every rank draws the same global batch of G = B x world and takes
its slice; the errors are exchanged as a SUM all-reduce of a zero-filled [G] buffer in which each rank filled its slice, and
every rank applies the same update, so the tables stay bit-identical.
"""
from __future__ import annotations

import torch

from . import _lib

EPS = 1e-6  # priority = (|TD error| + EPS) ^ alpha: a sample whose error is 0 stays drawable
MAX_GLOBAL_BATCH = 4096  # draws per update that vdqn_per_sample resolves (include/vdqn.h)


def check_config(alpha: float, beta: float, global_batch: int, n: int = None) -> None:
    """Raise ValueError for parameters the sampler does not take (host only: no device work).  n = None skips the table size."""
    if not alpha >= 0:
        raise ValueError(f"PER_ALPHA must be >= 0 (got {alpha})")
    if not 0 <= beta <= 1:
        raise ValueError(f"PER_BETA must be in [0, 1] (got {beta})")
    if not 1 <= global_batch <= MAX_GLOBAL_BATCH:
        raise ValueError(f"prioritized replay draws at most {MAX_GLOBAL_BATCH} samples per update: BATCH_SIZE x world size is {global_batch}")
    if n is not None and _lib.load().vdqn_per_workspace_bytes(int(n)) < 0:
        raise ValueError(f"prioritized replay: a table of {n} samples is outside what vdqn_per_sample takes (1 .. 8388608)")


def beta_at(beta0: float, step: int, num_steps: int) -> float:
    """Importance-sampling exponent of update `step`: beta0 annealed linearly to 1 at `num_steps`."""
    return beta0 + (1.0 - beta0) * min(1.0, step / max(1, num_steps))


class PrioritizedSampler:
    """The priority table of an N-sample dataset on `device` and the buffers of one update.

    ``sample(step)`` -> (idx, weight) of THIS rank's B samples (device int64 / f32 views, valid until the next call);
    ``err`` is the rank's [B] slice of the [G] error buffer the weighted loss writes into; ``update()`` applies
    p[i_j] = (e_j + EPS)^alpha for the whole global batch (after the caller's exchange of ``err_all``)."""

    def __init__(self, n: int, batch: int, device, alpha: float = 0.6, beta: float = 0.4, num_steps: int = 100000,
                 seed: int = 0, rank: int = 0, world_size: int = 1):
        check_config(alpha, beta, int(batch) * int(world_size), n)
        self.lib = _lib.load()
        ws = self.lib.vdqn_per_workspace_bytes(int(n))
        self.n, self.B, self.rank, self.world = int(n), int(batch), int(rank), int(world_size)
        self.G = self.B * self.world
        self.alpha, self.beta0, self.num_steps, self.seed = float(alpha), float(beta), int(num_steps), int(seed)
        self.device = torch.device(device)
        with torch.cuda.device(self.device):
            self.prio = torch.ones(self.n, dtype=torch.float32, device=self.device)
            self.workspace = torch.empty(ws, dtype=torch.uint8, device=self.device)
            self.idx_all = torch.zeros(self.G, dtype=torch.int64, device=self.device)
            self.weight_all = torch.ones(self.G, dtype=torch.float32, device=self.device)
            self.err_all = torch.zeros(self.G, dtype=torch.float32, device=self.device)
        lo = self.rank * self.B
        self.idx = self.idx_all[lo:lo + self.B]
        self.weight = self.weight_all[lo:lo + self.B]
        self.err = self.err_all[lo:lo + self.B]

    def beta(self, step: int) -> float:
        return beta_at(self.beta0, step, self.num_steps)

    def sample(self, step: int):
        """Queue the draws of update `step` on the current stream; -> this rank's (idx, weight)."""
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            _lib.check(self.lib.vdqn_per_sample(self.prio.data_ptr(), self.n, self.G, self.seed & (2**64 - 1), int(step) & (2**64 - 1),
                                                self.beta(step), self.workspace.data_ptr(), self.idx_all.data_ptr(),
                                                self.weight_all.data_ptr(), st), "vdqn_per_sample")
            if self.world > 1:
                self.err_all.zero_()  # the exchange SUMs the ranks' slices: the other ranks' entries must be 0 here
        return self.idx, self.weight

    def update(self):
        """p[idx_all[j]] = (err_all[j] + EPS)^alpha on the current stream (behind the loss and, with N ranks, the exchange)."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vdqn_per_update(self.prio.data_ptr(), self.n, self.idx_all.data_ptr(), self.err_all.data_ptr(),
                                                self.G, self.alpha, torch.cuda.current_stream().cuda_stream), "vdqn_per_update")

    def state_dict(self) -> dict:
        return {"priorities": self.prio.detach().float().cpu()}

    def load_state_dict(self, sd: dict) -> None:
        p = torch.as_tensor(sd["priorities"])
        if p.dim() != 1 or p.numel() != self.n:
            raise ValueError(f"replay_state holds {p.numel()} priorities, the dataset has {self.n} samples")
        p = p.to(torch.float32)
        if not bool(torch.isfinite(p).all()) or bool((p < 0).any()) or not bool((p > 0).any()):
            raise ValueError("replay_state priorities must be finite, >= 0 and not all zero")
        self.prio.copy_(p.to(self.device))
