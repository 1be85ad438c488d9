"""Held-out validation of the Q trainer: what the reference reserves and never fills (``metrics = {'losses': [],
'eval_losses': []}``, train_q_network.py:183-186, and ``# checkpoint and eval``, :240).

Every VAL_INTERVAL updates rank 0 walks the validation set in index order, in batches of BATCH_SIZE (the last short batch
included), without augmentation or importance weights, through ``TDStepper.eval_begin / eval_batch / eval_result``: two forward
passes and one metrics launch per batch, the sums kept in a small f64 table on the device and read back once per pass.  Under a
head algorithm (video_dqn_amd/algos.py) a second launch per batch sums the algorithm's own metrics into a second table, read back in
the same synchronisation and written as <slot name>/val beside the scalars below.  The pass
indexes the dataset directly and draws nothing from torch's or numpy's global generators, so the training run's later shuffles —
and with them its parameters — are those of the same run without validation.
"""
from __future__ import annotations

import numpy as np
import torch

from .algos import eval_tags
from .dataset import QLearningRealDataset, SyntheticTupleDataset
from .shards import ShardDataset, is_shard_dir

# scalar tag -> key of TDStepper.eval_result()
SCALARS = (("avg_q_loss/val", "loss"), ("td_abs_error/val", "td_abs_error"), ("q_data/val", "q_data"), ("q_max/val", "q_max"),
           ("td_target/val", "td_target"), ("cql_penalty/val", "cql_penalty"), ("action_agreement/val", "action_agreement"))
SYNTHETIC_LENGTH = 1024  # samples of VAL_DATASET: 'synthetic'


def check_config(config) -> None:
    """VAL_DATASET / VAL_INTERVAL / VAL_BATCHES: raise ValueError naming the key (before any device work)."""
    path = getattr(config, "VAL_DATASET", "")
    if not isinstance(path, str):
        raise ValueError(f"VAL_DATASET must be a string ('' = off, 'synthetic', or a dataset path as DATASET takes it), not {path!r}")
    for key in ("VAL_INTERVAL", "VAL_BATCHES"):
        v = getattr(config, key, 0)
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{key} must be an integer >= 0 (0 = {'off' if key == 'VAL_INTERVAL' else 'the whole validation set'}), not {v!r}")
    if getattr(config, "VAL_INTERVAL", 0) > 0:
        if not path:
            raise ValueError("VAL_INTERVAL > 0 needs VAL_DATASET: a dataset path as DATASET takes it, or 'synthetic'")
        if getattr(config, "TRAIN_ON_GROUND_TRUTH", False):
            raise ValueError("VAL_INTERVAL > 0 needs the TD branch: TRAIN_ON_GROUND_TRUTH regresses on given targets and has no "
                             "target network or TD error to validate")


def open_dataset(config):
    """The dataset VAL_DATASET names, built with the flags the training set takes."""
    path = config.VAL_DATASET
    if path == "synthetic":
        nf = config.NUM_FRAMES or (4 if (config.PANORAMA or config.PREVIOUS_IMAGES) else 1)
        return SyntheticTupleDataset(length=SYNTHETIC_LENGTH, num_frames=nf,
                                     action_dim=1 if (config.VALUE_LEARNING or config.ONE_ACTION) else 3, seed=int(config.SEED) + 1)
    kw = dict(one_action=True, confidence_reward=config.CONFIDENCE_REWARD, value_learning=config.VALUE_LEARNING,
              inverse_actions=config.USE_INVERSE_ACTIONS, previous_images=config.PREVIOUS_IMAGES)
    if is_shard_dir(path):
        return ShardDataset(path, **kw)
    return QLearningRealDataset(path, as_uint8=True, **kw)


def _collate(items):
    """The 7-tuples of consecutive indices as one batch (torch's default collate without the DataLoader around it)."""
    before, after, act, rew, term, gt, valid = zip(*items)
    arr = lambda xs: torch.from_numpy(np.stack([np.asarray(x) for x in xs]))  # noqa: E731
    return torch.stack(before), torch.stack(after), arr(act), arr(rew), arr(term), arr(gt), arr(valid)


def _to_device(batch, device):
    """Host -> device per batch, with plain (blocking) copies: validation is not the hot loop."""
    before, after, act, rew, term, _, valid = batch
    src_kind = 0 if before.dtype == torch.uint8 else 1
    if src_kind == 1:
        before, after = before.float(), after.float()
    f32 = lambda t: t.float().contiguous().to(device)  # noqa: E731
    return (before.contiguous().to(device), after.contiguous().to(device), src_kind, act.to(torch.int64).to(device), f32(rew), f32(term),
            f32(valid))


class Validator:
    """The validation set of one run and the pass over it."""

    def __init__(self, config, log=print):
        self.dataset = open_dataset(config)
        self.batch_size = int(config.BATCH_SIZE)
        self.interval, self.max_batches = int(config.VAL_INTERVAL), int(config.VAL_BATCHES)
        self.use_valid = bool(config.REMOVE_BEFORE_REWARD)
        n = len(self.dataset)
        self.n_batches = (n + self.batch_size - 1) // self.batch_size
        if self.max_batches > 0:
            self.n_batches = min(self.n_batches, self.max_batches)
        log(f"validation every {self.interval} updates: {min(n, self.n_batches * self.batch_size)} of {n} samples from "
            f"{config.VAL_DATASET} in {self.n_batches} batches of {self.batch_size}, metrics summed on the GPU and read back once per pass")

    def due(self, sample_number: int) -> bool:
        return self.interval > 0 and sample_number % self.interval == 0

    def run(self, stepper, sample_number: int, writer=None) -> dict:
        """One pass behind update `sample_number` on the current stream; appends (sample_number, result) to stepper.val_history and
        writes the scalars at `sample_number`."""
        device, n, B = stepper.net.device, len(self.dataset), self.batch_size
        stepper.eval_begin()
        for i in range(self.n_batches):
            lo, hi = i * B, min((i + 1) * B, n)
            before, after, src_kind, act, rew, term, valid = _to_device(_collate([self.dataset[j] for j in range(lo, hi)]), device)
            stepper.eval_batch(before, after, src_kind, act, rew, term, valid if self.use_valid else None)
        result = stepper.eval_result()
        stepper.val_history.append((sample_number, result))
        if writer is not None:
            for tag, key in SCALARS:
                writer.add_scalar(tag, result[key], sample_number)
            for c, v in enumerate(result["loss_cat"]):
                writer.add_scalar(f"avg_q_loss_cat{c}/val", v, sample_number)
            if "head" in result:  # the head algorithm's row: its slots' names are the tags
                for tag, key in eval_tags(stepper.algo):
                    writer.add_scalar(tag, result["head"][key], sample_number)
        return result
