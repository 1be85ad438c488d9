"""The Q-learning training loop with the reference's control flow and on-disk artefacts
(``train_q_network.py:84-250``), running every device-side step on the HIP engine.

Kept from the reference: seeding (:86-87), dataset/DataLoader construction (:98-114; batch size is a config
key here), model + target + Adam (:119-124), resume (:192-198), target sync before the update when
``sample_number % TARGET_UPDATE_INTERVAL == 0`` (:215-216), EMA of the loss and its tensorboard scalar
(:228-238), checkpoint dict and file name (:241-247).  Not kept: the crash after the first checkpoint
(:248-250) and the per-step host sync of ``loss.item()`` — the loss is read back one step late
from pinned memory so the GPU never idles.
"""
from __future__ import annotations

import os
from collections import OrderedDict, namedtuple
from functools import partial

import numpy as np
import torch
from torch.utils import data

from . import algos
from .augment import COLOR_KEYS, Augmenter, jr, jz
from .dataset import QLearningRealDataset, SyntheticTupleDataset
from .dist import BucketAllReduce, agree_all, broadcast_replica_state
from .engine import TDStepper
from .model import build_model, head_of
from .optim import lr_at, schedule_active
from .shards import (FRAME_BYTES, Batch, DeviceFrameStore, HostFrameStream, RankShardedFrameStore, ShardDataset, collate_batches,
                     is_shard_dir)
from .validate import Validator


def loopLoader(loader, on_reset=None):
    """train_q_network.py:60-67."""
    i = iter(loader)
    epoch = 0
    while True:
        try:
            yield next(i)
        except StopIteration:
            print("reset iterator")
            epoch += 1
            if on_reset:
                on_reset(epoch)
            i = iter(loader)


# ---- checkpoint: exactly the reference's dict (train_q_network.py:241-247) --------------------------------
def optimizer_state_dict(stepper: TDStepper) -> dict:
    """torch.optim.Adam.state_dict() layout: ids follow model.parameters() order (70 ids; resnet.fc = 60, 61
    never receives a gradient, so it has no state — as in the reference)."""
    net = stepper.net
    state = {}
    if stepper.adam_step > 0:
        for s in net.slots.values():
            if s.kind != 0 or s.name in head_of(net)[1]:  # (an extra head's moments: head_state)
                continue
            sl = slice(s.offset, s.offset + s.numel)
            state[s.param_id] = {"step": stepper.adam_step,
                                 "exp_avg": stepper.exp_avg[sl].view(s.shape).clone(),
                                 "exp_avg_sq": stepper.exp_avg_sq[sl].view(s.shape).clone()}
    n_params = sum(1 for s in net.slots.values() if s.kind in (0, 1) and s.name not in head_of(net)[1])
    # (GRAD_CLIP_NORM / WEIGHT_DECAY / LR_*: `lr` is the rate of the last update, `weight_decay` the AdamW factor, and `initial_lr`
    # — the key torch's schedulers add — is there only while a schedule is active: a default-config checkpoint keeps its exact keys)
    group = {"lr": stepper.lr, "betas": tuple(stepper.betas), "eps": stepper.eps, "weight_decay": getattr(stepper, "weight_decay", 0) or 0,
             "amsgrad": False}
    if getattr(stepper, "lr_fn", None) is not None:
        group["initial_lr"] = stepper.initial_lr
    group["params"] = list(range(n_params))
    return {"state": dict(sorted(state.items())), "param_groups": [group]}


def load_optimizer_state_dict(stepper: TDStepper, sd: dict) -> None:
    net = stepper.net
    by_id = {s.param_id: s for s in net.slots.values() if s.kind == 0 and s.name not in head_of(net)[1]}
    step = 0
    with torch.no_grad():
        for pid, st in sd["state"].items():
            s = by_id[int(pid)]
            sl = slice(s.offset, s.offset + s.numel)
            stepper.exp_avg[sl].copy_(st["exp_avg"].reshape(-1))
            stepper.exp_avg_sq[sl].copy_(st["exp_avg_sq"].reshape(-1))
            step = int(st["step"])
    stepper.adam_step = step
    g = sd["param_groups"][0]
    stepper.lr, stepper.betas, stepper.eps = g["lr"], tuple(g["betas"]), g["eps"]


def reference_state_dict(model) -> "OrderedDict[str, torch.Tensor]":
    """model.state_dict() without an extra head's tensors (value.*, spread.*): the reference's keys in the reference's shapes and
    order."""
    sd = model.state_dict()  # (without an extra head: the dict as it is)
    for k in head_of(model.engine)[1]:
        sd.pop(k, None)
    getattr(sd, "_metadata", {}).pop(getattr(model.engine, "head", None), None)
    return sd


def head_state(stepper: TDStepper, with_target: bool = False) -> dict:
    """IQL_EXPECTILE / DISTRIBUTIONAL: the extra head's parameters and Adam moments, what `model_state_dict` and
    `optimizer_state_dict` leave out so that the reference's class and its Adam load those two as they always did:
    {"state_dict": {"<head>.weight", "<head>.bias"}, "optimizer_state": {name: {step, exp_avg, exp_avg_sq}}} (no moments before the
    first update, as in torch).  with_target (the spread head under TARGET_TAU > 0, whose target rows the loss reads): also
    "target_state_dict", the head's rows of the averaged target weights."""
    net = stepper.net
    out = {"state_dict": OrderedDict(), "optimizer_state": {}}
    if with_target:
        out["target_state_dict"] = OrderedDict()
    for name in head_of(net)[1]:
        s = net.slots[name]
        sl = slice(s.offset, s.offset + s.numel)
        out["state_dict"][name] = net.params[sl].view(s.shape).clone()
        if stepper.adam_step > 0:
            out["optimizer_state"][name] = {"step": stepper.adam_step, "exp_avg": stepper.exp_avg[sl].view(s.shape).clone(),
                                            "exp_avg_sq": stepper.exp_avg_sq[sl].view(s.shape).clone()}
        if with_target:
            out["target_state_dict"][name] = stepper.target_params[sl].view(s.shape).clone()
    return out


def load_head_state(stepper: TDStepper, state: dict) -> None:
    """A `head_state` into the engine's parameters and the stepper's moments (behind load_optimizer_state_dict, which sets the step
    count).  Its "target_state_dict", when there, goes into `stepper.target_params` through load_target_state_dict."""
    net = stepper.net
    with torch.no_grad():
        for name in head_of(net)[1]:
            s = net.slots[name]
            sl = slice(s.offset, s.offset + s.numel)
            net.params[sl].copy_(state["state_dict"][name].to(torch.float32).reshape(-1))
            st = state.get("optimizer_state", {}).get(name)
            if st is not None:
                stepper.exp_avg[sl].copy_(st["exp_avg"].reshape(-1))
                stepper.exp_avg_sq[sl].copy_(st["exp_avg_sq"].reshape(-1))
    net.mark_dirty()


value_head_state, load_value_head_state = head_state, load_head_state  # (the names the value head came with)


def target_state_dict(stepper: TDStepper, model) -> "OrderedDict[str, torch.Tensor]":
    """TARGET_TAU > 0: the Polyak-averaged target weights as a state_dict with the model's own keys, names and shapes — every
    parameter from `stepper.target_params` through the engine's slot table, every BatchNorm buffer as the online network holds it
    (statistics are copied, not averaged) — so the reference's class loads it as the smoothed network."""
    net = stepper.net
    out = OrderedDict()
    for name, value in reference_state_dict(model).items():  # (reference keys only: an extra head's target rows travel in head_state)
        s = net.slots.get(name)
        if s is not None and s.kind in (0, 1):
            out[name] = stepper.target_params[s.offset:s.offset + s.numel].view(s.shape).clone()
        else:
            out[name] = value.clone()
    return out


def load_target_state_dict(stepper: TDStepper, sd, head_sd=None) -> None:
    """The parameters of a `target_state_dict` into `stepper.target_params`, then `packed_target` folded from them again.  head_sd:
    the extra head's target rows (head_state's "target_state_dict"); without it sync_target's copy of them stays — never read for
    value.*, the online spread.* for a checkpoint written without them."""
    net = stepper.net
    with torch.no_grad():
        for s in net.slots.values():
            if s.kind in (0, 1) and s.name not in head_of(net)[1]:
                stepper.target_params[s.offset:s.offset + s.numel].copy_(sd[s.name].to(torch.float32).reshape(-1))
            elif head_sd is not None and s.name in head_sd:
                stepper.target_params[s.offset:s.offset + s.numel].copy_(head_sd[s.name].to(torch.float32).reshape(-1))
    with torch.cuda.device(net.device):
        net.pack_weights(stepper.packed_target, with_dgrad=False, params=stepper.target_params)


def save_checkpoint(path, sample_number, model, stepper, replay_state=None, target_state_dict=None):
    """replay_state (PRIORITIZED_REPLAY): {'priorities': f32 CPU tensor [N]}, stored under its own key next to the reference's
    three, which stay as they are (load_model_number and the reference class read the file as before).  target_state_dict
    (TARGET_TAU > 0): the averaged target weights in the model's names and shapes, likewise under a key of its own."""
    ckpt = {"sample_number": sample_number,
            "model_state_dict": reference_state_dict(model),
            "optimizer_state_dict": optimizer_state_dict(stepper)}
    head_key = head_of(stepper.net)[0]
    if head_key:  # IQL_EXPECTILE / DISTRIBUTIONAL: the extra head beside the reference's three keys, not inside them
        ckpt[head_key] = head_state(stepper, with_target=(head_key == "spread_head" and target_state_dict is not None))
    if replay_state is not None:
        ckpt["replay_state"] = replay_state
    if target_state_dict is not None:
        ckpt["target_state_dict"] = target_state_dict
    torch.save(ckpt, path)


def check_prioritized_replay(config, world_size: int = 1) -> None:
    """PRIORITIZED_REPLAY applies to the TD branch on a decoded-frame shard dataset held in HBM: raise (before any device work)
    for every configuration it does not cover, naming the reason (the dataset's size and HBM fit are checked once it is opened)."""
    from .replay import check_config
    check_config(float(config.PER_ALPHA), float(config.PER_BETA), int(config.BATCH_SIZE) * world_size)
    if config.TRAIN_ON_GROUND_TRUTH:
        raise ValueError("PRIORITIZED_REPLAY needs the TD branch: TRAIN_ON_GROUND_TRUTH has no TD error to prioritise samples by")
    if config.SYNTHETIC_DATA or config.DATASET in ("none", "synthetic"):
        raise ValueError("PRIORITIZED_REPLAY needs a fixed dataset: SYNTHETIC_DATA generates its tuples on the fly")
    if not is_shard_dir(config.DATASET):
        raise ValueError("PRIORITIZED_REPLAY needs a decoded-frame shard dataset held in HBM, not a feather+JPEG dataset "
                         "(build one with python -m video_dqn_amd.shards)")
    if str(getattr(config, "DEVICE_RESIDENT_DATA", "auto")).lower() == "off":
        raise ValueError("PRIORITIZED_REPLAY draws any sample at any update: it needs the frames in HBM, "
                         "and DEVICE_RESIDENT_DATA is 'off'")


def check_augment(pad, flip, flip_actions, brightness=0.0, contrast=0.0, saturation=0.0, zoom=0.0, zoom_aspect=False, rotate=0.0) -> None:
    """AUG_SHIFT_PAD / AUG_FLIP / AUG_FLIP_ACTIONS / AUG_BRIGHTNESS / AUG_CONTRAST / AUG_SATURATION / AUG_ZOOM / AUG_ZOOM_ASPECT / AUG_ROTATE:
    raise ValueError naming the key (before any device work)."""
    from .augment import check_config
    check_config(pad, flip, flip_actions, brightness, contrast, saturation, zoom, zoom_aspect, rotate)


def check_optim(config) -> None:
    """GRAD_CLIP_NORM / WEIGHT_DECAY / LR_WARMUP_STEPS / LR_SCHEDULE / LR_FINAL_FRACTION: raise ValueError naming the key (before any
    device work)."""
    from .optim import check_config
    check_config(getattr(config, "GRAD_CLIP_NORM", 0.0), getattr(config, "WEIGHT_DECAY", 0.0), getattr(config, "LR_WARMUP_STEPS", 0),
                 getattr(config, "LR_SCHEDULE", "constant"), getattr(config, "LR_FINAL_FRACTION", 0.0), int(config.NUM_STEPS))


def check_cql(config) -> None:
    """CQL_ALPHA: raise ValueError naming the key (before any device work) for a value that is not a finite number >= 0 and, when it
    is on, for the configurations the penalty does not cover: the ground-truth branch and a network with one action column."""
    import math
    alpha = getattr(config, "CQL_ALPHA", 0.0)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha) or alpha < 0:
        raise ValueError(f"CQL_ALPHA must be a finite number >= 0 (0 = off), not {alpha!r}")
    if alpha > 0:
        if getattr(config, "TRAIN_ON_GROUND_TRUTH", False):
            raise ValueError("CQL_ALPHA needs the TD branch: TRAIN_ON_GROUND_TRUTH regresses Q(s, a) on given targets and bootstraps nothing")
        for key in ("VALUE_LEARNING", "ONE_ACTION"):
            if getattr(config, key, False):
                raise ValueError(f"CQL_ALPHA needs more than one action: {key} builds a network with one action column, "
                                 "where logsumexp_a Q(s, .) - Q(s, a) is identically zero")


def check_target(config) -> None:
    """TARGET_TAU: raise ValueError naming the key (before any device work) for a value that is not a finite number in [0, 1] and,
    when it is on, for the ground-truth branch, which has no target network."""
    import math
    tau = getattr(config, "TARGET_TAU", 0.0)
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau) or tau < 0 or tau > 1:
        raise ValueError(f"TARGET_TAU must be a finite number in [0, 1] (0 = hard copies every TARGET_UPDATE_INTERVAL), not {tau!r}")
    if tau > 0 and getattr(config, "TRAIN_ON_GROUND_TRUTH", False):
        raise ValueError("TARGET_TAU needs the TD branch: TRAIN_ON_GROUND_TRUTH regresses on given targets and has no target network")


def check_full_store(config, key: str, why: str) -> None:
    """The refusals shared by every key that needs row indices into a full DeviceFrameStore (N_STEP > 1, MC_RETURN_FLOOR,
    CQL_CALIBRATED): ValueError naming `key` (before any device work) for the ground-truth branch, LINEAR, generated tuples, a
    feather+JPEG dataset and DEVICE_RESIDENT_DATA 'off'.  `why` says what the key needs the store for."""
    if getattr(config, "TRAIN_ON_GROUND_TRUTH", False):
        raise ValueError(f"{key} needs the TD branch: TRAIN_ON_GROUND_TRUTH regresses Q(s, a) on given targets and bootstraps nothing")
    if getattr(config, "LINEAR", False):
        raise ValueError(f"{key} does not cover LINEAR: y = r + (Qa - 0.1) has no discount, so neither an n-step form nor a discounted return to compare with")
    if getattr(config, "SYNTHETIC_DATA", False) or config.DATASET in ("none", "synthetic"):
        raise ValueError(f"{key} needs a fixed dataset with a successor relation: SYNTHETIC_DATA generates unrelated tuples on the fly")
    if not is_shard_dir(config.DATASET):
        raise ValueError(f"{key} needs a decoded-frame shard dataset held in HBM, not a feather+JPEG dataset "
                         "(build one with python -m video_dqn_amd.shards)")
    if str(getattr(config, "DEVICE_RESIDENT_DATA", "auto")).lower() == "off":
        raise ValueError(f"{key} {why}: it needs the dataset in HBM, and DEVICE_RESIDENT_DATA is 'off'")


def full_store_keys(config) -> list:
    """[(key, why)] of the keys that are on and need the FULL dataset in HBM on every rank, whatever RANK_SHARDED_DATA says: the one
    statement of that policy (run_train sizes, fits and logs by it)."""
    keys = []
    if bool(getattr(config, "PRIORITIZED_REPLAY", False)):
        keys.append(("PRIORITIZED_REPLAY", "any sample may be drawn at any update"))
    if int(getattr(config, "N_STEP", 1)) > 1:
        keys.append(("N_STEP", "a chain's last frame may be any frame"))
    for key in ("MC_RETURN_FLOOR", "CQL_CALIBRATED"):
        if getattr(config, key, False):
            keys.append((key, "the return table is indexed by the rows of the full store (the other stores hand out no row indices)"))
    return keys


def check_mc(config) -> None:
    """MC_RETURN_FLOOR / CQL_CALIBRATED: raise ValueError naming the key (before any device work) for a value that is not a bool, for
    CQL_CALIBRATED without CQL_ALPHA > 0, and for everything check_nstep refuses when N_STEP > 1 (check_full_store)."""
    for key in ("MC_RETURN_FLOOR", "CQL_CALIBRATED"):
        v = getattr(config, key, False)
        if not isinstance(v, bool):
            raise ValueError(f"{key} must be True or False, not {v!r}")
        if not v:
            continue
        if key == "CQL_CALIBRATED" and not float(getattr(config, "CQL_ALPHA", 0.0)) > 0:
            raise ValueError("CQL_CALIBRATED needs CQL_ALPHA > 0: it calibrates the conservative penalty, and there is none")
        check_full_store(config, key, "indexes its return table by the rows of the resident store")


def check_iql(config) -> None:
    """IQL_EXPECTILE: raise ValueError naming the key (before any device work) for a value outside {0} and [0.5, 1) and, when it is
    on, for every configuration implicit Q-learning does not cover (algos.refuse)."""
    import math
    tau = getattr(config, "IQL_EXPECTILE", 0.0)
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not math.isfinite(tau) or not (tau == 0 or 0.5 <= tau < 1):
        raise ValueError(f"IQL_EXPECTILE must be 0 (off) or a number in [0.5, 1), not {tau!r}")
    algos.refuse(algos.IQL, config)


def check_dist(config) -> None:
    """DISTRIBUTIONAL, KL_BACKWARDS, LOG_SIGMA, DIST_SIGMA_MIN: raise ValueError naming the key (before any device work) for a value
    that is no bool, for a modifier without DISTRIBUTIONAL, for a floor outside [1e-4, 10] and, when the key is on, for every
    configuration Gaussian distributional Q-learning does not cover (algos.refuse)."""
    import math
    for key in ("DISTRIBUTIONAL", "KL_BACKWARDS", "LOG_SIGMA"):
        if not isinstance(getattr(config, key, False), bool):
            raise ValueError(f"{key} must be True or False, not {getattr(config, key)!r}")
    smin = getattr(config, "DIST_SIGMA_MIN", 0.1)
    if isinstance(smin, bool) or not isinstance(smin, (int, float)) or not math.isfinite(smin) or not (1e-4 <= smin <= 10):
        raise ValueError(f"DIST_SIGMA_MIN must be a number in [1e-4, 10], not {smin!r}")
    for key in ("KL_BACKWARDS", "LOG_SIGMA"):
        if getattr(config, key, False) and not getattr(config, "DISTRIBUTIONAL", False):
            raise ValueError(f"{key} has no effect without DISTRIBUTIONAL: it chooses the direction of the KL divergence / the "
                             "parametrisation of the spread of the distributional loss; set DISTRIBUTIONAL: True or leave it False")
    algos.refuse(algos.DIST, config)


def check_bcq(config) -> None:
    """BCQ_THRESHOLD, BCQ_BC_WEIGHT, BCQ_LOGIT_REG: raise ValueError naming the key (before any device work) for a threshold outside
    {-1} and [0, 1), a weight that is not finite and > 0, a regulariser that is not finite and >= 0, either of the two away from
    its default while BCQ is off and, when it is on, for every configuration discrete BCQ does not cover (algos.refuse)."""
    import math

    def number(key, default):
        v = getattr(config, key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{key} must be a finite number, not {v!r}")
        return float(v)
    tau, bc_weight, logit_reg = number("BCQ_THRESHOLD", -1.0), number("BCQ_BC_WEIGHT", 1.0), number("BCQ_LOGIT_REG", 0.01)
    if not (tau == -1.0 or 0.0 <= tau < 1.0):
        raise ValueError(f"BCQ_THRESHOLD must be -1 (off) or in [0, 1), not {tau!r}: an action is allowed when pi_b(a|s') / max pi_b > BCQ_THRESHOLD")
    if not bc_weight > 0:
        raise ValueError(f"BCQ_BC_WEIGHT must be > 0, not {bc_weight!r}")
    if not logit_reg >= 0:
        raise ValueError(f"BCQ_LOGIT_REG must be >= 0, not {logit_reg!r}")
    for key, val, default in (("BCQ_BC_WEIGHT", bc_weight, 1.0), ("BCQ_LOGIT_REG", logit_reg, 0.01)):
        if tau < 0 and val != default:
            raise ValueError(f"{key} has no effect without BCQ_THRESHOLD: it weighs a term of the behaviour head's loss; set "
                             f"BCQ_THRESHOLD in [0, 1) or leave {key} at {default}")
    algos.refuse(algos.BCQ, config)


def check_nstep(config, world_size: int = 1) -> None:
    """N_STEP: raise ValueError naming the key (before any device work) for a value that is not an integer in 1 .. 16 and, when it is
    above 1, for every configuration the chain walk does not cover: the ground-truth branch, LINEAR, generated tuples, a
    feather+JPEG dataset and DEVICE_RESIDENT_DATA 'off' (a chain's last frame may be any frame: the walk needs the full store in
    HBM; its size and fit are checked once the dataset is opened)."""
    from .nstep import check_config
    n = getattr(config, "N_STEP", 1)
    check_config(n)
    if int(n) == 1:
        return
    check_full_store(config, "N_STEP > 1", "ends a chain at any frame of the dataset")


def check_validation(config) -> None:
    """VAL_DATASET / VAL_INTERVAL / VAL_BATCHES: raise ValueError naming the key (before any device work) for a negative or
    non-integer value, for VAL_INTERVAL > 0 without VAL_DATASET, and for VAL_INTERVAL > 0 on the ground-truth branch."""
    from .validate import check_config
    check_config(config)


def _to_device_batch(batch, device, num_classes=5):
    before, after, act, rew, term, gt, valid = batch
    nb = dict(non_blocking=True)
    before, after = before.to(device, **nb), after.to(device, **nb)
    src_kind = 0 if before.dtype == torch.uint8 else 1
    if src_kind == 1:
        before, after = before.float().contiguous(), after.float().contiguous()
    act = torch.as_tensor(act).to(torch.int64).to(device, **nb)
    rew = torch.as_tensor(rew).float().to(device, **nb)
    term = torch.as_tensor(term).float().to(device, **nb)
    valid = torch.as_tensor(valid).float().to(device, **nb)
    gt = torch.as_tensor(gt).float()
    if gt.dim() == 1:
        gt = gt.view(-1, 1).expand(-1, num_classes)
    gt = gt.contiguous().to(device, **nb)
    return Batch(before.contiguous(), after.contiguous(), src_kind, act, rew, term, valid, gt)


class DevicePrefetcher:
    """Keeps one batch ahead on the device: the pinned host batch of step t+1 is copied on a separate stream while the
    kernels of step t run (measured with bench.py --h2d: copies on the compute stream cost 2.2 ms per 256-sample step,
    double-buffered on a copy stream they cost nothing)."""

    def __init__(self, iterator, device):
        self.it, self.device = iterator, device
        self.stream = torch.cuda.Stream(device=device)
        self._next = None
        self._fill()

    def _fill(self):
        batch = next(self.it)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))  # the buffers of two steps ago are free again
        with torch.cuda.stream(self.stream):
            dev_batch = _to_device_batch(batch, self.device)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._next = (dev_batch, ev)

    def __next__(self):
        dev_batch, ev = self._next
        torch.cuda.current_stream(self.device).wait_event(ev)
        for t in dev_batch:
            if torch.is_tensor(t):
                t.record_stream(torch.cuda.current_stream(self.device))  # allocated on the copy stream, consumed on the compute stream
        self._fill()
        return dev_batch


class LateScalar:
    """A device f32 scalar read on the host one update late: push() queues a copy into one of two pinned slots and an event behind
    it, waits for nothing, and hands back what the push before it queued — complete long ago, the GPU is busy with this update."""

    def __init__(self, tag=None, source=None, scaled=False):
        self.host = torch.zeros(2, dtype=torch.float32).pin_memory()
        self.pending = None  # (slot, event, update number) of the copy not read yet
        self.tag, self.source, self.scaled, self.seen = tag, source, scaled, None  # (late_scalars; seen: the last (number, value) kept)

    def push(self, src, number, stream=None, wait=None):
        """Queue the copy of update `number`'s value (on `stream`, behind wait(), when given: neither touches the compute stream).
        -> take() of the push before."""
        slot = number & 1
        ev = torch.cuda.Event()
        with torch.cuda.stream(stream):  # (None: the current stream)
            if wait is not None:
                wait()
            self.host[slot:slot + 1].copy_(src, non_blocking=True)
            ev.record()
        before = self.take()
        self.pending = (slot, ev, number)
        return before

    def take(self):
        """-> (update number, value) of the pending copy once it has landed, None when there is none."""
        if self.pending is None:
            return None
        slot, ev, number = self.pending
        self.pending = None
        ev.synchronize()
        return number, float(self.host[slot])


def check_run(config, world_size: int = 1) -> None:
    """Every check of the config, before any device work.  The order decides which error a config with several meets first."""
    check_augment(getattr(config, "AUG_SHIFT_PAD", 0), getattr(config, "AUG_FLIP", False), getattr(config, "AUG_FLIP_ACTIONS", [1, 2]),
                  *(getattr(config, k, 0.0) for k in COLOR_KEYS), getattr(config, "AUG_ZOOM", 0.0), getattr(config, "AUG_ZOOM_ASPECT", False),
                  getattr(config, "AUG_ROTATE", 0.0))
    check_optim(config)
    check_cql(config)
    check_target(config)
    check_validation(config)
    check_nstep(config, world_size)
    check_mc(config)
    check_iql(config)
    check_dist(config)
    check_bcq(config)
    if schedule_active(getattr(config, "LR_WARMUP_STEPS", 0), getattr(config, "LR_SCHEDULE", "constant")):
        float(config.LEARNING_RATE)  # (no check above looks at it: what is no number is refused here, not when the schedule is built)
    if getattr(config, "PRIORITIZED_REPLAY", False):
        check_prioritized_replay(config, world_size)


RunData = namedtuple("RunData", "dataset loader sampler store stream")


def open_data(config, rank, world_size, log) -> RunData:
    """The dataset, its loader and sampler and, for decoded-frame shards, where the frames live: `store` (resident in HBM, whole or
    sharded by rank) or `stream` (streamed from memory-mapped shards); with neither, batches come from `loader`."""
    B = int(config.BATCH_SIZE)
    store = stream = None
    if config.SYNTHETIC_DATA or config.DATASET in ("none", "synthetic"):
        nf = config.NUM_FRAMES or (4 if (config.PANORAMA or config.PREVIOUS_IMAGES) else 1)
        dataset = SyntheticTupleDataset(length=max(4 * B * world_size, 1024), num_frames=nf,
                                        action_dim=1 if (config.VALUE_LEARNING or config.ONE_ACTION) else 3, seed=config.SEED)
    else:
        kw = dict(one_action=True, confidence_reward=config.CONFIDENCE_REWARD, value_learning=config.VALUE_LEARNING,
                  inverse_actions=config.USE_INVERSE_ACTIONS, previous_images=config.PREVIOUS_IMAGES)
        if is_shard_dir(config.DATASET):  # pre-decoded uint8 frames (python -m video_dqn_amd.shards)
            dataset = ShardDataset(config.DATASET, **kw)
            resident = str(getattr(config, "DEVICE_RESIDENT_DATA", "auto")).lower()
            if resident not in ("auto", "on", "off"):
                raise ValueError("DEVICE_RESIDENT_DATA must be 'auto', 'on' or 'off'")
            sharded = world_size > 1 and bool(getattr(config, "RANK_SHARDED_DATA", True))
            gather_threads = int(getattr(config, "HOST_GATHER_THREADS", 0))
            headroom = 32 << 30  # activations, workspaces, allocator slack
            dataset_bytes = lambda: sum(np.load(p_, mmap_mode="r").shape[0] for p_ in dataset._paths) * FRAME_BYTES  # noqa: E731
            free_hbm = lambda: torch.cuda.mem_get_info(torch.device(config.device))[0]  # noqa: E731
            full = full_store_keys(config)
            if full:
                # prioritized replay may draw any sample at any update, an n-step chain may end at any frame, and the return table is
                # indexed by the store's rows: the full store on every rank, whatever RANK_SHARDED_DATA says
                key = full[0][0] + (" > 1" if full[0][0] == "N_STEP" else "")
                if getattr(config, "PRIORITIZED_REPLAY", False):
                    from .replay import check_config
                    check_config(float(config.PER_ALPHA), float(config.PER_BETA), B * world_size, len(dataset))
                need, free = dataset_bytes(), free_hbm()
                fits = need + headroom < free
                if world_size > 1:
                    fits = agree_all(fits, device=config.device)
                if not fits:
                    raise ValueError(f"{key} needs the dataset in HBM: its frames ({need / 2**30:.1f} GiB + {headroom >> 30} GiB "
                                     f"of headroom) do not fit in {free / 2**30:.1f} GiB of free HBM" + (" on every rank" if world_size > 1 else ""))
                if sharded:
                    for k_, why in sorted(full, key=lambda kw_: kw_[0] != "N_STEP"):  # (N_STEP's line first, as ever)
                        log(f"{k_}: every rank holds the full dataset in HBM (RANK_SHARDED_DATA does not apply: {why})")
                resident = True
            elif sharded and resident != "off":
                # N ranks: each holds only the frames its samples of the current epoch reference (re-uploaded per epoch), not a full
                # copy of the dataset; same minibatch sequence as the full per-rank copy.  Residency is decided from THIS rank's
                # subset (epoch 0's distinct frames + 10 % for later epochs), one decision for the whole job: a rank on another
                # input path would draw from a different sharding of the epoch than the resident ones
                store = RankShardedFrameStore(config.DATASET, config.device, rank, world_size, threads=gather_threads, **kw)
                need, free = store.epoch_frames(B, config.SEED) * FRAME_BYTES, free_hbm()
                fits = agree_all(need + need // 10 + headroom < free, device=config.device)
                if not fits and resident == "on":
                    raise RuntimeError(f"DEVICE_RESIDENT_DATA: 'on', but this rank's share of the frames ({need / 2**30:.1f} GiB + "
                                       f"{headroom >> 30} GiB of headroom) does not fit in {free / 2**30:.1f} GiB of free HBM on every rank")
                if fits:
                    log(f"dataset resident in HBM, sharded by rank: the frames of this rank's samples are uploaded per epoch "
                        f"({need / 2**30:.2f} GiB of the dataset's {store.total_frames * FRAME_BYTES / 2**30:.2f} GiB)")
                else:
                    store = None
                    log(f"this rank's share of the frames ({need / 2**30:.1f} GiB) does not fit in HBM on every rank: streaming")
                resident = fits
            elif resident != "auto":
                resident = resident == "on"
            else:  # frames + 32 GiB of headroom must fit in the GPU's free memory
                resident = dataset_bytes() + headroom < free_hbm()
                if world_size > 1:
                    resident = agree_all(resident, device=config.device)
            if store is None and resident:
                store = DeviceFrameStore(config.DATASET, config.device, **kw)
                log(f"dataset resident in HBM: {store.bytes() / 2**30:.2f} GiB of frames")
            elif store is None and str(getattr(config, "SHARD_INPUT", "stream")).lower() == "stream":
                # the frames do not fit (or residency is off): memory-mapped shards, native gather into pinned double buffers,
                # host-to-device copies on a prefetch stream — same minibatch sequence as the resident store
                stream = HostFrameStream(config.DATASET, config.device, B, config.SEED, rank, world_size,
                                         threads=gather_threads, **kw)
                log(f"dataset streamed from memory-mapped shards: {stream.threads} gather threads, {len(stream._slots)} pinned staging buffers")
        else:
            dataset = QLearningRealDataset(config.DATASET, as_uint8=True, **kw)
        log(f"Load data from {config.DATASET}")
        log(f"Reward Ratio: {dataset.reward_percentage()}")
    sampler = None
    if world_size > 1:
        sampler = data.distributed.DistributedSampler(dataset, num_replicas=world_size, rank=rank, shuffle=True,
                                                      seed=config.SEED, drop_last=True)
    batched = isinstance(dataset, ShardDataset)  # batched fetch: one gather per shard and batch instead of per-sample copies + collate
    if batched:
        dataset.batched_fetch = True
    loader = data.DataLoader(dataset, batch_size=B, num_workers=int(config.NUM_WORKERS), drop_last=True, shuffle=(sampler is None),
                             sampler=sampler, pin_memory=True, persistent_workers=int(config.NUM_WORKERS) > 0,
                             collate_fn=(collate_batches if batched else None))
    log(len(dataset))
    return RunData(dataset, loader, sampler, store, stream)


def build_helpers(config, dataset, store, model, comm, rank, world_size, log):
    """-> (stepper, replay, walker, returns, augmenter): the TDStepper and what the config's keys put beside it, each None when its keys
    are off — PrioritizedSampler, NStepWalker, ReturnTable, Augmenter — with their banner lines."""
    B, device = int(config.BATCH_SIZE), model.engine.device
    n_step = int(getattr(config, "N_STEP", 1))
    mc_floor, cql_calibrated = bool(getattr(config, "MC_RETURN_FLOOR", False)), bool(getattr(config, "CQL_CALIBRATED", False))
    cql_alpha, target_tau = float(getattr(config, "CQL_ALPHA", 0.0)), float(getattr(config, "TARGET_TAU", 0.0))
    clip_norm, weight_decay = float(getattr(config, "GRAD_CLIP_NORM", 0.0)), float(getattr(config, "WEIGHT_DECAY", 0.0))
    aug_pad, aug_flip = getattr(config, "AUG_SHIFT_PAD", 0), getattr(config, "AUG_FLIP", False)
    aug_actions, aug_color = getattr(config, "AUG_FLIP_ACTIONS", [1, 2]), tuple(getattr(config, k, 0.0) for k in COLOR_KEYS)
    aug_zoom, aug_zoom_aspect = float(getattr(config, "AUG_ZOOM", 0.0)), bool(getattr(config, "AUG_ZOOM_ASPECT", False))
    aug_rotate = float(getattr(config, "AUG_ROTATE", 0.0))
    lr_fn = None  # (when on, host arithmetic on the update number alone: a resumed run uses the uninterrupted run's rates)
    if schedule_active(getattr(config, "LR_WARMUP_STEPS", 0), getattr(config, "LR_SCHEDULE", "constant")):
        lr_fn = partial(lr_at, base=float(config.LEARNING_RATE), warmup=int(config.LR_WARMUP_STEPS), schedule=config.LR_SCHEDULE,
                        final_fraction=float(config.LR_FINAL_FRACTION), num_steps=int(config.NUM_STEPS))
    replay = None
    if getattr(config, "PRIORITIZED_REPLAY", False):
        from .replay import PrioritizedSampler
        replay = PrioritizedSampler(len(store), B, device, alpha=float(config.PER_ALPHA), beta=float(config.PER_BETA),
                                     num_steps=int(config.NUM_STEPS), seed=int(config.SEED), rank=rank, world_size=world_size)
        log(f"prioritized replay over {len(store)} samples: alpha {replay.alpha}, beta {replay.beta0} -> 1.0 at {replay.num_steps}")
    stepper = TDStepper(model.engine, B, lr=config.LEARNING_RATE, gamma=config.GAMMA,
                        clip_rect=(config.LOSS_CLIP == "rect"), linear=config.LINEAR,
                        remove_before_reward=config.REMOVE_BEFORE_REWARD,
                        train_on_ground_truth=config.TRAIN_ON_GROUND_TRUTH, value_learning=config.VALUE_LEARNING,
                        target_update_interval=config.TARGET_UPDATE_INTERVAL, world_size=world_size,
                        allreduce=(comm.launch if comm else None), loss_kind=getattr(config, "LOSS_KIND", "l2"),
                        allreduce_loss=(comm.launch_loss if comm else None), allreduce_wait=(comm.wait_last if comm else None),
                        allreduce_errors=((lambda: comm.launch_errors(replay.err_all)) if comm and replay else None),
                        grad_clip_norm=clip_norm, weight_decay=weight_decay, lr_fn=lr_fn, cql_alpha=cql_alpha,
                        target_tau=target_tau, mc_floor=mc_floor, cql_calibrated=cql_calibrated,
                        **{arg: v for a in algos.ALGOS for arg, v in a.kwargs(config).items()})
    walker = returns = next_row = None
    if n_step > 1 or mc_floor or cql_calibrated:
        from .nstep import successors
        next_row = successors(dataset.before[:, 0], dataset.after[:, 0])  # (host, once: shared by the walker and the return table)
    if mc_floor or cql_calibrated:
        # the Monte-Carlo return of every row at GAMMA, built once on the device over store.rew / store.term; every rank builds the
        # same bits (no atomics), a resume rebuilds it: nothing of it is exchanged or saved.  One read-back, here, for the log line
        from .mcreturn import ReturnTable
        with torch.cuda.device(device):
            returns = ReturnTable(next_row, store.rew, store.term, float(config.GAMMA), device)
            g_max, g_mean = returns.summary()
        log(f"Monte-Carlo returns: {returns.rows} rows, {returns.rounds} rounds of pointer doubling (the first {2 ** returns.rounds} rows "
            f"of every chain) at GAMMA {float(config.GAMMA):g}; table max {g_max:.6g}, mean {g_mean:.6g}; " +
            " and ".join((["MC_RETURN_FLOOR: y <- max(y, G) in front of the clip"] if mc_floor else []) +
                         (["CQL_CALIBRATED: the penalty's logsumexp over max(Q, G)"] if cql_calibrated else [])) +
            "; validation is unchanged")
    if n_step > 1:
        # the successor table from index.npz as it is (host, once), held on the device beside store.rew / store.term; the shares of
        # chain lengths are host arithmetic on that table: nothing is read back
        from .nstep import NStepWalker, chain_shares
        walker = NStepWalker(next_row, store.rew, store.term, B, n_step, float(config.GAMMA), device)
        shares = chain_shares(next_row, n_step)
        log(f"n-step returns: N_STEP {n_step}, one chain walk per update over {len(next_row)} rows; chains of " +
            ", ".join(f"{k + 1} row{'s' if k else ''}: {100 * s:.1f} %" for k, s in enumerate(shares)) +
            " (terminals ignored); validation stays one-step")
    if target_tau > 0:
        log(f"soft target updates: target <- target + {target_tau:g} * (online - target) inside every Adam launch, the target weights "
            "folded from the average in front of every update; TARGET_UPDATE_INTERVAL is unused")
    if stepper.algo is not None:
        log(f"{stepper.algo.title}: {stepper.algo.log(stepper)}; validation adds the head's held-out metrics, one more launch per batch"
            f"{' and a target pass over s' if stepper.algo.key == 'IQL_EXPECTILE' else ''}: "
            + ", ".join(tag for tag, _ in algos.eval_tags(stepper.algo)))
    if cql_alpha > 0:
        log(f"conservative Q-learning: {cql_alpha:g} * (logsumexp_a Q(s, .) - Q(s, a_data)) added to the TD loss in the loss launch")
    if clip_norm > 0 or weight_decay > 0 or lr_fn is not None:
        log("optimiser:" + (f" gradient clipped to a global norm of {clip_norm:g}" if clip_norm > 0 else "") +
            (f" decoupled weight decay {weight_decay:g}" if weight_decay > 0 else "") +
            (f" learning rate {config.LR_SCHEDULE} to {float(config.LR_FINAL_FRACTION):g} x LEARNING_RATE at {int(config.NUM_STEPS)}, "
             f"{int(config.LR_WARMUP_STEPS)} warm-up updates" if lr_fn is not None else ""))
    augmenter = None
    if aug_pad > 0 or aug_flip or any(j > 0 for j in aug_color) or jz(aug_zoom) > 0 or jr(aug_rotate) > 0:
        augmenter = Augmenter(B, device, pad=aug_pad, flip=aug_flip, flip_actions=aug_actions, seed=int(config.SEED),
                              rank=rank, world_size=world_size, brightness=aug_color[0], contrast=aug_color[1], saturation=aug_color[2],
                              zoom=aug_zoom, zoom_aspect=aug_zoom_aspect, rotate=aug_rotate)
        on = [f"random shift of up to {aug_pad} pixels"] if aug_pad > 0 or aug_flip else []
        if aug_flip:  # (one action column: nothing to exchange)
            on.append("random left-right mirror" + (f" with actions {aug_actions[0]} <-> {aug_actions[1]} exchanged" if model.engine.action_dim == 3 else ""))
        if augmenter.color is not None:
            on.append("colour jitter " + " ".join(f"{k[4:].lower()} x [{1 - j:g}, {1 + j:g}]" for k, j in zip(COLOR_KEYS, aug_color) if j > 0))
        if augmenter.zoom is not None:
            on.append(f"random zoom to a window of [{1 - aug_zoom:g}, 1] of the frame" +
                      (", its two sides drawn independently" if aug_zoom_aspect else ""))
        if augmenter.affine is not None:
            on.append(f"random rotation by up to ±{aug_rotate:g}°")
        log("augmentation: " + ", ".join(on) + ", one draw per sample and update, shared by s and s'")
    return stepper, replay, walker, returns, augmenter


HEAD_WORDS = {f"{a.head}_head": (a.title, a.head) for a in algos.ALGOS}


def restore_state(config, model, stepper, replay, resume_from, rank, world_size, log) -> None:
    """Resume (:192-198), bootstrap (:200-206), the replica broadcast, the :208 target sync and, behind it, the resumed soft target."""
    resumed_target = None  # TARGET_TAU: the checkpoint's averaged target weights, loaded behind the :208 sync below
    resumed_head_target = None  # ... and the spread head's rows of them (read by the distributional loss), from the head's own key
    if resume_from > -1:  # :192-198
        model_loc = f"{config.folder}/models/sample{resume_from}.torch"
        snapshot = torch.load(model_loc, map_location=config.device)
        log(f"Loading model from: {model_loc}")
        head_key = head_of(stepper.net)[0]
        has_head = head_key is not None and head_key in snapshot
        model.load_state_dict(OrderedDict(snapshot["model_state_dict"], **snapshot[head_key]["state_dict"]) if has_head
                              else snapshot["model_state_dict"])
        load_optimizer_state_dict(stepper, snapshot["optimizer_state_dict"])
        resumed_target = snapshot.get("target_state_dict")
        if head_key:
            what, head = HEAD_WORDS[head_key]
            if has_head:
                load_head_state(stepper, snapshot[head_key])
                resumed_head_target = snapshot[head_key].get("target_state_dict")
                log(f"{what}: the {head} head and its Adam moments restored from the checkpoint")
            else:
                log(f"{what}: the checkpoint has no {head_key}, the {head} head starts from its initialisation")
        if replay is not None:
            if "replay_state" in snapshot:
                replay.load_state_dict(snapshot["replay_state"])
                log("prioritized replay: priorities restored from the checkpoint")
            else:
                log("prioritized replay: the checkpoint has no replay_state, starting from the uniform table")
    if config.BOOTSTRAP:  # :200-206 — start from a network trained on ground truth (model AND optimiser state)
        log("\n\nBOOTSTRAP\n\n")
        model_loc = getattr(config, "BOOTSTRAP_CHECKPOINT", "") or "logs/trained_gt_0.99/models/epoch99.torch"  # :202
        snapshot = torch.load(model_loc, map_location=config.device)  # a missing file raises, as in the reference
        log(f"Loading model from: {model_loc}")
        model.load_state_dict(snapshot["model_state_dict"])
        load_optimizer_state_dict(stepper, snapshot["optimizer_state_dict"])
    if resume_from < 0 and not config.BOOTSTRAP and not getattr(model, "pretrained_loaded", False) and rank == 0:
        log("WARNING: the ResNet-18 trunk starts from a RANDOM initialisation — the reference builds "
            "models.resnet18(pretrained=True) (archs/HabitatDQNMultiAction.py:11); set PRETRAINED_WEIGHTS in config.yml "
            "(a torchvision resnet18 state_dict file) to train on ImageNet features as the reference does")
    if world_size > 1:  # replicas must start identical: rank 0's parameters, statistics and optimiser state everywhere
        # (TARGET_TAU: the target too; from then on every rank applies the same reduced gradient inside the same launch, so the
        # targets stay identical with no collective of their own — a resumed target comes from the one file every rank reads)
        eng = model.engine
        broadcast_replica_state([eng.params, eng.bnstats, eng.num_batches_tracked, stepper.exp_avg, stepper.exp_avg_sq] +
                                ([stepper.target_params] if stepper.target_tau > 0 else []))
        steps = torch.tensor([stepper.adam_step], dtype=torch.int64, device=eng.device)
        torch.distributed.broadcast(steps, src=0)
        stepper.adam_step = int(steps.item())
        eng.mark_dirty()
    stepper.sync_target()  # :208
    if stepper.target_tau > 0 and resume_from > -1:  # the averaged target of the interrupted run, in place of the copy :208 has just made
        if resumed_target is not None:
            load_target_state_dict(stepper, resumed_target, resumed_head_target)
            log("soft target updates: target weights restored from the checkpoint")
        else:
            log("soft target updates: the checkpoint has no target_state_dict, the target starts from the online weights")


def late_scalars(stepper, returns):
    """The device scalars logged beside the loss, each a LateScalar with its tag and source; scaled: this rank's share of a global mean."""
    late = []
    if stepper.grad_clip_norm > 0:  # the norm BEFORE clipping, as clip_grad_norm_ returns it; non-finite values show here
        late.append(LateScalar("grad_norm/train", stepper.clip_out[:1]))
    if stepper.cql_alpha > 0:  # the unscaled penalty; avg_q_loss/train is the full objective
        late.append(LateScalar("cql_penalty/train", stepper.cql_penalty, scaled=True))
    if returns is not None:
        late += [LateScalar("mc_floor_share/train", stepper.mc_stats[0:1], scaled=True), LateScalar("q_minus_return/train", stepper.mc_stats[1:2], scaled=True)]
    algo = getattr(stepper, "algo", None)
    if algo is not None:
        late += [LateScalar(f"{name}/train", getattr(stepper, algo.stats_attr)[i:i + 1], scaled=True) for i, name in enumerate(algo.stats)]
    return late


def run_train(config, resume_from=-1, max_steps=None, rank=0, world_size=1, log=print):
    """train_q_network.py:84-250."""
    check_run(config, world_size)
    torch.manual_seed(config.SEED)
    np.random.seed(config.SEED)
    log(f"Using: {config.device}")
    B = int(config.BATCH_SIZE)
    dataset, loader, sampler, store, stream = open_data(config, rank, world_size, log)
    model = build_model(config, max_batch=2 * B)
    comm = BucketAllReduce(world_size) if world_size > 1 else None
    stepper, replay, walker, returns, augmenter = build_helpers(config, dataset, store, model, comm, rank, world_size, log)
    swap = augmenter is not None and augmenter.flip and model.engine.action_dim == 3  # mirrored samples exchange their action labels
    if world_size > 1 and config.ARCHITECTURE != "extra_capacity" and getattr(config, "SYNC_BN", True):
        model.engine.set_bn_sync(world_size)  # train-mode BatchNorm over the global batch, as the single-GPU reference sees it
    if replay is not None:  # (nothing is drawn before the first update asks for its batch, behind the resume below)
        iterator = store.prioritized_batches(replay, resume_from + 1, walker=walker, returns=returns)
    elif isinstance(store, RankShardedFrameStore):  # (a key that needs a walker or a return table holds the full store instead)
        iterator = store.batches(B, config.SEED)
    elif store is not None:  # minibatches are gathered on the device; no loader, no host copies
        iterator = store.batches(B, config.SEED, rank, world_size, walker=walker, returns=returns)
    elif stream is not None:
        iterator = stream.batches()
    else:
        iterator = DevicePrefetcher(loopLoader(loader, on_reset=(sampler.set_epoch if sampler else None)), model.engine.device)
    os.makedirs(f"{config.folder}/models", exist_ok=True)
    sample_number = resume_from + 1
    restore_state(config, model, stepper, replay, resume_from, rank, world_size, log)
    stepper.sample_number = sample_number
    stepper.replay, stepper.augmenter, stepper.nstep, stepper.returns = replay, augmenter, walker, returns  # returned with the stepper
    # VAL_INTERVAL > 0: the held-out pass (validate.py) on rank 0 alone, the others wait in the next update's first collective; off: nothing is built
    validator = Validator(config, log=log) if int(getattr(config, "VAL_INTERVAL", 0)) > 0 and rank == 0 else None

    running_loss = None
    late_loss, late = LateScalar(), late_scalars(stepper, returns)
    loss_stream = None  # N > 1: where the all-reduced loss is waited for and copied to the host
    num_steps = config.NUM_STEPS if max_steps is None else min(config.NUM_STEPS, sample_number + max_steps)

    def average(taken):
        nonlocal running_loss
        if taken is not None:
            v = taken[1]
            running_loss = v if running_loss is None else running_loss * 0.99 + v * 0.01  # :228-231

    try:  # (the streaming input path owns a thread, pinned buffers and a prefetch stream: released on every exit)
        while sample_number < num_steps:
            sample_number += 1
            model.set_train()  # :221 (flags only; the engine's BatchNorm is always in eval mode in extra_capacity)
            batch = next(iterator)
            act = batch.act
            aug_params = aug_factors = aug_zoom = aug_affine = None
            if augmenter is not None:  # this update's draw(s) and the mirrored samples' action labels: small launches, nothing read back
                aug_params, aug_factors, aug_zoom, aug_affine = augmenter.draw(sample_number), augmenter.color, augmenter.zoom, augmenter.affine
                if aug_affine is not None:  # the affine rows contain the zoom: the update takes them instead
                    aug_zoom = None
                if swap:
                    act = augmenter.actions(act.contiguous())
            # the stepper performs the :215-216 target refresh itself (sample_number % TARGET_UPDATE_INTERVAL == 0)
            loss = stepper.step(batch.before, batch.after, batch.src_kind, act, batch.rew, batch.term,
                                batch.valid if config.REMOVE_BEFORE_REWARD else None,
                                batch.gt if config.TRAIN_ON_GROUND_TRUTH else None,
                                finish_allreduce=(comm.finish if comm else None), weights=batch.weight,
                                td_error=(replay.err if replay is not None else None), augment=aug_params, augment_color=aug_factors,
                                augment_zoom=aug_zoom, augment_affine=aug_affine, discount=batch.discount, mc_return=batch.mc_return)
            if replay is not None:
                replay.update()  # behind the loss launch (and, with N ranks, the error exchange that finish_allreduce joined)
            # every rank's `loss` is its share of the global mean (the TD kernel divides by the global batch): their SUM is the
            # batch-mean loss the reference feeds into its running average every update (:228-231).  The stepper has queued that
            # 4-byte all-reduce on the gradient stream behind the last gradient bucket (dist.launch_loss); it is waited for and
            # copied to the host on the read-back stream only — the compute stream, i.e. the next update's first kernel, never
            # waits for it — so the average that is printed, logged and returned is still the reference's: an EMA of the true
            # global batch-mean loss, one update late like the single-process read-back
            reduced = comm.take_loss() if comm is not None else None
            if reduced is not None:
                buf, work = reduced
                if loss_stream is None:
                    loss_stream = torch.cuda.Stream(device=model.engine.device)
                average(late_loss.push(buf, sample_number, stream=loss_stream, wait=work.wait))
            else:
                average(late_loss.push(loss, sample_number))
            for s in late:
                s.seen = s.push(s.source, sample_number) or s.seen  # (update number, value): one late
            log_now = sample_number % 100 == 0 and rank == 0 and hasattr(config, "writer")
            if log_now:  # the reference logs the average INCLUDING this update's loss (:228-238): take it in before writing
                average(late_loss.take())
            if rank == 0 and running_loss is not None:
                print(f"\rbatch:{sample_number}/{config.NUM_STEPS} avg_loss: {running_loss}", end="")
            if log_now and running_loss is not None:
                config.writer.add_scalar("avg_q_loss/train", running_loss, sample_number)  # :236-238
            if log_now:
                for s in late:
                    if s.seen is not None:  # at the update it was measured at, one back; a share times the world size: rank 0's own mean
                        config.writer.add_scalar(s.tag, s.seen[1] * world_size if s.scaled else s.seen[1], s.seen[0])
            if log_now and replay is not None:
                config.writer.add_scalar("per/beta", replay.beta(sample_number), sample_number)  # (host arithmetic: nothing read back)
            if validator is not None and validator.due(sample_number):  # :240 `# checkpoint and eval`: in front of the checkpoint
                validator.run(stepper, sample_number, writer=getattr(config, "writer", None))
            if sample_number % config.CHECKPOINT_INTERVAL == 0 and rank == 0:  # :241-247
                torch.cuda.synchronize()
                save_checkpoint(f"{config.folder}/models/sample{sample_number}.torch", sample_number, model, stepper,
                                replay_state=(replay.state_dict() if replay is not None else None),
                                target_state_dict=(target_state_dict(stepper, model) if stepper.target_tau > 0 else None))
        average(late_loss.take())
        torch.cuda.synchronize()
    finally:
        if stream is not None:
            stream.close()
    return model, stepper, running_loss
