"""Host-side driver of the HIP engine (libvdqn.so): owns the torch-allocated device buffers and calls
the C ABI.  PyTorch is used for device memory and streams only — all arithmetic runs in the HIP library.

Mirrors the pieces of ``train_q_network.py`` that touch the device:
  * model / target_net / Adam construction       (:119-124)
  * target sync                                   (:121,208,215-216)
  * zero_grad / process_batch / backward / step   (:222-227)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional

import torch

from . import _lib
from .algos import ALGOS, BCQ, HEAD_EVAL_SLOTS, LOSS_SLOTS, MODIFIERS, refuse

LOSS_KINDS = {"l2": 0, "huber": 1}  # vdqn_td_args.loss_kind

# "bf16x3": f32 storage (parameters, activations, workspaces and checkpoints exactly as "f32"), the convolutions / linear layers /
# weight gradients computed as split bf16 x 3 (include/vdqn.h VDQN_F32X3): f32-grade results at bf16 MFMA rates
DTYPES = {"f32": _lib.VDQN_F32, "fp32": _lib.VDQN_F32, "float32": _lib.VDQN_F32,
          "bf16": _lib.VDQN_BF16, "bfloat16": _lib.VDQN_BF16,
          "bf16x3": _lib.VDQN_F32X3}


# VDQN_EARLY_ADAM=0: `TDStepper.step` runs the whole optimiser update behind the backward pass (one launch)
_EARLY_ADAM = os.environ.get("VDQN_EARLY_ADAM", "1") != "0"
# VDQN_DIST_EARLY_ADAM=1: under a gradient exchange, stage 0 / 1 are updated behind their own bucket (TDStepper.allreduce_wait)
_DIST_EARLY_ADAM = os.environ.get("VDQN_DIST_EARLY_ADAM", "0") in ("1", "2", "3")
# diagnostic values (one rank only — they are wrong with more): 2 = the same without waiting for the bucket's collective (is the wait
# the cost?), 3 = waiting for it, but without the Adam launch (is the extra kernel the cost?)
_DIST_EARLY_ADAM_MODE = os.environ.get("VDQN_DIST_EARLY_ADAM", "0")



_SAID = set()


def _say_once(text: str) -> None:
    """Print `text` the first time it is said in this process."""
    if text not in _SAID:
        _SAID.add(text)
        print(text)


def head_kept_message(head: str) -> str:
    return f"{head} head: the state_dict has no {head}.weight / {head}.bias, the {head} head keeps its initialisation"


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.VdqnError("video_dqn_amd needs a ROCm GPU (gfx950); there is no CPU fallback")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def norm_pixel(values):
    """f32 [3] numpy: pixel values (0 .. 255, one per colour channel) in normalised units, (v / 255 - mean_c) / std_c in float32 with
    every operation rounded on its own: the bits vdqn_pack_input gives a uint8 pixel of that value."""
    import numpy as np
    v = np.asarray(values, dtype=np.float32).reshape(3)
    return (v / np.float32(255.0) - np.array([0.485, 0.456, 0.406], dtype=np.float32)) / np.array([0.229, 0.224, 0.225], dtype=np.float32)


def attrib_source_args(src: torch.Tensor, baseline=None):
    """The (src, src_kind, baseline, base_const, n_base) arguments the attribution entries share, plus what must stay alive.  src: uint8
    [n,224,224,3] or f32 [n,3,224,224], contiguous; baseline: None (zeros in normalised units), three floats in NORMALISED units, or
    a tensor of src's dtype and shape."""
    kind = 0 if src.dtype == torch.uint8 else 1
    shape = (224, 224, 3) if kind == 0 else (3, 224, 224)
    if src.dim() != 4 or tuple(src.shape[1:]) != shape or (kind == 1 and src.dtype != torch.float32) or not src.is_contiguous():
        raise ValueError(f"attribution source must be contiguous uint8 [n,224,224,3] or float32 [n,3,224,224], not {src.dtype} {tuple(src.shape)}")
    base_t, const = None, None
    if isinstance(baseline, torch.Tensor):
        if baseline.dtype != src.dtype or baseline.shape != src.shape or baseline.device != src.device:
            raise ValueError(f"baseline tensor must have the source's kind and shape ({src.dtype} {tuple(src.shape)}), not {baseline.dtype} "
                             f"{tuple(baseline.shape)}")
        base_t = baseline.contiguous()
    elif baseline is not None:
        vals = [float(v) for v in baseline]
        if len(vals) != 3:
            raise ValueError(f"baseline must be three per-channel values or a tensor shaped like the source, not {len(vals)} values")
        const = (C.c_float * 3)(*vals)
    return (_ptr(src), kind, _ptr(base_t), const, src.shape[0]), (src, base_t, const)


@dataclass
class ParamSlot:
    name: str
    offset: int
    numel: int
    shape: tuple
    kind: int      # 0 trainable, 1 frozen (resnet.fc), 2 running_mean, 3 running_var
    param_id: int
    stage: int


class NetEngine:
    """One HabitatDQNMultiAction instance on the device: flat f32 master parameters + BN statistics."""

    def __init__(self, action_dim=3, num_classes=5, num_frames=1, extra_capacity=True, dtype="bf16",
                 max_batch=512, device=None, deterministic=None, value_head=False, spread_head=False, policy_head=False):
        self.lib = _lib.load()
        # device="cpu" gives a storage-only instance (state_dict / checkpoint plumbing); every compute entry
        # point still requires the GPU and raises otherwise — there is no CPU arithmetic in this package.
        self.storage_only = device is not None and torch.device(device).type == "cpu"
        self.device = torch.device("cpu") if self.storage_only else require_gpu(device)
        self.extra_capacity = bool(extra_capacity)
        self.action_dim, self.num_classes, self.num_frames = action_dim, num_classes, num_frames
        # dtype_name is the STORAGE dtype ("bf16" | "f32": what torch tensors of activations / gradients use); compute_dtype adds
        # the GEMM mode ("bf16" | "f32" | "bf16x3")
        self.dtype_name = "bf16" if DTYPES[dtype] == _lib.VDQN_BF16 else "f32"
        self.compute_dtype = {_lib.VDQN_BF16: "bf16", _lib.VDQN_F32: "f32", _lib.VDQN_F32X3: "bf16x3"}[DTYPES[dtype]]
        # run-to-run bit-identical updates (the reference pins cudnn.deterministic, train_q_network.py:88-89): config key
        # DETERMINISTIC / this argument, or VDQN_DETERMINISTIC=1 in the environment
        if deterministic is None:
            deterministic = os.environ.get("VDQN_DETERMINISTIC", "0") == "1"
        self.deterministic = bool(deterministic)
        self.cfg = _lib.NetConfig(action_dim, num_classes, num_frames, int(self.extra_capacity), DTYPES[dtype], max_batch,
                                  int(self.deterministic))
        # The one extra head behind the Q layer (algos.py), its extra rows the parameters <head>.weight / <head>.bias, never among the
        # reference's keys; none: vdqn_net_create, the same tables and bits.  The create entries form a chain, each taking its
        # predecessors' flags in front of its own: the last flag set picks the entry, and the engine refuses more than one.
        given = {"value": bool(value_head), "spread": bool(spread_head), "policy": bool(policy_head)}
        self.value_head, self.spread_head, self.policy_head = given.values()
        flags = [given[a.head] for a in ALGOS]
        last = max((i for i, f in enumerate(flags) if f), default=-1)
        self.head, self.head_keys, create = (None, (), "vdqn_net_create") if last < 0 else (ALGOS[last].head, ALGOS[last].head_keys, ALGOS[last].create)
        h = C.c_void_p()
        _lib.check(getattr(self.lib, create)(C.byref(self.cfg), *map(int, flags[:last + 1]), C.byref(h)), create)
        self.handle = h
        self.max_batch = max_batch
        self.slots: "OrderedDict[str, ParamSlot]" = OrderedDict()
        info = _lib.ParamInfo()
        for i in range(self.lib.vdqn_net_num_params(h)):
            _lib.check(self.lib.vdqn_net_param_info(h, i, C.byref(info)), "vdqn_net_param_info")
            name = info.name.decode()
            self.slots[name] = ParamSlot(name, info.offset, info.numel, tuple(info.shape[:info.ndim]), info.kind,
                                         info.param_id, info.stage)
        self.params_numel = self.lib.vdqn_net_params_numel(h)
        self.trainable_numel = self.lib.vdqn_net_trainable_numel(h)
        self.bnstats_numel = self.lib.vdqn_net_bnstats_numel(h)
        self.packed_bytes = self.lib.vdqn_net_packed_bytes(h)
        self.params = torch.zeros(self.params_numel, dtype=torch.float32, device=self.device)
        self.bnstats = torch.zeros(self.bnstats_numel, dtype=torch.float32, device=self.device)
        # BatchNorm.num_batches_tracked of the 20 BatchNorm layers (only ever advanced by ARCHITECTURE='basic',
        # whose BatchNorm layers run in train mode)
        self.num_batches_tracked = torch.zeros(20, dtype=torch.long, device=self.device)
        self.packed = None if self.storage_only else torch.zeros(self.packed_bytes, dtype=torch.uint8, device=self.device)
        self._packed_version = None
        self._version = 0
        self._acts: Dict[int, torch.Tensor] = {}

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.vdqn_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- parameter views -------------------------------------------------------------------------
    def view(self, name: str) -> torch.Tensor:
        s = self.slots[name]
        base = self.params if s.kind in (0, 1) else self.bnstats
        return base[s.offset:s.offset + s.numel].view(s.shape)

    def stage_range(self, stage: int):
        b, e = C.c_int64(), C.c_int64()
        _lib.check(self.lib.vdqn_net_stage_range(self.handle, stage, C.byref(b), C.byref(e)), "stage_range")
        return b.value, e.value

    def load_tensors(self, state_dict) -> None:
        """Copy every tensor the engine owns (by its reference state_dict name) from ``state_dict``."""
        with torch.no_grad():
            for name in self.slots:
                if name in self.head_keys and name not in state_dict:
                    continue  # a DQN checkpoint into an engine with an extra head (warm start): the initialised head stays
                self.view(name).copy_(state_dict[name].to(torch.float32))
        if self.head and not all(n in state_dict for n in self.head_keys):
            _say_once(head_kept_message(self.head))
        self.mark_dirty()

    def mark_dirty(self):
        """Call after the master parameters changed through raw pointers (the Adam kernel, a broadcast)."""
        self._version += 1

    def version_key(self):
        """Identifies the parameter values the packed weights were made from: the explicit counter above plus the autograd
        version counters of the flat arrays, which every in-place torch op on a view of them (the module's Parameters under a
        torch optimiser, load_state_dict) advances."""
        return (self._version, self.params._version, self.bnstats._version)

    # ---- packing + forward -----------------------------------------------------------------------
    def _need_gpu(self):
        if self.storage_only:
            raise _lib.VdqnError("this NetEngine is storage-only (device='cpu'); compute needs the GPU — no CPU fallback")

    def pack_weights(self, packed: Optional[torch.Tensor] = None, with_dgrad: bool = False, params=None, bnstats=None):
        self._need_gpu()
        packed = self.packed if packed is None else packed
        _lib.check(self.lib.vdqn_net_pack_weights(self.handle, _ptr(self.params if params is None else params),
                                                  _ptr(self.bnstats if bnstats is None else bnstats),
                                                  _ptr(packed), int(with_dgrad), _stream()), "vdqn_net_pack_weights")

    def acts_bytes(self, n_samples: int) -> int:
        return self.lib.vdqn_net_acts_bytes(self.handle, n_samples)

    def bwd_bytes(self, n_samples: int) -> int:
        return self.lib.vdqn_net_bwd_bytes(self.handle, n_samples)

    def _acts_for(self, n: int) -> torch.Tensor:
        buf = self._acts.get(n)
        if buf is None:
            self._acts.clear()
            buf = torch.empty(self.acts_bytes(n), dtype=torch.uint8, device=self.device)
            self._acts[n] = buf
        return buf

    def forward(self, frames: torch.Tensor, src_kind: int, n_samples: int) -> torch.Tensor:
        """frames: contiguous device tensor (uint8 NHWC frames if src_kind == 0, f32 NCHW if 1)."""
        self._need_gpu()
        if n_samples > self.max_batch:
            raise _lib.VdqnError(f"batch {n_samples} exceeds max_batch {self.max_batch}")
        with torch.cuda.device(self.device):
            if self._packed_version != self.version_key():
                self.pack_weights()
                self._packed_version = self.version_key()
            q = torch.empty((n_samples, self.num_classes * self.action_dim), dtype=torch.float32, device=self.device)
            acts = self._acts_for(n_samples)
            _lib.check(self.lib.vdqn_net_forward(self.handle, _ptr(self.packed), _ptr(frames), src_kind, n_samples,
                                                 _ptr(acts), _ptr(q), _stream()), "vdqn_net_forward")
        return q

    def _last_qf(self, what: str, head: str, n_samples: int) -> torch.Tensor:
        """The f32 Q rows [n_samples][64], as bytes, that the LAST `forward(.., n_samples)` left in its workspace (no second pass)."""
        self._need_gpu()
        if self.head != head:
            raise _lib.VdqnError(f"{what}: this NetEngine has no {head} head (NetEngine({head}_head=True))")
        acts = self._acts.get(n_samples)
        if acts is None:
            raise _lib.VdqnError(f"{what}: no forward over {n_samples} samples has run")
        off = self.lib.vdqn_net_act_offset(self.handle, n_samples, b"qf")
        return acts[off:off + n_samples * 64 * 4]

    def state_values(self, n_samples: int) -> torch.Tensor:
        """V(s) f32 [n_samples, num_classes] of the last forward: the value head's columns of its f32 Q rows."""
        nq = self.num_classes * self.action_dim
        return self._last_qf("state_values", "value", n_samples).view(torch.float32).view(n_samples, 64)[:, nq:nq + self.num_classes].clone()

    def dist_moments(self, n_samples: int, log_sigma: bool, sigma_min: float) -> torch.Tensor:
        """f32 [n_samples, num_classes, action_dim, 2] = {mean, variance} of the last forward: vdqn_dist_moments over its f32 Q rows."""
        qf = self._last_qf("dist_moments", "spread", n_samples)
        out = torch.empty((n_samples, self.num_classes, self.action_dim, 2), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vdqn_dist_moments(qf.data_ptr(), out.data_ptr(), n_samples, self.num_classes, self.action_dim, 64,
                                                  2 if log_sigma else 0, float(sigma_min), _stream()), "vdqn_dist_moments")
        return out

    def bcq_constrain(self, n_samples: int, threshold: float):
        """(q f32 [n_samples, num_classes, action_dim] with the actions the behaviour head disallows at -inf, prob f32 [n_samples,
        action_dim] = the behaviour probabilities) of the last forward: vdqn_bcq_constrain over its f32 Q rows."""
        qf = self._last_qf("bcq_constrain", "policy", n_samples)
        q = torch.empty((n_samples, self.num_classes, self.action_dim), dtype=torch.float32, device=self.device)
        prob = torch.empty((n_samples, self.action_dim), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.vdqn_bcq_constrain(qf.data_ptr(), q.data_ptr(), prob.data_ptr(), n_samples, self.num_classes,
                                                   self.action_dim, 64, float(threshold), _stream()), "vdqn_bcq_constrain")
        return q, prob

    # ---- one model call with its own backward (torch.autograd over the module, model.py) ----------------------------
    def forward_saved(self, frames: torch.Tensor, src_kind: int, n_samples: int, packed: torch.Tensor):
        """`vdqn_net_forward` into a workspace of its own that the caller keeps for `backward_from_dq`: -> (q, acts).
        `packed` must hold this network's weights packed WITH the data-gradient operands (`pack_weights(.., with_dgrad=True)`)."""
        self._need_gpu()
        if n_samples > self.max_batch:
            raise _lib.VdqnError(f"batch {n_samples} exceeds max_batch {self.max_batch}")
        with torch.cuda.device(self.device):
            q = torch.empty((n_samples, self.num_classes * self.action_dim), dtype=torch.float32, device=self.device)
            acts = torch.empty(self.acts_bytes(n_samples), dtype=torch.uint8, device=self.device)
            _lib.check(self.lib.vdqn_net_forward(self.handle, _ptr(packed), _ptr(frames), src_kind, n_samples, _ptr(acts), _ptr(q),
                                                 _stream()), "vdqn_net_forward")
        return q, acts

    def backward_from_dq(self, acts: torch.Tensor, packed: torch.Tensor, dq: torch.Tensor, n_samples: int, want_input_grad: bool = False,
                         pixel_units: bool = False):
        """Backward of one `forward_saved` call from dL/dQ (f32 [n_samples, num_classes*action_dim]): the flat f32 gradient
        over the trainable range, complete on the current stream (loss.backward() through `model(before)`,
        train_q_network.py:131,226).  extra_capacity only.  want_input_grad: -> (grads, gx) with gx f32 [n_samples * num_frames, 3,
        224, 224] = dL/d(frames) (vdqn_net_input_grad: one more launch behind stage 2), with respect to the normalised frames or,
        with pixel_units, to the uint8 pixel values."""
        self._need_gpu()
        if want_input_grad and not self.extra_capacity:
            raise _lib.VdqnError("backward_from_dq(want_input_grad=True): ARCHITECTURE='basic' has no frame gradient (extra_capacity only)")
        with torch.cuda.device(self.device):
            bwd = getattr(self, "_bwd_ws", None)
            if bwd is None or bwd[0] != n_samples:
                bwd = self._bwd_ws = (n_samples, torch.empty(self.bwd_bytes(n_samples), dtype=torch.uint8, device=self.device))
            grads = torch.zeros(self.trainable_numel, dtype=torch.float32, device=self.device)
            dq = dq.to(device=self.device, dtype=torch.float32).contiguous()
            a = _lib.StepArgs()
            a.params, a.bnstats, a.packed_online = _ptr(self.params), _ptr(self.bnstats), _ptr(packed)
            a.batch = a.acts_samples = n_samples
            a.acts_online, a.bwd, a.grads = _ptr(acts), _ptr(bwd[1]), _ptr(grads)
            st = _stream()
            _lib.check(self.lib.vdqn_net_backward_begin(self.handle, C.byref(a), _ptr(dq), st), "vdqn_net_backward_begin")
            for stage in range(3):  # stage 2 joins the engine's gradient stream back into `st`
                _lib.check(self.lib.vdqn_net_backward_stage(self.handle, C.byref(a), stage, st), "vdqn_net_backward_stage")
            gx = None
            if want_input_grad:
                gx = torch.empty((n_samples * self.num_frames, 3, 224, 224), dtype=torch.float32, device=self.device)
                _lib.check(self.lib.vdqn_net_input_grad(self.handle, C.byref(a), _ptr(gx), int(bool(pixel_units)), st), "vdqn_net_input_grad")
            dq.record_stream(torch.cuda.current_stream())
        return (grads, gx) if want_input_grad else grads

    def _bwd_for(self, n_samples: int) -> torch.Tensor:
        bwd = getattr(self, "_bwd_ws", None)
        if bwd is None or bwd[0] != n_samples:
            bwd = self._bwd_ws = (n_samples, torch.empty(self.bwd_bytes(n_samples), dtype=torch.uint8, device=self.device))
        return bwd[1]

    def backward_data(self, acts: torch.Tensor, packed: torch.Tensor, dq: torch.Tensor, n_samples: int, pixel_units: bool = False) -> torch.Tensor:
        """dL/d(frames) f32 [n_samples * num_frames, 3, 224, 224] of one `forward_saved` / `forward_attrib` call from dL/dQ, and nothing
        else (vdqn_net_backward_data): the data-gradient chain on the current stream, no weight gradient, no flat gradient buffer.
        The bits of `backward_from_dq(.., want_input_grad=True)`'s gx.  extra_capacity only."""
        self._need_gpu()
        if not self.extra_capacity:
            raise _lib.VdqnError("backward_data: ARCHITECTURE='basic' has no frame gradient (extra_capacity only)")
        with torch.cuda.device(self.device):
            dq = dq.to(device=self.device, dtype=torch.float32).contiguous()
            a = _lib.StepArgs()
            a.packed_online = _ptr(packed)
            a.batch = a.acts_samples = n_samples
            a.acts_online, a.bwd = _ptr(acts), _ptr(self._bwd_for(n_samples))
            gx = torch.empty((n_samples * self.num_frames, 3, 224, 224), dtype=torch.float32, device=self.device)
            _lib.check(self.lib.vdqn_net_backward_data(self.handle, C.byref(a), _ptr(dq), _ptr(gx), int(bool(pixel_units)), _stream()),
                       "vdqn_net_backward_data")
            dq.record_stream(torch.cuda.current_stream())
        return gx

    def forward_attrib(self, src: torch.Tensor, n_copies: int, packed: torch.Tensor, *, coef: Optional[torch.Tensor] = None, baseline=None,
                       sigma=None, seed: int = 0, s0: int = 0, i0: int = 0, acts: Optional[torch.Tensor] = None):
        """`forward_saved` over `n_copies` perturbed copies of the frames `src` (uint8 [n,224,224,3] or f32 [n,3,224,224], n a whole
        number of samples), built by the pack itself (vdqn_net_forward_attrib; arguments as ops.attrib_pack): -> (q [n_copies * n /
        num_frames, num_classes * action_dim], acts).  Copy s of sample b is sample s * (n / num_frames) + b.  `acts`: a workspace
        of that many samples to reuse."""
        self._need_gpu()
        if not self.extra_capacity:
            raise _lib.VdqnError("forward_attrib: ARCHITECTURE='basic' has no frame gradient to attribute with (extra_capacity only)")
        if (coef is None) == (sigma is None):
            raise _lib.VdqnError("forward_attrib: give coef (path mode) or sigma (noise mode), not both")
        shared, keep = attrib_source_args(src, baseline)
        n_samples, rest = divmod(n_copies * src.shape[0], self.num_frames)
        if rest or src.shape[0] % self.num_frames or n_copies < 1:
            raise _lib.VdqnError(f"forward_attrib: {n_copies} copies of {src.shape[0]} frames are not whole samples of {self.num_frames} frames")
        if n_samples > self.max_batch:
            raise _lib.VdqnError(f"batch {n_samples} exceeds max_batch {self.max_batch}")
        with torch.cuda.device(self.device):
            q = torch.empty((n_samples, self.num_classes * self.action_dim), dtype=torch.float32, device=self.device)
            if acts is None:
                acts = torch.empty(self.acts_bytes(n_samples), dtype=torch.uint8, device=self.device)
            sg = None if sigma is None else (C.c_float * 3)(*[float(v) for v in sigma])
            _lib.check(self.lib.vdqn_net_forward_attrib(self.handle, _ptr(packed), *shared, n_copies, 0 if coef is not None else 1, _ptr(coef), sg,
                                                        int(seed) & (2**64 - 1), s0, i0, n_samples, _ptr(acts), _ptr(q), _stream()),
                       "vdqn_net_forward_attrib")
        del keep
        return q, acts

    # ---- SyncBN (ARCHITECTURE='basic' under data parallelism) ----------------------------------------
    def set_bn_sync(self, world_size: int, allreduce=None) -> None:
        """Make the train-mode BatchNorm statistics global over ``world_size`` ranks (N ranks == one big batch, as the
        single-process reference computes them).  ``allreduce(t)`` must SUM-all-reduce the f32 device tensor ``t`` in
        place on the current stream; default: ``torch.distributed.all_reduce``.  world_size <= 1 switches it off."""
        self._need_gpu()
        if world_size <= 1:
            _lib.check(self.lib.vdqn_net_set_bn_sync(self.handle, None, None, 1), "vdqn_net_set_bn_sync")
            self._bn_sync_cb = None
            return
        if allreduce is None:
            import torch.distributed as dist

            def allreduce(t):
                dist.all_reduce(t)
        owners = self._sync_buffers = getattr(self, "_sync_buffers", [])

        def cb(user, buf, count, stream):
            # `buf` lies inside one of the activation workspaces this engine was handed: wrap it as a tensor view
            for ref in owners:
                t = ref()
                if t is None:
                    continue
                off = buf - t.data_ptr()
                if 0 <= off and off + 4 * count <= t.numel():
                    allreduce(t[off:off + 4 * count].view(torch.float32))
                    return
            raise _lib.VdqnError("SyncBN: statistics buffer is not inside a registered activation workspace")
        self._bn_sync_cb = _lib.ALLREDUCE_FN(cb)  # keep the trampoline alive
        _lib.check(self.lib.vdqn_net_set_bn_sync(self.handle, C.cast(self._bn_sync_cb, C.c_void_p), None, int(world_size)),
                   "vdqn_net_set_bn_sync")

    def register_sync_buffer(self, t: torch.Tensor) -> None:
        import weakref
        lst = self._sync_buffers = getattr(self, "_sync_buffers", [])
        lst[:] = [r for r in lst if r() is not None]
        if not any(r() is t for r in lst):
            lst.append(weakref.ref(t))

    def forward_train(self, frames: torch.Tensor, src_kind: int, n_samples: int) -> torch.Tensor:
        """ARCHITECTURE='basic' with the module in train mode: batch statistics per frame slot, running statistics and
        num_batches_tracked updated (one model call, archs/HabitatDQNMultiAction.py:44-54 under model.train())."""
        self._need_gpu()
        if self.extra_capacity:
            raise _lib.VdqnError("forward_train: extra_capacity keeps BatchNorm in eval mode; use forward()")
        if n_samples > self.max_batch:
            raise _lib.VdqnError(f"batch {n_samples} exceeds max_batch {self.max_batch}")
        with torch.cuda.device(self.device):
            q = torch.empty((n_samples, self.num_classes * self.action_dim), dtype=torch.float32, device=self.device)
            acts = self._acts_for(n_samples)
            self.register_sync_buffer(acts)
            self._packed_version = None  # self.packed now holds the un-folded weights
            _lib.check(self.lib.vdqn_net_forward_train(self.handle, _ptr(self.params), _ptr(self.bnstats), _ptr(self.packed),
                                                       _ptr(frames), src_kind, n_samples, _ptr(acts), _ptr(q), _stream()),
                       "vdqn_net_forward_train")
            self.num_batches_tracked += self.num_frames
        return q


class TDStepper:
    """Device state of the training loop: target-network weights, Adam moments, workspaces, and one TD update.

    ``step()`` follows train_q_network.py:213-227: target sync check (before the update), forward x3 (the two
    online passes run as one 2B batch), Double-DQN target + loss, backward, Adam.

    target_tau > 0 replaces the hard target copy by the soft update target <- target + tau (online - target) after every optimiser
    step: `target_params` (f32, all of `net.params`) is updated inside the Adam launches and folded into `packed_target` in front of
    every update; target_update_interval is then unused.  BatchNorm running statistics are copied from the online network, not
    averaged: the fold uses the online `bnstats` as they stand (constant in extra_capacity; in 'basic', those of the previous
    update)."""

    def __init__(self, net: NetEngine, batch: int, lr: float, gamma: float, clip_rect: bool, linear: bool = False,
                 remove_before_reward: bool = False, train_on_ground_truth: bool = False, value_learning: bool = False,
                 target_update_interval: int = 8000, betas=(0.9, 0.999), eps: float = 1e-8, world_size: int = 1,
                 allreduce=None, loss_kind: str = "l2", allreduce_loss=None, allreduce_wait=None, allreduce_errors=None,
                 grad_clip_norm: float = 0.0, weight_decay: float = 0.0, lr_fn=None, cql_alpha: float = 0.0,
                 target_tau: float = 0.0, mc_floor: bool = False, cql_calibrated: bool = False, iql_expectile: float = 0.0,
                 distributional: bool = False, kl_backwards: bool = False, log_sigma: bool = False, sigma_min: float = 0.1,
                 bcq_threshold: float = -1.0, bcq_bc_weight: float = 1.0, bcq_logit_reg: float = 0.01):
        net._need_gpu()
        self.net, self.B = net, batch
        self.lib = net.lib
        if 2 * batch > net.max_batch:
            raise _lib.VdqnError(f"TDStepper(batch={batch}) needs NetEngine(max_batch>={2 * batch})")
        self.lr, self.gamma, self.betas, self.eps = lr, gamma, betas, eps
        # grad_clip_norm > 0 (torch.nn.utils.clip_grad_norm_): the f64 norm of the whole flat gradient and the clip coefficient are
        # computed on the device (vdqn_grad_sumsq / vdqn_clip_finalize) and the coefficient reaches the Adam launch through device
        # memory — `clip_out` = {norm, coef} of the last update, never read back for the update itself.  No Adam launch may run
        # before that norm is known, so both early-Adam paths are off under clipping.  weight_decay: decoupled, as torch.optim.AdamW.
        # lr_fn(t) (optim.lr_at): host arithmetic, evaluated once per update from `sample_number` and passed to every Adam launch
        # of that update; `initial_lr` keeps the base rate for the checkpoint.  All three off: vdqn_adam, launched as ever.
        if not (grad_clip_norm >= 0.0) or not (weight_decay >= 0.0) or weight_decay == float("inf"):
            raise _lib.VdqnError("TDStepper: grad_clip_norm and weight_decay must be >= 0 (0 = off)")
        self.grad_clip_norm, self.weight_decay, self.lr_fn = float(grad_clip_norm), float(weight_decay), lr_fn
        self.initial_lr = lr
        self.clip_ws = self.clip_out = None
        self._clip_slots = 0  # norm partials of this update already queued by forward_backward (one slot per stage)
        self.clip_rect, self.linear, self.rbr = clip_rect, linear, remove_before_reward
        self.gtb, self.value_learning = train_on_ground_truth, value_learning
        if loss_kind not in LOSS_KINDS:
            raise _lib.VdqnError(f"loss_kind must be one of {sorted(LOSS_KINDS)} (reference: 'l2', train_q_network.py:167)")
        self.loss_kind = loss_kind
        # cql_alpha > 0 (conservative Q-learning for logged data): the loss launch is vdqn_td_loss_cql — alpha * (logsumexp_a Q(s, .) -
        # Q(s, a_data)) added to the TD loss, dq dense over the actions — and `cql_penalty` receives this rank's share of the
        # unscaled penalty.  0: vdqn_net_td_forward, launched as ever.
        cql_alpha = float(cql_alpha)
        if not (cql_alpha >= 0.0) or cql_alpha == float("inf"):
            raise _lib.VdqnError(f"TDStepper: cql_alpha must be finite and >= 0 (0 = off), not {cql_alpha}")
        if cql_alpha > 0 and train_on_ground_truth:
            raise _lib.VdqnError("TDStepper: cql_alpha applies to the TD branch only (train_on_ground_truth regresses on given targets)")
        if cql_alpha > 0 and net.action_dim < 2:
            raise _lib.VdqnError("TDStepper: cql_alpha needs action_dim >= 2 (with one action the penalty is identically zero)")
        self.cql_alpha = cql_alpha
        # mc_floor / cql_calibrated (video_dqn_amd/mcreturn.py): `step(mc_return=...)` hands the loss launch the Monte-Carlo return of
        # every sampled row — the floor y = max(y, G) in front of the rect clip (vdqn_td_loss_mc, mc_flags bit 0) and the calibrated
        # penalty, whose logsumexp runs over max(Q, G) (bit 1) — and `mc_stats` receives this rank's share of {the share of targets the
        # floor raises, the mean of Q(s, a_data) - G}.  Both off: the entries above, launched as ever.
        self.mc_flags = (1 if mc_floor else 0) | (2 if cql_calibrated else 0)
        if self.mc_flags and (train_on_ground_truth or linear):
            raise _lib.VdqnError("TDStepper: mc_floor / cql_calibrated apply to the TD branch without linear (train_on_ground_truth has no "
                                 "target to floor; y = r + (Qa - 0.1) has no discount)")
        if cql_calibrated and not cql_alpha > 0:
            raise _lib.VdqnError("TDStepper: cql_calibrated needs cql_alpha > 0 (there is no penalty to calibrate)")
        # The head algorithms (algos.py: one row each; at most one is on, `self.algo`): each needs the NetEngine with its head and runs
        # the update through its own entry.  All off: the entries above, launched as ever.  Their value checks, then the row's refusals.
        self.iql_expectile = iql_expectile = float(iql_expectile)
        if iql_expectile != 0.0 and not (0.5 <= iql_expectile < 1.0):
            raise _lib.VdqnError(f"TDStepper: iql_expectile must be 0 (off) or in [0.5, 1), not {iql_expectile}")
        for key, val in (("distributional", distributional), ("kl_backwards", kl_backwards), ("log_sigma", log_sigma)):
            if not isinstance(val, bool):
                raise _lib.VdqnError(f"TDStepper: {key} must be a bool, not {val!r}")
        if (kl_backwards or log_sigma) and not distributional:
            raise _lib.VdqnError("TDStepper: kl_backwards / log_sigma have no effect without distributional")
        self.distributional, self.sigma_min = distributional, float(sigma_min)
        if distributional and not (1e-4 <= self.sigma_min <= 10.0):
            raise _lib.VdqnError(f"TDStepper: sigma_min must be in [1e-4, 10], not {self.sigma_min}")
        self.dist_flags = (1 if kl_backwards else 0) | (2 if log_sigma else 0)
        bcq_threshold, bcq_bc_weight, bcq_logit_reg = float(bcq_threshold), float(bcq_bc_weight), float(bcq_logit_reg)
        if not (bcq_threshold == -1.0 or 0.0 <= bcq_threshold < 1.0):
            raise _lib.VdqnError(f"TDStepper: bcq_threshold must be -1 (off) or in [0, 1), not {bcq_threshold}")
        if not (math.isfinite(bcq_bc_weight) and bcq_bc_weight > 0):
            raise _lib.VdqnError(f"TDStepper: bcq_bc_weight must be finite and > 0, not {bcq_bc_weight}")
        if not (math.isfinite(bcq_logit_reg) and bcq_logit_reg >= 0):
            raise _lib.VdqnError(f"TDStepper: bcq_logit_reg must be finite and >= 0, not {bcq_logit_reg}")
        self.bcq_threshold, self.bcq_bc_weight, self.bcq_logit_reg = bcq_threshold, bcq_bc_weight, bcq_logit_reg
        facts = SimpleNamespace(TRAIN_ON_GROUND_TRUTH=train_on_ground_truth, LINEAR=linear, LOSS_KIND=loss_kind, CQL_ALPHA=cql_alpha,
                                CQL_CALIBRATED=cql_calibrated, MC_RETURN_FLOOR=mc_floor, IQL_EXPECTILE=iql_expectile,
                                DISTRIBUTIONAL=distributional, BCQ_THRESHOLD=bcq_threshold)
        names = {key: arg for key, arg, *_ in MODIFIERS + tuple(p for a in ALGOS for p in a.params)}
        self.algo = None
        for algo in (a for a in ALGOS if a.is_on(facts)):
            if getattr(net, "head", None) != algo.head:
                raise _lib.VdqnError(f"TDStepper: {names[algo.key]} needs a network with the {algo.head} head (NetEngine({algo.head}_head=True))")
            refuse(algo, facts, lambda key: names.get(key, key.lower()), _lib.VdqnError, "TDStepper: ")
            self.algo = algo
        self.bcq = self.algo is BCQ
        # target_tau > 0 (soft / Polyak target updates): `target_params`, an f32 copy of the whole flat `net.params` (the trainable
        # prefix and the frozen resnet.fc tail), follows the online weights as target <- target + tau (params - target) inside every
        # Adam launch (vdqn_adam_polyak), and `packed_target` is folded from it in front of every update; target_update_interval is
        # not consulted.  The averaged weights live in f32 there, never in `packed_target`: a bf16 packed weight cannot hold an
        # increment of half a percent.  BatchNorm running statistics are copied, not averaged (as stable-baselines3's polyak_update
        # treats buffers): the fold takes the online `bnstats` as they stand — in extra_capacity they never change, in 'basic' they
        # are those the previous update left.  0: none of this exists — no allocation, no launch, the same bits.
        target_tau = float(target_tau)
        if not (0.0 <= target_tau <= 1.0):  # (a NaN fails both comparisons)
            raise _lib.VdqnError(f"TDStepper: target_tau must be a finite number in [0, 1] (0 = hard target copies), not {target_tau}")
        if target_tau > 0 and train_on_ground_truth:
            raise _lib.VdqnError("TDStepper: target_tau applies to the TD branch only (train_on_ground_truth has no target network)")
        self.target_tau = target_tau
        self.target_params = None
        self.tui = target_update_interval
        self.world_size = world_size
        self.allreduce = allreduce  # callable(tensor_slice, stage) or None
        # callable(loss) or None: called once per update behind the LAST gradient bucket, on the gradient stream — the exchange
        # sums the ranks' loss shares there, so the compute stream never waits for a 4-byte collective (dist.launch_loss)
        self.allreduce_loss = allreduce_loss
        # callable() or None: orders the current stream behind the bucket launched last (dist.wait_last).  With VDQN_DIST_EARLY_ADAM=1
        # the optimiser update of stage 0 / stage 1 then runs behind ITS bucket on a stream of its own, under the rest of the backward
        # pass, instead of behind the last bucket (off by default: DESIGN.md section 7 has the measurement)
        self.allreduce_wait = allreduce_wait
        # callable() or None: with step(td_error=...) under data parallelism, queued behind the loss exchange on the gradient stream
        # (dist.launch_errors: the SUM of the ranks' slices of the prioritized-replay error buffer; `finish_allreduce` waits for it)
        self.allreduce_errors = allreduce_errors
        self._post_stream = None
        self._post_used = False
        dev = net.device
        nt = net.trainable_numel
        with torch.cuda.device(dev):
            self.packed_online = torch.zeros(net.packed_bytes, dtype=torch.uint8, device=dev)
            self.packed_target = torch.zeros(net.packed_bytes, dtype=torch.uint8, device=dev)
            n_online = batch if self.gtb else 2 * batch
            self.layout_samples = n_online  # what vdqn_net_act_offset must be asked for to find a tensor inside acts_online
            self.acts_online = torch.empty(net.acts_bytes(n_online), dtype=torch.uint8, device=dev)
            self.acts_target = None if self.gtb else torch.empty(net.acts_bytes(batch), dtype=torch.uint8, device=dev)
            net.register_sync_buffer(self.acts_online)
            self.bwd = torch.empty(net.bwd_bytes(batch), dtype=torch.uint8, device=dev)
            self.grads = torch.zeros(nt, dtype=torch.float32, device=dev)
            self.exp_avg = torch.zeros(nt, dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(nt, dtype=torch.float32, device=dev)
            self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
            # what the loss launch writes beside the loss.  The TD family: cql_penalty in slot 0, mc_stats in slots 1..2; a head
            # algorithm (never beside them): its statistics from slot 0
            self.loss_stats = torch.zeros(LOSS_SLOTS, dtype=torch.float32, device=dev)
            self.cql_penalty, self.mc_stats = self.loss_stats[0:1], self.loss_stats[1:3]
            for a in ALGOS:
                setattr(self, a.stats_attr, self.loss_stats[:len(a.stats)])
            self.q_before = torch.zeros((batch, net.num_classes * net.action_dim), dtype=torch.float32, device=dev)
            self._ones = torch.ones((batch, net.num_classes), dtype=torch.float32, device=dev)
            if self.grad_clip_norm > 0:
                self.clip_ws = torch.zeros(self.lib.vdqn_clip_workspace_bytes(3) // 8, dtype=torch.float64, device=dev)
                self.clip_out = torch.zeros(2, dtype=torch.float32, device=dev)
            if self.target_tau > 0:
                self.target_params = torch.empty_like(net.params)
        self.eval_acc = None   # f64 [num_classes][8] metric sums of the validation pass, allocated by the first eval_begin
        self.eval_head_acc = None  # f64 [num_classes + 1][8], the head algorithm's sums beside them (None without one)
        self.val_history = []  # (update number, eval_result()) of every validation pass the trainer ran
        self.adam_step = 0
        self.sample_number = 0
        self._grad_stream = None  # torch view of the engine's side stream (vdqn_net_grad_stream)
        self._adam_done = []
        self._packed_bufs, self._ahead = [None, None], None
        self.stage_ranges = [net.stage_range(s) for s in range(3)]
        # the three stage ranges tile [0, trainable_numel) (in whatever order): a norm taken stage by stage covers every element once
        r = sorted(self.stage_ranges)
        self._stages_tile = r[0][0] == 0 and r[-1][1] == nt and all(e > b for b, e in r) and all(r[i][1] == r[i + 1][0] for i in range(2))
        self.sync_target()

    def sync_target(self):
        """target_net.load_state_dict(model.state_dict()) (train_q_network.py:121,208,216): the target network
        only ever runs forward, so its state is the packed (BN-folded) copy of the current online weights.

        With target_tau > 0 the copy goes into `target_params` (all of `net.params`, the frozen tail included), and the packed copy
        is made from there with the online BatchNorm statistics."""
        with torch.cuda.device(self.net.device):
            if self.target_params is not None:
                self.target_params.copy_(self.net.params)
                self.net.pack_weights(self.packed_target, with_dgrad=False, params=self.target_params)
                return
            self.net.pack_weights(self.packed_target, with_dgrad=False)

    def _args(self, before, after, src_kind, act, rew, term, valid, gt, weights=None, td_error=None, augment=None,
              discount=None, augment_color=None, augment_zoom=None) -> _lib.StepArgs:
        n = self.net
        a = _lib.StepArgs()
        a.params, a.bnstats = _ptr(n.params), _ptr(n.bnstats)
        a.packed_online, a.packed_target = _ptr(self.packed_online), _ptr(self.packed_target)
        a.before, a.after, a.src_kind, a.batch = _ptr(before), _ptr(after), src_kind, self.B
        a.act, a.rew, a.term, a.valid, a.gt = _ptr(act), _ptr(rew), _ptr(term), _ptr(valid), _ptr(gt)
        a.gamma = self.gamma
        a.inv_count = 1.0 / (n.num_classes * self.B * self.world_size)
        a.clip_rect, a.linear, a.use_valid = int(self.clip_rect), int(self.linear), int(self.rbr)
        a.train_on_ground_truth, a.value_learning = int(self.gtb), int(self.value_learning)
        a.acts_online, a.acts_target, a.bwd = _ptr(self.acts_online), _ptr(self.acts_target), _ptr(self.bwd)
        a.grads, a.loss, a.q_before = _ptr(self.grads), _ptr(self.loss), _ptr(self.q_before)
        a.loss_kind = LOSS_KINDS[self.loss_kind]
        a.packed_frames = None
        a.sample_weight, a.sample_err, a.aug_params = _ptr(weights), _ptr(td_error), _ptr(augment)
        a.aug_color, a.aug_zoom = _ptr(augment_color), _ptr(augment_zoom)
        a.sample_gamma = _ptr(discount)
        return a

    # ---- frames packed one update ahead (vdqn_step_args.packed_frames) -----------------------------------------------------
    def _dist_early_ok(self) -> bool:
        """Per-bucket Adam under an exchange (VDQN_DIST_EARLY_ADAM) is taken only where it is right: modes 2 / 3 are one-rank
        diagnostics (mode 2 would update with gradients that have not been reduced) and raise with more ranks; mode 1 needs a
        backend whose Work.wait() orders the STREAM (RCCL) — gloo's blocks the host thread, which would serialise the enqueue of the
        remaining backward stages — and falls back to the finish-time update elsewhere."""
        ok = getattr(self, "_dist_early_checked", None)
        if ok is None:
            ok = True
            if self.world_size > 1:
                if _DIST_EARLY_ADAM_MODE in ("2", "3"):
                    raise RuntimeError("VDQN_DIST_EARLY_ADAM=2/3 are one-rank diagnostics: with world_size > 1 they apply unreduced gradients")
                try:
                    import torch.distributed as dist
                    ok = not dist.is_initialized() or dist.get_backend() == "nccl"
                except Exception:  # noqa: BLE001 - a caller-supplied exchange without torch.distributed
                    ok = True
            self._dist_early_checked = ok
        return ok

    @staticmethod
    def _frames_key(before, after, src_kind):
        # identity AND content version: a loop that refills fixed staging buffers in place (copy_ advances `_version`) announces
        # a different key than the one that arrives, so the stale pack is discarded and the call packs its own frames
        return (before.data_ptr(), None if after is None else after.data_ptr(), int(src_kind), tuple(before.shape), before.dtype,
                before._version, None if after is None else after._version)

    def _packed_buffer(self, slot: int) -> torch.Tensor:
        if self._packed_bufs[slot] is None:
            n = self.net
            esz = 2 if n.dtype_name == "bf16" else 4
            nbytes = 2 * self.B * n.num_frames * 115 * 115 * 16 * esz
            self._packed_bufs[slot] = torch.empty(nbytes, dtype=torch.uint8, device=n.device)
        return self._packed_bufs[slot]

    def _pack_ahead(self, next_frames, slot: int):
        """Queue vdqn_pack_input for the NEXT update's frames on the engine's gradient stream — behind this update's target pass,
        i.e. under its head and backward pass — into packed-frame buffer `slot` (the other one is being read by this update)."""
        nb, na, nk = next_frames
        n = self.net
        buf = self._packed_buffer(slot)
        nf = self.B * n.num_frames
        half = buf.numel() // 2
        dt = _lib.VDQN_BF16 if n.dtype_name == "bf16" else _lib.VDQN_F32
        main = torch.cuda.current_stream()
        with self._grad_stream_ctx():
            # the announced tensors may have been produced on the caller's stream a moment ago (a host-to-device copy, a gather)
            torch.cuda.current_stream().wait_stream(main)
            _lib.check(self.lib.vdqn_pack_input(_ptr(nb), int(nk), buf.data_ptr(), nf, dt, _stream()), "vdqn_pack_input")
            if na is not None and not self.gtb:
                _lib.check(self.lib.vdqn_pack_input(_ptr(na), int(nk), buf.data_ptr() + half, nf, dt, _stream()), "vdqn_pack_input")
        self._ahead = (self._frames_key(nb, na, nk), slot, (nb, na))  # (the tensors are kept alive until they are consumed)

    def _pack_affine(self, before, after, augment, augment_color, augment_affine) -> int:
        """Pack this update's frames with vdqn_pack_input_aug_affine on the current stream — `before` into the first half of packed-frame
        buffer 0 and `after` (TD branch) into the second, with the same rows — and return the buffer's address for
        vdqn_step_args.packed_frames: the struct has no field for affine rows, and every engine entry already reads packed frames."""
        n = self.net
        buf = self._packed_buffer(0)
        nf = self.B * n.num_frames
        dt = _lib.VDQN_BF16 if n.dtype_name == "bf16" else _lib.VDQN_F32
        for src, off in ((before, 0),) if self.gtb else ((before, 0), (after, buf.numel() // 2)):
            _lib.check(self.lib.vdqn_pack_input_aug_affine(_ptr(src), buf.data_ptr() + off, nf, n.num_frames, _ptr(augment), _ptr(augment_color),
                                                           _ptr(augment_affine), self.B, dt, _stream()), "vdqn_pack_input_aug_affine")
        return buf.data_ptr()

    def forward_backward(self, before, after, src_kind, act, rew, term, valid=None, gt=None, early_adam: bool = False, next_frames=None,
                         *, weights=None, td_error=None, augment=None, discount=None, augment_color=None, mc_return=None,
                         augment_zoom=None, augment_affine=None):
        """Everything of one update up to (and including) the gradient all-reduce; no optimiser step.

        early_adam (only `step` passes it: single process, no exchange, eval-mode BatchNorm): the optimiser update of stage 0 and stage 1 is
        queued on the engine's gradient stream right behind that stage's gradient unpack, so it runs under the remaining data /
        weight gradients instead of behind them (nothing later in the update reads those master parameters: the kernels work on
        the packed copies); `optimizer_step` then only covers what is left.  Same arithmetic, same results.

        weights, td_error, augment, discount, augment_color, augment_zoom: as `step` describes and validates them (vdqn_step_args.
        sample_weight / sample_err / aug_params / sample_gamma / aug_color / aug_zoom); mc_return: vdqn_net_td_forward_mc's plain argument;
        augment_affine: as `step` describes it — the frames are packed here with `augment` and `augment_color` and handed over as
        vdqn_step_args.packed_frames, and the three aug_* pointers stay NULL."""
        if augment_affine is not None:
            self._check_affine(augment, augment_zoom, augment_affine, src_kind, next_frames)
        n = self.net
        self._adam_done = []
        self._clip_slots = 0
        keep = (before, after, act, rew, term, valid, gt, weights, td_error, augment, discount, augment_color, mc_return, augment_zoom,
                augment_affine)  # keep inputs alive until the launches are queued
        with torch.cuda.device(n.device):
            if augment_affine is None:
                a = self._args(before, after, src_kind, act, rew, term, valid if valid is not None else self._ones, gt, weights, td_error, augment,
                               discount, augment_color, augment_zoom)
            else:
                a = self._args(before, after, src_kind, act, rew, term, valid if valid is not None else self._ones, gt, weights, td_error,
                               discount=discount)
            st = _stream()
            ahead, self._ahead = self._ahead, None  # (with affine rows a pending pack-ahead, packed without them, is discarded here)
            slot = None
            if augment_affine is not None:
                a.packed_frames = self._pack_affine(before, after, augment, augment_color, augment_affine)
            elif ahead is not None and ahead[0] == self._frames_key(before, after, src_kind):
                slot = ahead[1]  # these frames were packed during the previous update (ordered in front of `st` by its last stage)
                a.packed_frames = self._packed_buffer(slot).data_ptr()
            if self.algo is not None:
                entry, args = self.algo.entry, (*self.algo.entry_args(self), getattr(self, self.algo.stats_attr).data_ptr())
            elif mc_return is not None:
                entry, args = "vdqn_net_td_forward_mc", (self.cql_alpha, self.cql_penalty.data_ptr(), mc_return.data_ptr(), self.mc_flags,
                                                         self.mc_stats.data_ptr())
            elif self.cql_alpha > 0:
                entry, args = "vdqn_net_td_forward_cql", (self.cql_alpha, self.cql_penalty.data_ptr())
            else:
                entry, args = "vdqn_net_td_forward", ()
            _lib.check(getattr(self.lib, entry)(n.handle, C.byref(a), *args, st), entry)
            err_ready = None
            if td_error is not None and self.allreduce_errors is not None:  # the loss launch has written this rank's errors on `st`
                err_ready = torch.cuda.Event()
                err_ready.record()
            if next_frames is not None:
                # next_frames that ALIAS this call's tensors (same storage) are packed ahead only under the caller's explicit promise
                # that the content stays as it is — a fourth element True: a loop that replays one resident minibatch.  Without the
                # promise an aliased announcement is ignored (the next call packs its own frames, always correct): `_version` in
                # _frames_key catches in-place refills through torch ops, but not writes through `.data`, DLPack / numpy views or a
                # native kernel's pointer, and a stale pack would train on the previous minibatch without any error.
                nb_, na_ = next_frames[0], next_frames[1]
                aliased = nb_.data_ptr() == before.data_ptr() or (na_ is not None and after is not None and na_.data_ptr() == after.data_ptr())
                if not aliased or (len(next_frames) > 3 and next_frames[3] is True):
                    self._pack_ahead(next_frames[:3], 1 if slot == 0 else 0)
            if not n.extra_capacity:  # train-mode BatchNorm: model(before) [+ model(after)], F feature calls each
                n.num_batches_tracked += (1 if self.gtb else 2) * n.num_frames
                n.mark_dirty()  # the running statistics changed: eval-mode packed weights are stale
            for stage in range(3):
                _lib.check(self.lib.vdqn_net_backward_stage(n.handle, C.byref(a), stage, st), "vdqn_net_backward_stage")
                if self.allreduce is not None:
                    # the stage's gradients are complete on the engine's gradient stream, not on `st` (which is already
                    # running the next stage's data gradients): the collective is ordered behind that stream
                    b, e = self.stage_ranges[stage]
                    with self._grad_stream_ctx():
                        self.allreduce(self.grads[b:e], stage)
                        if stage == 2 and self.allreduce_loss is not None:
                            self.allreduce_loss(self.loss)
                        if stage == 2 and err_ready is not None:
                            torch.cuda.current_stream().wait_event(err_ready)
                            self.allreduce_errors()
                    if _DIST_EARLY_ADAM and stage < 2 and self.allreduce_wait is not None and n.extra_capacity and self.grad_clip_norm == 0 \
                            and self._dist_early_ok():
                        b4, e4 = (b + 3) // 4 * 4, e // 4 * 4
                        if e4 > b4:
                            if self._post_stream is None:
                                self._post_stream = torch.cuda.Stream(device=n.device)
                            with torch.cuda.stream(self._post_stream):
                                if _DIST_EARLY_ADAM_MODE != "2":
                                    self.allreduce_wait()  # this bucket's collective, nothing else
                                else:  # (diagnostic: ordered behind the gradient stream only)
                                    torch.cuda.current_stream().wait_stream(self._grad_stream)
                                if _DIST_EARLY_ADAM_MODE != "3":
                                    self._adam_range(b4, e4, self.adam_step + 1)
                            if _DIST_EARLY_ADAM_MODE != "3":
                                self._adam_done.append((b4, e4))
                            self._post_used = True
                elif self.grad_clip_norm > 0 and self._stages_tile:
                    # single process: this stage's share of the norm right behind its gradient unpack, under the rest of the backward
                    # pass (stage 2's unpack has been joined back into `st`); finalise and Adam follow the last stage (optimizer_step).
                    # Under an exchange the norm is that of the REDUCED gradient, taken in optimizer_step behind `finish_allreduce`
                    b, e = self.stage_ranges[stage]
                    with (self._grad_stream_ctx() if stage < 2 else contextlib.nullcontext()):
                        _lib.check(self.lib.vdqn_grad_sumsq(self.grads.data_ptr() + 4 * b, e - b, self.clip_ws.data_ptr(), stage, _stream()),
                                   "vdqn_grad_sumsq")
                    self._clip_slots = stage + 1
                elif early_adam and stage < 2 and self.grad_clip_norm == 0:
                    b, e = self.stage_ranges[stage]
                    b, e = (b + 3) // 4 * 4, e // 4 * 4  # vdqn_adam wants 16-byte aligned ranges; the rest is left to optimizer_step
                    if e > b:
                        with self._grad_stream_ctx():
                            self._adam_range(b, e, self.adam_step + 1)
                        self._adam_done.append((b, e))
        del keep

    def _grad_stream_ctx(self):
        ptr = self.lib.vdqn_net_grad_stream(self.net.handle)
        if not ptr:
            return contextlib.nullcontext()
        if self._grad_stream is None or self._grad_stream.cuda_stream != ptr:
            self._grad_stream = torch.cuda.ExternalStream(ptr, device=self.net.device)
        return torch.cuda.stream(self._grad_stream)

    def _adam_range(self, b: int, e: int, step: int):
        """Adam (train_q_network.py:227) over the flat element range [b, e) on the current stream."""
        common = [t.data_ptr() + 4 * b for t in (self.net.params, self.grads, self.exp_avg, self.exp_avg_sq)]
        common += [e - b, step, self.lr, self.betas[0], self.betas[1], self.eps]
        scaled = [self.weight_decay, self.clip_out.data_ptr() + 4 if self.grad_clip_norm > 0 else None]
        if self.target_params is not None:
            # the soft target update rides in the Adam launch, wherever that is queued (optimizer_step, the early launches on the
            # gradient stream, the per-bucket ones on `_post_stream`): there is no window in which `params` has moved and
            # `target_params` has not, and whatever orders one array's writes orders the other's
            entry, args = "vdqn_adam_polyak", common + scaled + [self.target_params.data_ptr() + 4 * b, self.target_tau]
        elif self.grad_clip_norm > 0 or self.weight_decay != 0:
            entry, args = "vdqn_adam_scaled", common + scaled
        else:
            entry, args = "vdqn_adam", common
        _lib.check(getattr(self.lib, entry)(*args, _stream()), entry)

    def optimizer_step(self):
        n = self.net
        self.adam_step += 1
        done = sorted(getattr(self, "_adam_done", []))
        self._adam_done = []
        with torch.cuda.device(n.device):
            if self._post_used:  # per-bucket updates under an exchange ran on their own stream: join it
                torch.cuda.current_stream().wait_stream(self._post_stream)
                self._post_used = False
            if self.grad_clip_norm > 0:
                slots, self._clip_slots = self._clip_slots, 0
                if slots != 3:  # an exchange (or a caller's own gradient): the whole range as it stands on this stream, one slot
                    _lib.check(self.lib.vdqn_grad_sumsq(self.grads.data_ptr(), n.trainable_numel, self.clip_ws.data_ptr(), 0, _stream()),
                               "vdqn_grad_sumsq")
                    slots = 1
                _lib.check(self.lib.vdqn_clip_finalize(self.clip_ws.data_ptr(), slots, self.grad_clip_norm, self.clip_out.data_ptr(), _stream()),
                           "vdqn_clip_finalize")
            pos = 0  # everything of [0, trainable_numel) that `forward_backward(early_adam=True)` has not updated already
            for b, e in done + [(n.trainable_numel, n.trainable_numel)]:
                if b > pos:
                    self._adam_range(pos, b, self.adam_step)
                pos = max(pos, e)
        n.mark_dirty()

    # ---- held-out validation (vdqn_net_td_eval): forward-only TD metrics summed on the device ---------------------------------
    EVAL_SLOTS = ("count", "loss", "td_abs_error", "q_data", "q_max", "td_target", "cql_penalty", "action_agreement")

    def eval_begin(self):
        """Start a validation pass (the reference's unfilled `eval_losses`, train_q_network.py:183-186,240) on the current stream,
        behind `step()`: fold `packed_online` in eval mode — every training update refolds that buffer at its top, so it is free
        between updates — refold `packed_target` from the averaged weights under target_tau > 0, exactly as `step()` does in front
        of an update, and zero `eval_acc` (f64 [num_classes][8]).  What orders the next update's weight fold behind the Adam
        launches (stage 2's join of the gradient stream, `optimizer_step`'s wait for `_post_stream`) orders this fold the same way:
        it is queued on the stream they were joined into.  Nothing of the training state is written."""
        if self.gtb:
            raise _lib.VdqnError("TDStepper.eval_begin: validation covers the TD branch only (train_on_ground_truth has no target network)")
        n = self.net
        with torch.cuda.device(n.device):
            n.pack_weights(self.packed_online, with_dgrad=False)
            if self.target_params is not None:
                n.pack_weights(self.packed_target, with_dgrad=False, params=self.target_params)
            if self.eval_acc is None:
                self.eval_acc = torch.zeros((n.num_classes, 8), dtype=torch.float64, device=n.device)
            else:
                self.eval_acc.zero_()
            if self.algo is not None:  # the head table: the algorithm's own metrics, summed by a second launch per batch
                if self.eval_head_acc is None:
                    self.eval_head_acc = torch.zeros((n.num_classes + 1, HEAD_EVAL_SLOTS), dtype=torch.float64, device=n.device)
                else:
                    self.eval_head_acc.zero_()

    def eval_batch(self, before, after, src_kind, act, rew, term, valid=None):
        """Queue one held-out batch of 1 .. B samples behind `eval_begin`: the online pass over [s; s'], the target pass over s' and
        the metrics launch that adds this batch's sums into `eval_acc`.  No host synchronisation."""
        if self.eval_acc is None:
            raise _lib.VdqnError("TDStepper.eval_batch: call eval_begin first")
        nb = int(act.shape[0])
        if not 1 <= nb <= self.B:
            raise _lib.VdqnError(f"TDStepper.eval_batch: a batch of {nb} samples (1 .. {self.B})")
        if self.rbr and valid is None:
            raise _lib.VdqnError("TDStepper.eval_batch: remove_before_reward needs the valid mask")
        keep = (before, after, act, rew, term, valid)  # keep inputs alive until the launches are queued
        with torch.cuda.device(self.net.device):
            a = self._args(before, after, src_kind, act, rew, term, valid if valid is not None else self._ones, None)
            a.batch = nb
            if self.algo is not None:  # vdqn_net_td_eval and, behind its launch, the row's head metrics into eval_head_acc
                entry, args = self.algo.eval_entry, (*self.algo.eval_args(self), self.eval_acc.data_ptr(), self.eval_head_acc.data_ptr())
            else:
                entry, args = "vdqn_net_td_eval", (self.eval_acc.data_ptr(),)
            _lib.check(getattr(self.lib, entry)(self.net.handle, C.byref(a), *args, _stream()), entry)
        del keep

    def eval_result(self) -> dict:
        """Synchronise once and return the pass's means: {name: slot total / count} over all categories, {name + '_cat': [per
        category]}, 'count' (the number of valid (sample, category) terms) and 'table' (the raw f64 [num_classes][8] sums, CPU).
        Under a head algorithm also 'head': the same over the algorithm's eval_slots from the head table's category rows, for BCQ
        the means of eval_sample_slots over 'samples' from its per-sample row, and 'table' (f64 [num_classes + 1][8], CPU)."""
        if self.eval_acc is None:
            raise _lib.VdqnError("TDStepper.eval_result: call eval_begin first")
        if self.algo is not None:  # both tables in one copy: the one synchronisation of the pass
            both = torch.cat([self.eval_acc, self.eval_head_acc]).cpu()
            table, head = both[:self.eval_acc.shape[0]].clone(), both[self.eval_acc.shape[0]:].clone()
            out = self._eval_means(table)
            out["head"] = self._head_means(head)
            return out
        return self._eval_means(self.eval_acc.cpu())  # (the one synchronisation of the pass)

    def _eval_means(self, table) -> dict:
        total = table.sum(0)
        nan = float("nan")
        out = {"count": float(total[0]), "count_cat": [float(x) for x in table[:, 0]], "table": table}
        for k, name in enumerate(self.EVAL_SLOTS):
            if k == 0:
                continue
            out[name] = float(total[k] / total[0]) if total[0] > 0 else nan
            out[name + "_cat"] = [float(table[c, k] / table[c, 0]) if table[c, 0] > 0 else nan for c in range(table.shape[0])]
        return out

    def _head_means(self, head) -> dict:
        """eval_result()['head'] from the head table (CPU): the category rows as _eval_means reads its table, the per-sample row."""
        nan = float("nan")
        cats, per = head[:-1], head[-1]
        total = cats.sum(0)
        out = {"count": float(total[0]), "count_cat": [float(x) for x in cats[:, 0]], "table": head}
        for k, name in enumerate(self.algo.eval_slots):
            if k == 0:
                continue
            out[name] = float(total[k] / total[0]) if total[0] > 0 else nan
            out[name + "_cat"] = [float(cats[c, k] / cats[c, 0]) if cats[c, 0] > 0 else nan for c in range(cats.shape[0])]
        for k, name in enumerate(self.algo.eval_sample_slots):
            out[name] = float(per[0]) if k == 0 else (float(per[k] / per[0]) if per[0] > 0 else nan)
        return out

    @staticmethod
    def _check_input(name, t, dtype, shape):
        """`step`'s per-update input `t`, when given, is a contiguous `dtype` device tensor of `shape` ((n,): of n elements)."""
        if t is not None and not (t.dtype == dtype and t.is_contiguous() and t.is_cuda and
                                  (tuple(t.shape) == shape if len(shape) > 1 else t.numel() == shape[0])):
            raise _lib.VdqnError(f"TDStepper.step: {name} must be a contiguous {'f32' if dtype == torch.float32 else 'int32'} "
                                 f"{''.join(f'[{d}]' for d in shape)} device tensor")

    def _check_affine(self, augment, augment_zoom, augment_affine, src_kind, next_frames):
        """What `augment_affine` needs beside it; raised before anything is queued."""
        if augment is None:
            raise _lib.VdqnError("TDStepper.step: augment_affine needs augment as well (int32 zeros [B][4] = no shift, no mirror)")
        if augment_zoom is not None:
            raise _lib.VdqnError("TDStepper.step: augment_affine and augment_zoom are both given, but the affine rows already contain the zoom "
                                 "(aug_draw_rotate composes them): pass augment_affine alone")
        self._check_input("augment_affine", augment_affine, torch.int32, (self.B, 8))
        self._check_input("augment", augment, torch.int32, (self.B, 4))
        if src_kind != 0:
            raise _lib.VdqnError(f"TDStepper.step: augment_affine takes uint8 NHWC frames (src_kind 0), not src_kind {src_kind}")
        if next_frames is not None:
            raise _lib.VdqnError("TDStepper.step: next_frames are packed ahead without the augmentation; pass one or the other")

    def step(self, before, after, src_kind, act, rew, term, valid=None, gt=None, finish_allreduce=None, next_frames=None,
             weights=None, td_error=None, augment=None, discount=None, augment_color=None, mc_return=None,
             augment_zoom=None, augment_affine=None) -> torch.Tensor:
        """One iteration of the reference loop body (train_q_network.py:213-227).  Returns the device loss scalar
        (no host sync).

        next_frames = (before, after, src_kind) of the NEXT call, if the loop already has them (the reference's DataLoader does: it
        prefetches): they are normalised and packed for the stem while this update's head and backward pass run, instead of at
        the start of the next update.  The tensors must not change until that call (refills must go through version-bumping torch
        ops such as copy_; tensors that alias THIS call's are accepted only as (before, after, src_kind, True) — the caller's promise
        that they are replayed unchanged); a call whose frames are not the ones announced packs its own, as always.  Same arithmetic, same results — and, measured, a SLOWER update (5.81 against 5.74 ms,
        profiles/r03w_ab_pack_ahead.txt: the HBM-bound pack beside layer4 and the head costs more than the start of the update
        gains), so neither bench.py nor the trainer uses it by default; it stays for callers whose frames arrive packed
        (vdqn_step_args.packed_frames).

        weights (prioritized replay): f32 [B] importance weights on the device — the loss launch scales each sample's loss terms and
        dQ row by them (vdqn_step_args.sample_weight; ones give the unweighted update bit for bit).  td_error: f32 [B] on the device,
        where that launch writes each sample's mean |TD error| over the categories; under data parallelism `allreduce_errors` is
        then queued behind the loss exchange.  TD branch only.

        augment (video_dqn_amd/augment.py): int32 [B][4] {sx, sy, flip, 0} on the device — this update's frames (uint8 NHWC, src_kind
        0) are packed through vdqn_pack_input_aug with them, the same for `before` and `after` (vdqn_step_args.aug_params, this
        update only).  The caller passes the action labels that go with the mirrored samples (Augmenter.actions).

        discount (n-step returns, video_dqn_amd/nstep.py): f32 [B] on the device — sample b's target is rew[b] + discount[b] * (1 -
        term[b]) * Q(after[b]) where it is rew[b] + gamma * ... otherwise (vdqn_step_args.sample_gamma, this update only; nothing is
        kept between updates).  The caller passes the folded rewards and terminals and the `after` frames of each chain's last row
        (NStepWalker.walk).  A constant discount == gamma gives the update without it bit for bit.  TD branch without `linear`.

        augment_color (video_dqn_amd/augment.py): int32 [B][4] {f_b, f_c, f_s, 0} on the device, Q8 factors of brightness, contrast and
        saturation (256 = 1.0) — the frames go through vdqn_pack_input_aug_color with them and with `augment`, which must be given
        as well (zeros = no shift); the same for `before` and `after` (vdqn_step_args.aug_color, this update only).

        augment_zoom (video_dqn_amd/augment.py): int32 [B][4] {ax, ay, bx, by} on the device, the Q16 source step and origin of each
        sample's zoom window (65536, 65536, 0, 0 = the whole frame) — the frames go through vdqn_pack_input_aug_zoom with them, with
        `augment`, which must be given as well (zeros = no shift), and with `augment_color` when that is given; the same for `before`
        and `after` (vdqn_step_args.aug_zoom, this update only).

        augment_affine (video_dqn_amd/augment.py): int32 [B][8] {axx, axy, bx, 0, ayx, ayy, by, 0} on the device, each sample's rotation
        composed with its zoom (Augmenter.affine) — needs `augment` as well (zeros = no shift), goes with `augment_color` and refuses
        `augment_zoom` beside it (the rows contain the zoom).  vdqn_step_args has no field for them: the stepper packs `before` and
        `after` itself with vdqn_pack_input_aug_affine, on this stream in front of the engine entry, into a packed-frame buffer of
        its own (2 * B * F * 115 * 115 * 16 elements, allocated by the first such call) and hands that over as
        vdqn_step_args.packed_frames; the aug_* pointers stay NULL.  uint8 NHWC frames (src_kind 0) only; this update only.

        mc_return (video_dqn_amd/mcreturn.py): f32 [B][num_classes] on the device, the Monte-Carlo return of every sampled row
        (ReturnTable.G at the sampled rows; with n-step returns still the sampled row's, the whole-episode return against the n-step
        target).  Required exactly when the stepper was built with mc_floor or cql_calibrated; this update only.  A table of -inf
        gives the update without it bit for bit."""
        if (mc_return is not None) != bool(self.mc_flags):
            raise _lib.VdqnError("TDStepper.step: mc_return is required exactly when the stepper has mc_floor or cql_calibrated set "
                                 f"(mc_floor={bool(self.mc_flags & 1)}, cql_calibrated={bool(self.mc_flags & 2)}, "
                                 f"mc_return {'given' if mc_return is not None else 'missing'})")
        self._check_input("mc_return", mc_return, torch.float32, (self.B, self.net.num_classes))
        if augment_color is not None and augment is None:
            raise _lib.VdqnError("TDStepper.step: augment_color needs augment as well (int32 zeros [B][4] = no shift, no mirror)")
        self._check_input("augment_color", augment_color, torch.int32, (self.B, 4))
        if augment_zoom is not None and augment is None:
            raise _lib.VdqnError("TDStepper.step: augment_zoom needs augment as well (int32 zeros [B][4] = no shift, no mirror)")
        self._check_input("augment_zoom", augment_zoom, torch.int32, (self.B, 4))
        if augment_affine is not None:
            self._check_affine(augment, augment_zoom, augment_affine, src_kind, next_frames)
        if discount is not None and (self.gtb or self.linear):
            raise _lib.VdqnError("TDStepper.step: discount applies to the TD branch without LINEAR (TRAIN_ON_GROUND_TRUTH bootstraps "
                                 "nothing; y = r + (Qa - 0.1) has no discount)")
        self._check_input("discount", discount, torch.float32, (self.B,))
        self._check_input("augment", augment, torch.int32, (self.B, 4))
        if augment is not None:
            if next_frames is not None:
                raise _lib.VdqnError("TDStepper.step: next_frames are packed ahead without the augmentation; pass one or the other")
            self._ahead = None  # frames packed ahead by an earlier call were packed without it: this call packs its own
        if td_error is not None and weights is None:
            raise _lib.VdqnError("TDStepper.step: td_error needs weights (it is written by the weighted loss launch)")
        if weights is not None and self.gtb:
            raise _lib.VdqnError("TDStepper.step: sample weights apply to the TD branch only (TRAIN_ON_GROUND_TRUTH has no weighted loss)")
        self._check_input("weights", weights, torch.float32, (self.B,))
        self._check_input("td_error", td_error, torch.float32, (self.B,))
        self.sample_number += 1
        if self.target_params is not None:
            # Soft target: fold `packed_target` from the averaged weights for every update, on the caller's stream, immediately in
            # front of the online fold at the top of vdqn_net_td_forward.  No event of its own is needed: the Adam launches write
            # `params` and `target_params` together, so whatever already orders their writes of `params` before that online fold
            # (stage 2's join of the gradient stream, optimizer_step's wait for `_post_stream`) orders their writes of
            # `target_params` before this one; the previous update's target pass was joined into this stream before its loss
            # launch, so it has finished reading `packed_target`; and nothing else reads `target_params`.
            with torch.cuda.device(self.net.device):
                self.net.pack_weights(self.packed_target, with_dgrad=False, params=self.target_params)
        elif self.sample_number % self.tui == 0:
            self.sync_target()
        if self.lr_fn is not None:
            self.lr = float(self.lr_fn(self.sample_number))
        # (single process only: behind each RCCL bucket on a stream of its own it measured 7.22 vs 5.96 ms per update with one rank,
        # profiles/r03s_ab_rccl_early_adam.txt — with an exchange the whole optimiser update stays behind `finish_allreduce`)
        early = _EARLY_ADAM and self.net.extra_capacity and self.allreduce is None and finish_allreduce is None and self.grad_clip_norm == 0
        self.forward_backward(before, after, src_kind, act, rew, term, valid, gt, early_adam=early, next_frames=next_frames,
                              weights=weights, td_error=td_error, augment=augment, discount=discount, augment_color=augment_color, augment_zoom=augment_zoom,
                              mc_return=mc_return, augment_affine=augment_affine)
        if finish_allreduce is not None:
            finish_allreduce()
            self._clip_slots = 0  # the gradient has just been reduced: its norm is taken from what `grads` holds now
        self.optimizer_step()
        return self.loss
