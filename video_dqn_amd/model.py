"""``HabitatDQNMultiAction`` with the reference's Python surface, computing on the HIP engine.

Mirrors ``archs/HabitatDQNMultiAction.py:8-54`` and the factory/loader of ``train_q_network.py:36-57``:

  * same constructor arguments, same module tree (``resnet``, ``features``, ``top``) so ``state_dict()`` has
    the reference's 250 keys in the reference's order (``features.N.*`` alias ``resnet.*``), and
    ``load_state_dict(strict=True)`` accepts reference checkpoints unchanged;
  * ``forward(inp)`` takes ``float[B,3,224,224]`` / ``float[B,F,3,224,224]`` (normalised, as the reference's
    loader produces) and returns ``float32[B,5,A]``; raises ``Exception("bad shape")`` on a frame-count
    mismatch (:47-48).  Extension: a uint8 ``[B,(F,)224,224,3]`` tensor is normalised on the GPU inside the
    input-packing kernel (``util/torch.py:26-36`` semantics);
  * ``set_train()`` / ``eval()`` / ``train()`` set flags: in ``extra_capacity`` every BatchNorm layer runs on its
    running statistics in both modes (:37-40); in ``basic`` a forward in train mode normalises with batch statistics
    per frame slot and updates ``running_mean/var`` and ``num_batches_tracked`` like torch's BatchNorm2d.

The module's parameters and BatchNorm buffers are *views* into the engine's flat device arrays, so
``load_state_dict`` writes straight into what the kernels read.  The fast training path is the engine's fused update
(``video_dqn_amd.engine.TDStepper``: one 2B-frame online pass, early Adam, no autograd).  The module is ALSO
differentiable for ``extra_capacity`` (the shipped configuration): with grad mode on, ``forward`` runs as a
``torch.autograd.Function`` whose backward is the engine's staged backward of that one call
(``vdqn_net_backward_begin`` + ``vdqn_net_backward_stage``), parameters have ``requires_grad=True`` and receive
``.grad``, so the reference's own loop — ``model(before)``, ``target_net(after)``, ``model(after)``,
``loss.backward()``, ``optim.Adam(model.parameters()).step()`` (train_q_network.py:124,131,140-142,226-227) — runs
unmodified on the HIP kernels (three separate passes and torch's Adam: slower than ``TDStepper``, same numbers).
For ``extra_capacity`` a float input that requires a gradient receives one too (``vdqn_net_input_grad``: one more launch behind
the backward), and ``input_gradient`` / ``saliency`` give it without a graph.
No arithmetic happens on the CPU.
"""
from __future__ import annotations

import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import ops
from .algos import ALGOS
from .engine import NetEngine, _say_once, head_kept_message

# checkpoint key of an extra head -> its parameters: what the reference's three keys leave out and a key of its own carries
HEADS = {f"{a.head}_head": a.head_keys for a in ALGOS}


def head_of(net):
    """(checkpoint key, parameter names) of the extra head behind `net`'s Q layer, or (None, ()) without one."""
    name = getattr(net, "head", None)
    return (f"{name}_head", HEADS[f"{name}_head"]) if name else (None, ())


class _QFunction(torch.autograd.Function):
    """`model(x)` for autograd: forward = vdqn_net_forward into a workspace this call owns, backward = the engine's staged
    backward of that call from dL/dQ.  `params` are the module's trainable Parameters (slot order); their gradients are slices
    of one flat buffer.
    Frames that require a gradient (f32 [n_samples, F, 3, 224, 224]) receive dL/d(frames) from the same backward, one launch
    behind its last stage; where no parameter asks for a gradient, from the data-gradient chain alone (vdqn_net_backward_data)."""

    @staticmethod
    def forward(ctx, module, frames, src_kind, n_samples, *params):
        eng = module.engine
        packed = module._packed_with_dgrad()
        q, acts = eng.forward_saved(frames, src_kind, n_samples, packed)
        ctx.module, ctx.acts, ctx.packed, ctx.n = module, acts, packed, n_samples
        ctx.frames_shape = tuple(frames.shape)
        return q

    @staticmethod
    def backward(ctx, gq):
        module, eng = ctx.module, ctx.module.engine
        want_gx = ctx.needs_input_grad[1]
        if want_gx and not any(ctx.needs_input_grad[4:]):  # a frozen network: the data-gradient chain alone, the same bits
            gx = eng.backward_data(ctx.acts, ctx.packed, gq, ctx.n).view(ctx.frames_shape)
            ctx.acts = ctx.packed = None
            return (None, gx, None, None) + (None,) * len(ctx.needs_input_grad[4:])
        flat = eng.backward_from_dq(ctx.acts, ctx.packed, gq, ctx.n, want_input_grad=want_gx)
        gx = None
        if want_gx:
            flat, gx = flat
            gx = gx.view(ctx.frames_shape)
        ctx.acts = ctx.packed = None
        grads = tuple(flat[s.offset:s.offset + s.numel].view(s.shape) if need else None
                      for s, need in zip(module._trainable_slots, ctx.needs_input_grad[4:]))
        return (None, gx, None, None) + grads


class _Holder(nn.Module):
    """Parameter/buffer container that only contributes names to the state_dict (no forward)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("structure-only module: HabitatDQNMultiAction.forward runs on the HIP engine")


def _conv(holder_params, name, has_bias=False):
    m = _Holder()
    m.weight = holder_params(name + ".weight")
    m.bias = holder_params(name + ".bias") if has_bias else None
    return m


class _Stateless(_Holder):
    pass


def _init_like_reference(engine: NetEngine, seed=None):
    """Default initialisation when no pretrained file is given: torchvision's resnet init (kaiming_normal
    fan_out for convs, BatchNorm weight 1 / bias 0, running stats 0 / 1) and PyTorch's default Conv2d/Linear
    init for the head, drawn from the torch CPU generator (seeded by the trainer like train_q_network.py:86)."""
    g = None
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, s in engine.slots.items():
            v = engine.view(name)
            if s.kind == 2:
                v.zero_()
            elif s.kind == 3:
                v.fill_(1.0)
            elif name.startswith("resnet.") and len(s.shape) == 4:
                fan_out = s.shape[0] * s.shape[2] * s.shape[3]
                v.copy_(torch.randn(s.shape, generator=g) * (2.0 / fan_out) ** 0.5)
            elif name.startswith("resnet.") and (".bn" in name or ".downsample.1." in name):
                v.fill_(1.0 if name.endswith("weight") else 0.0)
            else:  # resnet.fc, features.8, top.*: kaiming_uniform(a=sqrt(5)) == U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                wname = name.rsplit(".", 1)[0] + ".weight"
                ws = engine.slots[wname].shape
                fan_in = ws[1] * (ws[2] * ws[3] if len(ws) == 4 else 1)
                bound = 1.0 / fan_in ** 0.5
                v.copy_((torch.rand(s.shape, generator=g) * 2 - 1) * bound)
    engine.mark_dirty()


def load_torchvision_resnet18(engine: NetEngine, sd, source: str = "state_dict") -> int:
    """`models.resnet18(pretrained=True)` (archs/HabitatDQNMultiAction.py:11) from a file: copy a torchvision-keyed ResNet-18
    state_dict ('conv1.weight', 'layer1.0.bn1.running_mean', ..., 'fc.bias') into the engine's `resnet.*` tensors.  Strict on
    everything the network computes with, as torchvision's own load_state_dict is: EVERY convolution and BatchNorm tensor of the
    trunk (20 convolutions, 20 BatchNorm layers with their running statistics) must be present with its exact shape; a file that
    covers only part of the trunk, or a tensor of the wrong shape (a ResNet-34 / a different width), is an error and nothing is
    copied.  The classifier `fc` is never on the path (archs/HabitatDQNMultiAction.py:30 cuts it off; it only rides along in the
    checkpoint): an ImageNet file's [1000, 512] fc is copied, a differently sized one — the 365-way fc of a Places365 ResNet-18,
    also wrapped as {'state_dict': ..., 'module.' prefixes} — is skipped with a warning and the engine keeps its own.
    `num_batches_tracked` entries are accepted and ignored (eval-mode statistics do not use them); any other unknown key is an
    error.  Returns the number of tensors copied."""
    if hasattr(sd, "state_dict"):
        sd = sd.state_dict()
    if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
        sd = sd["state_dict"]  # (Places365 checkpoints wrap the tensors this way)
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    want = {name[len("resnet."):]: s for name, s in engine.slots.items() if name.startswith("resnet.")}
    skip_fc = [k for k in ("fc.weight", "fc.bias") if k in sd and tuple(sd[k].shape) != tuple(want[k].shape)]
    if skip_fc or any(k not in sd for k in ("fc.weight", "fc.bias")):
        import warnings
        warnings.warn(f"{source}: the classifier fc ({[tuple(sd[k].shape) for k in skip_fc] or 'absent'}) does not match resnet.fc [1000, 512]; "
                      "it is not on the Q-network's path and is left at the engine's own values")
        want = {k: v for k, v in want.items() if not k.startswith("fc.")}
        sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
    missing = sorted(k for k in want if k not in sd)
    unknown = sorted(k for k in sd if k not in want and not k.endswith("num_batches_tracked"))
    wrong = sorted(f"{k}: {tuple(sd[k].shape)} != {tuple(want[k].shape)}" for k in want if k in sd and tuple(sd[k].shape) != tuple(want[k].shape))
    if missing or unknown or wrong:
        raise ValueError(f"{source} is not a torchvision ResNet-18 state_dict: {len(missing)} trunk tensors missing "
                         f"(e.g. {missing[:3]}), {len(unknown)} unknown keys (e.g. {unknown[:3]}), {len(wrong)} wrong shapes (e.g. {wrong[:3]})")
    with torch.no_grad():
        for k in want:
            engine.view("resnet." + k).copy_(sd[k].to(torch.float32))
    engine.mark_dirty()
    return len(want)


class HabitatDQNMultiAction(nn.Module):
    def __init__(self, action_dim, num_classes=5, extra_capacity=False, panorama=True, num_frames=None,
                 dtype=None, device=None, max_batch=64, pretrained_weights=None, deterministic=None, value_head=False,
                 distributional=False, log_sigma=False, sigma_min=0.1, policy_head=False):
        super().__init__()
        self.extra_capacity = extra_capacity
        self.num_classes = num_classes
        self.action_dim = action_dim
        self.panorama = panorama
        if num_frames is None:  # archs/HabitatDQNMultiAction.py:16-19
            num_frames = 4 if panorama else 1
        self.num_frames = num_frames
        dtype = dtype or os.environ.get("VDQN_DTYPE", "bf16")
        if extra_capacity:
            print("Model loading with extra_capacity")  # :28
        # value_head (implicit Q-learning, IQL_EXPECTILE): a child `value` with `weight` [num_classes, in] and `bias` [num_classes],
        # the rows of the Q layer behind the reference's; `forward` still returns the Q values alone, `state_values` the head's
        self.value_head = bool(value_head)
        # distributional (DISTRIBUTIONAL): a child `spread` with `weight` [num_classes * action_dim, in] and `bias`, one spread
        # parameter per Q column; `forward` still returns the means alone in (B, C, A), `distribution` mean and variance in
        # (B, C, A, 2) — what the reference's visualize_value.py:88-93 indexes — under log_sigma (LOG_SIGMA) and sigma_min
        self.distributional, self.log_sigma, self.sigma_min = bool(distributional), bool(log_sigma), float(sigma_min)
        # policy_head (BCQ_THRESHOLD): a child `policy` with `weight` [action_dim, in] and `bias` [action_dim], the behaviour logits;
        # `forward` still returns the Q values alone, `behaviour` the head's probabilities and `constrained_q` the Q values with
        # the actions the head finds implausible at -inf
        self.policy_head = bool(policy_head)
        self.engine = NetEngine(action_dim, num_classes, num_frames, extra_capacity, dtype, max_batch, device, deterministic,
                                value_head=self.value_head, spread_head=self.distributional, policy_head=self.policy_head)
        self._build_tree()
        _init_like_reference(self.engine)
        # models.resnet18(pretrained=True) (:11): the ImageNet weights come from a file (config key PRETRAINED_WEIGHTS, or the
        # VDQN_RESNET18_WEIGHTS environment variable) — without one the trunk keeps its random initialisation, and
        # `pretrained_loaded` stays False so the trainer can say so
        pre = pretrained_weights or os.environ.get("VDQN_RESNET18_WEIGHTS")
        self.pretrained_loaded = False
        if pre:
            load_torchvision_resnet18(self.engine, torch.load(pre, map_location="cpu"), source=str(pre))
            self.pretrained_loaded = True

    # ---- structure ----------------------------------------------------------------------------------
    def _build_tree(self):
        eng = self.engine
        cache = {}
        bn_count = [0]

        def P(name):
            # requires_grad as in the reference (every nn.Parameter, the never-used resnet.fc included: it simply never
            # receives a .grad, train_q_network.py:124); the Parameters share storage AND version counter with eng.params
            if name not in cache:
                cache[name] = nn.Parameter(eng.view(name), requires_grad=True)
            return cache[name]

        def bn(name):
            m = _Holder()
            m.weight, m.bias = P(name + ".weight"), P(name + ".bias")
            m.register_buffer("running_mean", eng.view(name + ".running_mean"))
            m.register_buffer("running_var", eng.view(name + ".running_var"))
            m.register_buffer("num_batches_tracked", eng.num_batches_tracked[bn_count[0]])  # 0-dim view
            bn_count[0] += 1
            return m

        resnet = _Holder()
        resnet.conv1 = _conv(P, "resnet.conv1")
        resnet.bn1 = bn("resnet.bn1")
        resnet.relu = _Stateless()
        resnet.maxpool = _Stateless()
        inpl = 64
        for li, planes in enumerate((64, 128, 256, 512), start=1):
            blocks = []
            for bi in range(2):
                p = f"resnet.layer{li}.{bi}"
                b = _Holder()
                b.conv1 = _conv(P, p + ".conv1")
                b.bn1 = bn(p + ".bn1")
                b.relu = _Stateless()
                b.conv2 = _conv(P, p + ".conv2")
                b.bn2 = bn(p + ".bn2")
                if (li > 1 and bi == 0) or inpl != planes:
                    b.downsample = nn.Sequential(_conv(P, p + ".downsample.0"), bn(p + ".downsample.1"))
                else:
                    b.downsample = None
                inpl = planes
                blocks.append(b)
            setattr(resnet, f"layer{li}", nn.Sequential(*blocks))
        resnet.avgpool = _Stateless()
        resnet.fc = _conv(P, "resnet.fc", has_bias=True)
        self.resnet = resnet
        # what torch.autograd differentiates `forward` with respect to: the trainable slots, in the engine's flat order
        self._trainable_slots = [s for s in eng.slots.values() if s.kind == 0]
        self._trainable_params = None  # filled after the tree is complete (below)
        self._cache = cache
        if self.extra_capacity:  # archs/HabitatDQNMultiAction.py:30-31
            self.features = nn.Sequential(*list(self.resnet.children())[:-2], _conv(P, "features.8", has_bias=True),
                                          _Stateless(), _Stateless())
            self.top = nn.Sequential(_conv(P, "top.0", True), _Stateless(), _conv(P, "top.2", True), _Stateless(),
                                     _conv(P, "top.4", True))
        else:  # :33-34
            self.features = nn.Sequential(*list(self.resnet.children())[:-1])
            self.top = _conv(P, "top", True)
        if eng.head:  # behind the reference's modules: state_dict() lists the reference's 250 keys first, then value.* / spread.* / policy.*
            setattr(self, eng.head, _conv(P, eng.head, True))
        object.__setattr__(self, "_trainable_params", [cache[s.name] for s in self._trainable_slots])
        del self._cache
        self._packed_grad = None      # packed weights incl. the data-gradient operands, for differentiable forwards
        self._packed_grad_key = None  # (engine version, version counter of the flat parameter array) they were packed from

    def _packed_with_dgrad(self):
        """The packed weights (BatchNorm folded, forward AND data-gradient operands) of the CURRENT parameters.  In-place
        updates by torch optimisers are seen through the version counter the Parameters share with the flat array; a new
        buffer is used whenever the parameters changed, so a graph that still holds the old one differentiates the weights
        its forward ran with."""
        eng = self.engine
        key = eng.version_key()
        if self._packed_grad is None or self._packed_grad_key != key:
            with torch.cuda.device(eng.device):
                self._packed_grad = torch.empty(eng.packed_bytes, dtype=torch.uint8, device=eng.device)
                eng.pack_weights(self._packed_grad, with_dgrad=True)
            self._packed_grad_key = key
        return self._packed_grad

    # ---- reference surface ----------------------------------------------------------------------------
    def set_train(self):  # :37-40
        self.train()
        if self.extra_capacity:
            self.resnet.eval()

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)

    def load_state_dict(self, state_dict, strict=True):
        keys = self.engine.head_keys
        if keys and not all(k in state_dict for k in keys):
            # a DQN (or reference) checkpoint into a model with an extra head, the warm start: the head keeps what it holds
            _say_once(head_kept_message(self.engine.head))
            state_dict = OrderedDict(state_dict)
            for k in keys:
                state_dict.setdefault(k, self.engine.view(k).detach().clone())
        r = super().load_state_dict(state_dict, strict=strict)
        self.engine.mark_dirty()
        return r

    def _apply(self, fn, recurse=True):
        # parameters are views into the engine's flat arrays; moving them would break the aliasing
        probe = fn(torch.empty(0, device=self.engine.device))
        if probe.device != self.engine.device or probe.dtype != torch.float32:
            raise RuntimeError("HabitatDQNMultiAction lives on its engine's device in f32 master precision; "
                               "construct it with device=... instead of calling .to()/.half()")
        return self

    def forward(self, inp):  # :44-54
        eng = self.engine
        if inp.dtype == torch.uint8:  # raw frames [B,(F,)224,224,3]
            if self.num_frames == 1 and inp.dim() == 4:
                inp = inp.unsqueeze(1)
            if inp.shape[1] != self.num_frames:
                raise Exception("bad shape")
            src_kind = 0
        else:
            if self.num_frames == 1 and len(inp.shape) == 4:
                inp = inp.unsqueeze(1)
            if inp.shape[1] != self.num_frames:
                raise Exception("bad shape")
            inp = inp.float()
            src_kind = 1
        if inp.requires_grad and not self.extra_capacity:
            raise NotImplementedError("HabitatDQNMultiAction with ARCHITECTURE='basic' on the HIP engine has no gradient of a frame (its "
                                      "train-mode BatchNorm backward exists inside the fused update only): detach the input, or use "
                                      "extra_capacity")
        b = inp.shape[0]
        inp = inp.to(eng.device).contiguous()
        if b > eng.max_batch:
            outs = [self.forward(inp[i:i + eng.max_batch]) for i in range(0, b, eng.max_batch)]
            return torch.cat(outs, 0)
        if self.training and not self.extra_capacity:  # the ResNet's BatchNorm layers are in train mode (:37-40)
            q = eng.forward_train(inp, src_kind, b)  # (no autograd graph: 'basic' trains through TDStepper)
        elif self.extra_capacity and torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in self._trainable_params)):
            # (frames that require a gradient build the graph on their own: saliency on a frozen network)
            q = _QFunction.apply(self, inp, src_kind, b, *self._trainable_params)
        else:
            q = eng.forward(inp, src_kind, b)
        return q.view((-1, self.num_classes, self.action_dim))

    def state_values(self, frames):
        """V(s) f32 [B, num_classes] of the value head, from the same forward pass that gives `forward(frames)` (no gradient)."""
        if not self.value_head:
            raise RuntimeError("state_values: the model was built without value_head=True")
        if frames.shape[0] > self.engine.max_batch:
            return torch.cat([self.state_values(frames[i:i + self.engine.max_batch]) for i in range(0, frames.shape[0], self.engine.max_batch)], 0)
        was_training = self.training
        self.training = False  # (this module's flag alone: the plain forward, 'basic' on its running statistics, nothing written)
        try:
            with torch.no_grad():
                q = self.forward(frames)
        finally:
            self.training = was_training
        return self.engine.state_values(q.shape[0])

    def distribution(self, frames):
        """f32 [B, num_classes, action_dim, 2]: [..., 0] the mean, the bits of `forward(frames)`, and [..., 1] the variance of the
        return of every (category, action), from one forward pass (no gradient)."""
        if not self.distributional:
            raise RuntimeError("distribution: the model was built without distributional=True")
        if frames.shape[0] > self.engine.max_batch:
            return torch.cat([self.distribution(frames[i:i + self.engine.max_batch]) for i in range(0, frames.shape[0], self.engine.max_batch)], 0)
        was_training = self.training
        self.training = False  # (this module's flag alone: the plain forward, 'basic' on its running statistics, nothing written)
        try:
            with torch.no_grad():
                q = self.forward(frames)
        finally:
            self.training = was_training
        return self.engine.dist_moments(q.shape[0], self.log_sigma, self.sigma_min)

    def _bcq_readout(self, frames, threshold):
        if not self.policy_head:
            raise RuntimeError("constrained_q / behaviour: the model was built without policy_head=True")
        if frames.shape[0] > self.engine.max_batch:
            parts = [self._bcq_readout(frames[i:i + self.engine.max_batch], threshold) for i in range(0, frames.shape[0], self.engine.max_batch)]
            return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)
        was_training = self.training
        self.training = False  # (this module's flag alone: the plain forward, 'basic' on its running statistics, nothing written)
        try:
            with torch.no_grad():
                q = self.forward(frames)
        finally:
            self.training = was_training
        return self.engine.bcq_constrain(q.shape[0], threshold)

    def constrained_q(self, frames, threshold):
        """f32 [B, num_classes, action_dim]: the bits of `forward(frames)`, with -inf at every action whose behaviour probability is
        not above `threshold` (in [0, 1)) times the largest one of its sample; from one forward pass (no gradient).  Its
        `argmax(-1)` is the BCQ policy."""
        return self._bcq_readout(frames, threshold)[0]

    def behaviour(self, frames):
        """f32 [B, action_dim]: the behaviour head's probabilities pi_b(a | s), from one forward pass (no gradient)."""
        return self._bcq_readout(frames, 0.0)[1]

    def input_gradient(self, frames, dq, pixel_units=False):
        """f32 [B, F, 3, 224, 224]: the gradient of sum(Q * dq) with respect to the frames, for `dq` [B, num_classes, action_dim].
        `frames` as `forward` takes them: uint8 [B,(F,)224,224,3] or normalised float [B,(F,)3,224,224]; the gradient is with
        respect to the normalised values, or with pixel_units to the uint8 pixel values (times 1 / (255 std_c)).  One forward and
        one backward on the engine in eval mode (the module's flag is left as it was); no autograd graph, no parameter gradient is
        kept.  extra_capacity only."""
        if not self.extra_capacity:
            raise NotImplementedError("input_gradient: ARCHITECTURE='basic' has no gradient of a frame on the HIP engine (extra_capacity only)")
        eng = self.engine
        src_kind = 0 if frames.dtype == torch.uint8 else 1
        if self.num_frames == 1 and frames.dim() == 4:
            frames = frames.unsqueeze(1)
        if frames.shape[1] != self.num_frames:
            raise Exception("bad shape")
        frames = (frames if src_kind == 0 else frames.detach().float()).to(eng.device).contiguous()
        b = frames.shape[0]
        dq = dq.reshape(b, self.num_classes * self.action_dim)
        if b > eng.max_batch:
            return torch.cat([self.input_gradient(frames[i:i + eng.max_batch], dq[i:i + eng.max_batch], pixel_units)
                              for i in range(0, b, eng.max_batch)], 0)
        was_training = self.training
        self.training = False  # (this module's flag alone, as in state_values)
        try:
            with torch.no_grad():
                packed = self._packed_with_dgrad()
                _, acts = eng.forward_saved(frames, src_kind, b, packed)
                gx = eng.backward_data(acts, packed, dq, b, pixel_units=pixel_units)
        finally:
            self.training = was_training
        return gx.view(b, self.num_frames, 3, 224, 224)

    def saliency(self, frames, category, action=None):
        """f32 [B, F, 224, 224]: the maximum over colour of |dQ[category, action] / d pixel|; action=None: the greedy action of
        every sample.  uint8 frames: per unit of the pixel value; float frames: per unit of the normalised value."""
        if not self.extra_capacity:
            raise NotImplementedError("saliency: ARCHITECTURE='basic' has no gradient of a frame on the HIP engine (extra_capacity only)")
        with torch.no_grad():
            q = self.forward(frames.detach())
        act = q[:, category].argmax(-1) if action is None else torch.full((q.shape[0],), int(action), device=q.device)
        dq = torch.zeros_like(q)
        dq[torch.arange(q.shape[0], device=q.device), category, act] = 1.0
        gx = self.input_gradient(frames, dq, pixel_units=(frames.dtype == torch.uint8))
        return ops.attrib_finish(gx.view(-1, 3, 224, 224)).view(gx.shape[0], self.num_frames, 224, 224)

    # ---- attribution: integrated gradients and SmoothGrad on the engine (csrc/attrib.hip) ------------------------------------------
    def _attrib_frames(self, what, frames):
        """-> (frames [B, F, ...] contiguous on the device, whether a frame axis was added); refuses 'basic' and bad shapes by name."""
        if not self.extra_capacity:
            raise NotImplementedError(f"{what}: ARCHITECTURE='basic' has no gradient of a frame on the HIP engine (extra_capacity only)")
        added = self.num_frames == 1 and frames.dim() == 4
        if added:
            frames = frames.unsqueeze(1)
        if frames.dim() != 5 or frames.shape[1] != self.num_frames:
            raise Exception("bad shape")
        frames = (frames if frames.dtype == torch.uint8 else frames.detach().float()).to(self.engine.device).contiguous()
        return frames, added

    def _attrib_target(self, frames, category, action):
        """(q [B, C, A], act [B], dq [B, C * A]) at `frames`: the one-hot dL/dQ of (category, action), action None = greedy."""
        with torch.no_grad():
            q = self.forward(frames)
        act = q[:, category].argmax(-1) if action is None else torch.full((q.shape[0],), int(action), device=q.device)
        dq = torch.zeros_like(q)
        dq[torch.arange(q.shape[0], device=q.device), category, act] = 1.0
        return q, act, dq.view(q.shape[0], -1)

    def _attrib_accumulate(self, frames, dq, n_copies, weight, squared, pixel_units, **pack):
        """sum over `n_copies` perturbed copies of weight * gradient (squared: weight * gradient^2), f32 [B * F, 3, 224, 224]: chunks of
        max(1, max_batch // B) copies per forward / backward pair, the perturbed operand built by the pack (`pack`: coef / baseline, or
        sigma / seed / i0, as NetEngine.forward_attrib takes them), the sum continued on the device in ascending copy order."""
        eng = self.engine
        b = frames.shape[0]
        src = frames.view((b * self.num_frames,) + tuple(frames.shape[2:]))
        chunk = max(1, eng.max_batch // b)
        w = torch.full((n_copies,), weight, dtype=torch.float32, device=eng.device)
        coef = pack.pop("coef", None)
        packed = self._packed_with_dgrad()
        acc, acts = None, None
        for k0 in range(0, n_copies, chunk):
            k = min(chunk, n_copies - k0)
            if acts is not None and k * b != acts_samples:
                acts = None
            part = dict(pack, coef=coef[k0:k0 + k]) if coef is not None else dict(pack, s0=k0)
            _, acts = eng.forward_attrib(src, k, packed, acts=acts, **part)
            acts_samples = k * b
            gx = eng.backward_data(acts, packed, dq.repeat(k, 1), k * b, pixel_units=pixel_units)
            acc = ops.attrib_reduce(gx, w[k0:k0 + k], acc, squared=squared)
        return acc

    def integrated_gradients(self, frames, category, action=None, steps=32, baseline=None, pixel_units=False, return_delta=False):
        """f32 [B, F, 3, 224, 224] (a 4-D input: [B, 3, 224, 224]): integrated gradients of Q[category, action] along the straight
        path from the baseline b to the frames x, (x - b) * mean_k dQ/dx at b + c_k (x - b) with the `steps` midpoints c_k =
        float32((k + 0.5) / steps); x, b and the gradient in normalised units, with pixel_units times 1 / (255 std_c).  baseline:
        None = a black frame (pixel value 0), three pixel values (0 .. 255, one per colour), or frames shaped and typed like `frames`.
        action None: the greedy action at `frames`.  return_delta: -> (attr, delta) with delta f32 [B] = sum(attr) - (Q(x) - Q(b)),
        the completeness gap (of the normalised-unit attribution), from one more forward over [x; b].  The path points are built
        inside the input pack and the sum runs on the device (vdqn_net_forward_attrib, vdqn_net_backward_data, vdqn_attrib_reduce /
        _finish); the module's training flag is left as it was.  extra_capacity only."""
        frames, added = self._attrib_frames("integrated_gradients", frames)
        if not isinstance(steps, int) or isinstance(steps, bool) or steps < 1:
            raise ValueError(f"integrated_gradients: steps must be an integer >= 1, not {steps!r}")
        if isinstance(baseline, torch.Tensor):
            if added and baseline.dim() == 4:
                baseline = baseline.unsqueeze(1)
            if baseline.shape != frames.shape or (baseline.dtype == torch.uint8) != (frames.dtype == torch.uint8):
                raise ValueError(f"integrated_gradients: a baseline tensor must have the frames' shape and kind ({frames.dtype} "
                                 f"{tuple(frames.shape)}), not {baseline.dtype} {tuple(baseline.shape)}")
            baseline = (baseline if baseline.dtype == torch.uint8 else baseline.detach().float()).to(frames.device).contiguous()
        else:
            try:
                pixels = [0.0, 0.0, 0.0] if baseline is None else [float(v) for v in baseline]
            except TypeError:
                pixels = []
            if len(pixels) != 3 or not all(0.0 <= v <= 255.0 for v in pixels):
                raise ValueError(f"integrated_gradients: baseline must be None, three pixel values in [0, 255] or frames shaped like the input, not {baseline!r}")
            baseline = ops.norm_pixel(pixels)
        eng = self.engine
        b = frames.shape[0]
        if b > eng.max_batch:
            parts = [self.integrated_gradients(frames[i:i + eng.max_batch], category, action, steps,
                                               baseline[i:i + eng.max_batch] if isinstance(baseline, torch.Tensor) else pixels, pixel_units, True)
                     for i in range(0, b, eng.max_batch)]
            attr = torch.cat([p[0] for p in parts], 0)
            attr = attr.squeeze(1) if added else attr
            return (attr, torch.cat([p[1] for p in parts], 0)) if return_delta else attr
        was_training = self.training
        self.training = False  # (this module's flag alone, as in state_values)
        try:
            with torch.no_grad():
                _, act, dq = self._attrib_target(frames, category, action)
                base_src = baseline.view((-1,) + tuple(frames.shape[2:])) if isinstance(baseline, torch.Tensor) else baseline
                coef = torch.tensor([(k + 0.5) / steps for k in range(steps)], dtype=torch.float32, device=eng.device)
                acc = self._attrib_accumulate(frames, dq, steps, 1.0 / steps, False, False, coef=coef, baseline=base_src)
                src = frames.view((-1,) + tuple(frames.shape[2:]))
                attr = ops.attrib_finish(acc, src, base_src, pixel_units=pixel_units)
                delta = None
                if return_delta:
                    plain = ops.attrib_finish(acc, src, base_src) if pixel_units else attr
                    ends = torch.tensor([1.0, 0.0], dtype=torch.float32, device=eng.device)
                    packed = self._packed_with_dgrad()
                    if 2 * b <= eng.max_batch:
                        q2, _ = eng.forward_attrib(src, 2, packed, coef=ends, baseline=base_src)
                    else:
                        q2 = torch.cat([eng.forward_attrib(src, 1, packed, coef=ends[k:k + 1], baseline=base_src)[0] for k in range(2)], 0)
                    q2 = q2.view(2, b, self.num_classes, self.action_dim)[:, torch.arange(b, device=eng.device), category, act]
                    delta = (plain.view(b, -1).double().sum(1) - (q2[0].double() - q2[1].double())).float()
        finally:
            self.training = was_training
        attr = attr.view(b, 3, 224, 224) if added else attr.view(b, self.num_frames, 3, 224, 224)
        return (attr, delta) if return_delta else attr

    def smoothgrad(self, frames, category, action=None, samples=32, sigma=0.15, squared=False, seed=0, _i0=0):
        """f32 [B, F, 224, 224] (a 4-D input: [B, 224, 224]): SmoothGrad, the maximum over colour of |mean over `samples` noisy copies of
        dQ[category, action] / d pixel| (squared: of the mean of its square).  The copies are x + sigma_c z with sigma_c = sigma / std_c,
        `sigma` a fraction of each channel's normalised range, and z the unit-variance counter-hash noise of (seed, copy, image,
        element) (include/vdqn.h), drawn inside the input pack: a run draws the same noise however it is cut into chunks or batches.
        Units as `saliency`: uint8 frames per unit of the pixel value, float frames per unit of the normalised value.  action None: the
        greedy action at the clean frames.  The module's training flag is left as it was.  extra_capacity only."""
        frames, added = self._attrib_frames("smoothgrad", frames)
        if not isinstance(samples, int) or isinstance(samples, bool) or samples < 1:
            raise ValueError(f"smoothgrad: samples must be an integer >= 1, not {samples!r}")
        sigma = float(sigma)
        if not (0.0 <= sigma <= 1.0):  # (a NaN fails both comparisons)
            raise ValueError(f"smoothgrad: sigma must be in [0, 1] (a fraction of each channel's normalised range), not {sigma}")
        eng = self.engine
        b = frames.shape[0]
        if b > eng.max_batch:
            out = torch.cat([self.smoothgrad(frames[i:i + eng.max_batch], category, action, samples, sigma, squared, seed, _i0 + i * self.num_frames)
                             for i in range(0, b, eng.max_batch)], 0)
            return out.squeeze(1) if added and out.dim() == 4 else out
        import numpy as np
        sig = np.float32(sigma) / np.array([0.229, 0.224, 0.225], dtype=np.float32)
        was_training = self.training
        self.training = False  # (this module's flag alone, as in state_values)
        try:
            with torch.no_grad():
                _, _, dq = self._attrib_target(frames, category, action)
                acc = self._attrib_accumulate(frames, dq, samples, 1.0 / samples, bool(squared), frames.dtype == torch.uint8,
                                              sigma=sig, seed=seed, i0=_i0)
                out = ops.attrib_finish(acc)
        finally:
            self.training = was_training
        return out.view(b, 224, 224) if added else out.view(b, self.num_frames, 224, 224)


def build_model(config, max_batch=None):
    """train_q_network.py:36-47 (config.device selects the GPU; dtype from config.COMPUTE_DTYPE)."""
    actions = 1 if (config.VALUE_LEARNING or config.ONE_ACTION) else 3
    nf = getattr(config, "NUM_FRAMES", 0) or None
    return HabitatDQNMultiAction(actions, 5, extra_capacity=(config.ARCHITECTURE == "extra_capacity"),
                                 panorama=(config.PANORAMA or config.PREVIOUS_IMAGES), num_frames=nf,
                                 dtype=getattr(config, "COMPUTE_DTYPE", None), device=config.device,
                                 max_batch=max_batch or max(64, 2 * getattr(config, "BATCH_SIZE", 16)),
                                 pretrained_weights=(getattr(config, "PRETRAINED_WEIGHTS", "") or None),
                                 deterministic=(True if getattr(config, "DETERMINISTIC", False) else None),
                                 log_sigma=bool(getattr(config, "LOG_SIGMA", False)),
                                 sigma_min=float(getattr(config, "DIST_SIGMA_MIN", 0.1)),
                                 **{a.model_arg: a.is_on(config) for a in ALGOS})


def load_model_number(config, number, model_loc=None):
    """train_q_network.py:50-57."""
    model = build_model(config)
    if model_loc is None:
        model_loc = f"{config.folder}/models/sample{number}.torch"
    snapshot = torch.load(model_loc, map_location=config.device)
    print(f"Loading model from: {model_loc}")
    sd = snapshot["model_state_dict"]
    if model.distributional and "spread_head" in snapshot:  # DISTRIBUTIONAL: the head travels beside the reference's keys
        sd = OrderedDict(sd, **snapshot["spread_head"]["state_dict"])
    model.load_state_dict(sd)
    return model
