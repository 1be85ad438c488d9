"""Gradient-norm clipping, AdamW decay and the learning-rate schedule on the GPU (csrc/optim.hip, TDStepper, run_train) against
the float64 oracle (tests/optim_oracle.py): the f64 sum of squares and the finalise launch, vdqn_adam_scaled, updates through the
engine, the trainer (scalar, checkpoint keys, resume) and two ranks over gloo on one device."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_oracle
from helpers import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ulps(got, want):
    """Distance of two f32 values in units of want's last place."""
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) / float(np.spacing(np.abs(want)))


# ---- 1. sum of squares + finalise -------------------------------------------------------------------------------------------------
def _pattern(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    if kind == "zero":
        return np.zeros(n, np.float32)
    x = np.full(n, 1e-6, np.float32)  # an f32 accumulator loses every 1e-12 behind the 1e6
    x[n // 2] = 1e3
    return x


def _sumsq(x, offset, slot=0, ws=None):
    """x (numpy f32) placed `offset` elements behind a 16-byte boundary, 1e30 all around it -> (workspace as numpy f64, device ws)."""
    from video_dqn_amd import ops
    n = x.size
    buf = torch.full((n + 16,), 1e30, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[4 + offset:4 + offset + n] = torch.from_numpy(x).to(DEV)
    if ws is None:
        ws = ops.clip_workspace(DEV, 3)
    ops.grad_sumsq(buf[4 + offset:4 + offset + n], ws, slot)
    torch.cuda.synchronize()
    assert float(buf[4 + offset - 1]) == float(np.float32(1e30)) == float(buf[4 + offset + n])  # the poison is where it was put
    return ws.cpu().numpy(), ws


def _exact(x):
    x = x.astype(np.float64)
    return math.fsum(x * x)  # (a square of an f32 is exact in f64)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 1025, 100003])
def test_sumsq_is_f64_exact_to_n_ulps_and_ignores_its_neighbours(n, offset):
    for kind in ("random", "zero", "outlier"):
        x = _pattern(kind, n, 1000 * n + offset)
        got_ws, _ = _sumsq(x, offset)
        got = optim_oracle.workspace_sum(got_ws, 1)
        exact = _exact(x)
        print(f"n {n} offset {offset} {kind}: sum {got!r}, exact {exact!r}, rel {abs(got - exact) / exact if exact else 0.0:.3e}")
        assert abs(got - exact) <= n * 2.0 ** -53 * exact, (kind, got, exact)  # (1e30 poison entering would be off by 1e60)
        count = int(got_ws[:1].view(np.int64)[0])
        assert count == min(512, -(-n // 4096))
        again, _ = _sumsq(x, offset)
        assert np.array_equal(got_ws[:1 + count].view(np.int64), again[:1 + count].view(np.int64))  # bit-identical run to run


def test_sumsq_at_the_block_cap():
    """n > 512 * 4096: the grid stops growing at 512 blocks and every thread walks further."""
    n = 512 * 4096 + 4099
    x = _pattern("random", n, 77)
    got_ws, _ = _sumsq(x, 1)
    assert int(got_ws[:1].view(np.int64)[0]) == 512
    got, exact = optim_oracle.workspace_sum(got_ws, 1), _exact(x)
    print(f"n {n}: rel {abs(got - exact) / exact:.3e}")
    assert abs(got - exact) <= n * 2.0 ** -53 * exact


def test_finalize_over_three_ranges():
    from video_dqn_amd import ops
    xs = [(_pattern("random", 100003, 1), 3), (_pattern("outlier", 257, 2), 1), (_pattern("random", 5, 3), 2)]
    outs = []
    for run in range(2):
        ws = ops.clip_workspace(DEV, 3)
        for slot, (x, off) in enumerate(xs):
            _sumsq(x, off, slot, ws)
        total = optim_oracle.workspace_sum(ws.cpu().numpy(), 3)
        norm64 = math.sqrt(total)
        for max_norm in (0.5 * norm64, 1e30):
            out = ops.clip_finalize(ws, 3, max_norm)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert got[0] == np.float32(norm64)  # the f64 value rounded to f32 once
            assert got[1] == np.float32(min(1.0, max_norm / (norm64 + 1e-6)))
            outs.append(got.copy())
        exact = math.sqrt(math.fsum(_exact(x) for x, _ in xs))
        assert _ulps(outs[-1][0], exact) <= 1
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(outs[:2], outs[2:]))


def test_non_finite_norm_is_not_special_cased():
    from video_dqn_amd import ops
    for bad, want in ((np.inf, 0.0), (np.nan, np.nan)):
        x = _pattern("random", 1025, 4)
        x[17] = bad
        _, ws = _sumsq(x, 0)
        out = ops.clip_finalize(ws, 1, 1.0).cpu().numpy()
        assert (np.isnan(out[0]) and np.isnan(out[1])) if np.isnan(want) else (np.isinf(out[0]) and out[1] == 0.0)


# ---- 2. vdqn_adam_scaled ------------------------------------------------------------------------------------------------------------
def _rnd(seed, name, shape, lo=-1.0, hi=1.0):
    from video_dqn_amd import synth
    return torch.from_numpy(synth.uniform(seed, name, shape, lo, hi))


def test_adam_scaled_matches_oracle_with_clipping_and_decay():
    """The shape of test_gpu_ops.py::test_adam_matches_torch (n = 100003: three elements in the tail loop), with the coefficient
    coming from the norm kernels on the device.  Bounds as there: the chain adds two f32 roundings per element and step (g * coef,
    p * decay; at |p| < 1 at most 2^-25 each, 6e-8 together against 2e-7 per step)."""
    from video_dqn_amd import ops
    n, lr, wd = 100003, 1e-4, 0.1
    p0 = _rnd(1, "p", (n,))
    p = torch.zeros(n + 1)[:n].copy_(p0).to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    ws = ops.clip_workspace(DEV, 1)
    po, mo, vo = p0.numpy().astype(np.float64), np.zeros(n), np.zeros(n)
    max_norm = None
    for step in range(1, 4):
        g = _rnd(10 + step, "g", (n,), -1e-3, 1e-3) * step  # another norm, and so another coefficient, at every step
        g[::7] = 0.0
        if max_norm is None:
            max_norm = 0.5 * optim_oracle.clip_coef(g.numpy(), 1.0)[0]
        norm, coef = optim_oracle.clip_coef(g.numpy(), max_norm)
        assert coef < 0.51
        gd = g.to(DEV)
        ops.grad_sumsq(gd, ws, 0)
        out = ops.clip_finalize(ws, 1, max_norm)
        ops.adam_scaled(p, gd, m, v, step, lr, weight_decay=wd, coef=out[1:])
        torch.cuda.synchronize()
        assert torch.equal(gd.cpu(), g)  # the gradient itself is left as it is
        assert _ulps(out[0].item(), norm) <= 1 and _ulps(out[1].item(), coef) <= 2
        po, mo, vo = optim_oracle.adamw_step(po, g.numpy(), mo, vo, step, lr, (0.9, 0.999), 1e-8, wd, coef)
        d_ref = torch.from_numpy(po - p0.numpy().astype(np.float64))
        d_got = p.cpu().double() - p0.double()
        err_p = (d_got - d_ref).abs().max().item()
        err_m, err_v = relerr(m, torch.from_numpy(mo)), relerr(v, torch.from_numpy(vo))
        print(f"step {step}: coef {coef:.4f}, |dp - ref| {err_p:.3e} (bound {2e-3 * lr * step:.1e}), m {err_m:.2e}, v {err_v:.2e}")
        assert err_p < 2e-3 * lr * step  # 0.2 % of one lr-sized step per step
        assert err_m < 1e-6 and err_v < 1e-6
        # a missing coefficient hides in p (Adam's first step is nearly scale invariant) and shows here
        assert relerr(m, torch.from_numpy(mo / coef)) > 0.1 if step == 1 else True


@pytest.mark.parametrize("coef_kind", ["one", "null"])
def test_adam_scaled_at_unit_factors_is_adam_bit_for_bit(coef_kind):
    from video_dqn_amd import ops
    n = 100003
    p0 = _rnd(1, "p", (n,))
    a = [torch.zeros(n + 1)[:n].copy_(p0).to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [t.clone() for t in a]
    coef = torch.ones(1, dtype=torch.float32, device=DEV) if coef_kind == "one" else None
    for step in range(1, 4):
        g = _rnd(10 + step, "g", (n,), -1e-3, 1e-3)
        g[::7] = 0.0
        gd = g.to(DEV)
        ops.adam(a[0], gd, a[1], a[2], step, 1e-4)
        ops.adam_scaled(b[0], gd, b[1], b[2], step, 1e-4, weight_decay=0.0, coef=coef)
    torch.cuda.synchronize()
    for name, x, y in zip(("p", "exp_avg", "exp_avg_sq"), a, b):
        assert torch.equal(x, y), name
    assert not torch.equal(a[0].cpu(), p0)


_PRISTINE = {}


def _pristine(n):
    """_adam_state(n) of tests/test_gpu_polyak.py (nonzero moments) on the device, made once per n and never written."""
    from test_gpu_polyak import _adam_state
    if n not in _PRISTINE:
        _PRISTINE[n] = [torch.from_numpy(x).to(DEV) for x in _adam_state(n, 5 * n + 2)]
    return _PRISTINE[n]


def _two_steps(entry, n, length, tau):
    """Fresh guarded copies of the n-element state, two steps of `entry` over their first `length` elements -> [(buffer, view)] * 5."""
    from test_gpu_polyak import POISON
    from video_dqn_amd import ops
    state = []
    for x in _pristine(n):
        buf = torch.full((n + 8,), POISON, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        buf[4:4 + n] = x
        state.append((buf, buf[4:4 + n]))
    p, g, m, v, t = (view[:length] for _, view in state)
    kw = dict(weight_decay=0.1, coef=torch.full((1,), 0.37, dtype=torch.float32, device=DEV))
    for step in (1, 2):
        if entry == "adam":
            ops.adam(p, g, m, v, step, 1e-3)
        elif entry == "adam_scaled":
            ops.adam_scaled(p, g, m, v, step, 1e-3, **kw)
        else:
            ops.adam_polyak(p, g, m, v, t, tau, step, 1e-3, **kw)
    return state


@pytest.mark.parametrize("n", [8, 260, 4096 * 256 * 4 + 8])
@pytest.mark.parametrize("entry", ["adam", "adam_scaled", "adam_polyak"])
def test_adam_element_does_not_depend_on_its_position_in_the_range(entry, n):
    """Two steps over [0, n) against the same two steps over [0, n - 1), [0, n - 2) and [0, n - 3): n is a multiple of 4, so the last
    elements of the shorter ranges sit in the float4 loop of one launch and in the scalar tail loop of the other (at the largest n every
    thread of the capped grid walks its float4 loop twice).  Every element both launches cover agrees bit for bit in p, exp_avg,
    exp_avg_sq and the target; what lies behind the shorter range, and the guards, are untouched.  One element function with every
    rounding written out serves both loops (csrc/optim.hip adam_element): two loops that the compiler may contract differently
    (exp_avg_sq as one fma in one, as two rounded products in the other) fail this in exp_avg_sq."""
    from test_gpu_polyak import _guards_intact
    names = ("p", "g", "exp_avg", "exp_avg_sq", "target")
    touched = (True, False, True, True, entry == "adam_polyak")
    for tau in ((0.005, 0.5) if entry == "adam_polyak" else (None,)):
        full = _two_steps(entry, n, n, tau)
        for name, (buf, view), x, moved in zip(names, full, _pristine(n), touched):
            assert _guards_intact(buf), (name, tau)
            assert torch.equal(view.view(torch.int32), x.view(torch.int32)) != moved, (name, tau)
        for cut in (1, 2, 3):
            part = _two_steps(entry, n, n - cut, tau)
            for name, (_, a), (buf, b), x in zip(names, full, part, _pristine(n)):
                assert torch.equal(a[:n - cut].view(torch.int32), b[:n - cut].view(torch.int32)), (name, cut, tau)
                assert torch.equal(b[n - cut:].view(torch.int32), x[n - cut:].view(torch.int32)), (name, cut, tau)
                assert _guards_intact(buf), (name, cut, tau)
            del part
        del full


# ---- 3. updates through the engine ---------------------------------------------------------------------------------------------------
BASE_LR, WD, WARMUP = 1e-3, 0.1, 4  # (the reference's rate: an lr-sized step stays well above the f32 spacing of the weights)


def _lr_fn(t):
    return optim_oracle.lr_at(t, BASE_LR, WARMUP, "constant", 0.0, 100)


def _make(dtype, B, extra_capacity=True, deterministic=True, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=deterministic)
    net.load_tensors(synth.make_state_dict(7, extra_capacity=extra_capacity))
    return net, TDStepper(net, B, lr=BASE_LR, gamma=0.99, clip_rect=True, target_update_interval=1000, **kw)


_BATCHES = {}


def _batch(seed, B):
    from video_dqn_amd import synth
    if (seed, B) not in _BATCHES:
        (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
        _BATCHES[(seed, B)] = (tup[0].contiguous(), tup[1].contiguous(), tup[2], tup[3].float(), tup[4].float())
    t = _BATCHES[(seed, B)]
    return [t[0].to(DEV), t[1].to(DEV), 1, t[2].to(DEV), t[3].to(DEV), t[4].to(DEV)]


def _first_norm(dtype, B, extra_capacity, deterministic):
    net, stp = _make(dtype, B, extra_capacity, deterministic)
    stp.forward_backward(*_batch(301, B))
    torch.cuda.synchronize()
    return optim_oracle.clip_coef(stp.grads.cpu().numpy(), 1.0)[0]


@pytest.mark.parametrize("dtype,extra_capacity,deterministic", [("f32", True, True), ("bf16", True, False), ("f32", False, True)],
                         ids=["f32", "bf16_default_atomic_mode", "f32_basic"])
def test_three_updates_match_forward_backward_plus_oracle(dtype, extra_capacity, deterministic):
    """Three TDStepper.step calls with clipping (half the first gradient's norm), decay and a warm-up against the float64 oracle
    applied to the engine's own gradient of each update.  In deterministic mode a twin stepper that is handed the same state and
    only runs forward_backward must produce that gradient bit for bit: the norm launches beside the backward pass disturb nothing."""
    B = 8
    max_norm = 0.5 * _first_norm(dtype, B, extra_capacity, deterministic)
    net, stp = _make(dtype, B, extra_capacity, deterministic, grad_clip_norm=max_norm, weight_decay=WD, lr_fn=_lr_fn)
    twin = _make(dtype, B, extra_capacity, deterministic) if (deterministic and extra_capacity) else None
    nt = net.trainable_numel
    p0 = net.params[:nt].cpu().numpy().astype(np.float64)
    po, mo, vo = p0.copy(), np.zeros(nt), np.zeros(nt)
    lr_sum, norms = 0.0, []
    for t in range(1, 4):
        if twin is not None:
            twin[0].params.copy_(net.params)
            twin[0].mark_dirty()
            twin[1].forward_backward(*_batch(300 + t, B))
        stp.step(*_batch(300 + t, B))
        torch.cuda.synchronize()
        g = stp.grads.cpu()
        if twin is not None:
            assert torch.equal(twin[1].grads.cpu(), g)
        lr = _lr_fn(t)
        assert stp.lr == lr and stp.adam_step == t
        lr_sum += lr
        norm, coef = optim_oracle.clip_coef(g.numpy(), max_norm)
        norms.append(norm)
        got = stp.clip_out.cpu().numpy()
        print(f"update {t}: norm {norm:.6e} coef {coef:.6f}; device {got[0]:.6e} {got[1]:.6f} ({_ulps(got[1], coef):.2f} ulps)")
        assert _ulps(got[0], norm) <= 2 and _ulps(got[1], coef) <= 2
        po, mo, vo = optim_oracle.adamw_step(po, g.numpy(), mo, vo, t, lr, (0.9, 0.999), 1e-8, WD, coef)
        err_m, err_v = relerr(stp.exp_avg, torch.from_numpy(mo)), relerr(stp.exp_avg_sq, torch.from_numpy(vo))
        err_p = np.abs((net.params[:nt].cpu().numpy().astype(np.float64) - p0) - (po - p0)).max()
        print(f"          m {err_m:.2e}, v {err_v:.2e}, |dp - ref| {err_p:.3e} (bound {2e-3 * lr_sum:.2e})")
        assert err_m < 1e-6 and err_v < 1e-6
        assert err_p < 2e-3 * lr_sum  # 0.2 % of one lr-sized step per step, at the warm-up's rates
    # clipping was active (at half the first norm the first update clips by construction; a later, smaller gradient may pass
    # unclipped), on a different gradient every update
    assert min(max_norm / (x + 1e-6) for x in norms) < 0.51 and len(set(norms)) == 3
    # resnet.fc never receives a gradient: no decay either
    from video_dqn_amd import synth
    ref = synth.make_state_dict(7, extra_capacity=extra_capacity)
    assert torch.equal(net.view("resnet.fc.weight").cpu(), ref["resnet.fc.weight"].float())


def test_clip_that_never_clips_equals_the_plain_stepper_bit_for_bit():
    B = 8
    net_a, stp_a = _make("f32", B)
    net_b, stp_b = _make("f32", B, grad_clip_norm=1e30)
    for t in range(1, 4):
        stp_a.step(*_batch(300 + t, B))
        stp_b.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    assert stp_b.clip_out[1].item() == 1.0 and stp_b.clip_out[0].item() > 0
    for name, x, y in (("params", net_a.params, net_b.params), ("exp_avg", stp_a.exp_avg, stp_b.exp_avg),
                       ("exp_avg_sq", stp_a.exp_avg_sq, stp_b.exp_avg_sq), ("loss", stp_a.loss, stp_b.loss)):
        assert torch.equal(x, y), name


def test_deterministic_mode_is_bit_identical_run_to_run():
    B = 8
    max_norm = 0.5 * _first_norm("bf16", B, True, True)
    runs = []
    for _ in range(2):
        net, stp = _make("bf16", B, True, True, grad_clip_norm=max_norm, weight_decay=WD, lr_fn=_lr_fn)
        clips = []
        for t in range(1, 4):
            stp.step(*_batch(300 + t, B))
            clips.append(stp.clip_out.clone())
        torch.cuda.synchronize()
        runs.append([net.params.cpu(), stp.exp_avg.cpu(), stp.exp_avg_sq.cpu(), torch.stack(clips).cpu()])
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert (runs[0][3][:, 1] < 1.0).all()


def test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit():
    """Six updates in one go against three updates, the trainer's optimiser checkpoint into a fresh stepper, three more: parameters
    and moments bit-identical.  Adam takes the rate as an input, so the resumed stepper used the uninterrupted run's rates (the
    checkpoint's `lr`, that of update 3, is overridden by the schedule).  (run_train's own resume keeps the reference's numbering —
    it restarts at resume_from + 2 and re-reads the epoch from its start, tests/test_gpu_augment.py — so its resumed run cannot equal
    an uninterrupted one whatever the optimiser does; its rates are checked in test_run_train_* below.)"""
    from video_dqn_amd.trainer import load_optimizer_state_dict, optimizer_state_dict
    B = 4
    max_norm = 0.5 * _first_norm("f32", B, True, True)

    def lr_fn(t):
        return optim_oracle.lr_at(t, BASE_LR, 2, "cosine", 0.1, 6)
    kw = dict(grad_clip_norm=max_norm, weight_decay=WD, lr_fn=lr_fn)
    net_u, stp_u = _make("f32", B, **kw)
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    net_i, stp_i = _make("f32", B, **kw)
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    sd = optimizer_state_dict(stp_i)
    g0 = sd["param_groups"][0]
    assert g0["lr"] == lr_fn(3) and g0["weight_decay"] == WD and g0["initial_lr"] == BASE_LR
    net_r, stp_r = _make("f32", B, **kw)
    net_r.params.copy_(net_i.params)
    net_r.mark_dirty()
    load_optimizer_state_dict(stp_r, sd)
    stp_r.sample_number = 3
    assert stp_r.adam_step == 3 and stp_r.lr == lr_fn(3)
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
        assert stp_r.lr == lr_fn(t)
    torch.cuda.synchronize()
    for name, x, y in (("params", net_u.params, net_r.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq)):
        assert torch.equal(x, y), name


# ---- 4. run_train ------------------------------------------------------------------------------------------------------------------
SEED = 4
OPTIM_ON = "GRAD_CLIP_NORM: 0.001\nWEIGHT_DECAY: 0.05\nLR_WARMUP_STEPS: 3\nLR_SCHEDULE: 'cosine'\nLR_FINAL_FRACTION: 0.1\n"


def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 4\nNUM_STEPS: {steps}\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def _train(folder, shards, steps, extra, monkeypatch, resume_from=-1, tensorboard=False):
    """-> (stepper, [(update number, rate of its Adam launches)], log lines, ExperimentConfig)"""
    from video_dqn_amd import engine
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    rates = []
    real = engine.TDStepper._adam_range

    def recording(self, b, e, step):
        rates.append((self.sample_number, self.lr, step))
        return real(self, b, e, step)
    _write_cfg(folder, shards, steps, extra)
    logs = []
    cfg = ExperimentConfig(str(folder), device=DEV, tensorboard=tensorboard, resume=resume_from > -1)
    with monkeypatch.context() as m:
        m.setattr(engine.TDStepper, "_adam_range", recording)
        model, stepper, running = run_train(cfg, resume_from=resume_from, log=lambda *a: logs.append(" ".join(map(str, a))))
    assert np.isfinite(running)
    return stepper, rates, logs, cfg


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    root = str(tmp_path_factory.mktemp("optim_shards") / "shards")
    _synthetic_shards(root)
    return root


def test_run_train_checkpoint_keys_rates_and_resume(tmp_path, monkeypatch, shards):
    steps = 8
    stepper, rates, logs, _ = _train(tmp_path / "a", shards, steps, OPTIM_ON, monkeypatch)
    assert any(l.startswith("optimiser:") and "clipped" in l and "weight decay" in l and "cosine" in l for l in logs)
    want = {t: optim_oracle.lr_at(t, 1e-4, 3, "cosine", 0.1, steps) for t in range(1, steps + 1)}
    assert sorted(set(rates)) == [(t, want[t], t) for t in range(1, steps + 1)]  # one rate per update, for every launch of it
    assert stepper.clip_out[1].item() < 1.0  # clipping was active
    for tag in ("sample4", "sample8"):
        g0 = torch.load(tmp_path / "a" / "models" / f"{tag}.torch", map_location="cpu")["optimizer_state_dict"]["param_groups"][0]
        t = int(tag[6:])
        assert g0["weight_decay"] == 0.05 and g0["initial_lr"] == 1e-4 and g0["lr"] == want[t]
    # resume (-r 4): the reference's loop performs updates 6 .. 8 then (tests/test_gpu_augment.py) — at the uninterrupted run's rates
    (tmp_path / "r").mkdir()
    (tmp_path / "r" / "models").mkdir()
    torch.save(torch.load(tmp_path / "a" / "models" / "sample4.torch", map_location="cpu"), tmp_path / "r" / "models" / "sample4.torch")
    r_stepper, r_rates, _, _ = _train(tmp_path / "r", shards, steps, OPTIM_ON, monkeypatch, resume_from=4)
    assert sorted(set(r_rates)) == [(t, want[t], t - 1) for t in (6, 7, 8)]
    assert r_stepper.lr == want[8]
    # every key at its default: the checkpoint's group keeps its exact keys, and the update launches plain vdqn_adam
    d_stepper, d_rates, d_logs, _ = _train(tmp_path / "d", shards, steps, "", monkeypatch)
    g0 = torch.load(tmp_path / "d" / "models" / "sample8.torch", map_location="cpu")["optimizer_state_dict"]["param_groups"][0]
    assert list(g0) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    assert g0["weight_decay"] == 0 and g0["lr"] == 1e-4
    assert d_stepper.clip_out is None and d_stepper.lr_fn is None and not any(l.startswith("optimiser:") for l in d_logs)
    assert {r[1] for r in d_rates} == {1e-4}
    assert not torch.equal(d_stepper.net.params, stepper.net.params)


def test_run_train_logs_the_gradient_norm(tmp_path, monkeypatch, shards):
    """100 updates with a scalar writer: `grad_norm/train` is written at update 100 with the norm of update 99 (read one update
    late, like the loss), next to the loss scalar; without clipping it is absent."""
    from video_dqn_amd.config import JsonlWriter
    stepper, _, _, cfg = _train(tmp_path / "a", shards, 100, "GRAD_CLIP_NORM: 0.001\nCHECKPOINT_INTERVAL: 1000\n", monkeypatch, tensorboard=True)
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    cfg.writer.close()
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    norm = [r for r in rows if r["tag"] == "grad_norm/train"]
    assert len(norm) == 1 and norm[0]["step"] == 99 and np.isfinite(norm[0]["value"]) and norm[0]["value"] > 0.001
    assert any(r["tag"] == "avg_q_loss/train" and r["step"] == 100 for r in rows)
    print(f"grad_norm/train at update 99: {norm[0]['value']:.4e}; the last update's: {stepper.clip_out[0].item():.4e}")


def test_run_train_with_prioritized_replay_and_augmentation(tmp_path, monkeypatch, shards):
    extra = "PRIORITIZED_REPLAY: True\nAUG_SHIFT_PAD: 8\nAUG_FLIP: True\n"
    runs = [_train(tmp_path / tag, shards, 8, extra + OPTIM_ON, monkeypatch)[0] for tag in ("p0", "p1")]
    assert torch.equal(runs[0].net.params, runs[1].net.params) and torch.equal(runs[0].exp_avg_sq, runs[1].exp_avg_sq)
    assert torch.equal(runs[0].clip_out, runs[1].clip_out) and runs[0].clip_out[1].item() < 1.0
    assert runs[0].replay is not None and runs[0].augmenter is not None
    off = _train(tmp_path / "off", shards, 8, extra, monkeypatch)[0]
    assert not torch.equal(off.net.params, runs[0].net.params)


# ---- 5. two ranks on one GPU over gloo -------------------------------------------------------------------------------------------------
def test_two_ranks_clip_the_reduced_gradient_alike_and_equal_the_big_batch(tmp_path):
    """Two ranks x 4 samples (gloo, one device; tests/scripts/optim_two_ranks.py) against one process on the 8 samples, two updates
    with clipping at half the first gradient's norm, decay and a warm-up: the ranks hold bit-identical coefficients, parameters and
    moments (the norm is that of the REDUCED gradient: same bytes, same kernels), and meet test_gpu_ddp.py's bounds against the
    big batch.  The coefficients agree to 1e-4: the two gradients differ by the f32 summation order over the batch alone."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "scripts"))
    import optim_two_ranks as prog
    from test_gpu_ddp import _free_port
    B, world = 4, 2
    probe = prog.run(B * world, 1, 0, 0.0)
    assert probe["clip"] is None
    max_norm = 0.5 * optim_oracle.clip_coef(probe["first_grad"].numpy(), 1.0)[0]
    port = str(_free_port())
    script = os.path.join(ROOT, "tests", "scripts", "optim_two_ranks.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), port, str(tmp_path), str(B), repr(max_norm)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    for key in ("clip", "params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(ranks[0][key], ranks[1][key]), key
    assert (ranks[0]["clip"][:, 1] < 1.0).all()
    big = prog.run(B * world, 1, 0, max_norm)
    nt = big["trainable"]
    rel = ((big["clip"] - ranks[0]["clip"]).abs() / big["clip"].abs()).max().item()
    delta = (big["params"][:nt] - ranks[0]["params"][:nt]).abs()
    print(f"two ranks against the big batch: norm / coef rel {rel:.3e}; params max {delta.max().item():.3e}, mean {delta.mean().item():.3e}")
    assert rel < 1e-4
    assert delta.max().item() <= 2.5e-4 and delta.mean().item() < 2e-6
    assert not torch.equal(big["params"], probe["params"])
