"""Gradient clipping, AdamW decay and the learning-rate schedule, host side: the float64 oracle (tests/optim_oracle.py) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, the schedule against hand-computed values, the config keys and their
validation, and the C ABI's new exports."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_oracle


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_oracle_equals_torch_clip_grad_norm_and_adamw_float64():
    n, lr, wd, betas, eps = 1003, 1e-3, 0.1, (0.9, 0.999), 1e-8
    rng = np.random.default_rng(3)
    p0 = rng.uniform(-1.0, 1.0, n)
    grads = [rng.uniform(-1e-2, 1e-2, n) * (1 + 3 * s) for s in range(3)]  # a different norm at every step
    for g in grads:
        g[::7] = 0.0
    max_norm = 0.5 * math.sqrt(float((grads[0] ** 2).sum()))  # every step clips
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([pt], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    for step, g in enumerate(grads, 1):
        pt.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([pt], max_norm)
        clipped = pt.grad.numpy().copy()
        opt.step()
        norm, coef = optim_oracle.clip_coef(g, max_norm)
        assert coef < 1.0
        assert abs(norm - float(total)) <= 1e-12 * norm
        assert _rel(g * coef, clipped) < 1e-12
        p, m, v = optim_oracle.adamw_step(p, g, m, v, step, lr, betas, eps, wd, coef)
        st = opt.state[pt]
        assert _rel(m, st["exp_avg"].numpy()) < 1e-12 and _rel(v, st["exp_avg_sq"].numpy()) < 1e-12
        assert _rel(p, pt.detach().numpy()) < 1e-12
        assert _rel(p - p0, pt.detach().numpy() - p0) < 1e-9  # (the deltas themselves: 1e-12 of |p| is ~1e-9 of an lr-sized step)
    # coef = 1 and wd = 0 is plain Adam
    pa = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    adam = torch.optim.Adam([pa], lr=lr, betas=betas, eps=eps)
    pa.grad = torch.from_numpy(grads[0].copy())
    adam.step()
    q, _, _ = optim_oracle.adamw_step(p0, grads[0], np.zeros(n), np.zeros(n), 1, lr, betas, eps, 0.0, 1.0)
    assert _rel(q, pa.detach().numpy()) < 1e-12
    assert optim_oracle.clip_coef(grads[0], 1e9)[1] == 1.0


BASE, W, N, F = 1e-3, 10, 110, 0.1
# t -> rate, by hand: warm-up t / 10; then progress = (t - 10) / 100; linear 1 - 0.9 * progress; cosine 0.1 + 0.45 * (1 + cos(pi * progress))
HAND = {
    "constant": {1: 1e-4, 5: 5e-4, 10: 1e-3, 11: 1e-3, 60: 1e-3, 110: 1e-3, 200: 1e-3},
    "linear": {1: 1e-4, 5: 5e-4, 10: 1e-3, 11: 9.91e-4, 35: 7.75e-4, 60: 5.5e-4, 110: 1e-4, 111: 1e-4, 200: 1e-4},
    "cosine": {1: 1e-4, 5: 5e-4, 10: 1e-3, 11: 9.997779521645793e-4, 35: 8.681980515339464e-4, 60: 5.5e-4, 110: 1e-4, 111: 1e-4, 200: 1e-4},
}


@pytest.mark.parametrize("schedule", ["constant", "linear", "cosine"])
def test_lr_at_matches_hand_computed_values(schedule):
    from video_dqn_amd.optim import lr_at
    for t, want in HAND[schedule].items():
        got = lr_at(t, BASE, W, schedule, F, N)
        assert abs(got - want) <= 1e-12 * want, (schedule, t, got, want)
        assert abs(optim_oracle.lr_at(t, BASE, W, schedule, F, N) - want) <= 1e-12 * want
    # no warm-up: the first update already runs at the schedule's rate
    w0 = {"constant": {1: 1e-3, 50: 1e-3, 100: 1e-3, 150: 1e-3},
          "linear": {1: 9.91e-4, 50: 5.5e-4, 100: 1e-4, 150: 1e-4},
          "cosine": {1: 9.997779521645793e-4, 50: 5.5e-4, 100: 1e-4, 150: 1e-4}}[schedule]
    for t, want in w0.items():
        assert abs(lr_at(t, BASE, 0, schedule, F, 100) - want) <= 1e-12 * want, (schedule, t)
    assert lr_at(7, 2e-3) == 2e-3  # every key at its default: the base rate itself, not a product that might round
    with pytest.raises(ValueError, match="LR_SCHEDULE"):
        lr_at(1, BASE, 0, "step", 0.0, 100)


def test_config_has_the_five_keys_and_yaml_round_trip(tmp_path):
    from video_dqn_amd.config import VALID_VALUES, get_cfg_defaults
    c = get_cfg_defaults()
    assert c.GRAD_CLIP_NORM == 0.0 and isinstance(c.GRAD_CLIP_NORM, float)
    assert c.WEIGHT_DECAY == 0.0 and isinstance(c.WEIGHT_DECAY, float)
    assert c.LR_WARMUP_STEPS == 0 and isinstance(c.LR_WARMUP_STEPS, int)
    assert c.LR_SCHEDULE == "constant" and c.LR_FINAL_FRACTION == 0.0
    assert VALID_VALUES["LR_SCHEDULE"] == ["constant", "linear", "cosine"]
    f = tmp_path / "config.yml"
    f.write_text("GRAD_CLIP_NORM: 10\nWEIGHT_DECAY: 0.01\nLR_WARMUP_STEPS: 500\nLR_SCHEDULE: 'cosine'\nLR_FINAL_FRACTION: 0.1\n")
    c.merge_from_file(str(f))
    assert c.GRAD_CLIP_NORM == 10.0 and isinstance(c.GRAD_CLIP_NORM, float) and c.WEIGHT_DECAY == 0.01
    assert c.LR_WARMUP_STEPS == 500 and c.LR_SCHEDULE == "cosine" and c.LR_FINAL_FRACTION == 0.1
    from video_dqn_amd.trainer import check_optim
    check_optim(c)
    check_optim(get_cfg_defaults())


@pytest.mark.parametrize("bad,key", [
    (dict(GRAD_CLIP_NORM=-1.0), "GRAD_CLIP_NORM"),
    (dict(GRAD_CLIP_NORM=float("nan")), "GRAD_CLIP_NORM"),
    (dict(GRAD_CLIP_NORM=float("inf")), "GRAD_CLIP_NORM"),
    (dict(WEIGHT_DECAY=-0.01), "WEIGHT_DECAY"),
    (dict(WEIGHT_DECAY=float("inf")), "WEIGHT_DECAY"),
    (dict(LR_WARMUP_STEPS=-1), "LR_WARMUP_STEPS"),
    (dict(LR_FINAL_FRACTION=-0.1), "LR_FINAL_FRACTION"),
    (dict(LR_FINAL_FRACTION=float("nan")), "LR_FINAL_FRACTION"),
    (dict(LR_FINAL_FRACTION=1.5), "LR_FINAL_FRACTION"),
    (dict(LR_SCHEDULE="step"), "LR_SCHEDULE"),
    (dict(LR_SCHEDULE="linear", LR_WARMUP_STEPS=100, NUM_STEPS=100), "LR_WARMUP_STEPS"),
    (dict(LR_SCHEDULE="cosine", LR_WARMUP_STEPS=200, NUM_STEPS=100), "LR_WARMUP_STEPS"),
])
def test_check_optim_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_optim
    c = get_cfg_defaults()
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=key):
        check_optim(c)


def test_constant_schedule_accepts_a_warmup_as_long_as_the_run():
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_optim
    c = get_cfg_defaults()
    c.LR_WARMUP_STEPS, c.NUM_STEPS = 100, 100  # 'constant': nothing decays towards NUM_STEPS
    check_optim(c)


def test_library_exports_the_optimiser_symbols_at_abi_15():
    from video_dqn_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_clip_workspace_bytes", "vdqn_grad_sumsq", "vdqn_clip_finalize", "vdqn_adam_scaled"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_clip_workspace_bytes(1) == optim_oracle.CLIP_SLOT_DOUBLES * 8
    assert loaded.vdqn_clip_workspace_bytes(3) == 3 * optim_oracle.CLIP_SLOT_DOUBLES * 8
    assert loaded.vdqn_clip_workspace_bytes(0) == -1 and loaded.vdqn_clip_workspace_bytes(9) == -1
