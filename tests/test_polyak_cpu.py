"""Soft (Polyak) target updates, host side: the float32 restatement of the kernel's arithmetic (tests/polyak_oracle.py) against
float64, the TARGET_TAU config key and its validation, the C ABI's two new exports and their argument checks (no GPU: every call
fails before it reaches the device), and the checkpoint's keys."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import polyak_oracle

TAUS = [1e-4, 0.005, 0.25, 0.499, 0.5, 0.75, 1.0]


def _inputs(scale, rel, seed=0, n=1 << 20):
    rng = np.random.default_rng(seed)
    t = (rng.standard_normal(n) * scale).astype(np.float32)
    p = (t.astype(np.float64) + rel * scale * rng.standard_normal(n)).astype(np.float32)
    p[::7] = t[::7]
    return t, p


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
@pytest.mark.parametrize("rel", [1e-3, 1.0])
def test_lerp_f32_within_four_half_ulps_of_f64(scale, rel):
    """|got - ref| <= 1.01 * 2^-24 * (3 |p - t| + |ref|): one half-ulp for each of d, tau, the product (each relative to |p - t|
    or less) and the sum (relative to the result).  tau = 1 returns p exactly, p == t returns t exactly."""
    t, p = _inputs(scale, rel, seed=int(scale * 1000) + int(rel * 10))
    gap = np.abs(p.astype(np.float64) - t.astype(np.float64))
    for tau in TAUS:
        got = polyak_oracle.lerp_f32(t, p, tau)
        assert got.dtype == np.float32
        ref = polyak_oracle.lerp(t, p, tau)
        bound = 1.01 * 2.0 ** -24 * (3.0 * gap + np.abs(ref))
        err = np.abs(got.astype(np.float64) - ref)
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
        print(f"scale {scale} rel {rel} tau {tau}: worst error / bound = {worst:.3f}")
        assert np.all(err <= bound)
        assert np.array_equal(got[::7].view(np.int32), t[::7].view(np.int32))  # p == t leaves t's bits
        if tau == 1.0:
            assert np.array_equal(got, p)
    assert not np.array_equal(polyak_oracle.lerp_f32(t, p, 0.25), polyak_oracle.lerp_f32(t, p, 0.75))


# ---- the config key ----------------------------------------------------------------------------------------------------------------
def test_config_has_target_tau_and_an_int_is_coerced(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_target
    c = get_cfg_defaults()
    assert c.TARGET_TAU == 0.0 and isinstance(c.TARGET_TAU, float)
    check_target(c)
    off = c.clone()
    off["TRAIN_ON_GROUND_TRUTH"] = True  # fine while the key is off
    check_target(off)
    f = tmp_path / "config.yml"
    f.write_text("TARGET_TAU: 1\n")
    c.merge_from_file(str(f))
    assert c.TARGET_TAU == 1.0 and isinstance(c.TARGET_TAU, float)
    check_target(c)
    f.write_text("TARGET_TAU: 0.005\n")
    c.merge_from_file(str(f))
    assert c.TARGET_TAU == 0.005
    check_target(c)


@pytest.mark.parametrize("bad,key", [(dict(TARGET_TAU=True), "TARGET_TAU"), (dict(TARGET_TAU="0.1"), "TARGET_TAU"),
                                     (dict(TARGET_TAU=float("nan")), "TARGET_TAU"), (dict(TARGET_TAU=float("inf")), "TARGET_TAU"),
                                     (dict(TARGET_TAU=-0.1), "TARGET_TAU"), (dict(TARGET_TAU=1.5), "TARGET_TAU"),
                                     (dict(TARGET_TAU=0.005, TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH")])
def test_check_target_raises_by_key_name(bad, key):
    from types import SimpleNamespace
    from video_dqn_amd.trainer import check_target
    c = SimpleNamespace(TARGET_TAU=0.0, TRAIN_ON_GROUND_TRUTH=False)  # (the config node itself refuses a value of another type)
    for k, v in bad.items():
        setattr(c, k, v)
    with pytest.raises(ValueError, match=key) as e:
        check_target(c)
    assert "TARGET_TAU" in str(e.value)


def test_run_train_checks_target_tau_before_any_device_work(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nTARGET_TAU: 0.005\nTRAIN_ON_GROUND_TRUTH: True\n")
    with pytest.raises(ValueError, match="TARGET_TAU"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


def test_stepper_takes_target_tau_off_by_default():
    from video_dqn_amd.engine import TDStepper
    assert inspect.signature(TDStepper.__init__).parameters["target_tau"].default == 0.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_polyak_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_polyak", "vdqn_adam_polyak"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_abi_struct_size(7) == -1  # no new argument struct: both entries take plain arguments


def _aligned(buf):
    """A 16-byte aligned address inside a host buffer (never dereferenced: every call below fails its argument check)."""
    return (C.addressof(buf) + 15) & ~15


BAD_TAUS = [0.0, -0.1, 1.5, float("nan"), float("inf")]


def test_polyak_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = _aligned(buf)
    q = p + 64
    for args in [(p, q, 8, tau) for tau in BAD_TAUS] + [(None, q, 8, 0.5), (p, None, 8, 0.5), (p + 4, q, 8, 0.5), (p, q + 8, 8, 0.5),
                                                         (p, q, 0, 0.5), (p, q, -3, 0.5), (p, p, 8, 0.5), (p, p + 16, 8, 0.5),
                                                         (p + 16, p, 8, 0.5)]:
        assert lib.vdqn_polyak(*args, None) != 0, args
        assert b"vdqn_polyak" in lib.vdqn_last_error(), args
    assert lib.vdqn_polyak(p, q, 8, 0.0, None) != 0 and b"tau" in lib.vdqn_last_error()
    assert lib.vdqn_polyak(p + 4, q, 8, 0.5, None) != 0 and b"aligned" in lib.vdqn_last_error()
    assert lib.vdqn_polyak(p, p + 16, 8, 0.5, None) != 0 and b"overlap" in lib.vdqn_last_error()


def test_adam_polyak_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 128)()
    base = _aligned(buf)
    p, g, m, v, t = (base + 64 * i for i in range(5))

    def call(p=p, g=g, m=m, v=v, t=t, n=8, step=1, wd=0.0, coef=None, tau=0.5):
        return lib.vdqn_adam_polyak(p, g, m, v, n, step, 1e-3, 0.9, 0.999, 1e-8, wd, coef, t, tau, None)
    cases = [dict(tau=tau) for tau in BAD_TAUS]
    cases += [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(t=None)]
    cases += [dict(p=p + 4), dict(g=g + 8), dict(m=m + 12), dict(v=v + 4), dict(t=t + 4), dict(coef=g + 2)]
    cases += [dict(n=0), dict(n=-1), dict(step=0), dict(wd=-1.0), dict(wd=float("nan"))]
    cases += [dict(t=p), dict(t=g), dict(t=m + 16), dict(t=v - 16)]  # the target inside another operand's range
    for kw in cases:
        assert call(**kw) != 0, kw
        assert b"vdqn_adam_polyak" in lib.vdqn_last_error(), kw
    assert call(tau=float("nan")) != 0 and b"tau" in lib.vdqn_last_error()
    assert call(t=t + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert call(t=p) != 0 and b"overlap" in lib.vdqn_last_error()


# ---- the checkpoint ----------------------------------------------------------------------------------------------------------------
def _cpu_model_and_stepper():
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    m = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, device="cpu")
    m.load_state_dict(synth.make_state_dict(5), strict=True)

    class FakeStepper:  # the checkpointed part of TDStepper without a GPU
        pass
    st = FakeStepper()
    st.net, st.lr, st.betas, st.eps, st.adam_step = m.engine, 1e-4, (0.9, 0.999), 1e-8, 0
    return m, st


def test_checkpoint_keys_without_and_with_the_target(tmp_path):
    """target_state_dict=None writes exactly the three keys the reference's loading lines read; given, it is one key more, and it
    loads (strict) into the oracle's restatement of the reference class as the smoothed network."""
    from oracle import ref_cpu
    from video_dqn_amd.trainer import save_checkpoint, target_state_dict
    m, st = _cpu_model_and_stepper()
    save_checkpoint(tmp_path / "a.torch", 3, m, st)
    save_checkpoint(tmp_path / "b.torch", 3, m, st, target_state_dict=None)
    for name in ("a.torch", "b.torch"):
        assert list(torch.load(tmp_path / name, map_location="cpu")) == ["sample_number", "model_state_dict", "optimizer_state_dict"]
    st.target_params = m.engine.params * 0.5
    tsd = target_state_dict(st, m)
    save_checkpoint(tmp_path / "c.torch", 3, m, st, target_state_dict=tsd)
    snap = torch.load(tmp_path / "c.torch", map_location="cpu")
    assert list(snap) == ["sample_number", "model_state_dict", "optimizer_state_dict", "target_state_dict"]
    msd, got = snap["model_state_dict"], snap["target_state_dict"]
    assert list(got) == list(msd) and all(got[k].shape == msd[k].shape and got[k].dtype == msd[k].dtype for k in msd)
    halved = 0
    for k in msd:
        if m.engine.slots.get(k) is not None and m.engine.slots[k].kind in (0, 1):
            assert torch.equal(got[k], msd[k] * 0.5), k
            halved += 1
        else:
            assert torch.equal(got[k], msd[k]), k  # BatchNorm buffers: copied, not averaged
    assert halved == sum(1 for s in m.engine.slots.values() if s.kind in (0, 1)) > 60
    ref = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False)
    ref.load_state_dict(got, strict=True)
    assert torch.equal(ref.state_dict()["top.4.weight"], msd["top.4.weight"] * 0.5)
