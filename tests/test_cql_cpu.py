"""The conservative Q-learning penalty, host side: the float64 autograd oracle (tests/cql_oracle.py) against its closed form, the
float32 restatement of the kernel's arithmetic against float64, the CQL_ALPHA config key and its validation, the C ABI's two new
exports and their argument checks (no GPU: every call fails before it reaches the device)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import cql_oracle

CASES = [(scale, alpha, loss_kind) for scale in (0.7, 2.5, 20.0) for alpha in (0.5, 1.0, 4.0) for loss_kind in (0, 1)]


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


@pytest.mark.parametrize("scale,alpha,loss_kind", CASES)
def test_autograd_gradient_equals_closed_form_f64(scale, alpha, loss_kind):
    inputs = cql_oracle.td_inputs(96, 11, scale=scale)
    for kw in (dict(), dict(weight=_weights(96), use_valid=False), dict(linear=1, clip_rect=0, gamma=0.5)):
        o = cql_oracle.objective(inputs, alpha, loss_kind=loss_kind, **kw)
        c = cql_oracle.closed_form(inputs, alpha, loss_kind=loss_kind, **kw)
        assert (o["dq"] - c["dq"]).abs().max().item() <= 1e-12 * o["dq"].abs().max().item()
        assert o["penalty"].item() > 0 and o["loss"].item() > alpha * o["penalty"].item() * (1 - 1e-12)


@pytest.mark.parametrize("scale,alpha,loss_kind", CASES)
def test_f32_restatement_within_1e6_of_f64(scale, alpha, loss_kind):
    """What the kernel's float32 arithmetic reaches against float64 on the operator test's inputs (B = 96, ldq = 64, 5 x 3): dq
    within 1e-6 of its maximum element, loss and penalty within 1e-5 relative — the tolerances tests/test_gpu_cql.py asserts."""
    worst = 0.0
    for use_valid in (False, True):
        for weight in (None, _weights(96)):
            inputs = cql_oracle.td_inputs(96, 11 + loss_kind + 2 * use_valid, scale=scale)
            o = cql_oracle.objective(inputs, alpha, loss_kind=loss_kind, use_valid=use_valid, weight=weight)
            r = cql_oracle.restate_f32(inputs, alpha, loss_kind=loss_kind, use_valid=use_valid, weight=weight)
            e = np.abs(r["dq"].astype(np.float64) - o["dq"].numpy()).max() / o["dq"].abs().max().item()
            worst = max(worst, e)
            assert e <= 1e-6
            assert abs(r["loss"] - o["loss"].item()) <= 1e-5 * abs(o["loss"].item())
            assert abs(r["penalty"] - o["penalty"].item()) <= 1e-5 * abs(o["penalty"].item())
            assert np.abs(r["err"].astype(np.float64) - o["err"].numpy()).max() <= 1e-6 * o["err"].abs().max().item()
    print(f"scale {scale} alpha {alpha} loss_kind {loss_kind}: dq max error / max element = {worst:.2e}")


def test_extreme_rows_are_finite_in_both_precisions():
    """[1e4, -1e4, 0] (exp overflows without the max subtraction) and rows of equal Qs (penalty log 3, gradient 1/3 - onehot)."""
    B = 6
    inputs = cql_oracle.td_inputs(B, 5)
    inputs[0][:3, :15] = torch.tensor([1e4, -1e4, 0.0]).repeat(5)
    inputs[0][3:, :15] = 0.25
    inputs[3] = torch.tensor([0, 1, 2, 0, 1, 2])
    o = cql_oracle.objective(inputs, 1.0, use_valid=False)
    r = cql_oracle.restate_f32(inputs, 1.0, use_valid=False)
    assert torch.isfinite(o["dq"]).all() and np.isfinite(r["dq"]).all() and math.isfinite(r["loss"]) and math.isfinite(r["penalty"])
    pen_grad = cql_oracle.closed_form(inputs, 1.0, use_valid=False)["pen_grad"].reshape(B, 5, 3) * (5 * B)
    third = torch.full((3,), 1 / 3, dtype=torch.float64)
    for b in (3, 4, 5):
        want = third.clone()
        want[b - 3] -= 1.0
        assert (pen_grad[b] - want).abs().max().item() < 1e-7
    # the penalty of the rows: act 0 is the maximum (0), act 1 is 2e4 below it, act 2 is 1e4 below; the equal rows give log 3
    want_pen = (0 + 2e4 + 1e4 + 3 * math.log(3.0)) * 5 * float(np.float32(1.0 / (5 * B)))  # (inv_count as the float32 it is passed as)
    assert abs(o["penalty"].item() - want_pen) <= 1e-9 * want_pen
    assert abs(r["penalty"] - want_pen) <= 1e-6 * want_pen
    assert np.abs(r["dq"].astype(np.float64) - o["dq"].numpy()).max() <= 1e-6 * o["dq"].abs().max().item()


# ---- the config key ----------------------------------------------------------------------------------------------------------------
def test_config_has_cql_alpha_and_yaml_round_trip(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_cql
    c = get_cfg_defaults()
    assert c.CQL_ALPHA == 0.0 and isinstance(c.CQL_ALPHA, float)
    check_cql(c)  # the defaults pass, and so do the configurations the penalty does not cover while it is off
    for key in ("TRAIN_ON_GROUND_TRUTH", "VALUE_LEARNING", "ONE_ACTION"):
        off = c.clone()
        off[key] = True
        check_cql(off)
    f = tmp_path / "config.yml"
    f.write_text("CQL_ALPHA: 1\n")  # (an integer in the file is coerced to the key's float)
    c.merge_from_file(str(f))
    assert c.CQL_ALPHA == 1.0 and isinstance(c.CQL_ALPHA, float)
    check_cql(c)
    f.write_text(c.dump())
    d = get_cfg_defaults()
    d.merge_from_file(str(f))
    assert d.CQL_ALPHA == 1.0 and dict(d) == dict(c)
    f.write_text("CQL_ALPHA: 'one'\n")
    with pytest.raises(ValueError, match="CQL_ALPHA"):
        get_cfg_defaults().merge_from_file(str(f))


@pytest.mark.parametrize("bad,key", [(dict(CQL_ALPHA=-0.5), "CQL_ALPHA"), (dict(CQL_ALPHA=float("nan")), "CQL_ALPHA"),
                                     (dict(CQL_ALPHA=float("inf")), "CQL_ALPHA"),
                                     (dict(CQL_ALPHA=1.0, TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
                                     (dict(CQL_ALPHA=1.0, VALUE_LEARNING=True), "VALUE_LEARNING"),
                                     (dict(CQL_ALPHA=0.25, ONE_ACTION=True), "ONE_ACTION")])
def test_check_cql_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_cql
    c = get_cfg_defaults()
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=key) as e:
        check_cql(c)
    assert "CQL_ALPHA" in str(e.value)


def test_run_train_checks_cql_before_any_device_work(tmp_path):
    """run_train raises from check_cql before it touches a device (this machine may have none)."""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nCQL_ALPHA: 1.0\nTRAIN_ON_GROUND_TRUTH: True\n")
    with pytest.raises(ValueError, match="TRAIN_ON_GROUND_TRUTH"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_cql_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_td_loss_cql", "vdqn_net_td_forward_cql"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_abi_struct_size(7) == -1  # no new argument struct: both entries take plain arguments


def _td_args(buf, **kw):
    from video_dqn_amd import _lib
    a = _lib.TdArgs()
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a.q_before = a.q_after_online = a.q_after_target = a.act = a.rew = a.term = a.valid = a.loss = a.dq = p
    a.batch, a.n_cat, a.n_act, a.ldq = 4, 5, 3, 64
    a.gamma, a.inv_count, a.clip_rect, a.dtype = 0.9, 0.05, 1, _lib.VDQN_F32
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_td_loss_cql_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def call(alpha=1.0, **kw):
        return lib.vdqn_td_loss_cql(C.byref(_td_args(buf, **kw)), p, p, alpha, p, None)
    assert lib.vdqn_td_loss_cql(None, p, p, 1.0, p, None) != 0
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(loss=None), dict(use_valid=1, valid=None), dict(batch=0), dict(ldq=14), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7),
               dict(loss_kind=2), dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=float("nan")), dict(alpha=float("inf"))):
        assert call(**kw) != 0, kw
        assert b"vdqn_td_loss_cql" in lib.vdqn_last_error(), kw
    assert call(alpha=0.0) != 0 and b"cql_alpha" in lib.vdqn_last_error()
    assert call(n_act=1, n_cat=15) != 0
    assert b"n_act is 1" in lib.vdqn_last_error()


def test_net_td_forward_cql_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def net(action_dim):
        h = C.c_void_p()
        cfg = _lib.NetConfig(action_dim, 5, 1, 1, _lib.VDQN_F32, 8, 0)
        assert lib.vdqn_net_create(C.byref(cfg), C.byref(h)) == 0  # (host tables only: no device call)
        return h
    n3, n1 = net(3), net(1)
    try:
        a = _lib.StepArgs()
        assert lib.vdqn_net_td_forward_cql(None, C.byref(a), 1.0, p, None) != 0
        assert b"vdqn_net_td_forward_cql: null arg" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_cql(n3, None, 1.0, p, None) != 0
        for alpha in (-1.0, float("nan"), float("inf")):
            assert lib.vdqn_net_td_forward_cql(n3, C.byref(a), alpha, p, None) != 0
            assert b"vdqn_net_td_forward_cql: cql_alpha" in lib.vdqn_last_error()
        a.train_on_ground_truth = 1
        assert lib.vdqn_net_td_forward_cql(n3, C.byref(a), 1.0, p, None) != 0
        assert b"vdqn_net_td_forward_cql" in lib.vdqn_last_error() and b"ground-truth" in lib.vdqn_last_error()
        a.train_on_ground_truth = 0
        assert lib.vdqn_net_td_forward_cql(n1, C.byref(a), 1.0, p, None) != 0
        assert b"vdqn_net_td_forward_cql: action_dim is 1" in lib.vdqn_last_error()
        # alpha 0 is vdqn_net_td_forward: it goes on to that entry's own checks (null buffers here)
        assert lib.vdqn_net_td_forward_cql(n1, C.byref(a), 0.0, None, None) != 0
        assert b"vdqn_net_td_forward: null buffer" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_forward_cql(n3, C.byref(a), 1.0, p, None) != 0  # alpha > 0, everything else missing: the same check
        assert b"vdqn_net_td_forward: null buffer" in lib.vdqn_last_error()
    finally:
        lib.vdqn_net_destroy(n3)
        lib.vdqn_net_destroy(n1)


def test_stepper_takes_cql_alpha_off_by_default():
    import inspect
    from video_dqn_amd.engine import TDStepper
    assert inspect.signature(TDStepper.__init__).parameters["cql_alpha"].default == 0.0
