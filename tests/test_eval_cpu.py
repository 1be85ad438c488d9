"""Held-out validation, host side: the float32 restatement of the metrics kernel against its float64 oracle (tests/eval_oracle.py),
the oracle against tests/cql_oracle.py's objective, the VAL_* config keys and their refusals, the C ABI's two new exports and their
argument checks (no GPU: every call fails before it reaches the device)."""
import ctypes as C

import numpy as np
import pytest
import torch

import cql_oracle
import eval_oracle

SHAPES = (1, 3, 52, 96, 257, 300)


@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
def test_f32_restatement_within_1e6_of_f64(loss_kind, use_valid):
    """What float32 term arithmetic reaches against float64: every slot within 1e-6 of the sum of its terms' absolute values, over
    B in {1, 3, 52, 96, 257, 300} and six seeds of cql_oracle.td_inputs (measured: at most 2.6e-7, slot 1); the counts and the
    agreement counts exactly.  (The gate is for these inputs: pen = logf(sum) + (m - q) is TD_CQL's formula, and where one action
    dominates by far, sum is 1 + a little and a single term's logf loses relative precision — 1.5e-4 of the term at a Q scale of
    2.5 with B = 1, seed 105.  A sum over a batch is dominated by its large terms.)"""
    worst = np.zeros(8)
    for B in SHAPES:
        for seed in range(6):
            inputs = cql_oracle.td_inputs(B, 100 + seed)
            kw = dict(loss_kind=loss_kind, use_valid=use_valid)
            want, mag = eval_oracle.sums_f64(inputs, **kw)
            got, mag32 = eval_oracle.restate_f32(inputs, **kw)
            assert np.all(np.abs(got - want) <= 1e-6 * mag), (B, seed)
            assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 7], want[:, 7])
            worst = np.maximum(worst, eval_oracle.worst_per_slot(got, want, mag))
    print("worst |f32 - f64| / sum |terms| per slot:", " ".join(f"{w:.1e}" for w in worst))


@pytest.mark.parametrize("kw", [dict(), dict(linear=1, clip_rect=0, gamma=0.5), dict(linear=0, clip_rect=0, gamma=0.99), dict(linear=1)],
                         ids=["rect", "linear-noclip", "noclip", "linear-rect"])
def test_target_variants_restate(kw):
    inputs = cql_oracle.td_inputs(96, 7, scale=2.5)
    for loss_kind in (0, 1):
        want, mag = eval_oracle.sums_f64(inputs, loss_kind=loss_kind, **kw)
        got, _ = eval_oracle.restate_f32(inputs, loss_kind=loss_kind, **kw)
        assert np.all(np.abs(got - want) <= 1e-6 * mag)


@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
def test_loss_and_penalty_slots_are_the_cql_objective(loss_kind, use_valid):
    """Slot 1 and slot 6 summed over the categories, times 1 / (n_cat * B), are cql_oracle.objective's TD loss (its loss minus alpha
    times its penalty) and its penalty, to 1e-12 relative."""
    B, alpha = 96, 0.5
    inputs = cql_oracle.td_inputs(B, 21 + loss_kind)
    o = cql_oracle.objective(inputs, alpha, loss_kind=loss_kind, use_valid=use_valid)
    table, _ = eval_oracle.sums_f64(inputs, loss_kind=loss_kind, use_valid=use_valid)
    inv = float(np.float32(1.0 / (5 * B)))  # (the float32 the objective scales by)
    pen, td = o["penalty"].item(), o["loss"].item() - alpha * o["penalty"].item()
    assert abs(table[:, 6].sum() * inv - pen) <= 1e-12 * abs(pen)
    assert abs(table[:, 1].sum() * inv - td) <= 1e-12 * abs(td)
    # the error slot against the objective's own per-sample error, and the count against the mask
    assert abs(table[:, 2].sum() / 5 - o["err"].sum().item()) <= 1e-12 * o["err"].sum().item()
    assert table[:, 0].sum() == (inputs[6].sum().item() if use_valid else 5 * B)


def test_one_action_has_no_penalty_and_full_agreement():
    inputs = cql_oracle.td_inputs(52, 3, n_act=1)
    for fn in (eval_oracle.sums_f64, eval_oracle.restate_f32):
        table, _ = fn(inputs, n_act=1)
        assert np.all(table[:, 6] == 0) and np.array_equal(table[:, 7], table[:, 0])


# ---- the config keys ---------------------------------------------------------------------------------------------------------------
def test_config_has_the_validation_keys_and_yaml_round_trip(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_validation
    c = get_cfg_defaults()
    assert c.VAL_DATASET == "" and c.VAL_INTERVAL == 0 and c.VAL_BATCHES == 0
    assert isinstance(c.VAL_INTERVAL, int) and isinstance(c.VAL_BATCHES, int)
    check_validation(c)  # the defaults pass, and so does the ground-truth branch while validation is off
    off = c.clone()
    off.TRAIN_ON_GROUND_TRUTH = True
    off.VAL_DATASET = "synthetic"
    check_validation(off)
    f = tmp_path / "config.yml"
    f.write_text("VAL_DATASET: 'synthetic'\nVAL_INTERVAL: 500\nVAL_BATCHES: 8\n")
    c.merge_from_file(str(f))
    assert (c.VAL_DATASET, c.VAL_INTERVAL, c.VAL_BATCHES) == ("synthetic", 500, 8)
    check_validation(c)
    f.write_text(c.dump())
    d = get_cfg_defaults()
    d.merge_from_file(str(f))
    assert dict(d) == dict(c)
    for text, key in (("VAL_INTERVAL: 2.5\n", "VAL_INTERVAL"), ("VAL_BATCHES: 'all'\n", "VAL_BATCHES"), ("VAL_DATASET: 3\n", "VAL_DATASET")):
        f.write_text(text)
        with pytest.raises(ValueError, match=key):
            get_cfg_defaults().merge_from_file(str(f))


@pytest.mark.parametrize("bad,key", [(dict(VAL_INTERVAL=2), "VAL_DATASET"), (dict(VAL_INTERVAL=2), "VAL_INTERVAL"),
                                     (dict(VAL_INTERVAL=-1, VAL_DATASET="synthetic"), "VAL_INTERVAL"),
                                     (dict(VAL_INTERVAL=2.5, VAL_DATASET="synthetic"), "VAL_INTERVAL"),
                                     (dict(VAL_INTERVAL=True, VAL_DATASET="synthetic"), "VAL_INTERVAL"),
                                     (dict(VAL_BATCHES=-3), "VAL_BATCHES"), (dict(VAL_BATCHES=1.5), "VAL_BATCHES"),
                                     (dict(VAL_DATASET=7), "VAL_DATASET"),
                                     (dict(VAL_INTERVAL=2, VAL_DATASET="synthetic", TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"),
                                     (dict(VAL_INTERVAL=2, VAL_DATASET="synthetic", TRAIN_ON_GROUND_TRUTH=True), "VAL_INTERVAL")])
def test_check_validation_raises_by_key_name(bad, key):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_validation
    c = get_cfg_defaults()
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=key):
        check_validation(c)


@pytest.mark.parametrize("text,key", [("VAL_INTERVAL: 2\n", "VAL_DATASET"), ("VAL_INTERVAL: -2\nVAL_DATASET: 'synthetic'\n", "VAL_INTERVAL"),
                                      ("VAL_INTERVAL: 2\nVAL_DATASET: 'synthetic'\nTRAIN_ON_GROUND_TRUTH: True\n", "TRAIN_ON_GROUND_TRUTH")])
def test_run_train_checks_validation_before_any_device_work(tmp_path, text, key):
    """run_train raises from check_validation before it touches a device (this machine may have none)."""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\n" + text)
    with pytest.raises(ValueError, match=key):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


def test_validation_walks_the_set_in_index_order_without_the_global_generators():
    """The pass indexes the dataset directly: VAL_DATASET 'synthetic' is seeded with SEED + 1, the batches are consecutive index
    ranges with the short last one, and neither torch's nor numpy's global generator moves."""
    from video_dqn_amd import validate
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.VAL_DATASET, c.VAL_INTERVAL, c.SEED, c.PANORAMA, c.BATCH_SIZE, c.VAL_BATCHES = "synthetic", 2, 4, False, 5, 3
    torch.manual_seed(9)
    np.random.seed(9)
    t0, n0 = torch.get_rng_state(), np.random.get_state()[1].copy()
    v = validate.Validator(c, log=lambda *a: None)
    assert v.dataset.seed == 5 and len(v.dataset) == validate.SYNTHETIC_LENGTH and v.n_batches == 3
    assert v.due(2) and v.due(4) and not v.due(3)
    batch = validate._collate([v.dataset[j] for j in range(5, 8)])
    assert batch[0].shape == (3, 224, 224, 3) and batch[0].dtype == torch.uint8 and batch[2].dtype == torch.int64
    assert torch.equal(batch[1][2], v.dataset[7][1]) and batch[3].shape == (3, 5)
    assert torch.equal(torch.get_rng_state(), t0) and np.array_equal(np.random.get_state()[1], n0)
    c.VAL_BATCHES = 0
    assert validate.Validator(c, log=lambda *a: None).n_batches == (validate.SYNTHETIC_LENGTH + 4) // 5


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_eval_symbols_at_abi_16():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_td_eval", "vdqn_net_td_eval"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert loaded.vdqn_abi_struct_size(7) == -1  # no new argument struct: both entries take the existing ones plus plain arguments


def _td_args(buf, **kw):
    from video_dqn_amd import _lib
    a = _lib.TdArgs()
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a.q_before = a.q_after_online = a.q_after_target = a.act = a.rew = a.term = a.valid = p
    a.batch, a.n_cat, a.n_act, a.ldq = 4, 5, 3, 64
    a.gamma, a.clip_rect = 0.9, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_td_eval_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    assert lib.vdqn_td_eval(None, p, None) != 0 and b"vdqn_td_eval" in lib.vdqn_last_error()
    assert lib.vdqn_td_eval(C.byref(_td_args(buf)), None, None) != 0 and b"vdqn_td_eval: null arg" in lib.vdqn_last_error()
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(use_valid=1, valid=None), dict(batch=0), dict(batch=-2), dict(n_cat=0), dict(n_act=0), dict(ldq=14), dict(n_cat=22),
               dict(loss_kind=2), dict(loss_kind=-1)):
        assert lib.vdqn_td_eval(C.byref(_td_args(buf, **kw)), p, None) != 0, kw
        assert b"vdqn_td_eval" in lib.vdqn_last_error(), kw
    assert lib.vdqn_td_eval(C.byref(_td_args(buf)), p + 4, None) != 0
    assert b"vdqn_td_eval: acc must be 8-byte aligned" in lib.vdqn_last_error()
    assert lib.vdqn_td_eval(C.byref(_td_args(buf, loss_kind=3)), p, None) != 0 and b"vdqn_td_eval: loss_kind 3" in lib.vdqn_last_error()


def test_net_td_eval_refuses_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    h = C.c_void_p()
    cfg = _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0)
    assert lib.vdqn_net_create(C.byref(cfg), C.byref(h)) == 0  # (host tables only: no device call)

    def args(**kw):
        a = _lib.StepArgs()
        a.packed_online = a.packed_target = a.before = a.after = a.act = a.rew = a.term = a.valid = a.acts_online = a.acts_target = p
        a.batch, a.gamma, a.clip_rect = 4, 0.9, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    try:
        assert lib.vdqn_net_td_eval(None, C.byref(args()), p, None) != 0 and b"vdqn_net_td_eval: null arg" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_eval(h, None, p, None) != 0 and b"vdqn_net_td_eval: null arg" in lib.vdqn_last_error()
        assert lib.vdqn_net_td_eval(h, C.byref(args()), None, None) != 0 and b"vdqn_net_td_eval: null arg" in lib.vdqn_last_error()
        for kw, word in ((dict(train_on_ground_truth=1), b"train_on_ground_truth"), (dict(sample_weight=p), b"sample_weight"),
                         (dict(sample_err=p), b"sample_err"), (dict(aug_params=p), b"aug_params"), (dict(packed_frames=p), b"packed_frames"),
                         (dict(acts_samples=4), b"acts_samples"), (dict(packed_online=None), b"null buffer"),
                         (dict(packed_target=None), b"null buffer"), (dict(before=None), b"null buffer"), (dict(after=None), b"null buffer"),
                         (dict(act=None), b"null buffer"), (dict(rew=None), b"null buffer"), (dict(term=None), b"null buffer"),
                         (dict(acts_online=None), b"null buffer"), (dict(acts_target=None), b"null buffer"),
                         (dict(use_valid=1, valid=None), b"use_valid"), (dict(batch=0), b"batch 0"), (dict(batch=5), b"batch 5"),
                         (dict(loss_kind=2), b"loss_kind 2")):
            assert lib.vdqn_net_td_eval(h, C.byref(args(**kw)), p, None) != 0, kw
            err = lib.vdqn_last_error()
            assert err.startswith(b"vdqn_net_td_eval: ") and word in err, (kw, err)
        assert lib.vdqn_net_td_eval(h, C.byref(args()), p + 4, None) != 0
        assert b"vdqn_net_td_eval: acc must be 8-byte aligned" in lib.vdqn_last_error()
    finally:
        lib.vdqn_net_destroy(h)


def test_stepper_has_the_eval_methods():
    from video_dqn_amd.engine import TDStepper
    for name in ("eval_begin", "eval_batch", "eval_result"):
        assert callable(getattr(TDStepper, name))
    assert len(TDStepper.EVAL_SLOTS) == 8
