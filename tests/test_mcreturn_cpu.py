"""Monte-Carlo returns without a GPU: the float32 restatement of the pointer-doubling rounds against the float64 walk of the
definition, `rounds_for`, the configuration keys and their refusals, and the C ABI (argument checks fail before any launch, so host
pointers are enough)."""
import ctypes as C
import os

import numpy as np
import pytest

import mc_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the table's arithmetic ------------------------------------------------------------------------------------------------------------
_TABLES = {}


def _tables(N, fractional):
    key = (N, fractional)
    if key not in _TABLES:
        _TABLES[key] = mc_oracle.tables(N, 5, 17 + N + int(fractional), fractional)
    return _TABLES[key]


@pytest.mark.parametrize("rounds", [1, 3, 8, 12])
@pytest.mark.parametrize("gamma", [0.9, 0.99, 1.0])
@pytest.mark.parametrize("fractional", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("N", [1, 7, 300, 5000])
def test_f32_rounds_against_the_f64_walk(N, fractional, gamma, rounds):
    """|f32 - f64| <= (3 R + 3) 2^-24 S per element, S the same sum over |r|, and exactly equal where S = 0: three roundings per round
    on a quantity bounded by S, plus the three of the initial state.  The worst case over these tables reaches about half of the
    bound."""
    next_row, rew, term = _tables(N, fractional)
    got = mc_oracle.returns_f32(next_row, rew, term, gamma, rounds)
    assert got.dtype == np.float32 and got.shape == rew.shape
    G, S = mc_oracle.returns_f64_walk(next_row, rew, term, gamma, rounds)
    err, lim = np.abs(got.astype(np.float64) - G), mc_oracle.bound(rounds, S)
    worst = (err[S > 0] / lim[S > 0]).max() if (S > 0).any() else 0.0
    print(f"N {N} gamma {gamma} R {rounds}: worst error {worst:.3f} of the bound")
    assert (err <= lim).all()
    assert np.array_equal(got[S == 0].astype(np.float64), G[S == 0])
    if not fractional:  # non-negative rewards: the return never falls below the row's own reward
        assert (got >= rew).all()


def test_tables_hold_the_special_entries():
    next_row, rew, term = mc_oracle.tables(300, 5, 1)
    assert next_row.dtype == np.int32 and next_row[0] == 0 and (next_row[1], next_row[2]) == (2, 1)
    assert (next_row[3], next_row[4], next_row[5]) == (-7, 300, 2**31 - 1)
    assert np.array_equal(term, rew) and set(np.unique(rew)) == {0.0, 1.0}
    assert (next_row[6:290] == np.arange(6, 290) + 3).mean() > 0.9 and (next_row[6:290] == -1).any()  # chains i -> i + 3, with breaks
    _, rew_f, term_f = mc_oracle.tables(300, 5, 1, True)
    assert 0 < rew_f.min() and rew_f.max() < 1 and term_f.max() < 0.9 and not np.array_equal(rew_f, term_f)
    # a cycle keeps adding its tail: with gamma 1 and no terminal, the self-loop's return doubles every round
    one = mc_oracle.returns_f32(np.array([0], np.int32), np.ones((1, 1), np.float32), np.zeros((1, 1), np.float32), 1.0, 5)
    assert one[0, 0] == 32.0


def test_rounds_for():
    from video_dqn_amd.mcreturn import rounds_for
    assert rounds_for(0.99, 10**6) == 12
    assert rounds_for(0.9, 10**6) == 8
    assert rounds_for(1.0, 300) == 9
    assert rounds_for(0.99, 1) == 1 and rounds_for(0.99, 2) == 1 and rounds_for(0.99, 3) == 2 and rounds_for(1.0, 2**31 - 1) == 31
    assert rounds_for(0.0, 10**6) == 1  # (clamped: one round at least)
    assert 0.99 ** (2.0 ** 12) <= 2.0 ** -30 < 0.99 ** (2.0 ** 11)


# ---- configuration --------------------------------------------------------------------------------------------------------------------
def _shard_dir(tmp_path):
    d = tmp_path / "shards"
    d.mkdir(exist_ok=True)
    np.savez(d / "index.npz", before=np.zeros((1, 4), np.int64))  # (is_shard_dir looks for the file; nothing here opens it)
    return str(d)


def test_config_keys_and_defaults(tmp_path):
    from video_dqn_amd import config
    from video_dqn_amd.trainer import check_mc, full_store_keys
    c = config.get_cfg_defaults()
    assert c.MC_RETURN_FLOOR is False and c.CQL_CALIBRATED is False
    assert "MC_RETURN_FLOOR" in config.__doc__ and "CQL_CALIBRATED" in config.__doc__
    check_mc(c)
    for key in ("TRAIN_ON_GROUND_TRUTH", "LINEAR", "SYNTHETIC_DATA"):  # nothing is refused while both keys are off
        off = c.clone()
        off[key] = True
        check_mc(off)
    assert full_store_keys(c) == []
    c.DATASET = _shard_dir(tmp_path)
    c.MC_RETURN_FLOOR, c.CQL_CALIBRATED, c.CQL_ALPHA, c.N_STEP, c.PRIORITIZED_REPLAY = True, True, 1.0, 3, True
    check_mc(c)
    assert [k for k, _ in full_store_keys(c)] == ["PRIORITIZED_REPLAY", "N_STEP", "MC_RETURN_FLOOR", "CQL_CALIBRATED"]
    f = tmp_path / "config.yml"
    f.write_text("MC_RETURN_FLOOR: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 0.5\n")
    d = config.get_cfg_defaults()
    d.merge_from_file(str(f))
    assert d.MC_RETURN_FLOOR is True and d.CQL_CALIBRATED is True


@pytest.mark.parametrize("key", ["MC_RETURN_FLOOR", "CQL_CALIBRATED"])
@pytest.mark.parametrize("bad,word", [(dict(TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"), (dict(LINEAR=True), "LINEAR"),
                                      (dict(SYNTHETIC_DATA=True), "SYNTHETIC_DATA"), (dict(DATASET="none"), "SYNTHETIC_DATA"),
                                      (dict(DATASET="dataset/data.feather"), "feather"),
                                      (dict(DEVICE_RESIDENT_DATA="off"), "DEVICE_RESIDENT_DATA")])
def test_check_mc_refuses_what_check_nstep_refuses_by_key_name(bad, word, key, tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_mc
    c = get_cfg_defaults()
    c.DATASET = _shard_dir(tmp_path)
    c[key] = True
    c.CQL_ALPHA = 1.0
    check_mc(c)
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=word) as e:
        check_mc(c)
    assert str(e.value).startswith(key)


def test_calibrated_needs_cql_alpha_and_bools_are_bools(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_mc
    c = get_cfg_defaults()
    c.DATASET = _shard_dir(tmp_path)
    c.CQL_CALIBRATED = True
    with pytest.raises(ValueError, match="CQL_CALIBRATED needs CQL_ALPHA > 0"):
        check_mc(c)
    for key in ("MC_RETURN_FLOOR", "CQL_CALIBRATED"):
        for bad in (1, "yes", None, 0.5):
            d = get_cfg_defaults()
            d[key] = bad
            with pytest.raises(ValueError, match=key):
                check_mc(d)


@pytest.mark.parametrize("text,word", [("SYNTHETIC_DATA: True\nMC_RETURN_FLOOR: True\n", "MC_RETURN_FLOOR.*SYNTHETIC_DATA"),
                                       ("SYNTHETIC_DATA: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 1.0\n", "CQL_CALIBRATED.*SYNTHETIC_DATA"),
                                       ("SYNTHETIC_DATA: True\nCQL_CALIBRATED: True\n", "CQL_CALIBRATED needs CQL_ALPHA")])
def test_run_train_checks_the_keys_before_any_device_work(tmp_path, text, word):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text(text)
    with pytest.raises(ValueError, match=word):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
NEW = ("vdqn_mc_returns", "vdqn_td_loss_mc", "vdqn_net_td_forward_mc")


def test_abi_is_16_structs_are_as_they_were_and_the_new_symbols_are_declared_and_exported():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "vdqn.h")).read()
    for name in NEW + ("vdqn_mc_returns_workspace_bytes",):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
        assert f" {name}(" in header, name
    loaded = _lib.load()
    assert loaded.vdqn_abi_version() == 16 and _lib.ABI_VERSION == 16
    for which, st in enumerate((_lib.ConvArgs, _lib.WgradArgs, _lib.TdArgs, _lib.NetConfig, _lib.ParamInfo, _lib.ProfEntry, _lib.StepArgs)):
        assert loaded.vdqn_abi_struct_size(which) == C.sizeof(st), st.__name__
    assert loaded.vdqn_abi_struct_size(7) == -1  # no eighth argument struct: every new argument is a plain one
    assert _lib.StepArgs._fields_[-1][0] == "sample_gamma"


def test_workspace_bytes():
    from video_dqn_amd import _lib
    lib = _lib.load()
    assert lib.vdqn_mc_returns_workspace_bytes(10**6, 5) == 4 * (2 * 10**6 + 3 * 5 * 10**6)
    assert lib.vdqn_mc_returns_workspace_bytes(1, 1) == 20
    assert lib.vdqn_mc_returns_workspace_bytes(2**31 - 1, 8) == 4 * 26 * (2**31 - 1)  # (past 2^32: the sizes are 64-bit)
    for n, c in ((0, 5), (2**31, 5), (10, 0), (10, 9)):
        assert lib.vdqn_mc_returns_workspace_bytes(n, c) == -1


def _mc_args(buf, **kw):
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a = dict(next_row=p, rew=p, term=p, n_rows=10, n_cat=5, gamma=0.99, rounds=4, G=p, workspace=p, workspace_bytes=4 * (20 + 150))
    a.update(kw)
    return [a[k] for k in ("next_row", "rew", "term", "n_rows", "n_cat", "gamma", "rounds", "G", "workspace", "workspace_bytes")] + [None]


@pytest.mark.parametrize("kw,word", [(dict(next_row=None), "null"), (dict(rew=None), "null"), (dict(term=None), "null"), (dict(G=None), "null"),
                                     (dict(workspace=None), "null"), (dict(n_rows=0), "n_rows"), (dict(n_rows=2**31), "n_rows"),
                                     (dict(n_cat=0), "n_cat"), (dict(n_cat=9), "n_cat"), (dict(rounds=0), "rounds 0"),
                                     (dict(rounds=32), "rounds 32"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("inf")), "gamma"),
                                     (dict(workspace_bytes=4 * (20 + 150) - 1), "workspace")])
def test_mc_returns_argument_checks_fail_by_name_before_any_launch(kw, word):
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    assert lib.vdqn_mc_returns(*_mc_args(buf, **kw)) == -1
    msg = lib.vdqn_last_error().decode()
    assert msg.startswith("vdqn_mc_returns:") and word in msg, msg


def test_td_loss_mc_argument_checks_fail_by_name_before_any_launch():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def args(**kw):
        a = _lib.TdArgs()
        a.q_before = a.q_after_online = a.q_after_target = a.act = a.rew = a.term = a.valid = a.loss = a.dq = p
        a.batch, a.n_cat, a.n_act, a.ldq = 4, 5, 3, 64
        a.gamma, a.inv_count, a.clip_rect = 0.99, 0.05, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def fails(a, weight, err, alpha, pen, sg, mc, flags, word):
        assert lib.vdqn_td_loss_mc(C.byref(a), weight, err, alpha, pen, sg, mc, flags, None, None) == -1
        msg = lib.vdqn_last_error().decode()
        assert msg.startswith("vdqn_td_loss_mc:") and word in msg, msg

    fails(args(), None, None, 0.0, None, None, None, 1, "mc_return is NULL")
    fails(args(), None, None, 0.0, None, None, p, 0, "mc_flags is 0")
    fails(args(), None, None, 1.0, None, None, p, 4, "unknown bits")
    fails(args(), None, None, 1.0, None, None, p, 7, "unknown bits")
    fails(args(), None, None, 0.0, None, None, p, 2, "calibrated")
    fails(args(), p, None, 0.0, None, None, p, 3, "calibrated")
    for alpha, weight in ((0.0, None), (0.0, p), (1.0, None)):  # plain, weighted, CQL; with and without a per-sample discount
        for sg in (None, p):
            fails(args(linear=1), weight, None, alpha, None, sg, p, 1, "linear")
    fails(args(), None, None, -1.0, None, None, p, 1, "cql_alpha")
    fails(args(), None, None, float("nan"), None, None, p, 1, "cql_alpha")
    fails(args(), None, p, 0.0, None, None, p, 1, "err_out")
    fails(args(), None, None, 0.0, p, None, p, 1, "penalty")
    fails(args(q_before=None), None, None, 0.0, None, None, p, 1, "null")
    fails(args(n_act=1), None, None, 1.0, None, None, p, 3, "n_act")
    fails(args(loss_kind=2), p, None, 0.0, None, None, p, 1, "loss_kind")


def test_engine_entry_refuses_by_name():
    """vdqn_net_td_forward_mc on a storage-only engine (no device): the ground-truth branch, linear, bad flags and calibrated without
    a penalty are refused by name before anything is launched; with mc_return NULL it is vdqn_net_td_forward_cql, refusals included."""
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, True, "f32", 8, device="cpu")
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def args(**kw):
        a = _lib.StepArgs()
        a.params = a.bnstats = a.packed_online = a.packed_target = a.before = a.after = a.act = a.rew = a.term = p
        a.acts_online = a.acts_target = a.bwd = a.loss = p
        a.batch = 4
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for a, alpha, flags, word in ((args(train_on_ground_truth=1, gt=p), 0.0, 1, "train_on_ground_truth"), (args(linear=1), 0.0, 1, "linear"),
                                  (args(), 0.0, 0, "mc_flags is 0"), (args(), 1.0, 8, "unknown bits"), (args(), 0.0, 2, "calibrated"),
                                  (args(), float("nan"), 1, "cql_alpha")):
        assert net.lib.vdqn_net_td_forward_mc(net.handle, C.byref(a), alpha, None, p, flags, None, None) == -1
        msg = net.lib.vdqn_last_error().decode()
        assert msg.startswith("vdqn_net_td_forward_mc:") and word in msg, msg
    a = args(train_on_ground_truth=1, gt=p)
    assert net.lib.vdqn_net_td_forward_mc(net.handle, C.byref(a), 1.0, None, None, 0, None, None) == -1
    assert net.lib.vdqn_last_error().decode().startswith("vdqn_net_td_forward_cql:")


def test_stepper_keys_are_validated_on_the_host():
    from video_dqn_amd import engine
    import inspect
    sig = inspect.signature(engine.TDStepper.__init__).parameters
    assert sig["mc_floor"].default is False and sig["cql_calibrated"].default is False
    assert inspect.signature(engine.TDStepper.step).parameters["mc_return"].default is None
