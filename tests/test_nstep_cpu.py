"""n-step returns without a device: the successor rule, the float32 restatement of the walk against the float64 nested formula,
the config key and every refusal (host checks of the trainer and the argument checks of the two new C entries, which run before
any HIP call)."""
import ctypes as C
import os

import numpy as np
import pytest

import nstep_oracle


# ---- the successor rule --------------------------------------------------------------------------------------------------------------
def test_successors_smallest_match_no_match_self_loop():
    from video_dqn_amd.nstep import successors
    #                row: 0   1   2   3   4   5
    before0 = np.array([5,  7,  7,  9,  3,  3])
    after0 = np.array([7,  9,  4,  9,  5,  3])
    got = successors(before0, after0)
    assert got.dtype == np.int32
    # row 0 -> the smallest of rows {1, 2}; row 1 -> 3; row 2: no row starts at 4; row 3 -> itself; row 4 -> 0; row 5 -> the smallest of {4, 5}
    assert got.tolist() == [1, 3, -1, 3, 0, 4]
    assert successors(np.array([4]), np.array([4])).tolist() == [0] and successors(np.array([4]), np.array([5])).tolist() == [-1]
    assert successors(np.empty(0, np.int64), np.empty(0, np.int64)).shape == (0,)
    with pytest.raises(ValueError, match="successors"):
        successors(np.arange(3), np.arange(4))


def test_successors_against_a_python_loop_on_random_indices():
    """Random frame numbers with many repeats: self-loops, cycles and rows without a successor all occur."""
    from video_dqn_amd.nstep import chain_shares, successors
    rng = np.random.default_rng(2)
    before0, after0 = rng.integers(0, 24, 37), rng.integers(0, 30, 37)
    before0[9] = after0[9] = 29  # a self-loop (no other row starts at frame 29)
    got = successors(before0, after0)
    want = [next((r2 for r2 in range(37) if before0[r2] == after0[r]), -1) for r in range(37)]
    assert got.tolist() == want and -1 in want and any(w == r for r, w in enumerate(want))
    shares = chain_shares(got, 3)
    lengths = [len(nstep_oracle.chain(r, got, 3, 37)) for r in range(37)]
    assert shares == [lengths.count(k) / 37 for k in (1, 2, 3)] and abs(sum(shares) - 1) < 1e-12
    assert chain_shares(got, 1) == [1.0]


def test_successors_of_built_shards_are_row_plus_three(tmp_path):
    """The nine-JPEG episode of tests/test_shards_cpu.py: one row per frame i = 2 .. 9, (before = i, after = i + 3).  From the index
    as build_shards writes it, row r is followed by row r + 3 inside the episode and by nothing at its end."""
    from test_shards_cpu import _make_dataset
    from video_dqn_amd.nstep import successors
    from video_dqn_amd.shards import build_shards
    feather = _make_dataset(tmp_path)
    out = str(tmp_path / "shards")
    for with_previous in (True, False):
        build_shards(feather, out, shard_frames=4, with_previous=with_previous, log=lambda *a: None)
        idx = np.load(os.path.join(out, "index.npz"))
        assert successors(idx["before"][:, 0], idx["after"][:, 0]).tolist() == [3, 4, 5, 6, 7, -1, -1, -1]


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fractional", [False, True], ids=["binary", "fractional"])
def test_n1_is_the_row_itself(fractional):
    next_row, rew, term = nstep_oracle.tables(300, 5, 1, fractional)
    idx = nstep_oracle.indices(300, 65, 2)
    rew_n, term_n, disc, last, steps = nstep_oracle.walk_f32(idx, next_row, rew, term, 1, 0.99)
    rows = np.clip(idx, 0, 299)
    assert np.array_equal(rew_n, rew[rows]) and np.array_equal(last, rows) and np.all(steps == 1)
    assert np.array_equal(disc, np.full(65, np.float32(0.99)))
    if fractional:
        assert np.array_equal(term_n, np.float32(1) - (np.float32(1) - term[rows]))
    else:
        assert np.array_equal(term_n, term[rows]) and set(np.unique(term_n)) <= {0.0, 1.0}


@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_forward_form_equals_nested_form_exactly(n):
    """Binary rewards and terminals, gamma = 0.5 and bootstrap values that are multiples of 1/4: every operation of both forms is
    exact, so the forward-accumulated float32 walk, put through the loss's y = rew_n + disc * (1 - term_n) * Q, equals the
    float64 nested formula exactly — early stop, clamping, cycles and all."""
    N, n_cat = 300, 5
    next_row, rew, term = nstep_oracle.tables(N, n_cat, 3)
    q_boot = (np.random.default_rng(4).integers(-8, 9, (N, n_cat)) / 4.0).astype(np.float32)
    idx = nstep_oracle.indices(N, 257, 5)
    walk = nstep_oracle.walk_f32(idx, next_row, rew, term, n, 0.5)
    y32 = nstep_oracle.target_from_walk(walk, q_boot)
    y64 = nstep_oracle.nested_f64(idx, next_row, rew, term, n, 0.5, q_boot)
    assert np.array_equal(y32.astype(np.float64), y64)
    steps = walk[4]
    assert steps.min() >= 1 and steps.max() <= n
    assert np.array_equal(walk[2], np.float32(0.5) ** steps)
    if n >= 3:
        assert len(set(steps.tolist())) >= 3  # chains shorter than n, of n rows, and single rows all occur
    # the chain stops early only where nothing further can reach the target: every category's (1 - term_n) is then 0
    for b in range(len(idx)):
        rows = nstep_oracle.chain(idx[b], next_row, n, N)
        assert steps[b] == len(rows) or np.all(walk[1][b] == 1.0)


# ---- the config key and the trainer's refusals ------------------------------------------------------------------------------------------
def test_config_has_n_step_and_yaml_round_trip(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_nstep
    c = get_cfg_defaults()
    assert c.N_STEP == 1 and isinstance(c.N_STEP, int)
    check_nstep(c)  # the defaults pass, and so does every configuration n > 1 refuses while it is off
    for key in ("TRAIN_ON_GROUND_TRUTH", "LINEAR", "SYNTHETIC_DATA"):
        off = c.clone()
        off[key] = True
        check_nstep(off)
    f = tmp_path / "config.yml"
    f.write_text("N_STEP: 3\n")
    c.merge_from_file(str(f))
    assert c.N_STEP == 3
    f.write_text(c.dump())
    d = get_cfg_defaults()
    d.merge_from_file(str(f))
    assert d.N_STEP == 3 and dict(d) == dict(c)


def _shard_dir(tmp_path):
    d = tmp_path / "shards"
    d.mkdir(exist_ok=True)
    np.savez(d / "index.npz", before=np.zeros((1, 4), np.int64))  # (is_shard_dir looks for the file; nothing here opens it)
    return str(d)


@pytest.mark.parametrize("bad", [0, -1, 17, True, 2.0, "3", None])
def test_check_nstep_refuses_values_by_key_name(bad, tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.nstep import check_config
    from video_dqn_amd.trainer import check_nstep
    with pytest.raises(ValueError, match="N_STEP"):
        check_config(bad)
    c = get_cfg_defaults()
    c.DATASET = _shard_dir(tmp_path)
    c["N_STEP"] = bad  # (set directly: a YAML file would already fail the key's type check for most of these)
    with pytest.raises(ValueError, match="N_STEP"):
        check_nstep(c, 1)


@pytest.mark.parametrize("bad,word", [(dict(TRAIN_ON_GROUND_TRUTH=True), "TRAIN_ON_GROUND_TRUTH"), (dict(LINEAR=True), "LINEAR"),
                                      (dict(SYNTHETIC_DATA=True), "SYNTHETIC_DATA"), (dict(DATASET="none"), "SYNTHETIC_DATA"),
                                      (dict(DATASET="dataset/data.feather"), "feather"),
                                      (dict(DEVICE_RESIDENT_DATA="off"), "DEVICE_RESIDENT_DATA")])
def test_check_nstep_refuses_configurations_by_key_name(bad, word, tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    from video_dqn_amd.trainer import check_nstep
    c = get_cfg_defaults()
    c.DATASET = _shard_dir(tmp_path)
    c.N_STEP = 3
    check_nstep(c, 1)  # a shard directory, the TD branch, residency 'auto': accepted
    check_nstep(c, 8)
    for k, v in bad.items():
        c[k] = v
    with pytest.raises(ValueError, match=word) as e:
        check_nstep(c, 1)
    assert "N_STEP" in str(e.value)


def test_run_train_checks_nstep_before_any_device_work(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\nN_STEP: 3\n")
    with pytest.raises(ValueError, match="N_STEP.*SYNTHETIC_DATA"):
        run_train(ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False), log=lambda *a: None)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_nstep_symbols_and_the_struct_sizes_agree():
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_nstep_walk", "vdqn_td_loss_nstep"):
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS
    loaded = _lib.load()  # (compares sizeof(vdqn_step_args), which gained sample_gamma, with the binding's)
    assert loaded.vdqn_abi_struct_size(6) == C.sizeof(_lib.StepArgs)
    assert _lib.StepArgs._fields_[-1][0] == "sample_gamma" and _lib.StepArgs.sample_gamma.offset == C.sizeof(_lib.StepArgs) - 8
    assert loaded.vdqn_abi_struct_size(2) == C.sizeof(_lib.TdArgs)  # vdqn_td_args is as it was


def _walk_args(buf, **kw):
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a = dict(idx=p, batch=4, next_row=p, rew=p, term=p, n_rows=10, n_cat=5, n=3, gamma=0.99, rew_n=p, term_n=p, disc=p, last_row=p, steps=p)
    a.update(kw)
    return [a[k] for k in ("idx", "batch", "next_row", "rew", "term", "n_rows", "n_cat", "n", "gamma", "rew_n", "term_n", "disc", "last_row",
                           "steps")] + [None]


@pytest.mark.parametrize("kw,word", [(dict(idx=None), "null"), (dict(next_row=None), "null"), (dict(rew=None), "null"), (dict(term=None), "null"),
                                     (dict(rew_n=None), "null"), (dict(term_n=None), "null"), (dict(disc=None), "null"),
                                     (dict(last_row=None), "null"), (dict(steps=None), "null"), (dict(batch=0), "batch"),
                                     (dict(n_rows=0), "n_rows"), (dict(n_rows=2**31), "n_rows"), (dict(n_cat=0), "n_cat"), (dict(n_cat=9), "n_cat"),
                                     (dict(n=0), "n 0"), (dict(n=17), "n 17"), (dict(gamma=float("nan")), "gamma"),
                                     (dict(gamma=float("inf")), "gamma")])
def test_nstep_walk_argument_checks_fail_by_name_before_any_launch(kw, word):
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 64)()
    assert lib.vdqn_nstep_walk(*_walk_args(buf, **kw)) == -1
    msg = lib.vdqn_last_error().decode()
    assert msg.startswith("vdqn_nstep_walk:") and word in msg, msg


def test_td_loss_nstep_argument_checks_fail_by_name_before_any_launch():
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

    def fails(a, weight, err, alpha, pen, sg, word):
        assert lib.vdqn_td_loss_nstep(C.byref(a), weight, err, alpha, pen, sg, None) == -1
        msg = lib.vdqn_last_error().decode()
        assert msg.startswith("vdqn_td_loss_nstep:") and word in msg, msg

    fails(args(), None, None, 0.0, None, None, "sample_gamma")
    for alpha, weight in ((0.0, None), (0.0, p), (1.0, None)):  # plain, weighted, CQL
        fails(args(linear=1), weight, None, alpha, None, p, "linear")
    fails(args(), None, None, -1.0, None, p, "cql_alpha")
    fails(args(), None, None, float("nan"), None, p, "cql_alpha")
    fails(args(), None, p, 0.0, None, p, "err_out")
    fails(args(), None, None, 0.0, p, p, "penalty")
    fails(args(q_before=None), None, None, 0.0, None, p, "null")
    fails(args(n_act=1), None, None, 1.0, None, p, "n_act")
    fails(args(loss_kind=2), p, None, 0.0, None, p, "loss_kind")


def test_engine_entries_refuse_sample_gamma_by_name():
    """vdqn_net_td_eval with sample_gamma, and vdqn_net_td_forward with it on the ground-truth branch and with linear: refused by
    name before anything is launched (a storage-only engine: no device)."""
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, True, "f32", 8, device="cpu")
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    acc = (C.c_double * 40)()
    a = _lib.StepArgs()
    a.sample_gamma = p
    assert net.lib.vdqn_net_td_eval(net.handle, C.byref(a), C.addressof(acc), None) == -1
    msg = net.lib.vdqn_last_error().decode()
    assert msg.startswith("vdqn_net_td_eval: sample_gamma"), msg
    for kw, word in ((dict(train_on_ground_truth=1, gt=p), "train_on_ground_truth"), (dict(linear=1), "linear")):
        a = _lib.StepArgs()
        a.params = a.bnstats = a.packed_online = a.packed_target = a.before = a.after = a.act = a.rew = a.term = p
        a.acts_online = a.acts_target = a.bwd = a.loss = p
        a.batch, a.sample_gamma = 4, p
        for k, v in kw.items():
            setattr(a, k, v)
        for call in (lambda: net.lib.vdqn_net_td_forward(net.handle, C.byref(a), None),
                     lambda: net.lib.vdqn_net_td_forward_cql(net.handle, C.byref(a), 0.0, None, None)):
            assert call() == -1
            msg = net.lib.vdqn_last_error().decode()
            assert "sample_gamma" in msg and word in msg, msg
