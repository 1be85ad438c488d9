"""Held-out metrics of the head algorithms, host side: the float32 restatement of the three head metrics launches against the float64
oracle (tests/evalhead_oracle.py), the margins of every indicator slot over every input the GPU tests generate, the evaluation fields
of the rows of algos.ALGOS, and the C ABI's six new exports and their argument checks (no GPU: every call fails before it reaches
the device)."""
import ctypes as C

import numpy as np
import pytest

import bcq_oracle
import dist_oracle
import evalhead_oracle as oracle

ALGOS = ("iql", "dist", "bcq")


def _variants(algo):
    if algo == "dist":
        return [dict(kl_backwards=b, log_sigma=s) for b, s in dist_oracle.FLAGS]
    extra = [dict(threshold=t) for t in bcq_oracle.THRESHOLDS] if algo == "bcq" else [dict()]
    return [dict(kw, loss_kind=k) for kw in extra for k in (0, 1)]


@pytest.mark.parametrize("algo", ALGOS)
def test_restatement_meets_the_f64_oracle_within_the_gate(algo):
    """1e-5 of the sum of the slot's terms' absolute values, the gate of tests/test_gpu_eval.py; counts and indicators exact."""
    exact = {"iql": [0, 7], "dist": [0, 5], "bcq": [0, 4, 5, 6]}[algo]
    for B in oracle.BATCHES:
        for ldq in (64, oracle.TIGHT[algo]):
            inp = oracle.make(algo, B, ldq)
            for kw in _variants(algo):
                for use_valid in (False, True):
                    want, mag = oracle.sums_f64(algo, inp, use_valid=use_valid, **kw)
                    got, _ = oracle.restate_f32(algo, inp, use_valid=use_valid, **kw)
                    assert want.shape == (6, 8) and np.all(np.isfinite(want))
                    assert np.all(np.abs(got - want) <= 1e-5 * mag), (algo, B, ldq, kw, oracle.worst_per_slot(got, want, mag))
                    assert np.array_equal(got[:5, exact], want[:5, exact])
                    if algo == "bcq":
                        assert np.array_equal(got[5, [0, 2, 4, 6, 7]], want[5, [0, 2, 4, 6, 7]]) and want[5, 0] == B
                    else:
                        assert not want[5].any() and not got[5].any()


@pytest.mark.parametrize("algo", ALGOS)
def test_every_gpu_input_keeps_every_indicator_away_from_its_kink(algo):
    """Every seed the GPU tests use: the smallest distance of every indicator's argument from its kink, over EVERY row (none moved,
    none left out), is at least 1e-4: the distance of d * d from s2 (both spreads), of u from 0, the arg-max gaps at s and s', the
    logit margins at s and s' for every threshold."""
    cases = [(B, ldq, oracle.seed_of(algo, B, ldq)) for B in oracle.BATCHES for ldq in (64, oracle.TIGHT[algo])]
    cases += [(52, 64, oracle.ACC_SEEDS[algo][0]), (3, 64, oracle.ACC_SEEDS[algo][1])]
    for B, ldq, seed in cases:
        for name, value in oracle.margins(algo, oracle.make(algo, B, ldq, seed=seed)).items():
            assert value >= oracle.MARGIN, (algo, B, ldq, seed, name, value)


def test_threshold_zero_and_filled_rows_reduce_to_the_plain_metrics_in_f64():
    """The cross-checks the GPU tests make bit for bit, in the oracle: BCQ at threshold 0 and IQL with target rows filled with V(s')
    give the loss, |TD error| and target of tests/eval_oracle.py.  (That oracle takes gamma = 0.9 in float64, this one the float32 the
    kernel is handed: they differ by 2.4e-8 of gamma, and the sums by no more than that share of their terms; the gate here is 1e-6.)"""
    import eval_oracle
    inp = oracle.make("bcq", 52, 64)
    head, _ = oracle.sums_f64("bcq", inp, threshold=0.0)
    plain, _ = eval_oracle.sums_f64(inp)
    assert np.allclose(head[:5, [1, 2, 3, 5, 7]], plain[:, [1, 2, 5, 7, 4]], rtol=1e-6, atol=0) and not head[:5, [4, 6]].any()
    inp = oracle.make("iql", 52, 64)
    filled = list(inp)
    filled[2] = inp[1][:, 15:20].repeat_interleave(3, dim=1)  # every action column of category c holds V(s')[c]
    head, _ = oracle.sums_f64("iql", inp)
    plain, _ = eval_oracle.sums_f64(filled)
    assert np.allclose(head[:5, [3, 4, 6]], plain[:, [1, 2, 5]], rtol=1e-6, atol=0)


def test_rows_of_the_algorithm_table_carry_their_evaluation_fields():
    from video_dqn_amd import _lib, algos, validate
    from video_dqn_amd.engine import TDStepper
    seen = {tag for tag, _ in validate.SCALARS} | {f"avg_q_loss_cat{c}/val" for c in range(5)}
    assert len(validate.SCALARS) == 7 and len(TDStepper.EVAL_SLOTS) == 8
    for a in algos.ALGOS:
        assert a.eval_entry == a.entry.replace("td_forward", "td_eval") and a.eval_entry in _lib.EXPORTS
        assert len(a.eval_slots) == algos.HEAD_EVAL_SLOTS == 8 and a.eval_slots[0] == "count"
        assert len(set(a.eval_slots + a.eval_sample_slots)) == len(a.eval_slots) + len(a.eval_sample_slots)
        tags = [t for t, _ in algos.eval_tags(a)]
        assert len(tags) == len(set(tags)) == 7 + max(len(a.eval_sample_slots) - 1, 0) and not (set(tags) & seen)
        seen |= set(tags)
        for name in a.stats:  # every training statistic has its held-out twin
            assert f"{name}/val" in tags, name
    assert algos.IQL.eval_slots[3] == "iql_q_loss" and algos.DIST.eval_slots[1:6] == ("dist_kl", "dist_sigma", "dist_z2", "dist_nll", "dist_coverage")
    assert algos.BCQ.eval_slots[5] == "bcq_policy_agreement" and algos.BCQ.eval_sample_slots[:3] == ("samples", "bcq_bc_loss", "bcq_accuracy")
    assert algos.IQL.eval_sample_slots == () and algos.DIST.eval_sample_slots == ()
    s = type("S", (), dict(iql_expectile=0.7, dist_flags=3, sigma_min=0.1, bcq_threshold=0.3))()
    assert [a.eval_args(s) for a in algos.ALGOS] == [(0.7,), (3, 0.1), (0.3,)]


EXPORTS = ("vdqn_td_eval_iql", "vdqn_td_eval_dist", "vdqn_td_eval_bcq", "vdqn_net_td_eval_iql", "vdqn_net_td_eval_dist", "vdqn_net_td_eval_bcq")


def test_library_exports_the_head_eval_symbols_at_abi_16():
    import os
    from video_dqn_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(_lib.LIB_PATH)), "..", "include", "vdqn.h")).read()
    for name in EXPORTS:
        assert hasattr(lib, name) and name in _lib.EXPORTS and f"int {name}(" in header, name
    assert lib.vdqn_abi_version() == 16 == _lib.ABI_VERSION


def _td_args(buf, **kw):
    from video_dqn_amd import _lib
    a = _lib.TdArgs()
    p = C.addressof(buf)  # host memory, never dereferenced: every call below fails its argument check
    a.q_before = a.q_after_online = a.q_after_target = a.act = a.rew = a.term = a.valid = p
    a.batch, a.n_cat, a.n_act, a.ldq, a.gamma = 4, 5, 3, 64, 0.9
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("algo", ALGOS)
def test_head_operators_refuse_bad_arguments(algo):
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    name = f"vdqn_td_eval_{algo}".encode()
    fn = getattr(lib, name.decode())
    scalars = {"iql": (0.7,), "dist": (0, 0.1), "bcq": (0.3,)}[algo]

    def call(scalars=scalars, acc=p, **kw):
        return fn(C.byref(_td_args(buf, **kw)), *scalars, acc, None)
    assert fn(None, *scalars, p, None) != 0 and name + b": null arg" in lib.vdqn_last_error()
    tight = {"iql": 19, "dist": 29, "bcq": 17}[algo]
    for kw in (dict(q_before=None), dict(q_after_online=None), dict(q_after_target=None), dict(act=None), dict(rew=None), dict(term=None),
               dict(use_valid=1, valid=None), dict(batch=0), dict(n_cat=0), dict(ldq=tight), dict(batch=1 << 25, ldq=64), dict(linear=1),
               dict(loss_kind=2), dict(acc=None), dict(acc=p + 4)):
        assert call(**kw) != 0, kw
        assert lib.vdqn_last_error().startswith(name + b":"), (kw, lib.vdqn_last_error())
    assert call(ldq=tight) != 0 and b"ldq" in lib.vdqn_last_error()
    assert call(linear=1) != 0 and b"linear" in lib.vdqn_last_error()
    assert call(batch=1 << 25) != 0 and b"32-bit" in lib.vdqn_last_error()
    assert call(acc=p + 4) != 0 and b"8-byte aligned" in lib.vdqn_last_error()
    bad = {"iql": [((0.4,), b"expectile"), ((1.0,), b"expectile"), ((float("nan"),), b"expectile")],
           "dist": [((4, 0.1), b"flags"), ((0, 0.0), b"sigma_min"), ((0, float("inf")), b"sigma_min")],
           "bcq": [((-0.1,), b"threshold"), ((1.0,), b"threshold"), ((float("nan"),), b"threshold")]}[algo]
    for sc, word in bad:
        assert call(scalars=sc) != 0 and name + b": " + word in lib.vdqn_last_error(), (sc, lib.vdqn_last_error())
    if algo == "dist":
        assert call(loss_kind=1) != 0 and b"no Huber form" in lib.vdqn_last_error()
    if algo == "bcq":
        assert call(n_act=1) != 0 and b"n_act" in lib.vdqn_last_error()


def test_net_entries_refuse_bad_arguments():
    """Each engine entry refuses by ITS name: a null net, a net without its head, train_on_ground_truth, linear, its scalars, a null or
    misaligned acc_head, and then whatever vdqn_net_td_eval refuses (here: the missing buffers), all before any device work."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    cfg, nets = _lib.NetConfig(3, 5, 1, 1, _lib.VDQN_F32, 8, 0), {}
    for key, heads in (("plain", (0, 0, 0)), ("iql", (1, 0, 0)), ("dist", (0, 1, 0)), ("bcq", (0, 0, 1))):
        h = C.c_void_p()
        assert lib.vdqn_net_create_p(C.byref(cfg), *heads, C.byref(h)) == 0
        nets[key] = h
    try:
        for algo, good, bad, word in (("iql", (0.7,), (0.3,), b"expectile"), ("dist", (1, 0.1), (8, 0.1), b"flags"),
                                      ("bcq", (0.3,), (1.5,), b"threshold")):
            name = f"vdqn_net_td_eval_{algo}".encode()
            fn = getattr(lib, name.decode())
            a = _lib.StepArgs()
            call = lambda net, sc=good, acc_head=p: fn(net, C.byref(a), *sc, p, acc_head, None)  # noqa: E731
            assert call(None) != 0 and name + b": null arg" in lib.vdqn_last_error()
            assert call(nets["plain"]) != 0 and name + b": the net has no" in lib.vdqn_last_error()
            a.train_on_ground_truth = 1
            assert call(nets[algo]) != 0 and name in lib.vdqn_last_error() and b"train_on_ground_truth" in lib.vdqn_last_error()
            a.train_on_ground_truth, a.linear = 0, 1
            assert call(nets[algo]) != 0 and name + b": linear" in lib.vdqn_last_error()
            a.linear = 0
            assert call(nets[algo], sc=bad) != 0 and name + b": " + word in lib.vdqn_last_error()
            assert call(nets[algo], acc_head=None) != 0 and name + b": null arg" in lib.vdqn_last_error()
            assert call(nets[algo], acc_head=p + 4) != 0 and name + b": acc_head must be 8-byte aligned" in lib.vdqn_last_error()
            if algo == "dist":
                a.loss_kind = 1
                assert call(nets[algo]) != 0 and name + b": loss_kind" in lib.vdqn_last_error()
                a.loss_kind = 0
            a.sample_gamma = p
            assert call(nets[algo]) != 0 and b"vdqn_net_td_eval: sample_gamma" in lib.vdqn_last_error()
            a.sample_gamma = None
            assert call(nets[algo]) != 0 and b"vdqn_net_td_eval: null buffer" in lib.vdqn_last_error()
    finally:
        for h in nets.values():
            lib.vdqn_net_destroy(h)
