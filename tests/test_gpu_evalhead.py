"""Held-out metrics of the head algorithms on the GPU: vdqn_td_eval_iql / _dist / _bcq against the float64 oracle
(tests/evalhead_oracle.py), their tolerance-free cross-checks against vdqn_td_eval, accumulation and determinism; the engine entries
through TDStepper.eval_begin / eval_batch / eval_result against the operators and against a stepper without the algorithm; a
validation pass between updates leaves training bit-identical; run_train with VAL_INTERVAL under each algorithm.

The gate of every slot is |got - oracle| <= 1e-5 of the sum of the slot's terms' absolute values, the gate tests/test_gpu_eval.py
holds; the count and indicator slots are exact (tests/test_evalhead_cpu.py asserts that no indicator of these inputs sits within 1e-4
of its kink).  The distributional slots that pass through log1pf / expf / a quotient were expected to need more; they do not: the worst
ratio measured on an MI355X against the float64 oracle over the shapes below is 5.4e-7 (slot 1, the KL; 1.7e-7 for z2 and 4.4e-7 for
the NLL; profiles/evalhead_record.txt), so the gate of every slot stays at 1e-5."""
import math

import numpy as np
import pytest
import torch

import bcq_oracle
import dist_oracle
import evalhead_oracle as oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = {"iql": [0, 7], "dist": [0, 5], "bcq": [0, 4, 5, 6]}
GATE = 1e-5


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _kw_ops(algo, kw):
    """The oracle's keywords as ops.td_eval_<algo> takes them."""
    out = dict(gamma=0.9, loss_kind=("l2", "huber")[kw.get("loss_kind", 0)])
    if algo == "iql":
        out["expectile"] = oracle.TAU
    elif algo == "dist":
        out.update(kl_backwards=kw.get("kl_backwards", False), log_sigma=kw.get("log_sigma", False), sigma_min=oracle.SIGMA_MIN)
    else:
        out["threshold"] = kw.get("threshold", 0.3)
    return out


def _head(algo, inputs, use_valid=True, acc=None, **kw):
    from video_dqn_amd import ops
    return getattr(ops, f"td_eval_{algo}")(*inputs[:6], inputs[6] if use_valid else None, acc=acc, **kw)


def _gate(algo, got, cpu_inputs, what="", **kw):
    """The oracle gate on a [n_cat + 1, 8] table; prints the measured worst per slot."""
    got = got.detach().cpu().numpy()
    want, mag = oracle.sums_f64(algo, cpu_inputs, **kw)
    worst = oracle.worst_per_slot(got, want, mag)
    print(f"evalhead {algo} {what} worst |got - f64| / sum |terms| per slot:", " ".join(f"{w:.1e}" for w in worst))
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[:5, EXACT[algo]], want[:5, EXACT[algo]])
    if algo == "bcq":
        assert np.array_equal(got[5, [0, 2, 4, 6, 7]], want[5, [0, 2, 4, 6, 7]])
    else:
        assert not got[5].any()
    assert np.all(np.abs(got - want) <= GATE * mag)
    return want, mag


# ---- 1. the operators --------------------------------------------------------------------------------------------------------------
def _variants(algo):
    if algo == "dist":
        return [dict(kl_backwards=b, log_sigma=s) for b, s in dist_oracle.FLAGS]
    extra = [dict(threshold=t) for t in bcq_oracle.THRESHOLDS] if algo == "bcq" else [dict()]
    return [dict(kw, loss_kind=k) for kw in extra for k in (0, 1)]


@pytest.mark.parametrize("B", oracle.BATCHES)
@pytest.mark.parametrize("ldq", ["64", "tight"])
@pytest.mark.parametrize("algo", ["iql", "dist", "bcq"])
def test_head_operator_vs_f64_oracle(algo, ldq, B):
    """One sample, fewer samples than a wave, several waves, 257 samples (a second pass of thread 0); ldq 64 and the tightest the layout
    allows; the valid mask on and off; both loss kinds, all four distributional instances, the three thresholds."""
    ldq = 64 if ldq == "64" else oracle.TIGHT[algo]
    cpu = oracle.make(algo, B, ldq)
    dev = _dev(cpu)
    for kw in _variants(algo):
        for use_valid in (False, True):
            got = _head(algo, dev, use_valid, **_kw_ops(algo, kw))
            _gate(algo, got, cpu, f"B {B} ldq {ldq} valid {int(use_valid)} {kw}", use_valid=use_valid, **kw)


# ---- 2. cross-checks that need no tolerance ----------------------------------------------------------------------------------------
def _plain(inputs, use_valid=True, **kw):
    from video_dqn_amd import ops
    return ops.td_eval(*inputs[:6], inputs[6] if use_valid else None, **kw)


@pytest.mark.parametrize("loss_kind", ["l2", "huber"])
def test_iql_with_target_rows_of_v_next_is_the_plain_launch_bit_for_bit(loss_kind):
    """vdqn_td_eval on a q_after_target whose every action column of category c holds V(s')[c] forms y from V(s'): its loss, |TD
    error| and target sums are slots 3, 4 and 6 of the IQL head table."""
    for B in (52, 257):
        x = _dev(oracle.make("iql", B, 64))
        x[0] = x[0] * 2.5  # |d| beyond 1: both Huber branches
        head = _head("iql", x, expectile=oracle.TAU, gamma=0.9, loss_kind=loss_kind)
        filled = list(x)
        filled[2] = torch.zeros_like(x[1])
        filled[2][:, :15] = x[1][:, 15:20].repeat_interleave(3, dim=1)
        plain = _plain(filled, gamma=0.9, loss_kind=loss_kind)
        assert torch.equal(head[:5, [0, 3, 4, 6]], plain[:, [0, 1, 2, 5]])


@pytest.mark.parametrize("loss_kind", ["l2", "huber"])
def test_bcq_at_threshold_zero_is_the_plain_launch_bit_for_bit(loss_kind):
    for B in (52, 257):
        x = _dev(oracle.make("bcq", B, 64))
        x[0] = x[0] * 2.5
        head = _head("bcq", x, threshold=0.0, gamma=0.9, loss_kind=loss_kind)
        plain = _plain(x, gamma=0.9, loss_kind=loss_kind)
        assert torch.equal(head[:5, [0, 1, 2, 3, 5, 7]], plain[:, [0, 1, 2, 5, 7, 4]])
        assert not head[:5, [4, 6]].any()
        assert head[5, 4].item() == 3 * B and head[5, 6].item() == 3 * B  # every action allowed, at s and at s'


@pytest.mark.parametrize("algo", ["iql", "dist", "bcq"])
def test_head_operator_accumulates_with_one_f64_addition_and_touches_nothing_else(algo):
    kw = _kw_ops(algo, {})
    sx_seed, sy_seed = oracle.ACC_SEEDS[algo]
    x, y = _dev(oracle.make(algo, 52, 64, seed=sx_seed)), _dev(oracle.make(algo, 3, 64, seed=sy_seed))
    before = [t.clone() for t in x]
    sx, sy = _head(algo, x, **kw).cpu(), _head(algo, y, **kw).cpu()
    buf = torch.full((50,), 7.0, dtype=torch.float64, device=DEV)  # a guard word on each side of the [6][8] table
    acc = buf[1:49].view(6, 8)
    assert _head(algo, x, acc=acc, **kw) is acc
    torch.cuda.synchronize()
    assert buf[0].item() == 7.0 and buf[49].item() == 7.0
    assert torch.equal(acc.cpu(), 7.0 + sx)
    for t, t0 in zip(x, before):
        assert torch.equal(t, t0)
    acc = _head(algo, x, **kw)
    _head(algo, y, acc=acc, **kw)
    assert torch.equal(acc.cpu(), sx + sy)


@pytest.mark.parametrize("algo", ["iql", "dist", "bcq"])
def test_head_operator_is_bit_identical_run_to_run(algo):
    x = _dev(oracle.make(algo, 257, 64))
    runs = [_head(algo, x, **_kw_ops(algo, {})).cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


# ---- 3. the engine -----------------------------------------------------------------------------------------------------------------
MODES = {"iql": (dict(value_head=True), dict(iql_expectile=0.7)), "dist": (dict(spread_head=True), dict(distributional=True, kl_backwards=True)),
         "bcq": (dict(policy_head=True), dict(bcq_threshold=0.3))}
B = 4


def _net(algo, dtype, extra_capacity=True, seed=7):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=True, **MODES[algo][0])
    net.load_tensors(synth.make_state_dict(seed, extra_capacity=extra_capacity))
    g = torch.Generator().manual_seed(seed + 1)
    for name in net.head_keys:
        v = net.view(name)
        v.copy_((0.05 * torch.randn(v.shape, generator=g)).to(v.device))
    net.mark_dirty()
    return net


def _stepper(net, algo=None, **kw):
    from video_dqn_amd.engine import TDStepper
    return TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **(MODES[algo][1] if algo else {}), **kw)


def _op_kw(stp):
    a = stp.algo
    if a.key == "IQL_EXPECTILE":
        return "iql", dict(expectile=stp.iql_expectile), dict(tau=stp.iql_expectile)
    if a.key == "DISTRIBUTIONAL":
        f = stp.dist_flags
        return "dist", dict(flags=f, sigma_min=stp.sigma_min), dict(kl_backwards=bool(f & 1), log_sigma=bool(f & 2), sigma_min=stp.sigma_min)
    return "bcq", dict(threshold=stp.bcq_threshold), dict(threshold=stp.bcq_threshold)


def _check_engine(algo, dtype, extra_capacity=True):
    from test_gpu_eval import _batch, _cpu_inputs, _first, _qf
    net = _net(algo, dtype, extra_capacity)
    stp, plain = _stepper(net, algo), _stepper(net)
    _net(algo, dtype, extra_capacity, seed=8).pack_weights(stp.packed_target)  # a target network of its own, head included
    plain.packed_target.copy_(stp.packed_target)
    assert plain.algo is None and stp.eval_head_acc is None
    batch, second = _batch(101, B), _batch(102, B)
    tables = {}
    for name, bs in (("x", [batch]), ("y", [second]), ("xy", [batch, second]), ("short", [_first(batch, 3)])):
        plain.eval_begin()
        stp.eval_begin()
        for b in bs:
            plain.eval_batch(*b)
        want = plain.eval_result()
        assert "head" not in want and plain.eval_head_acc is None
        for b in bs:
            stp.eval_batch(*b)
        res = stp.eval_result()
        assert torch.equal(res["table"], want["table"]), name  # the existing table: bit for bit that of a stepper without the algorithm
        assert all(res[key] == want[key] for key in want if key != "table")  # (every count is positive: no NaN mean)
        tables[name] = res["head"]["table"]
        if len(bs) == 1:  # the head table is the operator on the engine's own rows, bit for bit, and passes the oracle gate
            n = int(bs[0][3].shape[0])
            qb, qo, qt = _qf(net, stp, n)  # (IQL: the target workspace now holds Q_target(s))
            op, op_kw, oracle_kw = _op_kw(stp)
            ref = _head(op, [qb, qo, qt, bs[0][3], bs[0][4], bs[0][5], None], use_valid=False, gamma=0.99, **op_kw)
            assert torch.equal(stp.eval_head_acc, ref) and torch.equal(res["head"]["table"], ref.cpu()), name
            _gate(op, stp.eval_head_acc, _cpu_inputs(qb, qo, qt, bs[0]), f"engine {dtype} {name}", use_valid=False, gamma=0.99, **oracle_kw)
            head = res["head"]
            assert head["count"] == 5 * n and head["table"].shape == (6, 8)
            for k, slot in enumerate(stp.algo.eval_slots[1:], 1):
                assert head[slot] == float(ref.cpu()[:5, k].sum() / (5 * n)) and len(head[slot + "_cat"]) == 5
            if op == "bcq":
                assert head["samples"] == n and 0 <= head["bcq_accuracy"] <= 1 and 1 <= head["bcq_allowed_actions"] <= 3
    # a second batch queued directly behind the first: the per-batch tables' f64 sum (IQL: its second target pass is ordered behind the
    # first batch's standard launch, and the second batch's target pass behind the first batch's head launch)
    assert torch.equal(tables["xy"], tables["x"] + tables["y"])
    assert tables["short"][:5, 0].tolist() == [3.0] * 5


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("algo", ["iql", "dist", "bcq"])
def test_engine_head_table_is_the_operator_and_the_plain_table_is_untouched(algo, dtype):
    _check_engine(algo, dtype)


def test_engine_head_table_basic_architecture():
    _check_engine("dist", "f32", extra_capacity=False)


@pytest.mark.parametrize("algo", ["iql", "dist", "bcq"])
def test_validation_between_updates_leaves_head_training_bit_identical(algo):
    """Two deterministic steppers from one seed, three updates; one of them runs a validation pass of two batches (a full one and a
    short one) after every update.  Parameters (the head's included), Adam moments, BatchNorm statistics, the target and the loss
    statistics are bit-identical at the end."""
    from test_gpu_eval import _batch, _first
    ends = []
    for validate in (False, True):
        net = _net(algo, "f32")
        stp = _stepper(net, algo, target_update_interval=2)
        for t in (1, 2, 3):
            stp.step(*_batch(300 + t, B))
            if validate:
                stp.eval_begin()
                stp.eval_batch(*_batch(900, B))
                stp.eval_batch(*_first(_batch(901, B), 3))
                res = stp.eval_result()
                assert res["count"] == 5 * 7 and res["head"]["count"] == 5 * 7 and all(math.isfinite(res["head"][k]) for k in stp.algo.eval_slots)
        torch.cuda.synchronize()
        ends.append(dict(params=net.params.cpu(), exp_avg=stp.exp_avg.cpu(), exp_avg_sq=stp.exp_avg_sq.cpu(), bnstats=net.bnstats.cpu(),
                         nbt=net.num_batches_tracked.cpu(), loss=stp.loss.cpu(), stats=stp.loss_stats.cpu(), target=stp.packed_target.cpu()))
    for name in ends[0]:
        assert torch.equal(ends[0][name], ends[1][name]), name


# ---- 4. run_train ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,extra", [("iql", "IQL_EXPECTILE: 0.7\n"), ("dist", "DISTRIBUTIONAL: True\n"), ("bcq", "BCQ_THRESHOLD: 0.3\n"),
                                        (None, "")], ids=["iql", "dist", "bcq", "off"])
def test_run_train_with_validation_writes_the_head_scalars(algo, extra, tmp_path):
    from test_gpu_eval import _Writer, _write_cfg
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd import algos
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    from video_dqn_amd.validate import SCALARS
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    _write_cfg(tmp_path / "run", shards, f"VAL_DATASET: '{shards}'\nVAL_INTERVAL: 2\nVAL_BATCHES: 2\n" + extra)
    cfg = ExperimentConfig(str(tmp_path / "run"), device=DEV, tensorboard=False)
    cfg.writer = _Writer()
    logs = []
    model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
    rows = cfg.writer.rows
    assert np.isfinite(running) and [t for t, _ in stepper.val_history] == [2, 4]
    old = [t for t, _ in SCALARS] + [f"avg_q_loss_cat{c}/val" for c in range(5)]
    every = {t for a in algos.ALGOS for t, _ in algos.eval_tags(a)}
    mine = [t for t, _ in algos.eval_tags(stepper.algo)] if algo else []
    assert (stepper.algo is None) == (algo is None)
    for t, res in stepper.val_history:
        for tag in old + mine:
            assert len([r for r in rows if r[0] == tag and r[2] == t and math.isfinite(r[1])]) == 1, (tag, t)
        assert ("head" in res) == (algo is not None)
        if algo:
            assert res["head"]["count"] == res["count"] == 8 * 5 and res["head"]["table"].shape == (6, 8)
            assert [r[1] for r in rows if r[0] == mine[0] and r[2] == t] == [res["head"][mine[0][:-4]]]
    assert {r[0] for r in rows if r[0].endswith("/val")} == set(old + mine)  # the other algorithms' tags never appear
    assert not ({r[0] for r in rows} & (every - set(mine)))
    line = [l for l in logs if "validation adds" in l]
    if algo:
        assert len(line) == 1 and mine[0] in line[0] and not any("validation is unchanged" in l for l in logs)
    else:
        assert not line and stepper.eval_head_acc is None
