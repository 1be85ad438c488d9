"""Held-out validation on the GPU: vdqn_td_eval against the float64 oracle (tests/eval_oracle.py), its accumulation and its
determinism; vdqn_net_td_eval through TDStepper.eval_begin / eval_batch / eval_result against the operator and against the training
forward pass, both architectures; a validation pass between updates leaves training bit-identical; run_train with VAL_INTERVAL.

The gate of every slot is |got - oracle| <= 1e-5 of the sum of the slot's terms' absolute values (the relative 1e-5 that
tests/test_gpu_cql.py holds the loss and the penalty to, taken against the absolute sum because slots 3-5 cancel); slots 0 and 7
are sums of the 0/1 valid values and exact."""
import math

import numpy as np
import pytest
import torch

import cql_oracle
import eval_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _eval(inputs, use_valid=True, acc=None, **kw):
    """ops.td_eval on device inputs -> the [n_cat, 8] float64 table (still on the device)."""
    from video_dqn_amd import ops
    return ops.td_eval(*inputs[:6], inputs[6] if use_valid else None, acc=acc, **kw)


def _gate(got, cpu_inputs, what="", **kw):
    """The oracle gate on a [n_cat, 8] table; prints the measured worst per slot."""
    got = got.detach().cpu().numpy()
    want, mag = eval_oracle.sums_f64(cpu_inputs, **kw)
    worst = eval_oracle.worst_per_slot(got, want, mag)
    print(f"{what} worst |got - f64| / sum |terms| per slot:", " ".join(f"{w:.1e}" for w in worst))
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[:, 0], want[:, 0]) and np.array_equal(got[:, 7], want[:, 7])
    assert np.all(np.abs(got - want) <= 1e-5 * mag)
    return want, mag


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq", [(1, 64), (3, 64), (52, 64), (96, 64), (96, 15), (257, 64)],
                         ids=["B1", "B3", "B52", "B96", "ldq15", "B257"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_td_eval_vs_f64_oracle(loss_kind, use_valid, B, ldq):
    """One sample, fewer (sample, category) pairs than a wave, 260 pairs, 257 samples (a second pass of every block's threads)."""
    cpu = cql_oracle.td_inputs(B, 11 + loss_kind + 2 * use_valid, ldq=ldq)
    got = _eval(_dev(cpu), use_valid, gamma=0.9, loss_kind=("l2", "huber")[loss_kind])
    _gate(got, cpu, f"B {B} ldq {ldq}", loss_kind=loss_kind, use_valid=use_valid)


@pytest.mark.parametrize("linear,clip_rect,gamma", [(1, 1, 0.9), (0, 0, 0.99), (1, 0, 0.5)], ids=["linear-rect", "noclip", "linear-noclip"])
def test_td_eval_target_variants(linear, clip_rect, gamma):
    cpu = cql_oracle.td_inputs(96, 29)
    cpu[0] = cpu[0] * 2.5  # |d| beyond 1: both Huber branches
    for loss_kind in (0, 1):
        got = _eval(_dev(cpu), True, gamma=gamma, linear=bool(linear), clip_rect=bool(clip_rect), loss_kind=("l2", "huber")[loss_kind])
        _gate(got, cpu, f"linear {linear} clip {clip_rect}", loss_kind=loss_kind, linear=linear, clip_rect=clip_rect, gamma=gamma)


def test_td_eval_one_action_and_one_category():
    cpu = cql_oracle.td_inputs(52, 5, n_act=1)
    got = _eval(_dev(cpu), True, gamma=0.9, n_act=1)
    _gate(got, cpu, "n_act 1", n_act=1)
    assert torch.all(got[:, 6] == 0) and torch.equal(got[:, 7], got[:, 0])
    cpu = cql_oracle.td_inputs(52, 6, n_cat=1)
    got = _eval(_dev(cpu), True, gamma=0.9, n_cat=1)
    assert tuple(got.shape) == (1, 8)
    _gate(got, cpu, "n_cat 1", n_cat=1)


# ---- 2. accumulation ---------------------------------------------------------------------------------------------------------------
def test_td_eval_accumulates_with_one_f64_addition_and_touches_nothing_else():
    x_cpu, y_cpu = cql_oracle.td_inputs(96, 31), cql_oracle.td_inputs(52, 32)
    x, y = _dev(x_cpu), _dev(y_cpu)
    before = [t.clone() for t in x]
    sx, sy = _eval(x, gamma=0.9).cpu(), _eval(y, gamma=0.9).cpu()
    buf = torch.full((42,), 7.0, dtype=torch.float64, device=DEV)  # a guard word on each side of the [5][8] table
    acc = buf[1:41].view(5, 8)
    assert _eval(x, gamma=0.9, acc=acc) is acc
    torch.cuda.synchronize()
    assert buf[0].item() == 7.0 and buf[41].item() == 7.0
    assert torch.equal(acc.cpu(), 7.0 + sx)
    for t, t0 in zip(x, before):
        assert torch.equal(t, t0)
    # X and then Y into one table: the float64 sum of the separate results, bit for bit
    acc = _eval(x, gamma=0.9)
    _eval(y, gamma=0.9, acc=acc)
    assert torch.equal(acc.cpu(), sx + sy)


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------
def test_td_eval_is_bit_identical_run_to_run():
    x = _dev(cql_oracle.td_inputs(257, 41))
    runs = [_eval(x, gamma=0.9, loss_kind="huber").cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1])


# ---- 4. - 7. the engine -------------------------------------------------------------------------------------------------------------
def _stepper(dtype, B, deterministic=True, extra_capacity=True, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=deterministic)
    net.load_tensors(synth.make_state_dict(7, extra_capacity=extra_capacity))
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **kw)


_BATCHES = {}


def _batch(seed, B):
    """(before, after, src_kind, act, rew, term) on the device; made once per (seed, B) and never written."""
    if (seed, B) not in _BATCHES:
        from video_dqn_amd import synth
        (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
        before, after, act, rew, term = tup[:5]
        _BATCHES[(seed, B)] = (before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))
    return _BATCHES[(seed, B)]


def _first(batch, n):
    return tuple(t[:n].contiguous() if torch.is_tensor(t) else t for t in batch)


def _qf(net, stp, n):
    """The engine's f32 Q rows [.][64] of a pass over n samples: Q(s), the online Q(s') and the target network's Q(s'), as copies."""
    off = net.lib.vdqn_net_act_offset(net.handle, 2 * n, b"qf")
    off_t = net.lib.vdqn_net_act_offset(net.handle, n, b"qf")
    assert off >= 0 and off_t >= 0
    q = stp.acts_online[off:off + 2 * n * 64 * 4].view(torch.float32).view(2 * n, 64).clone()
    qt = stp.acts_target[off_t:off_t + n * 64 * 4].view(torch.float32).view(n, 64).clone()
    return q[:n], q[n:], qt


def _cpu_inputs(qb, qo, qt, batch):
    return [qb.cpu(), qo.cpu(), qt.cpu(), batch[3].cpu(), batch[4].cpu(), batch[5].cpu(), torch.ones_like(batch[4]).cpu()]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eval_pass_repeats_the_training_forward_and_is_the_operator(dtype):
    """After one forward_backward, eval_begin + eval_batch on the same batch leave the qf tensors of both workspaces as
    vdqn_net_td_forward left them, bit for bit (the eval-mode fold without the data-gradient operands, no arg-max bytes: the same
    forward), and eval_acc is ops.td_eval on them, bit for bit, within the oracle gate.  A short batch of 3 runs in the layout of 6
    samples inside the same workspaces: against the first 3 samples' rows within the operator gate."""
    from video_dqn_amd import ops
    B = 4
    net, stp = _stepper(dtype, B)
    from video_dqn_amd import synth
    other = type(net)(3, 5, 1, True, dtype, 2 * B, deterministic=True)
    other.load_tensors(synth.make_state_dict(8))
    other.pack_weights(stp.packed_target)  # a target network of its own
    batch = _batch(101, B)
    stp.forward_backward(*batch)
    torch.cuda.synchronize()
    trained = _qf(net, stp, B)
    grads, params = stp.grads.clone(), net.params.clone()
    stp.eval_begin()
    stp.eval_batch(*batch)
    res = stp.eval_result()
    qb, qo, qt = _qf(net, stp, B)
    for x, y in zip(trained, (qb, qo, qt)):
        assert torch.equal(x, y)
    ref = ops.td_eval(qb, qo, qt, batch[3], batch[4], batch[5], None, gamma=0.99, clip_rect=True)
    assert torch.equal(stp.eval_acc, ref) and torch.equal(res["table"], ref.cpu())
    want, _ = _gate(stp.eval_acc, _cpu_inputs(qb, qo, qt, batch), f"engine {dtype}", use_valid=False, gamma=0.99)
    assert res["count"] == 5 * B and abs(res["loss"] - want[:, 1].sum() / (5 * B)) <= 1e-5 * abs(want[:, 1]).sum() / (5 * B)
    assert torch.equal(stp.grads, grads) and torch.equal(net.params, params)
    # a short batch
    short = _first(batch, 3)
    stp.eval_begin()
    stp.eval_batch(*short)
    res3 = stp.eval_result()
    assert res3["count"] == 15
    rows = _cpu_inputs(trained[0][:3], trained[1][:3], trained[2][:3], short)
    _gate(stp.eval_acc, rows, f"engine {dtype}, 3 of 4", use_valid=False, gamma=0.99)


def test_eval_pass_basic_runs_on_running_statistics_and_leaves_them():
    """ARCHITECTURE 'basic', f32, batch 4: after one update (the running statistics have moved) the pass's online Q is
    NetEngine.forward — the eval-mode network — of the concatenated frames, and bnstats / num_batches_tracked are untouched."""
    B = 4
    net, stp = _stepper("f32", B, extra_capacity=False)
    batch = _batch(101, B)
    stp.step(*batch)
    torch.cuda.synchronize()
    bn, nbt, params = net.bnstats.clone(), net.num_batches_tracked.clone(), net.params.clone()
    stp.eval_begin()
    stp.eval_batch(*batch)
    res = stp.eval_result()
    qb, qo, qt = _qf(net, stp, B)
    assert torch.equal(net.bnstats, bn) and torch.equal(net.num_batches_tracked, nbt) and torch.equal(net.params, params)
    q = net.forward(torch.cat([batch[0], batch[1]]).contiguous(), 1, 2 * B)
    assert torch.equal(torch.cat([qb, qo])[:, :15], q)
    assert torch.equal(net.bnstats, bn)
    _gate(stp.eval_acc, _cpu_inputs(qb, qo, qt, batch), "basic", use_valid=False, gamma=0.99)
    assert res["count"] == 5 * B and all(math.isfinite(res[k]) for k in stp.EVAL_SLOTS)


@pytest.mark.parametrize("dtype,extra_capacity,kw", [("f32", True, dict(target_update_interval=2)),
                                                     ("bf16", True, dict(cql_alpha=1.0, target_tau=0.25, grad_clip_norm=10.0)),
                                                     ("f32", False, dict())], ids=["f32", "bf16-cql-tau-clip", "basic"])
def test_validation_between_updates_leaves_training_bit_identical(dtype, extra_capacity, kw):
    """Two deterministic steppers from one seed, three updates; one of them runs a validation pass of two batches (a full one and a
    short one) after every update.  Everything a later update or a checkpoint reads is bit-identical at the end."""
    B = 4
    ends = []
    for validate in (False, True):
        net, stp = _stepper(dtype, B, extra_capacity=extra_capacity, **kw)
        for t in (1, 2, 3):
            stp.step(*_batch(300 + t, B))
            if validate:
                stp.eval_begin()
                stp.eval_batch(*_batch(900, B))
                stp.eval_batch(*_first(_batch(901, B), 3))
                res = stp.eval_result()
                assert res["count"] == 5 * 7 and math.isfinite(res["loss"])
        torch.cuda.synchronize()
        ends.append(dict(params=net.params.cpu(), exp_avg=stp.exp_avg.cpu(), exp_avg_sq=stp.exp_avg_sq.cpu(), bnstats=net.bnstats.cpu(),
                         nbt=net.num_batches_tracked.cpu(), loss=stp.loss.cpu(),
                         target_params=(stp.target_params.cpu() if stp.target_params is not None else torch.zeros(1))))
    for name in ends[0]:
        assert torch.equal(ends[0][name], ends[1][name]), name


def test_soft_target_eval_sees_the_target_the_next_update_sees():
    """target_tau = 0.25: after two updates the eval pass's target qf on batch X is, bit for bit, the target qf the next step() on X
    leaves (eval_begin refolds packed_target from the averaged weights exactly as step() does)."""
    B = 4
    net, stp = _stepper("f32", B, target_tau=0.25)
    for t in (1, 2):
        stp.step(*_batch(300 + t, B))
    x = _batch(303, B)
    stp.eval_begin()
    stp.eval_batch(*x)
    stp.eval_result()
    seen = _qf(net, stp, B)[2]
    stp.step(*x)
    torch.cuda.synchronize()
    assert torch.equal(seen, _qf(net, stp, B)[2])
    net0, stp0 = _stepper("f32", B)  # (the target did move away from the hard copy)
    stp0.eval_begin()
    stp0.eval_batch(*x)
    stp0.eval_result()
    assert not torch.equal(seen, _qf(net0, stp0, B)[2])


def test_eval_batch_validation():
    from video_dqn_amd import _lib
    B = 4
    net, stp = _stepper("f32", B)
    batch = _batch(101, B)
    with pytest.raises(_lib.VdqnError, match="eval_begin"):
        stp.eval_batch(*batch)
    stp.eval_begin()
    big = tuple(torch.cat([t, t]) if torch.is_tensor(t) else t for t in batch)
    with pytest.raises(_lib.VdqnError, match="8 samples"):
        stp.eval_batch(*big)
    from video_dqn_amd.engine import TDStepper
    gt = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, train_on_ground_truth=True)
    with pytest.raises(_lib.VdqnError, match="train_on_ground_truth"):
        gt.eval_begin()


# ---- 8. run_train ------------------------------------------------------------------------------------------------------------------
class _Writer:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step=None):
        self.rows.append((tag, float(value), step))


def _write_cfg(folder, shards, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: 4\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def test_run_train_with_validation(tmp_path):
    """Four updates, VAL_INTERVAL 2, a validation set of 37 samples (nine batches of 4 and one of 1): passes at updates 2 and 4 over
    37 x 5 terms, finite means, every listed scalar written at the pass's update; VAL_BATCHES 1 caps the pass at one batch; and the
    run's final parameters are those of the same run without validation, bit for bit."""
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    from video_dqn_amd.validate import SCALARS
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    runs = {}
    for tag, extra in (("val", f"VAL_DATASET: '{shards}'\nVAL_INTERVAL: 2\n"), ("cap", f"VAL_DATASET: '{shards}'\nVAL_INTERVAL: 2\nVAL_BATCHES: 1\n"),
                       ("off", "")):
        _write_cfg(tmp_path / tag, shards, extra)
        cfg = ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False)
        cfg.writer = _Writer()
        logs = []
        model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
        runs[tag] = (model.engine.params.cpu(), stepper, cfg.writer.rows, logs)
        assert np.isfinite(running)
    params, stepper, rows, logs = runs["val"]
    assert [t for t, _ in stepper.val_history] == [2, 4]
    assert any(l.startswith("validation every 2 updates: 37 of 37 samples") for l in logs)
    tags = [t for t, _ in SCALARS] + [f"avg_q_loss_cat{c}/val" for c in range(5)]
    assert len(tags) == 12
    for t, res in stepper.val_history:
        assert res["count"] == 37 * 5 and res["table"][:, 0].tolist() == [37.0] * 5
        assert all(math.isfinite(res[k]) for k in stepper.EVAL_SLOTS) and all(math.isfinite(v) for v in res["loss_cat"])
        assert 0 <= res["action_agreement"] <= 1 and res["cql_penalty"] > 0 and res["loss"] >= 0
        for tag in tags:
            assert len([r for r in rows if r[0] == tag and r[2] == t and math.isfinite(r[1])]) == 1, (tag, t)
    assert sorted({r[2] for r in rows if r[0].endswith("/val")}) == [2, 4]
    assert [r[1] for r in rows if r[0] == "avg_q_loss/val"] == [res["loss"] for _, res in stepper.val_history]
    _, capped, _, _ = runs["cap"]
    assert [t for t, _ in capped.val_history] == [2, 4] and all(res["count"] == 4 * 5 for _, res in capped.val_history)
    off_params, off_stepper, off_rows, off_logs = runs["off"]
    assert off_stepper.val_history == [] and off_stepper.eval_acc is None and not any(r[0].endswith("/val") for r in off_rows)
    assert not any(l.startswith("validation every") for l in off_logs)
    assert torch.equal(params, off_params) and torch.equal(runs["cap"][0], off_params)
    assert torch.equal(stepper.exp_avg_sq, off_stepper.exp_avg_sq)
