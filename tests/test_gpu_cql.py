"""The conservative Q-learning penalty on the GPU: vdqn_td_loss_cql against the float64 autograd oracle (tests/cql_oracle.py) and
against vdqn_td_loss_weighted, its deterministic mode, TDStepper(cql_alpha=...) against the operator and the float64 network
oracle, both architectures and bf16x3, run_train with CQL_ALPHA, and two ranks against one process."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import cql_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _cql(inputs, alpha, dtype=None, loss_kind=0, use_valid=True, weight=None, with_err=True, linear=0, clip_rect=1, gamma=0.9,
         deterministic=1, n_cat=5, n_act=3, q_copy=False):
    """vdqn_td_loss_cql through the raw ABI -> (loss, penalty, dq as f32, dq_f32, err, q_copy), all on the CPU."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    dtype = _lib.VDQN_F32 if dtype is None else dtype
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    loss, pen = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    dq = torch.full((B, ldq), 7.0, dtype=torch.bfloat16 if dtype == _lib.VDQN_BF16 else torch.float32, device=DEV)
    dq32 = torch.full((B, ldq), 7.0, device=DEV)
    err = torch.full((B,), -1.0, device=DEV) if with_err else None
    qc = torch.full((B, n_cat * n_act), -7.0, device=DEV) if q_copy else None
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = qb.data_ptr(), qo.data_ptr(), qt.data_ptr()
    a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
    a.loss, a.dq, a.dq_f32 = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr()
    a.batch, a.n_cat, a.n_act, a.ldq = B, n_cat, n_act, ldq
    a.gamma, a.inv_count = gamma, 1.0 / (n_cat * B)
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, linear, int(use_valid), dtype, loss_kind, deterministic
    a.q_copy = qc.data_ptr() if q_copy else None
    _lib.check(lib.vdqn_td_loss_cql(C.byref(a), weight.data_ptr() if weight is not None else None, err.data_ptr() if with_err else None,
                                    alpha, pen.data_ptr(), torch.cuda.current_stream().cuda_stream), "vdqn_td_loss_cql")
    torch.cuda.synchronize()
    return loss.cpu(), pen.cpu(), dq.float().cpu(), dq32.cpu(), (err.cpu() if with_err else None), (qc.cpu() if q_copy else None)


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _check_against_oracle(inputs, alpha, got, n=15, **kw):
    """The issue's operator gate: every dq column within 1e-6 of the maximum element, padding exactly 0, loss and penalty within
    1e-5 relative, err within 1e-6."""
    loss, pen, _, dq32, err, _ = got
    o = cql_oracle.objective(inputs, alpha, **kw)
    dq_max = o["dq"].abs().max().item()
    e_dq = (dq32[:, :n].double() - o["dq"]).abs().max().item() / dq_max
    e_loss = abs(loss.item() - o["loss"].item()) / abs(o["loss"].item())
    e_pen = abs(pen.item() - o["penalty"].item()) / abs(o["penalty"].item())
    print(f"dq {e_dq:.2e} of the max element, loss {e_loss:.2e}, penalty {e_pen:.2e} relative")
    assert torch.isfinite(dq32).all() and math.isfinite(loss.item()) and math.isfinite(pen.item())
    assert e_dq <= 1e-6
    assert torch.all(dq32[:, n:] == 0)
    assert e_loss <= 1e-5 and e_pen <= 1e-5
    if err is not None:
        e_err = (err.double() - o["err"]).abs().max().item() / max(o["err"].abs().max().item(), 1e-30)
        print(f"err {e_err:.2e}")
        assert e_err <= 1e-6
    return o


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq", [(96, 64), (1, 64), (3, 64), (96, 15)], ids=["B96", "B1", "B3", "ldq15"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_td_loss_cql_vs_f64_oracle(loss_kind, use_valid, weighted, B, ldq):
    """Inputs as tests/test_gpu_replay.py::_td_inputs; both deterministic settings; bf16 dq is dq_f32 rounded once."""
    from video_dqn_amd import _lib
    cpu = cql_oracle.td_inputs(B, 11 + loss_kind + 2 * use_valid, ldq=ldq)
    if use_valid:
        cpu[6][0, 0] = 1.0  # (B = 1: at least one valid term, so the relative gates have something to divide by)
    w = _weights(B) if weighted else None
    inputs = _dev(cpu)
    kw = dict(loss_kind=loss_kind, use_valid=use_valid)
    for alpha in (1.0, 0.5):
        for det in (1, 0):
            got = _cql(inputs, alpha, weight=None if w is None else w.to(DEV), deterministic=det, q_copy=True, **kw)
            _check_against_oracle(cpu, alpha, got, weight=w, **kw)
            assert torch.equal(got[2], got[3])  # the f32 dq and dq_f32 are the same values
            assert torch.equal(got[5], cpu[0][:, :15])
    bf = _cql(inputs, 1.0, dtype=_lib.VDQN_BF16, weight=None if w is None else w.to(DEV), with_err=False, **kw)
    f32 = _cql(inputs, 1.0, weight=None if w is None else w.to(DEV), with_err=False, **kw)
    assert torch.equal(bf[3], f32[3]) and torch.equal(bf[0], f32[0]) and torch.equal(bf[1], f32[1])
    assert torch.all((bf[2] - bf[3]).abs() <= bf[3].abs() * 2.0 ** -8)  # one bf16 rounding: 8 significand bits
    assert torch.equal(bf[2], bf[3].bfloat16().float())  # ... to nearest even, as every other kernel stores bf16


@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_taken_action_part_is_the_weighted_td_loss(loss_kind):
    """All four target options: dq_cql minus the penalty's own gradient alpha * (p - onehot) * s * inv (float64 closed form) is
    vdqn_td_loss_weighted's dq, and err_out is that kernel's (the same td_error_of)."""
    from test_gpu_replay import _td
    from video_dqn_amd import _lib
    B, alpha = 70, 1.0
    cpu = cql_oracle.td_inputs(B, 29)
    cpu[0] = cpu[0] * 2.5  # |d| beyond 1: both Huber branches
    inputs = _dev(cpu)
    w = _weights(B, 4)
    for use_valid in (False, True):
        for linear, clip_rect, gamma in ((0, 1, 0.9), (1, 1, 0.9), (0, 0, 0.99), (1, 0, 0.5)):
            kw = dict(linear=linear, clip_rect=clip_rect, gamma=gamma)
            ref = _td(inputs, _lib.VDQN_F32, loss_kind, use_valid, weight=w.to(DEV), **kw)
            got = _cql(inputs, alpha, loss_kind=loss_kind, use_valid=use_valid, weight=w.to(DEV), **kw)
            _check_against_oracle(cpu, alpha, got, weight=w, loss_kind=loss_kind, use_valid=use_valid, **kw)
            pen_grad = cql_oracle.closed_form(cpu, alpha, weight=w, loss_kind=loss_kind, use_valid=use_valid, **kw)["pen_grad"]
            td_part = got[3][:, :15].double() - pen_grad
            assert (td_part - ref[2][:, :15].double()).abs().max().item() <= 1e-6 * got[3].abs().max().item(), (use_valid, kw)
            assert (got[4] - ref[3]).abs().max().item() <= 1e-6 * ref[3].abs().max().item()
            # the loss is the weighted TD loss plus alpha times the penalty
            assert abs(got[0].item() - (ref[0].item() + alpha * got[1].item())) <= 1e-5 * abs(got[0].item())


def test_extreme_rows_are_finite_and_match_the_oracle():
    """Rows [1e4, -1e4, 0] (no finite exp without the max subtraction) and rows of equal Qs, every action taken once."""
    B = 6
    cpu = cql_oracle.td_inputs(B, 5)
    cpu[0][:3, :15] = torch.tensor([1e4, -1e4, 0.0]).repeat(5)
    cpu[0][3:, :15] = 0.25
    cpu[3] = torch.tensor([0, 1, 2, 0, 1, 2])
    for loss_kind in (0, 1):
        got = _cql(_dev(cpu), 1.0, loss_kind=loss_kind, use_valid=False)
        _check_against_oracle(cpu, 1.0, got, loss_kind=loss_kind, use_valid=False)
    # alone, without the 1e4-sized TD terms beside them: the equal rows' gradient is (1/3 - onehot) * inv exactly to rounding
    eq = [t[3:].contiguous() for t in cpu]
    got = _cql(_dev(eq), 2.0, use_valid=False)
    o = _check_against_oracle(eq, 2.0, got, use_valid=False)
    td = cql_oracle.objective(eq, 1e-30, use_valid=False)["dq"]  # (the TD part alone)
    want = torch.full((3, 5, 3), 1 / 3, dtype=torch.float64)
    want[torch.arange(3), :, eq[3]] -= 1.0
    assert ((o["dq"] - td).reshape(3, 5, 3) * 15 / 2.0 - want).abs().max().item() < 1e-7
    assert abs(got[1].item() - math.log(3.0)) <= 1e-6 * math.log(3.0)


def test_deterministic_is_bit_identical_and_agrees_with_the_atomic_sum():
    cpu = cql_oracle.td_inputs(96, 41)
    inputs = _dev(cpu)
    w = _weights(96).to(DEV)
    runs = [_cql(inputs, 1.0, weight=w, loss_kind=1, deterministic=1) for _ in range(2)]
    for x, y in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(x, y)
    free = _cql(inputs, 1.0, weight=w, loss_kind=1, deterministic=0)
    assert abs(free[0].item() - runs[0][0].item()) <= 1e-5 * abs(runs[0][0].item())
    assert abs(free[1].item() - runs[0][1].item()) <= 1e-5 * abs(runs[0][1].item())
    assert torch.equal(free[3], runs[0][3]) and torch.equal(free[4], runs[0][4])


def test_ops_td_loss_cql_and_null_outputs():
    """ops.td_loss_cql mirrors ops.td_loss; weight, err_out and penalty may each be NULL."""
    from video_dqn_amd import _lib, ops
    cpu = cql_oracle.td_inputs(5, 2)
    inputs = _dev(cpu)
    loss, dq, dq32, pen, err = ops.td_loss_cql(*inputs[:6], inputs[6], cql_alpha=1.5, gamma=0.9, with_err=True, deterministic=True)
    raw = _cql(inputs, 1.5)
    assert torch.equal(loss.cpu(), raw[0]) and torch.equal(pen.cpu(), raw[1]) and torch.equal(dq32.cpu(), raw[3]) and torch.equal(err.cpu(), raw[4])
    assert torch.equal(dq.cpu(), raw[3])
    loss2, _, dq32_2, _, err2 = ops.td_loss_cql(*inputs[:6], inputs[6], cql_alpha=1.5, gamma=0.9, deterministic=True)
    assert err2 is None and torch.equal(loss2, loss) and torch.equal(dq32_2, dq32)
    with pytest.raises(_lib.VdqnError, match="cql_alpha"):
        ops.td_loss_cql(*inputs[:6], cql_alpha=0.0)


# ---- 2. the engine -----------------------------------------------------------------------------------------------------------------
def _stepper(dtype, B, deterministic=True, extra_capacity=True, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=deterministic)
    net.load_tensors(synth.make_state_dict(7, extra_capacity=extra_capacity))
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **kw)


def _batch(seed, B):
    from video_dqn_amd import synth
    (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
    before, after, act, rew, term = tup[:5]
    return (before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))


def _qf(net, stp, B):
    """The engine's own f32 Q rows [.][64]: Q(s), the online Q(s') and the target network's Q(s')."""
    off = net.lib.vdqn_net_act_offset(net.handle, stp.layout_samples, b"qf")
    off_t = net.lib.vdqn_net_act_offset(net.handle, B, b"qf")
    assert off >= 0 and off_t >= 0
    q = stp.acts_online[off:off + 2 * B * 64 * 4].view(torch.float32).view(2 * B, 64)
    qt = stp.acts_target[off_t:off_t + B * 64 * 4].view(torch.float32).view(B, 64)
    return q[:B], q[B:], qt


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stepper_alpha_zero_is_the_stepper_without_the_argument(dtype):
    B = 8
    runs = []
    for kw in (dict(), dict(cql_alpha=0.0)):
        net, stp = _stepper(dtype, B, **kw)
        losses = []
        for s in (1, 2):
            losses.append(stp.step(*_batch(300 + s, B)).clone())
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), torch.cat(losses).cpu(), stp.grads.cpu(), stp.exp_avg_sq.cpu()))
        assert stp.cql_penalty.item() == 0.0
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_stepper_validation():
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, True, "f32", 8)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.VdqnError, match="cql_alpha"):
            TDStepper(net, 4, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=bad)
    with pytest.raises(_lib.VdqnError, match="cql_alpha.*train_on_ground_truth"):
        TDStepper(net, 4, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=1.0, train_on_ground_truth=True)
    one = NetEngine(1, 5, 1, True, "f32", 8)
    with pytest.raises(_lib.VdqnError, match="cql_alpha.*action_dim"):
        TDStepper(one, 4, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=1.0)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_td_forward_cql_writes_the_operators_dq(weighted):
    """After vdqn_net_td_forward_cql (alpha = 1) the dq tensor of the backward workspace, the loss and the penalty are
    ops.td_loss_cql on the engine's own Q rows, bit for bit."""
    from video_dqn_amd import _lib, ops
    B = 8
    net, stp = _stepper("f32", B, cql_alpha=1.0)
    before, after, kind, act, rew, term = _batch(101, B)
    w = _weights(B, 12).to(DEV) if weighted else None
    err = torch.zeros(B, device=DEV) if weighted else None
    a = stp._args(before, after, kind, act, rew, term, stp._ones, None, w, err)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(net.lib.vdqn_net_td_forward_cql(net.handle, C.byref(a), 1.0, stp.cql_penalty.data_ptr(), st), "vdqn_net_td_forward_cql")
    torch.cuda.synchronize()
    off = net.lib.vdqn_net_bwd_offset(net.handle, B, b"dq")
    assert off >= 0
    dq = stp.bwd[off:off + B * 64 * 4].view(torch.float32).view(B, 64).clone()
    qb, qo, qt = _qf(net, stp, B)
    loss, _, dq32, pen, e = ops.td_loss_cql(qb, qo, qt, act, rew, term, None, cql_alpha=1.0, weights=w, with_err=weighted, gamma=0.99,
                                            clip_rect=True, deterministic=True)
    assert torch.equal(dq, dq32) and torch.equal(stp.loss, loss) and torch.equal(stp.cql_penalty, pen)
    assert (dq[:, :15] != 0).all() and torch.all(dq[:, 15:] == 0)  # dense over the actions
    assert torch.equal(stp.q_before, qb[:, :15])
    if weighted:
        assert torch.equal(err, e)
    # alpha 0 through the same entry: vdqn_net_td_forward's one-hot dq and loss, and the penalty buffer left alone
    stp.cql_penalty.fill_(5.0)
    _lib.check(net.lib.vdqn_net_td_forward_cql(net.handle, C.byref(a), 0.0, stp.cql_penalty.data_ptr(), st), "vdqn_net_td_forward_cql")
    torch.cuda.synchronize()
    dq0, loss0 = stp.bwd[off:off + B * 64 * 4].view(torch.float32).view(B, 64).clone(), stp.loss.clone()
    _lib.check(net.lib.vdqn_net_td_forward(net.handle, C.byref(a), st), "vdqn_net_td_forward")
    torch.cuda.synchronize()
    assert torch.equal(dq0, stp.bwd[off:off + B * 64 * 4].view(torch.float32).view(B, 64)) and torch.equal(loss0, stp.loss)
    assert (dq0[:, :15] != 0).sum().item() <= 5 * B and stp.cql_penalty.item() == 5.0


def test_cql_step_gradient_matches_f64_oracle():
    """One update with alpha = 1 and random importance weights, f32 engine at B = 8: every gradient tensor against the float64
    oracle that takes the engine's ReLU decisions — the recipe and the gate of
    tests/test_gpu_replay.py::test_weighted_step_gradient_matches_f64_oracle (relative L2 <= 1e-3, max element <= 5e-3 of the
    tensor's max, more than 60 tensors).  The oracle has neither weights nor a penalty: the test forms the objective itself from
    its per-sample TD losses, its Q(s) and the taken action's Q."""
    from oracle import ref_cpu
    from test_gpu_engine import _EngineReLU, _engine_relu_masks, make_engine
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B, alpha = 8, 1.0
    net = make_engine("f32", seed=7, max_batch=2 * B)
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_alpha=alpha)
    make_engine("f32", seed=8, max_batch=2 * B).pack_weights(stp.packed_target)  # a target network of its own
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05
    err = torch.zeros(B, device=DEV)
    loss = stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV),
                    tup[4].float().to(DEV), weights=w.to(DEV), td_error=err)
    torch.cuda.synchronize()
    grads = stp.grads.cpu()
    masks = _engine_relu_masks(net, stp.acts_online, stp.layout_samples, B)
    tr = ref_cpu.Trainer(ref_cpu.default_config(), synth.make_state_dict(7))
    tr.target_net.load_state_dict(synth.make_state_dict(8))
    tr.model.double()
    tr.target_net.double()
    for b in range(8):
        getattr(tr.model.resnet, f"layer{b // 2 + 1}")[b % 2].relu = _EngineReLU(masks[b])
    tr.model.set_train()
    d = {}
    ref_cpu.process_batch(tr.model, tr.target_net, tr.config, (tup[0].double(), tup[1].double()) + tuple(tup[2:]), detail=d)
    wd = w.double().view(B, 1)
    pen = torch.logsumexp(d["before_values"], 2) - d["Q_b"]
    objective = (d["losses"] * wd).mean() + alpha * (pen * wd).mean()
    objective.backward()
    # (the f32 engine's Q(s) against float64: smoke() gates it at 1e-3 relative, and both sums are smooth in Q)
    print(f"objective {loss.item():.6f} / {objective.item():.6f}, penalty {stp.cql_penalty.item():.6f} / {(pen * wd).mean().item():.6f}")
    assert abs(loss.item() - objective.item()) <= 1e-3 * abs(objective.item())
    assert abs(stp.cql_penalty.item() - (pen * wd).mean().item()) <= 1e-3 * (pen * wd).mean().item()
    d_ref = (d["Q_b"] - d["learn_targets"]).detach().abs().mean(1)
    assert (err.cpu().double() - d_ref).abs().max().item() <= 1e-4 * d_ref.abs().max().item()
    bad, n = [], 0
    for name, p in tr.model.named_parameters():
        if p.grad is None:
            continue
        s = net.slots[name]
        ge, r = grads[s.offset:s.offset + s.numel].view(s.shape).double(), p.grad.double()
        l2 = ((ge - r).norm() / r.norm().clamp_min(1e-300)).item()
        mx = ((ge - r).abs().max() / r.abs().max().clamp_min(1e-300)).item()
        n += 1
        if l2 > 1e-3 or mx > 5e-3:
            bad.append((name, l2, mx))
    assert n > 60 and not bad, bad


@pytest.mark.parametrize("dtype,extra_capacity", [("f32", False), ("bf16x3", True), ("bf16", True)], ids=["basic", "bf16x3", "bf16"])
def test_other_architecture_and_compute_modes(dtype, extra_capacity):
    """ARCHITECTURE='basic' and the bf16x3 / bf16 compute modes: one finite update whose loss and penalty are the operator's on the
    engine's own Q rows (the loss launch runs behind the forward pass and knows nothing of them)."""
    from video_dqn_amd import ops
    B = 8
    net, stp = _stepper(dtype, B, extra_capacity=extra_capacity, cql_alpha=1.0)
    p0 = net.params.clone()
    batch = _batch(301, B)
    loss = stp.step(*batch)
    torch.cuda.synchronize()
    qb, qo, qt = _qf(net, stp, B)
    ref = ops.td_loss_cql(qb, qo, qt, batch[3], batch[4], batch[5], None, cql_alpha=1.0, gamma=0.99, clip_rect=True, deterministic=True)
    assert torch.equal(stp.cql_penalty, ref[3]) and torch.equal(loss, ref[0])
    assert torch.isfinite(net.params).all() and torch.isfinite(stp.grads).all() and not torch.equal(net.params, p0)
    spread = (qb[:, :15].view(B, 5, 3).max(2).values - qb[:, :15].view(B, 5, 3).min(2).values).max().item()
    assert 0 < stp.cql_penalty.item() <= math.log(3.0) + spread


def test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit():
    """Nothing of the penalty lives in a checkpoint: six updates in one go against three updates, the trainer's model and optimiser
    state dicts into a fresh stepper built with the same cql_alpha, three more — parameters and moments bit-identical."""
    from video_dqn_amd.trainer import load_optimizer_state_dict, optimizer_state_dict
    B = 4
    net_u, stp_u = _stepper("f32", B, cql_alpha=1.0)
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    net_i, stp_i = _stepper("f32", B, cql_alpha=1.0)
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    sd = optimizer_state_dict(stp_i)
    assert list(sd["param_groups"][0]) == ["lr", "betas", "eps", "weight_decay", "amsgrad", "params"]
    net_r, stp_r = _stepper("f32", B, cql_alpha=1.0)
    net_r.params.copy_(net_i.params)
    net_r.mark_dirty()
    load_optimizer_state_dict(stp_r, sd)
    stp_r.sample_number = 3
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", net_u.params, net_r.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq), ("penalty", stp_u.cql_penalty, stp_r.cql_penalty)):
        assert torch.equal(x, y), name
    net_0, stp_0 = _stepper("f32", B)
    for t in range(1, 7):
        stp_0.step(*_batch(300 + t, B))
    assert not torch.equal(net_0.params, net_u.params)  # (the penalty did move the parameters)


# ---- 3. run_train ------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def test_run_train_with_cql_alpha(tmp_path):
    """100 updates with CQL_ALPHA 1 and a scalar writer (scalars are written every 100 updates): `cql_penalty/train` is written at
    update 100 with the penalty of update 99 (read one update late, like the loss), positive and at most log(3) plus the largest
    spread of Q(s) over the actions; the checkpoint has the reference's three keys and nothing else; two runs resumed from it end
    bit-identical.  (run_train's resume keeps the reference's numbering — it goes on at resume_from + 2 and reads the epoch from
    its start, tests/test_gpu_augment.py — so no resumed run_train equals an uninterrupted one, whatever the loss;
    test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit above has that comparison.)"""
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd.config import ExperimentConfig, JsonlWriter
    from video_dqn_amd.trainer import run_train
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    _write_cfg(tmp_path / "a", shards, 100, "CQL_ALPHA: 1.0\n")
    cfg = ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=True)
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    logs = []
    model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
    cfg.writer.close()
    assert np.isfinite(running) and stepper.cql_alpha == 1.0
    assert any(l.startswith("conservative Q-learning: 1 * (logsumexp") for l in logs)
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    pen = [r for r in rows if r["tag"] == "cql_penalty/train"]
    assert len(pen) == 1 and pen[0]["step"] == 99
    q = stepper.q_before.view(4, 5, 3)
    spread = (q.max(2).values - q.min(2).values).max().item()
    print(f"cql_penalty/train at update 99: {pen[0]['value']:.4f}; the last update's: {stepper.cql_penalty.item():.4f}; Q spread {spread:.4f}")
    assert 0 < pen[0]["value"] <= math.log(3.0) + spread
    assert any(r["tag"] == "avg_q_loss/train" and r["step"] == 100 for r in rows)
    snap = torch.load(tmp_path / "a" / "models" / "sample96.torch", map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict"}
    finals = []
    for tag in ("r1", "r2"):
        _write_cfg(tmp_path / tag, shards, 100, "CQL_ALPHA: 1.0\n")
        (tmp_path / tag / "models").mkdir()
        torch.save(snap, tmp_path / tag / "models" / "sample96.torch")
        m, s, _ = run_train(ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False, resume=True), resume_from=96,
                            log=lambda *a: None)
        assert s.adam_step == 99 and s.cql_alpha == 1.0
        finals.append((m.engine.params.cpu(), s.exp_avg_sq.cpu(), s.cql_penalty.cpu()))
    for x, y in zip(*finals):
        assert torch.equal(x, y)
    # the same resume without the penalty goes elsewhere, and logs nothing about it
    _write_cfg(tmp_path / "off", shards, 100)
    (tmp_path / "off" / "models").mkdir()
    torch.save(snap, tmp_path / "off" / "models" / "sample96.torch")
    logs = []
    m, s, _ = run_train(ExperimentConfig(str(tmp_path / "off"), device=DEV, tensorboard=False, resume=True), resume_from=96,
                        log=lambda *a: logs.append(" ".join(map(str, a))))
    assert s.cql_alpha == 0.0 and not any("conservative" in l for l in logs) and not torch.equal(m.engine.params.cpu(), finals[0][0])


# ---- 4. data parallelism: two ranks on one GPU over gloo (the harness of tests/test_gpu_ddp.py) -------------------------------------
def _dp_run(B, world, lo, hi, hook=None, finish=None):
    net, stp = _stepper("f32", B, world_size=world, allreduce=hook, cql_alpha=1.0)
    pens = []
    for step in (1, 2):
        full = _batch(200 + step, 8)
        stp.step(*[t[lo:hi].contiguous() if torch.is_tensor(t) else t for t in full], finish_allreduce=finish)
        torch.cuda.synchronize()
        pens.append(stp.cql_penalty.cpu().clone())
    return net.params.cpu(), torch.cat(pens), stp.loss.cpu()


def _dp_worker(rank, world, port, out_dir, B):
    import sys
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)

    def through_host(t, stage=None):  # test transport (as test_gpu_ddp.py): whatever gloo's GPU support is
        torch.cuda.synchronize()
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)

    params, pens, loss = _dp_run(B, world, rank * B, (rank + 1) * B, through_host)
    torch.save({"params": params, "pens": pens, "loss": loss}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process_on_the_big_batch(tmp_path):
    """Two ranks x B = 4 on one GPU (gloo) against one process at B = 8, two updates with alpha = 1: the replicas hold bit-identical
    parameters and meet tests/test_gpu_ddp.py's bound against the big batch; each rank's penalty is its share of the global mean
    (the kernel divides by the global batch), so the shares sum to the one-process penalty."""
    import torch.multiprocessing as mp
    from test_gpu_ddp import _free_port
    B, world = 4, 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), B), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    assert torch.equal(ranks[0]["params"], ranks[1]["params"])
    params, pens, loss = _dp_run(B * world, 1, 0, B * world)
    from video_dqn_amd.engine import NetEngine
    nt = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True).trainable_numel
    delta = (params[:nt] - ranks[0]["params"][:nt]).abs()
    print(f"two ranks against one process: max {delta.max().item():.2e}, mean {delta.mean().item():.2e}")
    assert delta.max().item() <= 2.5e-4 and delta.mean().item() < 2e-6
    share = ranks[0]["pens"] + ranks[1]["pens"]
    print(f"penalty shares {ranks[0]['pens'].tolist()} + {ranks[1]['pens'].tolist()} against {pens.tolist()}")
    # update 1: the same parameters, so only the order of an f32 sum of 40 terms differs; update 2 runs on parameters that differ
    # by the summation order of update 1's gradient (tests/test_gpu_replay.py bounds the TD errors of that situation by 1e-4)
    assert abs(share[0].item() - pens[0].item()) <= 1e-5 * pens[0].item()
    assert abs(share[1].item() - pens[1].item()) <= 1e-4 * pens[1].item()
    assert abs((ranks[0]["loss"] + ranks[1]["loss"]).item() - loss.item()) <= 1e-4 * abs(loss.item())
