"""Implicit Q-learning on the GPU: vdqn_td_loss_iql against the float64 autograd oracle (tests/iql_oracle.py) and against
vdqn_td_loss_weighted, its deterministic mode, half batches, vdqn_net_td_forward_iql against the operator and the float64 network
oracle, both architectures and the compute modes, resume, and run_train with IQL_EXPECTILE."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import iql_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _iql(inputs, tau, dtype=None, loss_kind=0, use_valid=True, weight=None, with_err=True, clip_rect=1, gamma=0.9, deterministic=1,
         n_cat=5, n_act=3, q_copy=False, discount=None, inv_count=None, with_stats=True):
    """vdqn_td_loss_iql through the raw ABI -> (loss, stats, dq as f32, dq_f32, err, q_copy), all on the CPU."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    dtype = _lib.VDQN_F32 if dtype is None else dtype
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    loss, stats = torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    dq = torch.full((B, ldq), 7.0, dtype=torch.bfloat16 if dtype == _lib.VDQN_BF16 else torch.float32, device=DEV)
    dq32 = torch.full((B, ldq), 7.0, device=DEV)
    err = torch.full((B,), -1.0, device=DEV) if with_err else None
    qc = torch.full((B, n_cat * n_act), -7.0, device=DEV) if q_copy else None
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = qb.data_ptr(), qo.data_ptr(), qt.data_ptr()
    a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
    a.loss, a.dq, a.dq_f32 = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr()
    a.batch, a.n_cat, a.n_act, a.ldq = B, n_cat, n_act, ldq
    a.gamma, a.inv_count = gamma, (1.0 / (n_cat * B) if inv_count is None else inv_count)
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, 0, int(use_valid), dtype, loss_kind, deterministic
    a.q_copy = qc.data_ptr() if q_copy else None
    _lib.check(lib.vdqn_td_loss_iql(C.byref(a), weight.data_ptr() if weight is not None else None, err.data_ptr() if with_err else None,
                                    discount.data_ptr() if discount is not None else None, tau, stats.data_ptr() if with_stats else None,
                                    torch.cuda.current_stream().cuda_stream), "vdqn_td_loss_iql")
    torch.cuda.synchronize()
    return loss.cpu(), stats.cpu(), dq.float().cpu(), dq32.cpu(), (err.cpu() if with_err else None), (qc.cpu() if q_copy else None)


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _discount(B, seed=6):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.45


def _rel(x, want):
    return abs(x - want) / max(abs(want), 1e-30)


def _check_against_oracle(inputs, tau, got, n_cat=5, n_act=3, **kw):
    """The project's operator gate (tests/test_gpu_cql.py): dq within 1e-6 of the maximum element, every column other than the n_cat
    taken-action columns and the n_cat value columns exactly 0, loss and both stats within 1e-5 relative, err within 1e-6."""
    loss, stats, _, dq32, err, _ = got
    n = n_cat * n_act
    o = iql_oracle.objective(inputs, tau, n_cat=n_cat, n_act=n_act, **kw)
    dq_max = o["dq"].abs().max().item()
    e_dq = (dq32[:, :n + n_cat].double() - o["dq"]).abs().max().item() / dq_max
    e_loss, e_v, e_adv = _rel(loss.item(), o["loss"].item()), _rel(stats[0].item(), o["v_loss"].item()), _rel(stats[1].item(), o["advantage"].item())
    print(f"dq {e_dq:.2e} of the max element, loss {e_loss:.2e}, v_loss {e_v:.2e}, advantage {e_adv:.2e} relative")
    assert torch.isfinite(dq32).all() and math.isfinite(loss.item()) and torch.isfinite(stats).all()
    assert e_dq <= 1e-6
    B = dq32.shape[0]
    live = torch.zeros_like(dq32, dtype=torch.bool)
    live[:, n:n + n_cat] = True
    live[torch.arange(B).repeat_interleave(n_cat), torch.arange(n_cat).repeat(B) * n_act + inputs[3].repeat_interleave(n_cat)] = True
    assert torch.all(dq32[~live] == 0)
    assert e_loss <= 1e-5 and e_v <= 1e-5 and e_adv <= 1e-5
    if err is not None:
        e_err = (err.double() - o["err"]).abs().max().item() / max(o["err"].abs().max().item(), 1e-30)
        print(f"err {e_err:.2e}")
        assert e_err <= 1e-6
    return o


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq,n_cat,n_act", iql_oracle.OPERATOR_SHAPES, ids=["B96", "B1", "B3", "ldq20", "C2A2"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_td_loss_iql_vs_f64_oracle(loss_kind, use_valid, weighted, B, ldq, n_cat, n_act):
    """Scalar and per-sample discount, three expectiles, both deterministic settings; bf16 dq is dq_f32 rounded once."""
    from video_dqn_amd import _lib
    cpu = iql_oracle.inputs(B, 11 + loss_kind + 2 * use_valid, ldq=ldq, n_cat=n_cat, n_act=n_act)
    assert iql_oracle.min_abs_u(cpu, n_cat, n_act) >= iql_oracle.MIN_ABS_U
    if use_valid:
        cpu[6][0, 0] = 1.0  # (B = 1: at least one valid term, so the relative gates have something to divide by)
    w = _weights(B) if weighted else None
    wd = None if w is None else w.to(DEV)
    inputs = _dev(cpu)
    kw = dict(loss_kind=loss_kind, use_valid=use_valid)
    shape = dict(n_cat=n_cat, n_act=n_act)
    for disc in (None, _discount(B)):
        dd = None if disc is None else disc.to(DEV)
        for tau in (0.7, 0.5, 0.9):
            for det in (1, 0):
                got = _iql(inputs, tau, weight=wd, deterministic=det, q_copy=True, discount=dd, **kw, **shape)
                _check_against_oracle(cpu, tau, got, weight=w, discount=disc, **kw, **shape)
                assert torch.equal(got[2], got[3])  # the f32 dq and dq_f32 are the same values
                assert torch.equal(got[5], cpu[0][:, :n_cat * n_act])
    bf = _iql(inputs, 0.7, dtype=_lib.VDQN_BF16, weight=wd, with_err=False, **kw, **shape)
    f32 = _iql(inputs, 0.7, weight=wd, with_err=False, **kw, **shape)
    assert torch.equal(bf[3], f32[3]) and torch.equal(bf[0], f32[0]) and torch.equal(bf[1], f32[1])
    assert torch.equal(bf[2], bf[3].bfloat16().float())  # one rounding to nearest even, as every other kernel stores bf16


def test_ops_td_loss_iql_and_null_outputs():
    """ops.td_loss_iql mirrors the raw entry; weight, err_out, sample_gamma, stats, q_copy and dq_f32's twin may each be NULL."""
    from video_dqn_amd import _lib, ops
    B, ldq, n_cat, n_act, seed = iql_oracle.OPS_CASE
    cpu = iql_oracle.inputs(B, seed)
    inputs = _dev(cpu)
    loss, dq, dq32, stats, err = ops.td_loss_iql(*inputs[:6], inputs[6], expectile=0.7, gamma=0.9, with_err=True, deterministic=True)
    raw = _iql(inputs, 0.7)
    assert torch.equal(loss.cpu(), raw[0]) and torch.equal(stats.cpu(), raw[1]) and torch.equal(dq32.cpu(), raw[3]) and torch.equal(err.cpu(), raw[4])
    assert torch.equal(dq.cpu(), raw[3])
    loss2, _, dq32_2, stats2, err2 = ops.td_loss_iql(*inputs[:6], inputs[6], expectile=0.7, gamma=0.9, deterministic=True, with_stats=False)
    assert err2 is None and stats2 is None and torch.equal(loss2, loss) and torch.equal(dq32_2, dq32)
    for bad in (0.0, 0.3, 1.0):
        with pytest.raises(_lib.VdqnError, match="expectile"):
            ops.td_loss_iql(*inputs[:6], expectile=bad)
    with pytest.raises(_lib.VdqnError, match="linear"):
        ops.td_loss_iql(*inputs[:6], expectile=0.7, linear=True)


# ---- 2. the Q part is the weighted TD loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_q_part_is_the_weighted_td_loss_bit_for_bit(loss_kind):
    """With a Q_target(s') row whose three actions all hold v' = V(s'), vdqn_td_loss_weighted bootstraps from v' whatever the arg-max:
    its taken-action dq columns and err are the IQL launch's, bit for bit (the same expression order for y and d)."""
    from test_gpu_replay import _td
    from video_dqn_amd import _lib
    B, ldq, n_cat, n_act, seed = iql_oracle.TWIN_CASE
    cpu = iql_oracle.inputs(B, seed)
    cpu[0][:, :15] = cpu[0][:, :15] * 2.5  # |d| beyond 1: both Huber branches
    twin = [t.clone() for t in cpu]
    twin[2][:, :15] = cpu[1][:, 15:20].repeat_interleave(3, dim=1)
    inputs, tw = _dev(cpu), _dev(twin)
    w = _weights(B, 4)
    cols = torch.arange(5).view(1, 5) * 3 + cpu[3].view(B, 1)
    for use_valid in (False, True):
        for clip_rect, gamma in ((1, 0.9), (0, 0.99), (0, 0.5), (1, 0.5)):
            kw = dict(clip_rect=clip_rect, gamma=gamma)
            ref = _td(tw, _lib.VDQN_F32, loss_kind, use_valid, weight=w.to(DEV), **kw)
            got = _iql(inputs, 0.7, loss_kind=loss_kind, use_valid=use_valid, weight=w.to(DEV), **kw)
            _check_against_oracle(cpu, 0.7, got, weight=w, loss_kind=loss_kind, use_valid=use_valid, **kw)
            assert torch.equal(got[3].gather(1, cols), ref[2].gather(1, cols)), (use_valid, kw)
            assert torch.equal(got[4], ref[3]), (use_valid, kw)
            assert torch.equal(got[3][:, :15], ref[2][:, :15])  # (and zeros elsewhere among the Q columns, in both)
            # the loss is the weighted TD loss plus the V loss
            assert abs(got[0].item() - (ref[0].item() + got[1][0].item())) <= 1e-5 * abs(got[0].item())


# ---- 3. deterministic --------------------------------------------------------------------------------------------------------------
def test_deterministic_is_bit_identical_and_agrees_with_the_atomic_sum():
    B, ldq, n_cat, n_act, seed = iql_oracle.DET_CASE
    inputs = _dev(iql_oracle.inputs(B, seed))
    w = _weights(B).to(DEV)
    runs = [_iql(inputs, 0.7, weight=w, loss_kind=1, deterministic=1) for _ in range(2)]
    for x, y in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(x, y)
    free = _iql(inputs, 0.7, weight=w, loss_kind=1, deterministic=0)
    assert _rel(free[0].item(), runs[0][0].item()) <= 1e-5
    assert _rel(free[1][0].item(), runs[0][1][0].item()) <= 1e-5 and _rel(free[1][1].item(), runs[0][1][1].item()) <= 1e-5
    assert torch.equal(free[3], runs[0][3]) and torch.equal(free[4], runs[0][4])


# ---- 4. two half batches -----------------------------------------------------------------------------------------------------------
def test_two_half_batches_at_the_global_inv_count_are_the_full_batch():
    """What two ranks compute: each half at inv_count = 1 / (n_cat * global batch) writes the full batch's dq rows bit for bit, and
    the loss and stats shares sum to the full batch's."""
    B, ldq, n_cat, n_act, seed = iql_oracle.HALVES_CASE
    cpu = iql_oracle.inputs(B, seed)
    w = _weights(B, 9)
    inv = 1.0 / (n_cat * B)
    full = _iql(_dev(cpu), 0.7, weight=w.to(DEV), inv_count=inv)
    halves = []
    for lo in (0, B // 2):
        part = [t[lo:lo + B // 2].contiguous() for t in cpu]
        halves.append(_iql(_dev(part), 0.7, weight=w[lo:lo + B // 2].contiguous().to(DEV), inv_count=inv))
    assert torch.equal(torch.cat([halves[0][3], halves[1][3]]), full[3])
    assert torch.equal(torch.cat([halves[0][4], halves[1][4]]), full[4])
    assert _rel((halves[0][0] + halves[1][0]).item(), full[0].item()) <= 1e-6
    for k in (0, 1):
        assert _rel((halves[0][1][k] + halves[1][1][k]).item(), full[1][k].item()) <= 1e-5


# ---- 5. the engine -----------------------------------------------------------------------------------------------------------------
def _value_rows(seed, in_f):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.rand(5, in_f, generator=g) * 2 - 1) * 0.04, (torch.rand(5, generator=g) * 2 - 1) * 0.04


def _net(dtype, max_batch, seed=7, extra_capacity=True, deterministic=True, value_head=True):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, extra_capacity, dtype, max_batch, deterministic=deterministic, value_head=value_head)
    net.load_tensors(synth.make_state_dict(seed, extra_capacity=extra_capacity))
    if value_head:
        vw, vb = _value_rows(seed, 256 if extra_capacity else 512)
        net.view("value.weight").copy_(vw)
        net.view("value.bias").copy_(vb)
        net.mark_dirty()
    return net


def _stepper(dtype, B, deterministic=True, extra_capacity=True, value_head=True, **kw):
    from video_dqn_amd.engine import TDStepper
    net = _net(dtype, 2 * B, extra_capacity=extra_capacity, deterministic=deterministic, value_head=value_head)
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **kw)


def _batch(seed, B):
    from video_dqn_amd import synth
    (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
    before, after, act, rew, term = tup[:5]
    return (before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))


def _qf(net, stp, B):
    """The engine's own f32 rows [.][64]: the online pass at s and s', and the target pass."""
    off = net.lib.vdqn_net_act_offset(net.handle, stp.layout_samples, b"qf")
    off_t = net.lib.vdqn_net_act_offset(net.handle, B, b"qf")
    assert off >= 0 and off_t >= 0
    q = stp.acts_online[off:off + 2 * B * 64 * 4].view(torch.float32).view(2 * B, 64)
    qt = stp.acts_target[off_t:off_t + B * 64 * 4].view(torch.float32).view(B, 64)
    return q[:B], q[B:], qt


def _dq(net, stp, B):
    off = net.lib.vdqn_net_bwd_offset(net.handle, B, b"dq")
    assert off >= 0
    return stp.bwd[off:off + B * 64 * 4].view(torch.float32).view(B, 64).clone()


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_td_forward_iql_writes_the_operators_dq_and_runs_the_target_over_s(weighted):
    from video_dqn_amd import _lib, ops
    B = 8
    net, stp = _stepper("f32", B, iql_expectile=0.7)
    target = _net("f32", 2 * B, seed=8)
    target.pack_weights(stp.packed_target)  # a target network of its own
    before, after, kind, act, rew, term = _batch(101, B)
    w = _weights(B, 12).to(DEV) if weighted else None
    err = torch.zeros(B, device=DEV) if weighted else None
    a = stp._args(before, after, kind, act, rew, term, stp._ones, None, w, err)
    st = torch.cuda.current_stream().cuda_stream
    stp.iql_stats.fill_(5.0)  # (cleared beside the loss)
    _lib.check(net.lib.vdqn_net_td_forward_iql(net.handle, C.byref(a), 0.7, stp.iql_stats.data_ptr(), st), "vdqn_net_td_forward_iql")
    torch.cuda.synchronize()
    dq = _dq(net, stp, B)
    qb, qo, qt = _qf(net, stp, B)
    loss, _, dq32, stats, e = ops.td_loss_iql(qb, qo, qt, act, rew, term, None, expectile=0.7, weights=w, with_err=weighted, gamma=0.99,
                                              clip_rect=True, deterministic=True)
    assert torch.equal(dq, dq32) and torch.equal(stp.loss, loss) and torch.equal(stp.iql_stats, stats)
    assert (dq[:, 15:20] != 0).all() and torch.all(dq[:, 20:] == 0) and (dq[:, :15] != 0).sum().item() <= 5 * B
    assert stats[0].item() > 0 and (qb[:, 15:20] != 0).all()
    assert torch.equal(stp.q_before, qb[:, :15])
    if weighted:
        assert torch.equal(err, e)
    # the target workspace holds the target network at s (`before`), not at s'
    q_s = target.forward(before, kind, B)
    v_s = target.state_values(B)
    q_after = target.forward(after, kind, B)
    torch.cuda.synchronize()
    assert torch.equal(qt[:, :15], q_s) and torch.equal(qt[:, 15:20], v_s) and not torch.equal(qt[:, :15], q_after)
    # the Double-DQN entry on the same value-head net: zeros in the V columns and the parent's loss (the target pass over s' again)
    _lib.check(net.lib.vdqn_net_td_forward(net.handle, C.byref(a), st), "vdqn_net_td_forward")
    torch.cuda.synchronize()
    dq0 = _dq(net, stp, B)
    qb0, qo0, qt0 = _qf(net, stp, B)
    assert torch.equal(qt0[:, :15], q_after) and torch.equal(qb0, qb)
    # (the engine is deterministic, and ops.td_loss has no such switch: the per-sample-discount entry at a constant 0.99 launches the
    # plain / weighted instance's twin, which writes its bits)
    ref = ops.td_loss_nstep(qb0, qo0, qt0, act, rew, term, None, discount=torch.full((B,), 0.99, device=DEV), weights=w, with_err=weighted,
                            clip_rect=True, deterministic=True)
    assert torch.all(dq0[:, 15:] == 0) and torch.equal(dq0, ref[2]) and torch.equal(stp.loss, ref[0])


def test_model_forward_keeps_its_shape_and_state_values_match_the_oracle():
    """HabitatDQNMultiAction(value_head=True): forward still returns [B, 5, 3], state_values [B, 5] from the same forward; both against
    the reference class with four action columns (the gate of tests/test_gpu_engine.py::test_forward_matches_oracle, 1e-3)."""
    from oracle import ref_cpu
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    B = 3
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=8, value_head=True)
    model.load_state_dict(synth.make_state_dict(7))  # (no value.*: the initialised head stays)
    vw, vb = _value_rows(7, 256)
    with torch.no_grad():
        model.value.weight.copy_(vw)
        model.value.bias.copy_(vb)
    model.engine.mark_dirty()
    model.eval()
    (tup, _) = synth.make_batch(24, B, 1, structured=True)
    with torch.no_grad():
        q = model(tup[0].to(DEV))
    v = model.state_values(tup[0].to(DEV))
    assert tuple(q.shape) == (B, 5, 3) and tuple(v.shape) == (B, 5)
    oracle = ref_cpu.HabitatDQNMultiAction(4, 5, extra_capacity=True, panorama=False)
    oracle.load_state_dict(_oracle_state_dict(7))
    oracle.eval()
    with torch.no_grad():
        ref = oracle(tup[0])
    e_q = ((q.cpu() - ref[:, :, :3]).abs().max() / ref[:, :, :3].abs().max()).item()
    e_v = ((v.cpu() - ref[:, :, 3]).abs().max() / ref[:, :, 3].abs().max()).item()
    print(f"Q {e_q:.2e}, V {e_v:.2e} of the maximum")
    assert e_q < 1e-3 and e_v < 1e-3
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=8)
    with pytest.raises(RuntimeError, match="value_head"):
        plain.state_values(tup[0].to(DEV))


def test_stepper_validation():
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine, TDStepper
    valued = NetEngine(3, 5, 1, True, "f32", 8, value_head=True)
    plain = NetEngine(3, 5, 1, True, "f32", 8)
    kw = dict(lr=1e-4, gamma=0.99, clip_rect=True)
    for bad in (-0.7, 0.3, 1.0, float("nan")):
        with pytest.raises(_lib.VdqnError, match="iql_expectile"):
            TDStepper(valued, 4, iql_expectile=bad, **kw)
    with pytest.raises(_lib.VdqnError, match="iql_expectile.*value head"):
        TDStepper(plain, 4, iql_expectile=0.7, **kw)
    for more in (dict(train_on_ground_truth=True), dict(linear=True), dict(cql_alpha=1.0), dict(mc_floor=True)):
        with pytest.raises(_lib.VdqnError, match="iql_expectile"):
            TDStepper(valued, 4, iql_expectile=0.7, **kw, **more)
    with pytest.raises(_lib.VdqnError, match="value_head"):
        NetEngine(1, 5, 1, True, "f32", 8, value_head=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stepper_expectile_zero_is_the_stepper_without_the_argument(dtype):
    """With the key at its default nothing changes: the same entries, launches and bits on a network without the value head."""
    B = 8
    runs = []
    for kw in (dict(), dict(iql_expectile=0.0)):
        net, stp = _stepper(dtype, B, value_head=False, **kw)
        losses = []
        for s in (1, 2):
            losses.append(stp.step(*_batch(300 + s, B)).clone())
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), torch.cat(losses).cpu(), stp.grads.cpu(), stp.exp_avg_sq.cpu()))
        assert stp.iql_stats.abs().sum().item() == 0.0
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ---- 6. one update against the float64 network oracle --------------------------------------------------------------------------------
def _oracle_state_dict(seed):
    """synth's state_dict for the reference class with FOUR action columns: oracle row c * 4 + a is the engine's Q row c * 3 + a,
    oracle row c * 4 + 3 the engine's value row 15 + c."""
    from video_dqn_amd import synth
    sd = synth.make_state_dict(seed)
    vw, vb = _value_rows(seed, 256)
    w4, b4 = torch.zeros(20, 256), torch.zeros(20)
    for c in range(5):
        w4[c * 4:c * 4 + 3], b4[c * 4:c * 4 + 3] = sd["top.4.weight"][c * 3:c * 3 + 3], sd["top.4.bias"][c * 3:c * 3 + 3]
        w4[c * 4 + 3], b4[c * 4 + 3] = vw[c], vb[c]
    sd["top.4.weight"], sd["top.4.bias"] = w4, b4
    return sd


def test_iql_step_gradient_matches_f64_oracle():
    """One update with tau = 0.7 and random importance weights, f32 engine at B = 8: every gradient tensor against the float64
    oracle that takes the engine's ReLU decisions — the recipe and the gates of
    tests/test_gpu_cql.py::test_cql_step_gradient_matches_f64_oracle (objective within 1e-3 relative; relative L2 <= 1e-3 and max
    element <= 5e-3 of the tensor's max; more than 60 tensors, value.* among them).  The oracle is the reference class with four
    action columns (the fourth is V); the objective is formed here from its outputs."""
    from oracle import ref_cpu
    from test_gpu_engine import _EngineReLU, _engine_relu_masks
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B, tau, gamma = 8, 0.7, 0.99
    net = _net("f32", 2 * B, seed=7)
    stp = TDStepper(net, B, lr=1e-4, gamma=gamma, clip_rect=True, iql_expectile=tau)
    _net("f32", 2 * B, seed=8).pack_weights(stp.packed_target)  # a target network of its own
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05
    err = torch.zeros(B, device=DEV)
    loss = stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV),
                    tup[4].float().to(DEV), weights=w.to(DEV), td_error=err)
    torch.cuda.synchronize()
    grads = stp.grads.cpu()
    masks = _engine_relu_masks(net, stp.acts_online, stp.layout_samples, B)
    model = ref_cpu.HabitatDQNMultiAction(4, 5, extra_capacity=True, panorama=False)
    model.load_state_dict(_oracle_state_dict(7))
    target = ref_cpu.HabitatDQNMultiAction(4, 5, extra_capacity=True, panorama=False)
    target.load_state_dict(_oracle_state_dict(8))
    model.double()
    target.double()
    target.eval()
    for b in range(8):
        getattr(model.resnet, f"layer{b // 2 + 1}")[b % 2].relu = _EngineReLU(masks[b])
    model.set_train()
    act, rew, term = tup[2], tup[3].double(), tup[4].double()
    out_s = model(tup[0].double())  # (the pass gradients flow through: it meets the engine's ReLU decisions)
    with torch.no_grad():
        v_next = model(tup[1].double())[:, :, 3]
        q_t = target(tup[0].double())[:, :, :3]
    idx = act.view(B, 1, 1).expand(B, 5, 1)
    q_s, v = out_s[:, :, :3].gather(2, idx).squeeze(2), out_s[:, :, 3]
    u = q_t.gather(2, idx).squeeze(2) - v
    l_v = torch.where(u > 0, torch.full_like(u, tau), torch.full_like(u, 1 - tau)) * u ** 2
    y = (rew + gamma * ((1 - term) * v_next)).clamp(0, 1)
    d = q_s - y
    wd = w.double().view(B, 1)
    objective = ((0.5 * d ** 2 + l_v) * wd).mean()
    objective.backward()
    v_loss, adv = (l_v * wd).mean().item(), u.mean().item()
    print(f"objective {loss.item():.6f} / {objective.item():.6f}, v_loss {stp.iql_stats[0].item():.6f} / {v_loss:.6f}, "
          f"advantage {stp.iql_stats[1].item():.6f} / {adv:.6f}, min |u| {u.abs().min().item():.2e}")
    assert u.abs().min().item() >= 1e-4  # (no term on the kink: the f32 engine and the oracle weigh every term alike)
    assert abs(loss.item() - objective.item()) <= 1e-3 * abs(objective.item())
    assert abs(stp.iql_stats[0].item() - v_loss) <= 1e-3 * v_loss
    d_ref = d.detach().abs().mean(1)
    assert (err.cpu().double() - d_ref).abs().max().item() <= 1e-4 * d_ref.abs().max().item()
    bad, names = [], []

    def compare(name, ge, r):
        l2 = ((ge - r).norm() / r.norm().clamp_min(1e-300)).item()
        mx = ((ge - r).abs().max() / r.abs().max().clamp_min(1e-300)).item()
        names.append(name)
        if l2 > 1e-3 or mx > 5e-3:
            bad.append((name, l2, mx))

    def engine_grad(name):
        s = net.slots[name]
        return grads[s.offset:s.offset + s.numel].view(s.shape).double()

    q_rows = torch.tensor([c * 4 + a for c in range(5) for a in range(3)])
    v_rows = torch.tensor([c * 4 + 3 for c in range(5)])
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        if name.startswith("top.4."):
            kind = name.rsplit(".", 1)[1]
            compare(name, engine_grad(name), p.grad.double()[q_rows])
            compare("value." + kind, engine_grad("value." + kind), p.grad.double()[v_rows])
        else:
            compare(name, engine_grad(name), p.grad.double())
    assert len(names) > 60 and "value.weight" in names and "value.bias" in names and not bad, bad


# ---- 7. the other architecture and the compute modes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,extra_capacity", [("f32", False), ("bf16x3", True), ("bf16", True)], ids=["basic", "bf16x3", "bf16"])
def test_other_architecture_and_compute_modes(dtype, extra_capacity):
    """One finite update each: loss and stats are the operator's on the engine's own rows, and value.weight moved."""
    from video_dqn_amd import ops
    B = 8
    net, stp = _stepper(dtype, B, extra_capacity=extra_capacity, iql_expectile=0.7)
    p0, v0 = net.params.clone(), net.view("value.weight").clone()
    batch = _batch(301, B)
    loss = stp.step(*batch)
    torch.cuda.synchronize()
    qb, qo, qt = _qf(net, stp, B)
    ref = ops.td_loss_iql(qb, qo, qt, batch[3], batch[4], batch[5], None, expectile=0.7, gamma=0.99, clip_rect=True, deterministic=True)
    assert torch.equal(loss, ref[0]) and torch.equal(stp.iql_stats, ref[3])
    assert torch.isfinite(net.params).all() and torch.isfinite(stp.grads).all() and not torch.equal(net.params, p0)
    assert not torch.equal(net.view("value.weight"), v0) and stp.iql_stats[0].item() > 0


# ---- 8. resume -----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit():
    """Six updates in one go against three updates, the trainer's dicts and `value_head` into a fresh stepper, three more: parameters
    (value.* included) and moments bit-identical."""
    from video_dqn_amd.trainer import load_optimizer_state_dict, load_value_head_state, optimizer_state_dict, value_head_state
    B = 4
    net_u, stp_u = _stepper("f32", B, iql_expectile=0.7)
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    net_i, stp_i = _stepper("f32", B, iql_expectile=0.7)
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    sd, vh = optimizer_state_dict(stp_i), value_head_state(stp_i)
    n_ref = sum(1 for s in net_i.slots.values() if s.kind in (0, 1)) - 2
    assert sd["param_groups"][0]["params"] == list(range(n_ref)) and max(sd["state"]) < n_ref
    model_sd = {n: net_i.view(n).clone() for n in net_i.slots if not n.startswith("value.")}
    net_r, stp_r = _stepper("f32", B, iql_expectile=0.7)
    net_r.view("value.weight").zero_()  # (whatever it held: the checkpoint's comes back)
    net_r.load_tensors(model_sd)
    load_optimizer_state_dict(stp_r, sd)
    load_value_head_state(stp_r, vh)
    stp_r.sample_number = 3
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", net_u.params, net_r.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq), ("stats", stp_u.iql_stats, stp_r.iql_stats)):
        assert torch.equal(x, y), name
    assert not torch.equal(net_u.view("value.weight"), net_i.view("value.weight"))


# ---- 9. run_train --------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def test_run_train_with_iql_expectile(tmp_path):
    """100 updates with IQL_EXPECTILE 0.7 together with N_STEP 3, PRIORITIZED_REPLAY and TARGET_TAU 0.01, and a scalar writer: both
    scalars are written at update 100 (with the values of update 99, one update late like the loss), the V loss positive; the
    checkpoint has the reference's three keys in the reference's shapes plus value_head, replay_state and target_state_dict; two runs
    resumed from it end bit-identical."""
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd.config import ExperimentConfig, JsonlWriter
    from video_dqn_amd.trainer import run_train
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    keys = "IQL_EXPECTILE: 0.7\nN_STEP: 3\nPRIORITIZED_REPLAY: True\nTARGET_TAU: 0.01\n"
    _write_cfg(tmp_path / "a", shards, 100, keys)
    cfg = ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=True)
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    logs = []
    model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
    cfg.writer.close()
    assert np.isfinite(running) and stepper.iql_expectile == 0.7 and model.value_head
    assert any(l.startswith("implicit Q-learning: a value head") for l in logs)
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    v_loss = [r for r in rows if r["tag"] == "iql_v_loss/train"]
    adv = [r for r in rows if r["tag"] == "iql_advantage/train"]
    assert len(v_loss) == 1 and len(adv) == 1 and v_loss[0]["step"] == 99 and adv[0]["step"] == 99
    print(f"iql_v_loss/train {v_loss[0]['value']:.6f}, iql_advantage/train {adv[0]['value']:.6f}")
    assert v_loss[0]["value"] > 0 and math.isfinite(adv[0]["value"])
    assert any(r["tag"] == "avg_q_loss/train" and r["step"] == 100 for r in rows)
    snap = torch.load(tmp_path / "a" / "models" / "sample96.torch", map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "value_head", "replay_state", "target_state_dict"}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_state_dict.json")) as f:
        ref = json.load(f)["ec1_pano0"]
    for key in ("model_state_dict", "target_state_dict"):
        assert list(snap[key]) == ref["keys"] and [list(v.shape) for v in snap[key].values()] == ref["shapes"], key
    assert max(snap["optimizer_state_dict"]["state"]) < len(ref["params"])
    assert set(snap["value_head"]["state_dict"]) == {"value.weight", "value.bias"}
    assert snap["value_head"]["optimizer_state"]["value.weight"]["step"] == 96
    # the greedy policy loads from the reference's keys alone
    from video_dqn_amd.model import load_model_number
    greedy = load_model_number(ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=False), 96)
    assert tuple(greedy(torch.zeros(2, 3, 224, 224)).shape) == (2, 5, 3) and torch.equal(greedy.engine.view("top.4.weight").cpu(), snap["model_state_dict"]["top.4.weight"])
    finals = []
    for tag in ("r1", "r2"):
        _write_cfg(tmp_path / tag, shards, 100, keys)
        (tmp_path / tag / "models").mkdir()
        torch.save(snap, tmp_path / tag / "models" / "sample96.torch")
        logs = []
        m, s, _ = run_train(ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False, resume=True), resume_from=96,
                            log=lambda *a: logs.append(" ".join(map(str, a))))
        assert s.adam_step == 99 and s.iql_expectile == 0.7
        assert any("the value head and its Adam moments restored" in l for l in logs)
        finals.append((m.engine.params.cpu(), s.exp_avg_sq.cpu(), s.iql_stats.cpu(), s.target_params.cpu()))
    for x, y in zip(*finals):
        assert torch.equal(x, y)
    # a checkpoint without the key: the head starts from its initialisation, and the run says so
    old = {k: v for k, v in snap.items() if k != "value_head"}
    _write_cfg(tmp_path / "warm", shards, 98, keys)
    (tmp_path / "warm" / "models").mkdir()
    torch.save(old, tmp_path / "warm" / "models" / "sample96.torch")
    logs = []
    run_train(ExperimentConfig(str(tmp_path / "warm"), device=DEV, tensorboard=False, resume=True), resume_from=96,
              log=lambda *a: logs.append(" ".join(map(str, a))))
    assert any("the checkpoint has no value_head" in l for l in logs)
