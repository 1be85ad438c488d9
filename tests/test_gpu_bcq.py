"""Discrete BCQ on the GPU: vdqn_td_loss_bcq against the float64 autograd oracle (tests/bcq_oracle.py) and against
vdqn_td_loss_weighted / vdqn_td_loss_nstep, a hand-built row, its deterministic mode, half batches, the read-out, vdqn_net_td_forward_bcq
against the operator and the float64 network oracle, both architectures and the compute modes, AUG_FLIP, resume, and run_train with
BCQ_THRESHOLD."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import bcq_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _bcq(inputs, threshold, dtype=None, loss_kind=0, use_valid=True, weight=None, with_err=True, clip_rect=1, gamma=0.9, deterministic=1,
         n_cat=5, n_act=3, q_copy=False, discount=None, inv_count=None, with_stats=True, bc_weight=1.0, logit_reg=0.01):
    """vdqn_td_loss_bcq through the raw ABI -> (loss, stats, dq as f32, dq_f32, err, q_copy), all on the CPU."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    dtype = _lib.VDQN_F32 if dtype is None else dtype
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    loss, stats = torch.zeros(1, device=DEV), torch.zeros(3, device=DEV)
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
    _lib.check(lib.vdqn_td_loss_bcq(C.byref(a), weight.data_ptr() if weight is not None else None, err.data_ptr() if with_err else None,
                                    discount.data_ptr() if discount is not None else None, threshold, bc_weight, logit_reg,
                                    stats.data_ptr() if with_stats else None, torch.cuda.current_stream().cuda_stream), "vdqn_td_loss_bcq")
    torch.cuda.synchronize()
    return loss.cpu(), stats.cpu(), dq.float().cpu(), dq32.cpu(), (err.cpu() if with_err else None), (qc.cpu() if q_copy else None)


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _discount(B, seed=6):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.45


def _rel(x, want):
    return abs(x - want) / max(abs(want), 1e-30)


def _check_against_oracle(inputs, threshold, got, n_cat=5, n_act=3, **kw):
    """The project's operator gate (tests/test_gpu_iql.py): dq within 1e-6 of the maximum element, every column other than the n_cat
    taken-action columns and the n_act logit columns exactly 0, loss and the stats within 1e-5 relative, err within 1e-6."""
    loss, stats, _, dq32, err, _ = got
    n = n_cat * n_act
    o = bcq_oracle.objective(inputs, threshold, n_cat=n_cat, n_act=n_act, **kw)
    dq_max = o["dq"].abs().max().item()
    e_dq = (dq32[:, :n + n_act].double() - o["dq"]).abs().max().item() / dq_max
    e_loss, e_ce = _rel(loss.item(), o["loss"].item()), _rel(stats[0].item(), o["ce"].item())
    # (the two counting stats may be exactly 0: then the kernel's must be)
    e_share = _rel(stats[1].item(), o["constrained_share"].item()) if o["constrained_share"].item() else abs(stats[1].item())
    e_acc = _rel(stats[2].item(), o["accuracy"].item()) if o["accuracy"].item() else abs(stats[2].item())
    print(f"dq {e_dq:.2e} of the max element, loss {e_loss:.2e}, ce {e_ce:.2e}, share {e_share:.2e}, accuracy {e_acc:.2e} relative")
    assert torch.isfinite(dq32).all() and math.isfinite(loss.item()) and torch.isfinite(stats).all()
    assert e_dq <= 1e-6
    B = dq32.shape[0]
    live = torch.zeros_like(dq32, dtype=torch.bool)
    live[:, n:n + n_act] = True
    live[torch.arange(B).repeat_interleave(n_cat), torch.arange(n_cat).repeat(B) * n_act + inputs[3].repeat_interleave(n_cat)] = True
    assert torch.all(dq32[~live] == 0)
    assert e_loss <= 1e-5 and e_ce <= 1e-5 and e_share <= 1e-5 and e_acc <= 1e-5
    if err is not None:
        e_err = (err.double() - o["err"]).abs().max().item() / max(o["err"].abs().max().item(), 1e-30)
        print(f"err {e_err:.2e}")
        assert e_err <= 1e-6
    return o


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq,n_cat,n_act", bcq_oracle.OPERATOR_SHAPES, ids=["B96", "B1", "B3", "ldq18", "C2A2"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_td_loss_bcq_vs_f64_oracle(loss_kind, use_valid, weighted, B, ldq, n_cat, n_act):
    """Scalar and per-sample discount, three thresholds, both deterministic settings; bf16 dq is dq_f32 rounded once."""
    from video_dqn_amd import _lib
    cpu = bcq_oracle.inputs(B, 11 + loss_kind + 2 * use_valid, ldq=ldq, n_cat=n_cat, n_act=n_act)
    for t in bcq_oracle.THRESHOLDS:
        assert min(bcq_oracle.margin(cpu, t, n_cat, n_act)) >= bcq_oracle.MARGIN
    if use_valid:
        cpu[6][0, 0] = 1.0  # (B = 1: at least one valid term, so the relative gates have something to divide by)
    w = _weights(B) if weighted else None
    wd = None if w is None else w.to(DEV)
    inputs = _dev(cpu)
    kw = dict(loss_kind=loss_kind, use_valid=use_valid)
    shape = dict(n_cat=n_cat, n_act=n_act)
    shares = {}
    for disc in (None, _discount(B)):
        dd = None if disc is None else disc.to(DEV)
        for t in bcq_oracle.THRESHOLDS:
            for det in (1, 0):
                got = _bcq(inputs, t, weight=wd, deterministic=det, q_copy=True, discount=dd, **kw, **shape)
                o = _check_against_oracle(cpu, t, got, weight=w, discount=disc, **kw, **shape)
                shares[t] = o["constrained_share"].item()
                assert torch.equal(got[2], got[3])  # the f32 dq and dq_f32 are the same values
                assert torch.equal(got[5], cpu[0][:, :n_cat * n_act])
    assert shares[0.0] == 0.0
    if B >= 3 and not use_valid:
        assert 0.1 <= shares[0.3] <= 0.9
    bf = _bcq(inputs, 0.3, dtype=_lib.VDQN_BF16, weight=wd, with_err=False, **kw, **shape)
    f32 = _bcq(inputs, 0.3, weight=wd, with_err=False, **kw, **shape)
    assert torch.equal(bf[3], f32[3]) and torch.equal(bf[0], f32[0]) and torch.equal(bf[1], f32[1])
    assert torch.equal(bf[2], bf[3].bfloat16().float())  # one rounding to nearest even, as every other kernel stores bf16


def test_bc_weight_logit_reg_and_bad_action_rows():
    """Other weights of the behaviour terms against the oracle; a row whose action is outside [0, A) writes zeros and adds nothing."""
    B, ldq, n_cat, n_act, seed = bcq_oracle.OPS_CASE
    cpu = bcq_oracle.inputs(B, seed)
    inputs = _dev(cpu)
    for bcw, reg in ((0.25, 0.0), (3.0, 0.5)):
        got = _bcq(inputs, 0.3, bc_weight=bcw, logit_reg=reg)
        _check_against_oracle(cpu, 0.3, got, bc_weight=bcw, logit_reg=reg)
    bad = [t.clone() for t in cpu]
    bad[3][1], bad[3][3] = 3, -1
    got = _bcq(_dev(bad), 0.3, q_copy=True)
    keep = torch.tensor([0, 2, 4])
    part = [t[keep].contiguous() for t in cpu]
    ref = _bcq(_dev(part), 0.3, inv_count=1.0 / (n_cat * B))
    assert torch.all(got[3][1] == 0) and torch.all(got[3][3] == 0) and got[4][1].item() == 0 and got[4][3].item() == 0
    assert torch.equal(got[3][keep], ref[3]) and torch.equal(got[4][keep], ref[4])
    assert _rel(got[0].item(), ref[0].item()) <= 1e-6 and torch.equal(got[5], cpu[0][:, :15])
    for k in range(3):
        assert abs(got[1][k].item() - ref[1][k].item()) <= 1e-6 * max(abs(ref[1][k].item()), 1e-30)


def test_ops_td_loss_bcq_and_null_outputs():
    """ops.td_loss_bcq mirrors the raw entry; weight, err_out, sample_gamma, stats, q_copy and dq_f32's twin may each be NULL."""
    from video_dqn_amd import _lib, ops
    B, ldq, n_cat, n_act, seed = bcq_oracle.OPS_CASE
    cpu = bcq_oracle.inputs(B, seed)
    inputs = _dev(cpu)
    loss, dq, dq32, stats, err, qc = ops.td_loss_bcq(*inputs[:6], inputs[6], threshold=0.3, gamma=0.9, with_err=True, deterministic=True)
    raw = _bcq(inputs, 0.3)
    assert torch.equal(loss.cpu(), raw[0]) and torch.equal(stats.cpu(), raw[1]) and torch.equal(dq32.cpu(), raw[3]) and torch.equal(err.cpu(), raw[4])
    assert torch.equal(dq.cpu(), raw[3]) and qc is None
    loss2, _, dq32_2, stats2, err2, _ = ops.td_loss_bcq(*inputs[:6], inputs[6], threshold=0.3, gamma=0.9, deterministic=True, with_stats=False,
                                                        with_dq32=False)
    assert err2 is None and stats2 is None and dq32_2 is None and torch.equal(loss2, loss)
    for bad in (-1.0, 1.0, float("nan")):
        with pytest.raises(_lib.VdqnError, match="threshold"):
            ops.td_loss_bcq(*inputs[:6], threshold=bad)
    with pytest.raises(_lib.VdqnError, match="linear"):
        ops.td_loss_bcq(*inputs[:6], threshold=0.3, linear=True)
    with pytest.raises(_lib.VdqnError, match="bc_weight"):
        ops.td_loss_bcq(*inputs[:6], threshold=0.3, bc_weight=0.0)


# ---- 2. threshold 0 is the weighted TD loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
def test_threshold_zero_is_the_weighted_td_loss_bit_for_bit(loss_kind):
    """Every action allowed: the Q columns of dq and err are vdqn_td_loss_weighted's bits, and vdqn_td_loss_nstep's with a per-sample
    discount (the same expression order for y and d); the loss is the weighted TD loss plus the behaviour term."""
    from test_gpu_replay import _td
    from video_dqn_amd import _lib, ops
    B, ldq, n_cat, n_act, seed = bcq_oracle.TWIN_CASE
    cpu = bcq_oracle.inputs(B, seed)
    cpu[0][:, :15] = cpu[0][:, :15] * 2.5  # |d| beyond 1: both Huber branches
    inputs = _dev(cpu)
    w = _weights(B, 4)
    for use_valid in (False, True):
        for clip_rect, gamma in ((1, 0.9), (0, 0.99), (0, 0.5), (1, 0.5)):
            kw = dict(clip_rect=clip_rect, gamma=gamma)
            ref = _td(inputs, _lib.VDQN_F32, loss_kind, use_valid, weight=w.to(DEV), **kw)
            got = _bcq(inputs, 0.0, loss_kind=loss_kind, use_valid=use_valid, weight=w.to(DEV), **kw)
            o = _check_against_oracle(cpu, 0.0, got, weight=w, loss_kind=loss_kind, use_valid=use_valid, **kw)
            assert torch.equal(got[3][:, :15], ref[2][:, :15]), (use_valid, kw)
            assert torch.equal(got[4], ref[3]), (use_valid, kw)
            assert got[1][1].item() == 0.0
            bc = (o["loss"] - o["td_loss"]).item()
            assert abs(got[0].item() - (ref[0].item() + bc)) <= 1e-5 * abs(got[0].item())
        disc = _discount(B, 8).to(DEV)
        ref = ops.td_loss_nstep(*inputs[:6], inputs[6] if use_valid else None, discount=disc, weights=w.to(DEV), with_err=True,
                                loss_kind=("huber" if loss_kind else "l2"), deterministic=True)
        got = _bcq(inputs, 0.0, loss_kind=loss_kind, use_valid=use_valid, weight=w.to(DEV), discount=disc)
        assert torch.equal(got[3][:, :15], ref[2].cpu()[:, :15]) and torch.equal(got[4], ref[4].cpu())


# ---- 3. a hand-built row -------------------------------------------------------------------------------------------------------------
def test_hand_built_row_takes_the_best_allowed_action():
    """One sample: the free arg-max of the online Q(s') is action 2 in every category, and its behaviour probability is 0.2 of the
    largest, below tau = 0.3: the target takes action 0 (category 0: the better of the two allowed) or action 1 (the others), and y
    differs from the Double-DQN y by gamma * (Q_target(a') - Q_target(2)) exactly as set up.  At tau = 0.1 action 2 is allowed."""
    B, gamma = 1, 0.5
    qb, qo, qt = torch.zeros(B, 64), torch.zeros(B, 64), torch.zeros(B, 64)
    for c in range(5):
        qo[0, c * 3:c * 3 + 3] = torch.tensor([0.5, 0.25, 1.0]) if c == 0 else torch.tensor([0.25, 0.5, 1.0])
        qt[0, c * 3:c * 3 + 3] = torch.tensor([0.125, 0.25, 0.75])
    qo[0, 15:18] = torch.tensor([0.0, math.log(0.5), math.log(0.2)])
    qb[0, 15:18] = torch.tensor([0.3, -0.2, 0.1])
    act = torch.tensor([1])
    rew, term, valid = torch.full((B, 5), 0.125), torch.zeros(B, 5), torch.ones(B, 5)
    inputs = _dev([qb, qo, qt, act, rew, term, valid])
    con = _bcq(inputs, 0.3, gamma=gamma, clip_rect=0)
    free = _bcq(inputs, 0.1, gamma=gamma, clip_rect=0)
    ddqn = _bcq(inputs, 0.0, gamma=gamma, clip_rect=0)
    # d = Q(s, a*) - y with Q(s, .) = 0: dq at the taken column is -y / 5
    y_con = -con[3][0, 1:15:3] * 5
    y_free = -free[3][0, 1:15:3] * 5
    want_con = torch.tensor([0.125 + 0.5 * 0.125] + [0.125 + 0.5 * 0.25] * 4)
    want_free = torch.full((5,), 0.125 + 0.5 * 0.75)
    assert torch.allclose(y_con, want_con, rtol=0, atol=5e-7) and torch.allclose(y_free, want_free, rtol=0, atol=5e-7)
    assert torch.equal(free[3], ddqn[3]) and torch.equal(free[0], ddqn[0])
    assert torch.allclose(y_free - y_con, gamma * torch.tensor([0.75 - 0.125] + [0.75 - 0.25] * 4), rtol=0, atol=5e-7)
    assert abs(con[1][1].item() - 1.0) <= 1e-6 and free[1][1].item() == 0.0 and ddqn[1][1].item() == 0.0
    # the behaviour terms do not depend on the threshold; the head's arg-max (0) is not the logged action (1)
    assert torch.equal(con[3][0, 15:18], free[3][0, 15:18]) and con[1][0].item() == free[1][0].item() and con[1][2].item() == 0.0
    lg = qb[0, 15:18].double()
    assert abs(con[1][0].item() - (torch.logsumexp(lg, 0) - lg[1]).item()) <= 1e-6


# ---- 4. deterministic, half batches --------------------------------------------------------------------------------------------------
def test_deterministic_is_bit_identical_and_agrees_with_the_atomic_sum():
    B, ldq, n_cat, n_act, seed = bcq_oracle.DET_CASE
    inputs = _dev(bcq_oracle.inputs(B, seed))
    w = _weights(B).to(DEV)
    runs = [_bcq(inputs, 0.3, weight=w, loss_kind=1, deterministic=1) for _ in range(2)]
    for x, y in zip(runs[0][:5], runs[1][:5]):
        assert torch.equal(x, y)
    free = _bcq(inputs, 0.3, weight=w, loss_kind=1, deterministic=0)
    assert _rel(free[0].item(), runs[0][0].item()) <= 1e-5
    for k in range(3):
        assert _rel(free[1][k].item(), runs[0][1][k].item()) <= 1e-5
    assert torch.equal(free[3], runs[0][3]) and torch.equal(free[4], runs[0][4])


def test_two_half_batches_at_the_global_inv_count_are_the_full_batch():
    """What two ranks compute: each half at inv_count = 1 / (n_cat * global batch) writes the full batch's dq rows bit for bit, and
    the loss and stats shares sum to the full batch's."""
    B, ldq, n_cat, n_act, seed = bcq_oracle.HALVES_CASE
    cpu = bcq_oracle.inputs(B, seed)
    w = _weights(B, 9)
    inv = 1.0 / (n_cat * B)
    full = _bcq(_dev(cpu), 0.3, weight=w.to(DEV), inv_count=inv)
    halves = []
    for lo in (0, B // 2):
        part = [t[lo:lo + B // 2].contiguous() for t in cpu]
        halves.append(_bcq(_dev(part), 0.3, weight=w[lo:lo + B // 2].contiguous().to(DEV), inv_count=inv))
    assert torch.equal(torch.cat([halves[0][3], halves[1][3]]), full[3])
    assert torch.equal(torch.cat([halves[0][4], halves[1][4]]), full[4])
    assert _rel((halves[0][0] + halves[1][0]).item(), full[0].item()) <= 1e-6
    for k in range(3):
        assert abs((halves[0][1][k] + halves[1][1][k]).item() - full[1][k].item()) <= 1e-5 * max(abs(full[1][k].item()), 1e-30)


# ---- 5. the read-out -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq,n_cat,n_act", bcq_oracle.OPERATOR_SHAPES, ids=["B96", "B1", "B3", "ldq18", "C2A2"])
def test_bcq_constrain_vs_oracle(B, ldq, n_cat, n_act):
    """The rows of s' serve as rows to read out: their logits keep the margin from every threshold's boundary."""
    from video_dqn_amd import ops
    cpu = bcq_oracle.inputs(B, 13, ldq=ldq, n_cat=n_cat, n_act=n_act)
    rows = cpu[1].to(DEV)
    n = n_cat * n_act
    for t in bcq_oracle.THRESHOLDS:
        q, prob = ops.bcq_constrain(rows, t, n_cat=n_cat, n_act=n_act)
        ok = bcq_oracle.allowed_set(cpu[1].double(), t, n_cat, n_act).view(B, 1, n_act).expand(B, n_cat, n_act)
        q3 = cpu[1][:, :n].reshape(B, n_cat, n_act)
        assert torch.equal(q.cpu(), torch.where(ok, q3, torch.full_like(q3, -math.inf)))
        want = torch.softmax(cpu[1][:, n:n + n_act].double(), 1)
        assert (prob.cpu().double() - want).abs().max().item() <= 1e-6
        best, _ = bcq_oracle.choices(cpu[1].double(), t, n_cat, n_act)
        assert torch.equal(q.argmax(-1).cpu(), best)
    assert ops.bcq_constrain(rows, 0.3, n_cat=n_cat, n_act=n_act, with_prob=False)[1] is None


# ---- 6. the engine -------------------------------------------------------------------------------------------------------------------
def _policy_rows(seed, in_f):
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.rand(3, in_f, generator=g) * 2 - 1) * 0.02, (torch.rand(3, generator=g) * 2 - 1) * 0.3  # (logits of a few units: mixed allowed sets)


def _net(dtype, max_batch, seed=7, extra_capacity=True, deterministic=True, policy_head=True):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, extra_capacity, dtype, max_batch, deterministic=deterministic, policy_head=policy_head)
    net.load_tensors(synth.make_state_dict(seed, extra_capacity=extra_capacity))
    if policy_head:
        pw, pb = _policy_rows(seed, 256 if extra_capacity else 512)
        net.view("policy.weight").copy_(pw)
        net.view("policy.bias").copy_(pb)
        net.mark_dirty()
    return net


def _stepper(dtype, B, deterministic=True, extra_capacity=True, policy_head=True, **kw):
    from video_dqn_amd.engine import TDStepper
    net = _net(dtype, 2 * B, extra_capacity=extra_capacity, deterministic=deterministic, policy_head=policy_head)
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
def test_td_forward_bcq_writes_the_operators_dq(weighted):
    from video_dqn_amd import _lib, ops
    B = 4
    net, stp = _stepper("f32", B, bcq_threshold=0.3)
    target = _net("f32", 2 * B, seed=8)
    target.pack_weights(stp.packed_target)  # a target network of its own
    before, after, kind, act, rew, term = _batch(101, B)
    w = _weights(B, 12).to(DEV) if weighted else None
    err = torch.zeros(B, device=DEV) if weighted else None
    a = stp._args(before, after, kind, act, rew, term, stp._ones, None, w, err)
    st = torch.cuda.current_stream().cuda_stream
    stp.bcq_stats.fill_(5.0)  # (cleared beside the loss)
    _lib.check(net.lib.vdqn_net_td_forward_bcq(net.handle, C.byref(a), 0.3, 1.0, 0.01, stp.bcq_stats.data_ptr(), st), "vdqn_net_td_forward_bcq")
    torch.cuda.synchronize()
    dq = _dq(net, stp, B)
    qb, qo, qt = _qf(net, stp, B)
    loss, _, dq32, stats, e, _ = ops.td_loss_bcq(qb, qo, qt, act, rew, term, None, threshold=0.3, weights=w, with_err=weighted, gamma=0.99,
                                                 clip_rect=True, deterministic=True)
    assert torch.equal(dq, dq32) and torch.equal(stp.loss, loss) and torch.equal(stp.bcq_stats, stats)
    assert (dq[:, 15:18] != 0).all() and torch.all(dq[:, 18:] == 0) and (dq[:, :15] != 0).sum().item() <= 5 * B
    assert stats[0].item() > 0 and (qb[:, 15:18] != 0).all() and torch.all(qb[:, 18:] == 0)
    assert torch.equal(stp.q_before, qb[:, :15])
    if weighted:
        assert torch.equal(err, e)
    # the target pass ran over s', and the logits the loss read at s' are the ONLINE network's
    q_after = target.forward(after, kind, B)
    torch.cuda.synchronize()
    assert torch.equal(qt[:, :15], q_after)
    # the Double-DQN entry on the same policy-head net: zeros in the logit columns and the parent's loss
    _lib.check(net.lib.vdqn_net_td_forward(net.handle, C.byref(a), st), "vdqn_net_td_forward")
    torch.cuda.synchronize()
    dq0 = _dq(net, stp, B)
    qb0, qo0, qt0 = _qf(net, stp, B)
    ref = ops.td_loss_nstep(qb0, qo0, qt0, act, rew, term, None, discount=torch.full((B,), 0.99, device=DEV), weights=w, with_err=weighted,
                            clip_rect=True, deterministic=True)
    assert torch.all(dq0[:, 15:] == 0) and torch.equal(dq0, ref[2]) and torch.equal(stp.loss, ref[0]) and torch.equal(qb0, qb)


def _oracle_state_dict(seed):
    """synth's state_dict for the reference class with SIX categories: its rows c * 3 + a, c < 5, are the engine's Q rows, and the rows
    of the sixth category, 15 + a, the engine's policy rows."""
    from video_dqn_amd import synth
    sd = synth.make_state_dict(seed)
    pw, pb = _policy_rows(seed, 256)
    sd["top.4.weight"], sd["top.4.bias"] = torch.cat([sd["top.4.weight"], pw]), torch.cat([sd["top.4.bias"], pb])
    return sd


def test_model_forward_keeps_its_shape_and_the_read_outs_match_the_oracle():
    """HabitatDQNMultiAction(policy_head=True): forward still returns [B, 5, 3] with the bits of a model without the head; behaviour
    [B, 3] and constrained_q [B, 5, 3] from the same forward, against the reference class with six categories (the gate of
    tests/test_gpu_engine.py::test_forward_matches_oracle, 1e-3)."""
    from oracle import ref_cpu
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    B = 3
    model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=8, policy_head=True)
    model.load_state_dict(synth.make_state_dict(7))  # (no policy.*: the initialised head stays)
    pw, pb = _policy_rows(7, 256)
    with torch.no_grad():
        model.policy.weight.copy_(pw)
        model.policy.bias.copy_(pb)
    model.engine.mark_dirty()
    model.eval()
    (tup, _) = synth.make_batch(24, B, 1, structured=True)
    frames = tup[0].to(DEV)
    with torch.no_grad():
        q = model(frames)
    prob = model.behaviour(frames)
    cq = model.constrained_q(frames, 0.3)
    assert tuple(q.shape) == (B, 5, 3) and tuple(prob.shape) == (B, 3) and tuple(cq.shape) == (B, 5, 3)
    oracle = ref_cpu.HabitatDQNMultiAction(3, 6, extra_capacity=True, panorama=False)
    oracle.load_state_dict(_oracle_state_dict(7))
    oracle.eval()
    with torch.no_grad():
        ref = oracle(tup[0])
    e_q = ((q.cpu() - ref[:, :5]).abs().max() / ref[:, :5].abs().max()).item()
    want = torch.softmax(ref[:, 5].double(), 1)
    e_p = (prob.cpu().double() - want).abs().max().item()
    print(f"Q {e_q:.2e} of the maximum, behaviour probabilities {e_p:.2e}")
    assert e_q < 1e-3 and e_p < 1e-3 and (prob.sum(1) - 1).abs().max().item() < 1e-5
    # constrained_q is forward's bits or -inf, -inf exactly where the model's own probabilities say so (no probability near the boundary)
    ratio = prob / prob.max(1, keepdim=True).values
    assert ((ratio - 0.3).abs() > 1e-3).all()
    ok = (ratio > 0.3).view(B, 1, 3).expand(B, 5, 3)
    assert torch.equal(cq, torch.where(ok, q, torch.full_like(q, -math.inf))) and torch.equal(model.constrained_q(frames, 0.0), q)
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=8)
    plain.load_state_dict(synth.make_state_dict(7))
    plain.eval()
    with torch.no_grad():
        assert torch.equal(plain(frames), q)
    with pytest.raises(RuntimeError, match="policy_head"):
        plain.constrained_q(frames, 0.3)


def test_stepper_validation():
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine, TDStepper
    headed = NetEngine(3, 5, 1, True, "f32", 8, policy_head=True)
    plain = NetEngine(3, 5, 1, True, "f32", 8)
    kw = dict(lr=1e-4, gamma=0.99, clip_rect=True)
    for bad in (-0.7, 1.0, float("nan")):
        with pytest.raises(_lib.VdqnError, match="bcq_threshold"):
            TDStepper(headed, 4, bcq_threshold=bad, **kw)
    with pytest.raises(_lib.VdqnError, match="bcq_bc_weight"):
        TDStepper(headed, 4, bcq_threshold=0.3, bcq_bc_weight=0.0, **kw)
    with pytest.raises(_lib.VdqnError, match="bcq_logit_reg"):
        TDStepper(headed, 4, bcq_threshold=0.3, bcq_logit_reg=-1.0, **kw)
    with pytest.raises(_lib.VdqnError, match="bcq_threshold.*policy head"):
        TDStepper(plain, 4, bcq_threshold=0.3, **kw)
    for more in (dict(train_on_ground_truth=True), dict(linear=True), dict(cql_alpha=1.0), dict(mc_floor=True)):
        with pytest.raises(_lib.VdqnError, match="bcq_threshold"):
            TDStepper(headed, 4, bcq_threshold=0.3, **kw, **more)
    for more in (dict(value_head=True), dict(spread_head=True)):
        with pytest.raises(_lib.VdqnError, match="out of scope"):
            NetEngine(3, 5, 1, True, "f32", 8, policy_head=True, **more)
    with pytest.raises(_lib.VdqnError, match="policy_head"):
        NetEngine(1, 5, 1, True, "f32", 8, policy_head=True)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stepper_threshold_off_is_the_stepper_without_the_argument(dtype):
    """With the key at its default nothing changes: the same entries, launches and bits on a network without the policy head."""
    B = 4
    runs = []
    for kw in (dict(), dict(bcq_threshold=-1.0)):
        net, stp = _stepper(dtype, B, policy_head=False, **kw)
        losses = []
        for s in (1, 2):
            losses.append(stp.step(*_batch(300 + s, B)).clone())
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), torch.cat(losses).cpu(), stp.grads.cpu(), stp.exp_avg_sq.cpu()))
        assert stp.bcq_stats.abs().sum().item() == 0.0 and not stp.bcq
    for x, y in zip(*runs):
        assert torch.equal(x, y)


# ---- 7. one update against the float64 network oracle --------------------------------------------------------------------------------
def test_bcq_step_gradient_matches_f64_oracle():
    """One update with tau = 0.3 and random importance weights, f32 engine at B = 8: every gradient tensor against the float64
    oracle that takes the engine's ReLU decisions — the recipe, shape and gates of
    tests/test_gpu_iql.py::test_iql_step_gradient_matches_f64_oracle (objective within 1e-3 relative; relative L2 <= 1e-3 and max
    element <= 5e-3 of the tensor's max; more than 60 tensors, policy.* among them).  The oracle is the reference class with six
    categories (the sixth holds the logits); the objective is formed here from its outputs, with the engine's own allowed set and
    choice checked to be far from their boundaries."""
    from oracle import ref_cpu
    from test_gpu_engine import _EngineReLU, _engine_relu_masks
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B, tau, gamma = 8, 0.3, 0.99
    net = _net("f32", 2 * B, seed=7)
    stp = TDStepper(net, B, lr=1e-4, gamma=gamma, clip_rect=True, bcq_threshold=tau)
    _net("f32", 2 * B, seed=8).pack_weights(stp.packed_target)  # a target network of its own
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05
    err = torch.zeros(B, device=DEV)
    loss = stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV),
                    tup[4].float().to(DEV), weights=w.to(DEV), td_error=err)
    torch.cuda.synchronize()
    grads = stp.grads.cpu()
    masks = _engine_relu_masks(net, stp.acts_online, stp.layout_samples, B)
    model = ref_cpu.HabitatDQNMultiAction(3, 6, extra_capacity=True, panorama=False)
    model.load_state_dict(_oracle_state_dict(7))
    target = ref_cpu.HabitatDQNMultiAction(3, 6, extra_capacity=True, panorama=False)
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
        out_next = model(tup[1].double())
        q_t = target(tup[1].double())[:, :5]
    lg_next = out_next[:, 5]
    rel = lg_next - lg_next.max(1, keepdim=True).values
    ok = rel > math.log(float(np.float32(tau)))
    q_next = out_next[:, :5]
    masked = torch.where(ok.view(B, 1, 3), q_next, torch.full_like(q_next, -math.inf))
    best, free = masked.argmax(2), q_next.argmax(2)
    top = masked.sort(2, descending=True).values
    not_max = rel < 0
    m_logit = (rel - math.log(float(np.float32(tau)))).abs()[not_max].min().item()
    m_gap = (top[:, :, 0] - top[:, :, 1]).min().item()
    idx = act.view(B, 1, 1).expand(B, 5, 1)
    q_s, lg = out_s[:, :5].gather(2, idx).squeeze(2), out_s[:, 5]
    y = (rew + gamma * ((1 - term) * q_t.gather(2, best.unsqueeze(2)).squeeze(2))).clamp(0, 1)
    d = q_s - y
    ce = torch.logsumexp(lg, 1) - lg.gather(1, act.view(B, 1)).squeeze(1)
    l_b = 1.0 * (ce + float(np.float32(0.01)) * (lg ** 2).mean(1))
    wd = w.double()
    objective = (0.5 * d ** 2 * wd.view(B, 1)).mean() + (l_b * wd).mean()
    objective.backward()
    share, acc = (best != free).double().mean().item(), (lg.argmax(1) == act).double().mean().item()
    print(f"objective {loss.item():.6f} / {objective.item():.6f}, ce {stp.bcq_stats[0].item():.6f} / {ce.mean().item():.6f}, "
          f"share {stp.bcq_stats[1].item():.4f} / {share:.4f}, accuracy {stp.bcq_stats[2].item():.4f} / {acc:.4f}, "
          f"margins {m_logit:.2e} {m_gap:.2e}")
    assert m_logit >= 1e-4 and m_gap >= 1e-4  # (no decision on its boundary: the f32 engine and the oracle choose alike)
    assert abs(loss.item() - objective.item()) <= 1e-3 * abs(objective.item())
    assert abs(stp.bcq_stats[0].item() - ce.mean().item()) <= 1e-3 * ce.mean().item()
    assert abs(stp.bcq_stats[1].item() - share) <= 1e-5 and abs(stp.bcq_stats[2].item() - acc) <= 1e-5
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

    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        if name.startswith("top.4."):
            kind = name.rsplit(".", 1)[1]
            compare(name, engine_grad(name), p.grad.double()[:15])
            compare("policy." + kind, engine_grad("policy." + kind), p.grad.double()[15:])
        else:
            compare(name, engine_grad(name), p.grad.double())
    assert len(names) > 60 and "policy.weight" in names and "policy.bias" in names and not bad, bad


# ---- 8. the other architecture and the compute modes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,extra_capacity", [("f32", False), ("bf16x3", True), ("bf16", True)], ids=["basic", "bf16x3", "bf16"])
def test_other_architecture_and_compute_modes(dtype, extra_capacity):
    """One finite update each at B = 4: loss and stats are the operator's on the engine's own rows, and policy.weight moved."""
    from video_dqn_amd import ops
    B = 4
    net, stp = _stepper(dtype, B, extra_capacity=extra_capacity, bcq_threshold=0.3)
    p0, v0 = net.params.clone(), net.view("policy.weight").clone()
    batch = _batch(301, B)
    loss = stp.step(*batch)
    torch.cuda.synchronize()
    qb, qo, qt = _qf(net, stp, B)
    ref = ops.td_loss_bcq(qb, qo, qt, batch[3], batch[4], batch[5], None, threshold=0.3, gamma=0.99, clip_rect=True, deterministic=True)
    assert torch.equal(loss, ref[0]) and torch.equal(stp.bcq_stats, ref[3])
    assert torch.isfinite(net.params).all() and torch.isfinite(stp.grads).all() and not torch.equal(net.params, p0)
    assert not torch.equal(net.view("policy.weight"), v0) and stp.bcq_stats[0].item() > 0


# ---- 9. AUG_FLIP ---------------------------------------------------------------------------------------------------------------------
def test_aug_flip_exchanges_the_behaviour_target():
    """The augmentation exchanges the action labels of the mirrored samples before the loss sees them, so the behaviour head's
    cross-entropy target follows the mirror with no code of its own: with the logit regulariser at 0 the logit columns of dq are
    softmax - onehot times a positive factor, so the only negative one is the column of the -1 of the one-hot, and that is the
    exchanged action's, for every sample."""
    from video_dqn_amd.augment import Augmenter
    B = 8
    net, stp = _stepper("f32", B, bcq_threshold=0.3, bcq_logit_reg=0.0)
    from video_dqn_amd import synth
    _, _, _, _, rew, term = _batch(101, B)
    before, after = (torch.from_numpy(np.ascontiguousarray(synth.make_frames_uint8(101, which, B, 1, structured=True)).reshape(B, 224, 224, 3)).to(DEV)
                     for which in ("before", "after"))
    act = torch.tensor([1, 2, 1, 2, 0, 1, 2, 0], device=DEV)
    aug = Augmenter(B, DEV, pad=0, flip=True, flip_actions=(1, 2), seed=5)
    params = None
    for step in range(1, 9):  # the first draw that mirrors a sample whose action is one of the exchanged pair
        params = aug.draw(step)
        if ((params[:, 2] == 1) & (act != 0)).any().item():
            break
    mirrored = (params[:, 2] == 1).cpu()
    assert (mirrored & (act.cpu() != 0)).any()
    swapped = aug.actions(act).clone()
    want = act.cpu().clone()
    want[mirrored & (act.cpu() == 1)], want[mirrored & (act.cpu() == 2)] = 2, 1
    assert torch.equal(swapped.cpu(), want) and not torch.equal(want, act.cpu())
    stp.step(before, after, 0, swapped, rew, term, augment=params)
    torch.cuda.synchronize()
    dq = _dq(net, stp, B)[:, 15:18].cpu()
    assert ((dq < 0).sum(1) == 1).all() and torch.equal(dq.argmin(1), want)


# ---- 10. resume ----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit():
    """Six updates in one go against three updates, the trainer's dicts and `policy_head` into a fresh stepper, three more: parameters
    (policy.* included) and moments bit-identical."""
    from video_dqn_amd.trainer import head_state, load_head_state, load_optimizer_state_dict, optimizer_state_dict
    B = 4
    net_u, stp_u = _stepper("f32", B, bcq_threshold=0.3)
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    net_i, stp_i = _stepper("f32", B, bcq_threshold=0.3)
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    sd, ph = optimizer_state_dict(stp_i), head_state(stp_i)
    n_ref = sum(1 for s in net_i.slots.values() if s.kind in (0, 1)) - 2
    assert sd["param_groups"][0]["params"] == list(range(n_ref)) and max(sd["state"]) < n_ref
    model_sd = {n: net_i.view(n).clone() for n in net_i.slots if not n.startswith("policy.")}
    net_r, stp_r = _stepper("f32", B, bcq_threshold=0.3)
    net_r.view("policy.weight").zero_()  # (whatever it held: the checkpoint's comes back)
    net_r.load_tensors(model_sd)
    load_optimizer_state_dict(stp_r, sd)
    load_head_state(stp_r, ph)
    stp_r.sample_number = 3
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", net_u.params, net_r.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq), ("stats", stp_u.bcq_stats, stp_r.bcq_stats)):
        assert torch.equal(x, y), name
    assert not torch.equal(net_u.view("policy.weight"), net_i.view("policy.weight"))


# ---- 11. run_train -------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def test_run_train_with_bcq_threshold(tmp_path):
    """100 updates with BCQ_THRESHOLD 0.3 together with N_STEP 3, PRIORITIZED_REPLAY and TARGET_TAU 0.01, and a scalar writer: the three
    scalars are written at update 100 with finite values (those of update 99, one update late like the loss); the checkpoint has the
    reference's three keys in the reference's shapes plus policy_head, replay_state and target_state_dict; two runs resumed from it
    end bit-identical, and a checkpoint without the key starts the head from its initialisation and says so."""
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd.config import ExperimentConfig, JsonlWriter
    from video_dqn_amd.trainer import run_train
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    keys = "BCQ_THRESHOLD: 0.3\nN_STEP: 3\nPRIORITIZED_REPLAY: True\nTARGET_TAU: 0.01\n"
    _write_cfg(tmp_path / "a", shards, 100, keys)
    cfg = ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=True)
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    logs = []
    model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
    cfg.writer.close()
    assert np.isfinite(running) and stepper.bcq_threshold == 0.3 and stepper.bcq and model.policy_head
    assert any(l.startswith("batch-constrained Q-learning: a policy head") for l in logs)
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    tags = {t: [r for r in rows if r["tag"] == t] for t in ("bcq_bc_loss/train", "bcq_constrained_share/train", "bcq_accuracy/train")}
    for t, rs in tags.items():
        assert len(rs) == 1 and rs[0]["step"] == 99 and math.isfinite(rs[0]["value"]), t
    assert any(r["tag"] == "avg_q_loss/train" and r["step"] == 100 for r in rows)
    print(", ".join(f"{t} {rs[-1]['value']:.6f}" for t, rs in tags.items()))
    assert all(r["value"] > 0 for r in tags["bcq_bc_loss/train"])
    assert all(0 <= r["value"] <= 1 + 1e-6 for t in ("bcq_constrained_share/train", "bcq_accuracy/train") for r in tags[t])
    snap = torch.load(tmp_path / "a" / "models" / "sample96.torch", map_location="cpu")
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "policy_head", "replay_state", "target_state_dict"}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_state_dict.json")) as f:
        ref = json.load(f)["ec1_pano0"]
    for key in ("model_state_dict", "target_state_dict"):
        assert list(snap[key]) == ref["keys"] and [list(v.shape) for v in snap[key].values()] == ref["shapes"], key
    assert max(snap["optimizer_state_dict"]["state"]) < len(ref["params"])
    assert set(snap["policy_head"]) == {"state_dict", "optimizer_state"} and set(snap["policy_head"]["state_dict"]) == {"policy.weight", "policy.bias"}
    assert snap["policy_head"]["optimizer_state"]["policy.weight"]["step"] == 96
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
        assert s.adam_step == 99 and s.bcq_threshold == 0.3
        assert any("the policy head and its Adam moments restored" in l for l in logs)
        finals.append((m.engine.params.cpu(), s.exp_avg_sq.cpu(), s.bcq_stats.cpu(), s.target_params.cpu()))
    for x, y in zip(*finals):
        assert torch.equal(x, y)
    old = {k: v for k, v in snap.items() if k != "policy_head"}
    _write_cfg(tmp_path / "warm", shards, 98, keys)
    (tmp_path / "warm" / "models").mkdir()
    torch.save(old, tmp_path / "warm" / "models" / "sample96.torch")
    logs = []
    run_train(ExperimentConfig(str(tmp_path / "warm"), device=DEV, tensorboard=False, resume=True), resume_from=96,
              log=lambda *a: logs.append(" ".join(map(str, a))))
    assert any("the checkpoint has no policy_head" in l for l in logs)
