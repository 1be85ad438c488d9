"""Gaussian distributional Q-learning on the GPU: vdqn_td_loss_dist against the float64 oracle over torch's kl_divergence
(tests/dist_oracle.py) and, for err, against vdqn_td_loss_weighted; the clamp and the tails, the deterministic mode, half batches,
vdqn_dist_moments, vdqn_net_td_forward_dist against the operator and the float64 network oracle, both architectures and the compute
modes, resume, and run_train with DISTRIBUTIONAL."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import dist_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAG_IDS = ["fwd-softplus", "bwd-softplus", "fwd-logsigma", "bwd-logsigma"]


def _dev(inputs):
    return [t.to(DEV) for t in inputs]


def _dist(inputs, kl_backwards=False, log_sigma=False, sigma_min=0.1, dtype=None, use_valid=True, weight=None, with_err=True, clip_rect=1, gamma=0.9,
          deterministic=1, n_cat=5, n_act=3, q_copy=False, discount=None, inv_count=None, with_stats=True):
    """vdqn_td_loss_dist through the raw ABI -> (loss, stats, dq as f32, dq_f32, err, q_copy), all on the CPU."""
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
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, 0, int(use_valid), dtype, 0, deterministic
    a.q_copy = qc.data_ptr() if q_copy else None
    flags = (1 if kl_backwards else 0) | (2 if log_sigma else 0)
    _lib.check(lib.vdqn_td_loss_dist(C.byref(a), weight.data_ptr() if weight is not None else None, err.data_ptr() if with_err else None,
                                     discount.data_ptr() if discount is not None else None, flags, sigma_min,
                                     stats.data_ptr() if with_stats else None, torch.cuda.current_stream().cuda_stream), "vdqn_td_loss_dist")
    torch.cuda.synchronize()
    return loss.cpu(), stats.cpu(), dq.float().cpu(), dq32.cpu(), (err.cpu() if with_err else None), (qc.cpu() if q_copy else None)


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _discount(B, seed=6):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.45


def _rel(x, want):
    return abs(x - want) / max(abs(want), 1e-30)


def _case_gate(inputs, settings, n_cat=5, n_act=3):
    """The dq gate of one case — one generated input — in units of the largest dq element: 4 x the case's restate_f32 deviation, the
    worst over the settings (flags, weights, mask, discount, clip) the test launches on that input, and never above the project's
    operator gate of 1e-6 (tests/test_gpu_iql.py).  The oracle's two statements give it, never the kernel; the factor covers a
    device expf / logf / division that differ from numpy's by an ulp or two each through three chained transcendentals.
    The deviation is taken per case and not per launch: on the smallest inputs (10 to 30 live elements) a single launch's
    restatement happens to land within 2e-9 .. 2e-8 of the oracle, a gate of 9e-9 .. 7e-8 of the largest element, which is less
    than half an ulp of float32 (6e-8) and covers no differing ulp at all; measured on an MI355X, four such launches gave 5.7e-8
    (per-launch gate 9.0e-9), 8.0e-8 (3.7e-8), 9.4e-8 (7.4e-8) and 1.6e-7 (1.4e-7); the other 373 launches of this file stayed
    inside even their per-launch gate, most of them with the restatement's very bits, and the worst of all was 3.5e-7."""
    return min(4 * max(dist_oracle.deviation(inputs, n_cat=n_cat, n_act=n_act, **kw)[0] for kw in settings), 1e-6)


def _check_against_oracle(inputs, got, gate, n_cat=5, n_act=3, **kw):
    """dq within `gate` (_case_gate) of the largest element; every column outside the 2 * n_cat live ones exactly 0; loss and both
    stats within the project's 1e-5 relative, err within 1e-6; every term's L >= 0."""
    loss, stats, _, dq32, err, _ = got
    n = n_cat * n_act
    o = dist_oracle.objective(inputs, n_cat=n_cat, n_act=n_act, **kw)
    r = dist_oracle.restate_f32(inputs, n_cat=n_cat, n_act=n_act, **kw)
    dq_max = o["dq"].abs().max().item()
    e_dq = (dq32[:, :2 * n].double() - o["dq"]).abs().max().item() / dq_max
    e_loss, e_sig, e_z2 = _rel(loss.item(), o["loss"].item()), _rel(stats[0].item(), o["sigma"].item()), _rel(stats[1].item(), o["z2"].item())
    print(f"dq {e_dq:.2e} of the max element (gate {gate:.2e}), loss {e_loss:.2e}, sigma {e_sig:.2e}, z2 {e_z2:.2e} relative")
    assert torch.isfinite(dq32).all() and math.isfinite(loss.item()) and torch.isfinite(stats).all()
    assert e_dq <= gate
    B = dq32.shape[0]
    live = torch.zeros_like(dq32, dtype=torch.bool)
    rows, cols = torch.arange(B).repeat_interleave(n_cat), torch.arange(n_cat).repeat(B) * n_act + inputs[3].repeat_interleave(n_cat)
    live[rows, cols] = True
    live[rows, n + cols] = True
    assert torch.all(dq32[~live] == 0)
    assert e_loss <= 1e-5 and e_sig <= 1e-5 and e_z2 <= 1e-5
    assert o["L"].min().item() >= 0 and r["L"].min() >= 0 and loss.item() >= 0
    if err is not None:
        e_err = (err.double() - o["err"]).abs().max().item() / max(o["err"].abs().max().item(), 1e-30)
        print(f"err {e_err:.2e}")
        assert e_err <= 1e-6
    return o


# ---- 1. the operator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ldq,n_cat,n_act", dist_oracle.OPERATOR_SHAPES, ids=["B96", "B1", "B3", "ldq32", "C2A2", "A1"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
def test_td_loss_dist_vs_f64_oracle(use_valid, weighted, B, ldq, n_cat, n_act):
    """The four flag combinations, scalar and per-sample discount, both deterministic settings; bf16 dq is dq_f32 rounded once."""
    from video_dqn_amd import _lib
    cpu = dist_oracle.inputs(B, 11 + use_valid, ldq=ldq, n_cat=n_cat, n_act=n_act)
    assert dist_oracle.argmax_gap(cpu, n_cat, n_act) >= dist_oracle.ARGMAX_GAP and dist_oracle.clamp_margin(cpu, n_cat, n_act) >= dist_oracle.CLAMP_MARGIN
    if use_valid:
        cpu[6][0, 0] = 1.0  # (B = 1: at least one valid term, so the relative gates have something to divide by)
    w = _weights(B) if weighted else None
    wd = None if w is None else w.to(DEV)
    inputs = _dev(cpu)
    shape = dict(n_cat=n_cat, n_act=n_act)
    discounts = (None, _discount(B))
    gate = _case_gate(cpu, [dict(kl_backwards=kb, log_sigma=ls, use_valid=use_valid, weight=w, discount=disc)
                            for kb, ls in dist_oracle.FLAGS for disc in discounts], **shape)
    for kb, ls in dist_oracle.FLAGS:
        kw = dict(kl_backwards=kb, log_sigma=ls, use_valid=use_valid)
        for disc in discounts:
            dd = None if disc is None else disc.to(DEV)
            for det in (1, 0):
                got = _dist(inputs, weight=wd, deterministic=det, q_copy=True, discount=dd, **kw, **shape)
                _check_against_oracle(cpu, got, gate, weight=w, discount=disc, **kw, **shape)
                assert torch.equal(got[2], got[3])  # the f32 dq and dq_f32 are the same values
                assert torch.equal(got[5], cpu[0][:, :n_cat * n_act])
        bf = _dist(inputs, dtype=_lib.VDQN_BF16, weight=wd, with_err=False, **kw, **shape)
        f32 = _dist(inputs, weight=wd, with_err=False, **kw, **shape)
        assert torch.equal(bf[3], f32[3]) and torch.equal(bf[0], f32[0]) and torch.equal(bf[1], f32[1])
        assert torch.equal(bf[2], bf[3].bfloat16().float())  # one rounding to nearest even, as every other kernel stores bf16


def test_sigma_min_enters_the_floor_and_an_action_outside_the_range_writes_zeros():
    B, ldq, n_cat, n_act, seed = dist_oracle.OPS_CASE
    cpu = dist_oracle.inputs(B, seed)
    settings = [dict(kl_backwards=kb, log_sigma=ls, sigma_min=smin) for smin in (0.01, 1.0) for kb, ls in dist_oracle.FLAGS]
    gate = _case_gate(cpu, settings)
    for kw in settings:
        _check_against_oracle(cpu, _dist(_dev(cpu), **kw), gate, **kw)
    bad = [t.clone() for t in cpu]
    bad[3][1], bad[3][3] = 3, -1
    got = _dist(_dev(bad), q_copy=True)
    assert torch.all(got[3][1] == 0) and torch.all(got[3][3] == 0) and got[4][1].item() == 0 and got[4][3].item() == 0
    keep = [t[[0, 2, 4]].contiguous() for t in cpu]
    ref = _dist(_dev(keep), inv_count=1.0 / (n_cat * B))
    assert torch.equal(got[3][[0, 2, 4]], ref[3]) and torch.equal(got[4][[0, 2, 4]], ref[4]) and torch.equal(got[5], cpu[0][:, :15])
    assert _rel(got[0].item(), ref[0].item()) <= 1e-6


# ---- 2. err is the weighted TD loss's -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kl_backwards,log_sigma", dist_oracle.FLAGS, ids=FLAG_IDS)
def test_err_is_the_weighted_td_loss_err_bit_for_bit(kl_backwards, log_sigma):
    """m is formed as td_error_of forms y, so err carries the bits vdqn_td_loss_weighted writes for the same mean columns: under the
    four clip / discount settings, with the scalar discount and with a per-sample discount that holds the same value."""
    from test_gpu_replay import _td
    from video_dqn_amd import _lib
    B, ldq, n_cat, n_act, seed = dist_oracle.TWIN_CASE
    cpu = dist_oracle.inputs(B, seed)
    inputs = _dev(cpu)
    w = _weights(B, 4)
    four = ((1, 0.9), (0, 0.99), (0, 0.5), (1, 0.5))
    gate = _case_gate(cpu, [dict(kl_backwards=kl_backwards, log_sigma=log_sigma, weight=w, use_valid=uv, clip_rect=c, gamma=g)
                            for uv in (False, True) for c, g in four])
    for use_valid in (False, True):
        for clip_rect, gamma in four:
            kw = dict(clip_rect=clip_rect, gamma=gamma)
            ref = _td(inputs, _lib.VDQN_F32, 0, use_valid, weight=w.to(DEV), **kw)
            got = _dist(inputs, kl_backwards, log_sigma, use_valid=use_valid, weight=w.to(DEV), **kw)
            _check_against_oracle(cpu, got, gate, kl_backwards=kl_backwards, log_sigma=log_sigma, weight=w, use_valid=use_valid, **kw)
            assert torch.equal(got[4], ref[3]), (use_valid, kw)
            per_sample = torch.full((B,), gamma, device=DEV)
            got_sg = _dist(inputs, kl_backwards, log_sigma, use_valid=use_valid, weight=w.to(DEV), discount=per_sample, clip_rect=clip_rect, gamma=0.123)
            assert torch.equal(got_sg[4], ref[3]) and torch.equal(got_sg[3], got[3]) and torch.equal(got_sg[0], got[0]), (use_valid, kw)


# ---- 3. the clamp and the tails -----------------------------------------------------------------------------------------------------
def test_the_clamp_and_the_tails():
    """rho in {-9, 5, 30} under LOG_SIGMA: exactly zero rho gradient, everything finite; rho = +-30 under softplus: finite; terminal
    rows: v == smin2 (seen through the loss of a one-term launch); a prediction a hair off its backup: L stays >= 0."""
    B, ldq, n_cat, n_act, seed = dist_oracle.TAILS_CASE
    cpu = dist_oracle.inputs(B, seed)
    n = n_cat * n_act
    for b, rho in enumerate((-9.0, 5.0, 30.0)):
        cpu[0][b, n:2 * n] = rho
        cpu[2][b + 3, n:2 * n] = rho  # the target's spreads too
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + cpu[3].view(B, 1)
    gate = _case_gate(cpu, [dict(kl_backwards=kb, log_sigma=True, use_valid=False) for kb in (False, True)])
    for kb in (False, True):
        got = _dist(_dev(cpu), kl_backwards=kb, log_sigma=True, use_valid=False)
        _check_against_oracle(cpu, got, gate, kl_backwards=kb, log_sigma=True, use_valid=False)
        rho_grad = got[3].gather(1, n + cols)
        assert torch.all(rho_grad[:3] == 0) and (rho_grad[3:] != 0).all() and (got[3].gather(1, cols) != 0).all()
    soft = [t.clone() for t in cpu]
    soft[0][0, n:2 * n], soft[0][1, n:2 * n], soft[2][3, n:2 * n], soft[2][4, n:2 * n] = 30.0, -30.0, 30.0, -30.0
    gate = _case_gate(soft, [dict(kl_backwards=kb, log_sigma=False, use_valid=False) for kb in (False, True)])
    for kb in (False, True):
        got = _dist(_dev(soft), kl_backwards=kb, log_sigma=False, use_valid=False)
        _check_against_oracle(soft, got, gate, kl_backwards=kb, log_sigma=False, use_valid=False)
    # terminal rows: g = 0, so v is the floor and m = r; one sample, one valid category, the loss is that term's L
    one = [t[:1].clone() for t in dist_oracle.inputs(B, seed)]
    one[5][:] = 1.0
    one[6][:] = 0.0
    one[6][0, 2] = 1.0
    for smin in (0.1, 0.5):
        for kb, ls in dist_oracle.FLAGS:
            got = _dist(_dev(one), kl_backwards=kb, log_sigma=ls, sigma_min=smin, clip_rect=0)
            o = dist_oracle.objective(one, kl_backwards=kb, log_sigma=ls, sigma_min=smin, clip_rect=0)
            smin2 = dist_oracle.smin2_of(smin)
            assert torch.all(o["v"] == smin2)
            mu, s2, d = one[0][0, 2 * n_act + one[3][0]].double(), o["s2"][0, 2], o["d"][0, 2]
            assert d.item() == (mu - one[4][0, 2].double()).item()  # m = r
            want = 0.5 * (math.log(smin2 / s2) + (s2 + d * d) / smin2 - 1) if kb else 0.5 * (math.log(s2 / smin2) + (smin2 + d * d) / s2 - 1)
            assert _rel(got[0].item() * n_cat, float(want)) <= 1e-5  # (inv_count = 1 / n_cat at B = 1)
    # a prediction a hair off its backup: gamma = 1, no clip, no reward, the online arg-max at the data action, Q(s) = Q_target(s') + 1e-4
    near = dist_oracle.inputs(B, seed)
    near[4][:], near[5][:] = 0.0, 0.0
    near[1][:, :n] = -1.0
    near[1][torch.arange(B).repeat_interleave(n_cat), cols.reshape(-1)] = 1.0
    near[0][:, :2 * n] = near[2][:, :2 * n] + 1e-4
    for kb, ls in dist_oracle.FLAGS:
        got = _dist(_dev(near), kl_backwards=kb, log_sigma=ls, gamma=1.0, clip_rect=0, use_valid=False)
        o = dist_oracle.objective(near, kl_backwards=kb, log_sigma=ls, gamma=1.0, clip_rect=0, use_valid=False)
        assert 0 <= got[0].item() <= 1e-6 and o["loss"].item() <= 1e-6 and torch.isfinite(got[3]).all()


# ---- 4. deterministic, and two half batches ------------------------------------------------------------------------------------------
def test_deterministic_is_bit_identical_and_agrees_with_the_atomic_sum():
    B, ldq, n_cat, n_act, seed = dist_oracle.DET_CASE
    inputs = _dev(dist_oracle.inputs(B, seed))
    w = _weights(B).to(DEV)
    for kb, ls in dist_oracle.FLAGS:
        runs = [_dist(inputs, kb, ls, weight=w, deterministic=1) for _ in range(2)]
        for x, y in zip(runs[0][:5], runs[1][:5]):
            assert torch.equal(x, y)
        free = _dist(inputs, kb, ls, weight=w, deterministic=0)
        assert _rel(free[0].item(), runs[0][0].item()) <= 1e-5
        assert _rel(free[1][0].item(), runs[0][1][0].item()) <= 1e-5 and _rel(free[1][1].item(), runs[0][1][1].item()) <= 1e-5
        assert torch.equal(free[3], runs[0][3]) and torch.equal(free[4], runs[0][4])


def test_two_half_batches_at_the_global_inv_count_are_the_full_batch():
    """What two ranks compute: each half at inv_count = 1 / (n_cat * global batch) writes the full batch's dq rows bit for bit, and
    the loss and stats shares sum to the full batch's."""
    B, ldq, n_cat, n_act, seed = dist_oracle.HALVES_CASE
    cpu = dist_oracle.inputs(B, seed)
    w = _weights(B, 9)
    inv = 1.0 / (n_cat * B)
    for kb, ls in dist_oracle.FLAGS:
        full = _dist(_dev(cpu), kb, ls, weight=w.to(DEV), inv_count=inv)
        halves = []
        for lo in (0, B // 2):
            part = [t[lo:lo + B // 2].contiguous() for t in cpu]
            halves.append(_dist(_dev(part), kb, ls, weight=w[lo:lo + B // 2].contiguous().to(DEV), inv_count=inv))
        assert torch.equal(torch.cat([halves[0][3], halves[1][3]]), full[3])
        assert torch.equal(torch.cat([halves[0][4], halves[1][4]]), full[4])
        assert _rel((halves[0][0] + halves[1][0]).item(), full[0].item()) <= 1e-6
        for k in (0, 1):
            assert _rel((halves[0][1][k] + halves[1][1][k]).item(), full[1][k].item()) <= 1e-5


# ---- 5. ops.td_loss_dist and NULL outputs --------------------------------------------------------------------------------------------
def test_ops_td_loss_dist_and_null_outputs():
    """ops.td_loss_dist mirrors the raw entry; weight, err_out, sample_gamma, stats, q_copy and dq_f32 may each be NULL."""
    from video_dqn_amd import _lib, ops
    B, ldq, n_cat, n_act, seed = dist_oracle.OPS_CASE
    cpu = dist_oracle.inputs(B, seed)
    inputs = _dev(cpu)
    for kb, ls in dist_oracle.FLAGS:
        kw = dict(kl_backwards=kb, log_sigma=ls, gamma=0.9, deterministic=True)
        loss, dq, dq32, stats, err, qc = ops.td_loss_dist(*inputs[:6], inputs[6], with_err=True, with_q_copy=True, **kw)
        raw = _dist(inputs, kb, ls, q_copy=True)
        assert torch.equal(loss.cpu(), raw[0]) and torch.equal(stats.cpu(), raw[1]) and torch.equal(dq32.cpu(), raw[3]) and torch.equal(err.cpu(), raw[4])
        assert torch.equal(dq.cpu(), raw[3]) and torch.equal(qc.cpu(), raw[5])
        loss2, dq2, dq32_2, stats2, err2, qc2 = ops.td_loss_dist(*inputs[:6], inputs[6], with_stats=False, with_dq32=False, **kw)
        assert err2 is None and stats2 is None and dq32_2 is None and qc2 is None and torch.equal(loss2, loss) and torch.equal(dq2, dq32)
        w, disc = _weights(B).to(DEV), _discount(B).to(DEV)
        full = ops.td_loss_dist(*inputs[:6], inputs[6], weights=w, discount=disc, with_err=True, **kw)
        raw = _dist(inputs, kb, ls, weight=w, discount=disc)
        assert torch.equal(full[0].cpu(), raw[0]) and torch.equal(full[2].cpu(), raw[3]) and torch.equal(full[4].cpu(), raw[4])
    with pytest.raises(_lib.VdqnError, match="sigma_min"):
        ops.td_loss_dist(*inputs[:6], sigma_min=0.0)
    with pytest.raises(_lib.VdqnError, match="linear"):
        ops.td_loss_dist(*inputs[:6], linear=True)
    with pytest.raises(_lib.VdqnError, match="Huber"):
        ops.td_loss_dist(*inputs[:6], loss_kind="huber")
    with pytest.raises(_lib.VdqnError, match="unknown bits"):
        ops.td_loss_dist(*inputs[:6], flags=4)


# ---- 6. moments ----------------------------------------------------------------------------------------------------------------------
def _spread_rows(seed, in_f, n=15):
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.rand(n, in_f, generator=g) * 2 - 1) * 0.04, (torch.rand(n, generator=g) * 2 - 1) * 0.3


@pytest.mark.parametrize("B,ldq,n_cat,n_act", [dist_oracle.MOMENTS_CASE[:4], (7, 8, 2, 2), (3, 64, 5, 1)], ids=["B9", "C2A2", "A1"])
def test_dist_moments_against_the_oracle_var(B, ldq, n_cat, n_act):
    """The variance within the operator's dq gate — 4 x the distance of the float32 restatement of var from the float64 one, in
    units of the largest element, and never below four half-ulps of that element, which float32 cannot undercut where the
    restatement happens to round like the oracle — the mean the row's own bits; rho beyond the clamp and in the softplus tails included."""
    from video_dqn_amd import ops
    seed = dist_oracle.MOMENTS_CASE[4]
    rows = dist_oracle.inputs(B, seed, ldq=ldq, n_cat=n_cat, n_act=n_act)[0]
    n = n_cat * n_act
    for k, rho in enumerate((-9.0, 5.0, 30.0, -30.0)):
        rows[k % B, n + (k % n)] = rho
    for ls in (False, True):
        for smin in (0.1, 0.01):
            out = ops.dist_moments(rows.to(DEV), n_cat=n_cat, n_act=n_act, log_sigma=ls, sigma_min=smin).cpu()
            assert tuple(out.shape) == (B, n_cat, n_act, 2)
            assert torch.equal(out[..., 0].reshape(B, n), rows[:, :n])
            smin2 = dist_oracle.smin2_of(smin)
            want = dist_oracle.var_of(rows[:, n:2 * n].double(), ls, smin2)
            restated = torch.from_numpy(dist_oracle._var_f32(rows[:, n:2 * n].numpy(), ls, np.float32(smin) * np.float32(smin))[0]).double()
            gate = max(4 * (restated - want).abs().max().item(), 4 * 2.0 ** -24 * want.max().item()) / want.max().item()
            e = (out[..., 1].reshape(B, n).double() - want).abs().max().item() / want.max().item()
            print(f"var {e:.2e} of the max element (gate {gate:.2e})")
            assert e <= gate and out[..., 1].min().item() >= smin2 and torch.isfinite(out).all()


def test_model_distribution_has_the_layout_the_value_map_tool_indexes():
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    B = 3
    for ls, smin in ((False, 0.1), (True, 0.05)):
        model = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=2, distributional=True,
                                      log_sigma=ls, sigma_min=smin)
        model.load_state_dict(synth.make_state_dict(7))  # (no spread.*: the initialised head stays)
        model.eval()
        (tup, _) = synth.make_batch(24, B, 1, structured=True)
        frames = tup[0].to(DEV)
        with torch.no_grad():
            q = model(frames)
        dist = model.distribution(frames)  # (B above max_batch: in chunks)
        assert tuple(q.shape) == (B, 5, 3) and tuple(dist.shape) == (B, 5, 3, 2)
        assert torch.equal(dist[..., 0], q) and dist[..., 1].min().item() >= dist_oracle.smin2_of(smin) and torch.isfinite(dist).all()
        assert dist[..., 1].max().item() > dist[..., 1].min().item()
    plain = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=8)
    with pytest.raises(RuntimeError, match="distributional"):
        plain.distribution(frames)


# ---- 7. the engine -------------------------------------------------------------------------------------------------------------------
def _net(dtype, max_batch, seed=7, extra_capacity=True, deterministic=True, spread_head=True):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, extra_capacity, dtype, max_batch, deterministic=deterministic, spread_head=spread_head)
    net.load_tensors(synth.make_state_dict(seed, extra_capacity=extra_capacity))
    if spread_head:
        sw, sb = _spread_rows(seed, 256 if extra_capacity else 512)
        net.view("spread.weight").copy_(sw)
        net.view("spread.bias").copy_(sb)
        net.mark_dirty()
    return net


def _stepper(dtype, B, deterministic=True, extra_capacity=True, spread_head=True, **kw):
    from video_dqn_amd.engine import TDStepper
    net = _net(dtype, 2 * B, extra_capacity=extra_capacity, deterministic=deterministic, spread_head=spread_head)
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


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_td_forward_dist_writes_the_operators_dq_and_runs_the_target_over_s_next(weighted, B):
    from video_dqn_amd import _lib, ops
    net, stp = _stepper("f32", B, distributional=True, kl_backwards=True, log_sigma=True, sigma_min=0.2)
    target = _net("f32", 2 * B, seed=8)
    target.pack_weights(stp.packed_target)  # a target network of its own
    before, after, kind, act, rew, term = _batch(101, B)
    w = _weights(B, 12).to(DEV) if weighted else None
    err = torch.zeros(B, device=DEV) if weighted else None
    a = stp._args(before, after, kind, act, rew, term, stp._ones, None, w, err)
    st = torch.cuda.current_stream().cuda_stream
    stp.dist_stats.fill_(5.0)  # (cleared beside the loss)
    _lib.check(net.lib.vdqn_net_td_forward_dist(net.handle, C.byref(a), 3, 0.2, stp.dist_stats.data_ptr(), st), "vdqn_net_td_forward_dist")
    torch.cuda.synchronize()
    dq = _dq(net, stp, B)
    qb, qo, qt = _qf(net, stp, B)
    loss, _, dq32, stats, e, _ = ops.td_loss_dist(qb, qo, qt, act, rew, term, None, kl_backwards=True, log_sigma=True, sigma_min=0.2, weights=w,
                                                  with_err=weighted, gamma=0.99, clip_rect=True, deterministic=True)
    assert torch.equal(dq, dq32) and torch.equal(stp.loss, loss) and torch.equal(stp.dist_stats, stats)
    rho = qb[:, 15:30].gather(1, torch.arange(5, device=DEV).view(1, 5) * 3 + act.view(B, 1))
    inside = ((rho > -8) & (rho < 4)).sum().item()  # (LOG_SIGMA: a spread beyond the clamp carries no gradient)
    assert (dq[:, :15] != 0).sum().item() == 5 * B and (dq[:, 15:30] != 0).sum().item() == inside > 0 and torch.all(dq[:, 30:] == 0)
    assert stats[0].item() > 0 and (qb[:, 15:30] != 0).all()
    assert torch.equal(stp.q_before, qb[:, :15])
    if weighted:
        assert torch.equal(err, e)
    # the target workspace holds the target network at s' (`after`)
    q_after = target.forward(after, kind, B)
    moments = target.dist_moments(B, True, 0.2)
    q_s = target.forward(before, kind, B)
    torch.cuda.synchronize()
    assert torch.equal(qt[:, :15], q_after) and not torch.equal(qt[:, :15], q_s)
    assert torch.equal(moments[..., 0].reshape(B, 15), q_after)
    assert torch.equal(moments, ops.dist_moments(qt, log_sigma=True, sigma_min=0.2))
    # the Double-DQN entry on the same spread-head net: zeros in the spread columns and the parent's loss
    _lib.check(net.lib.vdqn_net_td_forward(net.handle, C.byref(a), st), "vdqn_net_td_forward")
    torch.cuda.synchronize()
    dq0 = _dq(net, stp, B)
    qb0, qo0, qt0 = _qf(net, stp, B)
    assert torch.equal(qb0, qb) and torch.equal(qt0, qt)
    ref = ops.td_loss_nstep(qb0, qo0, qt0, act, rew, term, None, discount=torch.full((B,), 0.99, device=DEV), weights=w, with_err=weighted,
                            clip_rect=True, deterministic=True)
    assert torch.all(dq0[:, 15:] == 0) and torch.equal(dq0, ref[2]) and torch.equal(stp.loss, ref[0])


def test_stepper_validation():
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine, TDStepper
    spread = NetEngine(3, 5, 1, True, "f32", 8, spread_head=True)
    plain = NetEngine(3, 5, 1, True, "f32", 8)
    kw = dict(lr=1e-4, gamma=0.99, clip_rect=True)
    for bad in (0.0, 5e-5, 11.0, float("nan")):
        with pytest.raises(_lib.VdqnError, match="sigma_min"):
            TDStepper(spread, 4, distributional=True, sigma_min=bad, **kw)
    with pytest.raises(_lib.VdqnError, match="distributional.*spread head"):
        TDStepper(plain, 4, distributional=True, **kw)
    for more in (dict(kl_backwards=True), dict(log_sigma=True)):
        with pytest.raises(_lib.VdqnError, match="no effect"):
            TDStepper(spread, 4, **kw, **more)
    with pytest.raises(_lib.VdqnError, match="bool"):
        TDStepper(spread, 4, distributional=1, **kw)
    for more in (dict(train_on_ground_truth=True), dict(linear=True), dict(cql_alpha=1.0), dict(mc_floor=True), dict(loss_kind="huber")):
        with pytest.raises(_lib.VdqnError, match="distributional"):
            TDStepper(spread, 4, distributional=True, **kw, **more)
    with pytest.raises(_lib.VdqnError, match="value head"):
        TDStepper(spread, 4, iql_expectile=0.7, **kw)
    with pytest.raises(_lib.VdqnError, match="out of scope"):
        NetEngine(3, 5, 1, True, "f32", 8, value_head=True, spread_head=True)


# ---- 8. one update against the float64 network oracle --------------------------------------------------------------------------------
def _oracle_state_dict(seed):
    """synth's state_dict for the reference class with SIX action columns: oracle row c * 6 + a is the engine's mean row c * 3 + a,
    oracle row c * 6 + 3 + a the engine's spread row 15 + c * 3 + a."""
    from video_dqn_amd import synth
    sd = synth.make_state_dict(seed)
    sw, sb = _spread_rows(seed, 256)
    w6, b6 = torch.zeros(30, 256), torch.zeros(30)
    for c in range(5):
        w6[c * 6:c * 6 + 3], b6[c * 6:c * 6 + 3] = sd["top.4.weight"][c * 3:c * 3 + 3], sd["top.4.bias"][c * 3:c * 3 + 3]
        w6[c * 6 + 3:c * 6 + 6], b6[c * 6 + 3:c * 6 + 6] = sw[c * 3:c * 3 + 3], sb[c * 3:c * 3 + 3]
    sd["top.4.weight"], sd["top.4.bias"] = w6, b6
    return sd


@pytest.mark.parametrize("kl_backwards,log_sigma", [(False, False), (True, True)], ids=["fwd-softplus", "bwd-logsigma"])
def test_dist_step_gradient_matches_f64_oracle(kl_backwards, log_sigma):
    """One update with random importance weights, f32 engine at B = 2: every gradient tensor against the float64 oracle that takes
    the engine's ReLU decisions — the recipe and the gates of tests/test_gpu_iql.py::test_iql_step_gradient_matches_f64_oracle
    (objective within 1e-3 relative; relative L2 <= 1e-3 and max element <= 5e-3 of the tensor's max; more than 60 tensors, spread.*
    among them).  The oracle is the reference class with six action columns (three means, three spreads per category); the objective
    is formed here from its outputs with torch.distributions."""
    from oracle import ref_cpu
    from test_gpu_engine import _EngineReLU, _engine_relu_masks
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B, gamma, smin = 2, 0.99, 0.1
    net = _net("f32", 2 * B, seed=7)
    stp = TDStepper(net, B, lr=1e-4, gamma=gamma, clip_rect=True, distributional=True, kl_backwards=kl_backwards, log_sigma=log_sigma, sigma_min=smin)
    _net("f32", 2 * B, seed=8).pack_weights(stp.packed_target)  # a target network of its own
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05
    err = torch.zeros(B, device=DEV)
    loss = stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV),
                    tup[4].float().to(DEV), weights=w.to(DEV), td_error=err)
    torch.cuda.synchronize()
    grads = stp.grads.cpu()
    masks = _engine_relu_masks(net, stp.acts_online, stp.layout_samples, B)
    model = ref_cpu.HabitatDQNMultiAction(6, 5, extra_capacity=True, panorama=False)
    model.load_state_dict(_oracle_state_dict(7))
    target = ref_cpu.HabitatDQNMultiAction(6, 5, extra_capacity=True, panorama=False)
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
        online_next = model(tup[1].double())[:, :, :3]
        out_t = target(tup[1].double())
    smin2 = dist_oracle.smin2_of(smin)
    idx = act.view(B, 1, 1).expand(B, 5, 1)
    best = online_next.argmax(dim=2, keepdim=True)
    gap = online_next.topk(2, dim=2).values
    mu, s2 = out_s[:, :, :3].gather(2, idx).squeeze(2), dist_oracle.var_of(out_s[:, :, 3:].gather(2, idx).squeeze(2), log_sigma, smin2)
    mt, vt = out_t[:, :, :3].gather(2, best).squeeze(2), dist_oracle.var_of(out_t[:, :, 3:].gather(2, best).squeeze(2), log_sigma, smin2)
    m = (rew + gamma * ((1 - term) * mt)).clamp(0, 1)
    v = ((gamma * (1 - term)) ** 2 * vt).clamp(min=smin2)
    backup, pred = torch.distributions.Normal(m, v.sqrt()), torch.distributions.Normal(mu, s2.sqrt())
    L = torch.distributions.kl_divergence(pred, backup) if kl_backwards else torch.distributions.kl_divergence(backup, pred)
    wd = w.double().view(B, 1)
    objective = (L * wd).mean()
    objective.backward()
    d = (mu - m).detach()
    sigma, z2 = s2.detach().sqrt().mean().item(), (d * d / s2.detach()).mean().item()
    print(f"objective {loss.item():.6f} / {objective.item():.6f}, sigma {stp.dist_stats[0].item():.6f} / {sigma:.6f}, "
          f"z2 {stp.dist_stats[1].item():.6f} / {z2:.6f}, min arg-max gap {(gap[..., 0] - gap[..., 1]).min().item():.2e}")
    assert (gap[..., 0] - gap[..., 1]).min().item() >= 1e-4  # (no tie: the f32 engine and the oracle choose the same action)
    assert abs(loss.item() - objective.item()) <= 1e-3 * abs(objective.item())
    assert abs(stp.dist_stats[0].item() - sigma) <= 1e-3 * sigma and abs(stp.dist_stats[1].item() - z2) <= 1e-3 * z2
    d_ref = d.abs().mean(1)
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

    q_rows = torch.tensor([c * 6 + a for c in range(5) for a in range(3)])
    for name, p in model.named_parameters():
        if p.grad is None:
            continue
        if name.startswith("top.4."):
            kind = name.rsplit(".", 1)[1]
            compare(name, engine_grad(name), p.grad.double()[q_rows])
            compare("spread." + kind, engine_grad("spread." + kind), p.grad.double()[q_rows + 3])
        else:
            compare(name, engine_grad(name), p.grad.double())
    assert len(names) > 60 and "spread.weight" in names and "spread.bias" in names and not bad, bad


# ---- 9. off by default ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stepper_without_the_argument_is_the_stepper_with_distributional_false(dtype):
    """With the key at its default nothing changes: the same entries, launches and bits over three updates on a network without the
    spread head; and a spread-head engine under the plain stepper leaves spread.* with a zero gradient."""
    B = 4
    runs = []
    for kw in (dict(), dict(distributional=False)):
        net, stp = _stepper(dtype, B, spread_head=False, **kw)
        losses = []
        for s in (1, 2, 3):
            losses.append(stp.step(*_batch(300 + s, B)).clone())
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), torch.cat(losses).cpu(), stp.grads.cpu(), stp.exp_avg_sq.cpu()))
        assert stp.dist_stats.abs().sum().item() == 0.0
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    net, stp = _stepper(dtype, B)
    s0 = {n: net.view(n).clone() for n in ("spread.weight", "spread.bias")}
    stp.step(*_batch(301, B))
    torch.cuda.synchronize()
    for name in ("spread.weight", "spread.bias"):
        s = net.slots[name]
        assert torch.all(stp.grads[s.offset:s.offset + s.numel] == 0), name
        assert torch.equal(net.view(name), s0[name])  # (a zero gradient from the first update on: Adam moves nothing)
    t = net.slots["top.4.weight"]
    assert (stp.grads[t.offset:t.offset + t.numel] != 0).any()


# ---- 10. the other architecture and the compute modes --------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_capacity", [True, False], ids=["extra_capacity", "basic"])
@pytest.mark.parametrize("dtype", ["bf16", "f32", "bf16x3"])
def test_both_architectures_and_the_compute_modes(dtype, extra_capacity):
    """Two updates each: finite, the loss and stats the operator's on the engine's own rows, and spread.* moved."""
    from video_dqn_amd import ops
    B = 4
    net, stp = _stepper(dtype, B, extra_capacity=extra_capacity, distributional=True, log_sigma=True)
    p0, s0, b0 = net.params.clone(), net.view("spread.weight").clone(), net.view("spread.bias").clone()
    for seed in (301, 302):
        batch = _batch(seed, B)
        loss = stp.step(*batch)
        torch.cuda.synchronize()
        qb, qo, qt = _qf(net, stp, B)
        ref = ops.td_loss_dist(qb, qo, qt, batch[3], batch[4], batch[5], None, log_sigma=True, gamma=0.99, clip_rect=True, deterministic=True)
        assert torch.equal(loss, ref[0]) and torch.equal(stp.dist_stats, ref[3])
        assert math.isfinite(loss.item()) and loss.item() > 0 and stp.dist_stats[0].item() > 0
    assert torch.isfinite(net.params).all() and torch.isfinite(stp.grads).all() and not torch.equal(net.params, p0)
    assert not torch.equal(net.view("spread.weight"), s0) and not torch.equal(net.view("spread.bias"), b0)


# ---- 11. resume ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.0, 0.01], ids=["hard", "polyak"])
def test_checkpoint_resume_continues_the_uninterrupted_run_bit_for_bit(tau):
    """Six updates in one go against three updates, the trainer's dicts and `spread_head` into a fresh stepper, three more: parameters
    (spread.* included), moments and, under TARGET_TAU, the averaged target with its spread rows, bit-identical."""
    from video_dqn_amd.trainer import head_state, load_head_state, load_optimizer_state_dict, load_target_state_dict, optimizer_state_dict
    B = 2
    kw = dict(distributional=True, kl_backwards=True, target_tau=tau)
    net_u, stp_u = _stepper("f32", B, **kw)
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    net_i, stp_i = _stepper("f32", B, **kw)
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    sd, sh = optimizer_state_dict(stp_i), head_state(stp_i, with_target=tau > 0)
    n_ref = sum(1 for s in net_i.slots.values() if s.kind in (0, 1)) - 2
    assert sd["param_groups"][0]["params"] == list(range(n_ref)) and max(sd["state"]) < n_ref
    assert set(sh) == ({"state_dict", "optimizer_state", "target_state_dict"} if tau > 0 else {"state_dict", "optimizer_state"})
    model_sd = {n: net_i.view(n).clone() for n in net_i.slots if not n.startswith("spread.")}
    target_sd = None
    if tau > 0:  # the reference-shaped target_state_dict: every parameter but the head's
        target_sd = {s.name: stp_i.target_params[s.offset:s.offset + s.numel].view(s.shape).clone()
                     for s in net_i.slots.values() if s.kind in (0, 1) and not s.name.startswith("spread.")}
        w = net_i.slots["spread.weight"]
        assert not torch.equal(stp_i.target_params[w.offset:w.offset + w.numel], net_i.params[w.offset:w.offset + w.numel])
    net_r, stp_r = _stepper("f32", B, **kw)
    net_r.view("spread.weight").zero_()  # (whatever it held: the checkpoint's comes back)
    net_r.load_tensors(model_sd)
    load_optimizer_state_dict(stp_r, sd)
    load_head_state(stp_r, sh)
    if tau > 0:
        stp_r.sync_target()
        load_target_state_dict(stp_r, target_sd, sh["target_state_dict"])
        assert torch.equal(stp_r.target_params[:net_r.trainable_numel], stp_i.target_params[:net_i.trainable_numel])
    stp_r.sample_number = 3
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", net_u.params, net_r.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq), ("stats", stp_u.dist_stats, stp_r.dist_stats)):
        assert torch.equal(x, y), name
    if tau > 0:
        assert torch.equal(stp_u.target_params, stp_r.target_params)
    assert not torch.equal(net_u.view("spread.weight"), net_i.view("spread.weight"))


# ---- 12. run_train -------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    path = str(tmp_path_factory.mktemp("dist") / "shards")
    _synthetic_shards(path)
    return path


@pytest.mark.parametrize("keys,flags", [("KL_BACKWARDS: True\n", 1), ("LOG_SIGMA: True\nDIST_SIGMA_MIN: 0.05\n", 2),
                                        ("N_STEP: 3\nPRIORITIZED_REPLAY: True\nTARGET_TAU: 0.01\n", 0)], ids=["kl_backwards", "log_sigma", "nstep_per_tau"])
def test_run_train_with_distributional(tmp_path, shards, keys, flags):
    """100 updates on the resident synthetic store with a scalar writer: both scalars are written at update 100 (with the values of
    update 99, one update late like the loss) and finite; the checkpoint has the reference's three keys in the reference's shapes plus
    spread_head; load_model_number returns a model whose distribution() works; a resumed run says what it restored."""
    from video_dqn_amd.config import ExperimentConfig, JsonlWriter
    from video_dqn_amd.model import load_model_number
    from video_dqn_amd.trainer import run_train
    _write_cfg(tmp_path / "a", shards, 100, "DISTRIBUTIONAL: True\n" + keys)
    cfg = ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=True)
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    logs = []
    model, stepper, running = run_train(cfg, log=lambda *a: logs.append(" ".join(map(str, a))))
    cfg.writer.close()
    assert np.isfinite(running) and stepper.distributional and stepper.dist_flags == flags and model.distributional
    assert any(l.startswith("distributional Q-learning: a Gaussian") for l in logs)
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    sigma = [r for r in rows if r["tag"] == "dist_sigma/train"]
    z2 = [r for r in rows if r["tag"] == "dist_z2/train"]
    assert len(sigma) == 1 and len(z2) == 1 and sigma[0]["step"] == 99 and z2[0]["step"] == 99
    print(f"dist_sigma/train {sigma[0]['value']:.6f}, dist_z2/train {z2[0]['value']:.6f}")
    assert sigma[0]["value"] >= stepper.sigma_min and math.isfinite(sigma[0]["value"]) and math.isfinite(z2[0]["value"]) and z2[0]["value"] >= 0
    assert any(r["tag"] == "avg_q_loss/train" and r["step"] == 100 for r in rows)
    snap = torch.load(tmp_path / "a" / "models" / "sample96.torch", map_location="cpu")
    tau = "TARGET_TAU" in keys
    assert set(snap) == {"sample_number", "model_state_dict", "optimizer_state_dict", "spread_head"} | ({"replay_state", "target_state_dict"} if tau else set())
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_state_dict.json")) as f:
        ref = json.load(f)["ec1_pano0"]
    for key in ("model_state_dict",) + (("target_state_dict",) if tau else ()):
        assert list(snap[key]) == ref["keys"] and [list(v.shape) for v in snap[key].values()] == ref["shapes"], key
    assert max(snap["optimizer_state_dict"]["state"]) < len(ref["params"])
    assert set(snap["spread_head"]["state_dict"]) == {"spread.weight", "spread.bias"}
    assert snap["spread_head"]["optimizer_state"]["spread.weight"]["step"] == 96
    assert ("target_state_dict" in snap["spread_head"]) == tau
    # the greedy policy and the distribution load from the file
    loaded = load_model_number(ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=False), 96)
    frames = torch.zeros(2, 3, 224, 224)
    assert tuple(loaded(frames).shape) == (2, 5, 3) and torch.equal(loaded.engine.view("top.4.weight").cpu(), snap["model_state_dict"]["top.4.weight"])
    assert torch.equal(loaded.engine.view("spread.weight").cpu(), snap["spread_head"]["state_dict"]["spread.weight"])
    dist = loaded.distribution(frames)
    assert tuple(dist.shape) == (2, 5, 3, 2) and torch.equal(dist[..., 0], loaded(frames)) and dist[..., 1].min().item() >= stepper.sigma_min ** 2 * 0.999
    if tau:  # resumed: the head, its moments and the target's spread rows come back; without the key the run says so
        _write_cfg(tmp_path / "r", shards, 98, "DISTRIBUTIONAL: True\n" + keys)
        (tmp_path / "r" / "models").mkdir()
        torch.save(snap, tmp_path / "r" / "models" / "sample96.torch")
        logs = []
        m, s, _ = run_train(ExperimentConfig(str(tmp_path / "r"), device=DEV, tensorboard=False, resume=True), resume_from=96,
                            log=lambda *a: logs.append(" ".join(map(str, a))))
        assert s.adam_step == 97 and any("the spread head and its Adam moments restored" in l for l in logs)
        assert any("target weights restored from the checkpoint" in l for l in logs)
        old = {k: v for k, v in snap.items() if k != "spread_head"}
        torch.save(old, tmp_path / "r" / "models" / "sample96.torch")
        logs = []
        run_train(ExperimentConfig(str(tmp_path / "r"), device=DEV, tensorboard=False, resume=True), resume_from=96,
                  log=lambda *a: logs.append(" ".join(map(str, a))))
        assert any("the checkpoint has no spread_head" in l for l in logs)
