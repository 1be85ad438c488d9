"""Monte-Carlo returns on the GPU: vdqn_mc_returns against the numpy float32 restatement bit for bit, vdqn_td_loss_mc against the
float64 autograd oracle (tests/mc_oracle.py) and, with a table of -inf, against every existing TD-loss entry bit for bit,
TDStepper(mc_floor=, cql_calibrated=) and run_train with MC_RETURN_FLOOR / CQL_CALIBRATED against a manual loop."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

import cql_oracle
import mc_oracle
import nstep_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR, CAL = mc_oracle.FLOOR, mc_oracle.CALIBRATED


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fractional", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("n_cat", [1, 5])
@pytest.mark.parametrize("N", [1, 7, 300, 1025])
def test_mc_returns_equal_the_f32_oracle_bit_for_bit(N, n_cat, fractional):
    """Every gamma and R in {1, 2, 3, 12} (R >= 2 is where a round that updated in place would show; N = 1025 spans block and wave
    edges).  The workspace and the output are pre-filled with 0x7f bytes; rew, term and next_row are unchanged; two runs agree."""
    from video_dqn_amd import _lib, ops
    lib = _lib.load()
    next_row, rew, term = mc_oracle.tables(N, n_cat, 31 + N + n_cat + int(fractional), fractional)
    d_next, d_rew, d_term = (torch.from_numpy(x).to(DEV) for x in (next_row, rew, term))
    ws_bytes = lib.vdqn_mc_returns_workspace_bytes(N, n_cat)
    assert ws_bytes == 4 * (2 * N + 3 * N * n_cat)
    for gamma in (0.9, 0.99, 1.0):
        for rounds in (1, 2, 3, 12):
            want = mc_oracle.returns_f32(next_row, rew, term, gamma, rounds)
            runs = []
            for _ in range(2):
                ws = torch.full((ws_bytes,), 0x7f, dtype=torch.uint8, device=DEV)
                out = torch.full((N, n_cat), 0x7f, dtype=torch.uint8, device=DEV).repeat_interleave(4, 1).view(torch.float32)
                G = ops.mc_returns(d_next, d_rew, d_term, gamma=gamma, rounds=rounds, out=out, workspace=ws)
                torch.cuda.synchronize()
                runs.append(G.cpu().numpy())
            assert runs[0].tobytes() == want.tobytes(), (gamma, rounds, np.abs(runs[0] - want).max())
            assert runs[1].tobytes() == runs[0].tobytes()
    assert np.array_equal(d_next.cpu().numpy(), next_row) and np.array_equal(d_rew.cpu().numpy(), rew) and np.array_equal(d_term.cpu().numpy(), term)


def test_return_table_class_and_default_rounds():
    from video_dqn_amd.mcreturn import ReturnTable, rounds_for
    next_row, rew, term = mc_oracle.tables(300, 5, 3)
    tab = ReturnTable(next_row, torch.from_numpy(rew).to(DEV), torch.from_numpy(term).to(DEV), 0.99, DEV)
    assert tab.rounds == rounds_for(0.99, 300) == 9 and tab.G.shape == (300, 5)
    want = mc_oracle.returns_f32(next_row, rew, term, 0.99, 9)
    assert tab.G.cpu().numpy().tobytes() == want.tobytes()
    mx, mean = tab.summary()
    assert mx == float(want.max()) and abs(mean - want.astype(np.float64).mean()) <= 1e-12
    with pytest.raises(ValueError, match="ReturnTable"):
        ReturnTable(next_row[:10], torch.from_numpy(rew).to(DEV), torch.from_numpy(term).to(DEV), 0.99, DEV)


# ---- 2. bad arguments -----------------------------------------------------------------------------------------------------------------
def test_mc_returns_bad_arguments_fail_by_name_and_write_nothing():
    from video_dqn_amd import _lib, ops
    lib = _lib.load()
    next_row, rew, term = mc_oracle.tables(300, 5, 3)
    d_next, d_rew, d_term = (torch.from_numpy(x).to(DEV) for x in (next_row, rew, term))
    out = torch.full((300, 5), 7.0, device=DEV)
    need = lib.vdqn_mc_returns_workspace_bytes(300, 5)
    for kw, word in ((dict(rounds=0), "rounds 0"), (dict(rounds=32), "rounds 32"), (dict(gamma=float("nan")), "gamma"),
                     (dict(workspace=torch.zeros(need - 1, dtype=torch.uint8, device=DEV)), "workspace")):
        args = dict(gamma=0.99, rounds=4)
        args.update(kw)
        with pytest.raises(_lib.VdqnError, match="vdqn_mc_returns: .*" + word):
            ops.mc_returns(d_next, d_rew, d_term, out=out, **args)
    out9 = torch.full((300, 9), 7.0, device=DEV)
    with pytest.raises(_lib.VdqnError, match="vdqn_mc_returns: n_cat 9"):
        ops.mc_returns(d_next, torch.zeros(300, 9, device=DEV), torch.zeros(300, 9, device=DEV), gamma=0.99, rounds=4, out=out9)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((out9 == 7.0).all())


# ---- 3. the loss launch against the float64 oracle ------------------------------------------------------------------------------------
def _call(inputs, entry, *, G=None, flags=0, alpha=0.0, weight=None, with_err=False, disc=None, bf16=False, loss_kind=0, use_valid=True,
          clip_rect=1, gamma=0.9, deterministic=1, linear=0, with_stats=True):
    """One of the TD-loss entries through the raw ABI -> dict(loss, pen, dq (as f32), dq32, err, stats), all on the CPU."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    n_cat, n_act = rew.shape[1], 3
    loss, pen, stats = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV), torch.zeros(2, device=DEV)
    dq = torch.full((B, ldq), 7.0, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
    dq32 = torch.full((B, ldq), 7.0, device=DEV)
    err = torch.full((B,), -1.0, device=DEV) if with_err else None
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = qb.data_ptr(), qo.data_ptr(), qt.data_ptr()
    a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
    a.loss, a.dq, a.dq_f32 = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr()
    a.batch, a.n_cat, a.n_act, a.ldq = B, n_cat, n_act, ldq
    a.gamma, a.inv_count = gamma, 1.0 / (n_cat * B)
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = (clip_rect, linear, int(use_valid),
                                                                                 _lib.VDQN_BF16 if bf16 else _lib.VDQN_F32, loss_kind, deterministic)
    p = lambda t: t.data_ptr() if t is not None else None
    st = torch.cuda.current_stream().cuda_stream
    pen_p = pen.data_ptr() if alpha > 0 else None
    if entry == "mc":
        rc = lib.vdqn_td_loss_mc(C.byref(a), p(weight), p(err), alpha, pen_p, p(disc), p(G), flags, stats.data_ptr() if with_stats else None, st)
    elif entry == "nstep":
        rc = lib.vdqn_td_loss_nstep(C.byref(a), p(weight), p(err), alpha, pen_p, p(disc), st)
    elif entry == "cql":
        rc = lib.vdqn_td_loss_cql(C.byref(a), p(weight), p(err), alpha, pen_p, st)
    elif entry == "weighted":
        rc = lib.vdqn_td_loss_weighted(C.byref(a), p(weight), p(err), st)
    else:
        rc = lib.vdqn_td_loss(C.byref(a), st)
    _lib.check(rc, "vdqn_td_loss_" + entry)
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), pen=pen.cpu(), dq=dq.float().cpu(), dq32=dq32.cpu(), err=err.cpu() if with_err else None, stats=stats.cpu())


def _weights(B, seed=3):
    return torch.rand(B, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1


def _discount(B, seed=9):
    return (0.99 ** torch.randint(1, 4, (B,), generator=torch.Generator().manual_seed(seed)).double()).float()


def _rel(got, want):
    return abs(got - want) / abs(want)


MODES = {"plain": dict(alpha=0.0, weighted=False), "weighted": dict(alpha=0.0, weighted=True), "cql": dict(alpha=1.0, weighted=True)}
MODE_FLAGS = [("plain", FLOOR), ("weighted", FLOOR), ("cql", FLOOR), ("cql", CAL), ("cql", FLOOR | CAL)]


@pytest.mark.parametrize("mode,flags", MODE_FLAGS, ids=[f"{m}-flags{f}" for m, f in MODE_FLAGS])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_td_loss_mc_vs_f64_oracle(B, mode, flags):
    """test_gpu_cql.py's operator gates — every dq element within 1e-6 of the largest, padding exactly 0, loss / penalty / stats within
    1e-5 relative, err within 1e-6 — over scalar / per-sample discount x both loss kinds x rect clip on / off x valid on / off, each
    under both deterministic settings and with f32 and bf16 dq (the bf16 dq is dq_f32 rounded once).  The oracle leaves no element
    out; on it, the floor raises between a quarter and three quarters of the targets, and no |y - G| is below 1e-4 except the ties
    built from exactly representable values, which are there, as are Q(s, a) == G ties."""
    alpha, weighted = MODES[mode]["alpha"], MODES[mode]["weighted"]
    w = _weights(B) if weighted else None
    worst = dict(dq=0.0, loss=0.0, pen=0.0, s0=0.0, s1=0.0, err=0.0)
    for per_sample in (False, True):
        disc = _discount(B) if per_sample else None
        cpu, G, tie_y, tie_q = mc_oracle.loss_inputs(B, 40 + B, gamma=0.9, discount=disc)
        cpu[6][0, 0] = 1.0  # (B = 1: at least one valid term for the relative gates)
        inputs = [t.to(DEV) for t in cpu]
        dev = dict(G=G.to(DEV), weight=None if w is None else w.to(DEV), disc=None if disc is None else disc.to(DEV))
        for loss_kind in (0, 1):
            for clip_rect in (1, 0):
                for use_valid in (False, True):
                    kw = dict(loss_kind=loss_kind, clip_rect=clip_rect, use_valid=use_valid)
                    o = mc_oracle.objective(cpu, alpha, G, flags, weight=w, gamma=0.9, discount=disc, **kw)
                    share = o["raised"].double().mean().item()
                    assert 0.25 <= share <= 0.75, share
                    gap = (o["y_pre"] - G.double()).abs()
                    assert bool(((gap >= 1e-4) | tie_y).all()) and bool((gap[tie_y] == 0).all()) and tie_y.any() and tie_q.any()
                    assert bool((cpu[0][:, :15].reshape(B, 5, 3)[tie_q] == G.unsqueeze(2).expand(B, 5, 3)[tie_q]).all())
                    dq_max = o["dq"].abs().max().item()
                    for det in (1, 0):
                        for bf16 in (False, True):
                            got = _call(inputs, "mc", flags=flags, alpha=alpha, with_err=weighted, bf16=bf16, deterministic=det, **dev, **kw)
                            assert torch.isfinite(got["dq32"]).all()
                            assert torch.all(got["dq32"][:, 15:] == 0) and torch.all(got["dq"][:, 15:] == 0)
                            if bf16:
                                assert torch.equal(got["dq"], got["dq32"].bfloat16().float())
                            else:
                                assert torch.equal(got["dq"], got["dq32"])
                            worst["dq"] = max(worst["dq"], (got["dq32"][:, :15].double() - o["dq"]).abs().max().item() / dq_max)
                            worst["loss"] = max(worst["loss"], _rel(got["loss"].item(), o["loss"].item()))
                            if alpha > 0:
                                worst["pen"] = max(worst["pen"], _rel(got["pen"].item(), o["penalty"].item()))
                            worst["s0"] = max(worst["s0"], _rel(got["stats"][0].item(), o["stats"][0].item()))
                            worst["s1"] = max(worst["s1"], _rel(got["stats"][1].item(), o["stats"][1].item()))
                            if weighted:
                                worst["err"] = max(worst["err"], (got["err"].double() - o["err"]).abs().max().item() / o["err"].abs().max().item())
    print(f"B {B} {mode} flags {flags}: worst " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["dq"] <= 1e-6 and worst["err"] <= 1e-6
    assert worst["loss"] <= 1e-5 and worst["pen"] <= 1e-5 and worst["s0"] <= 1e-5 and worst["s1"] <= 1e-5


def test_floor_and_calibration_change_what_they_should():
    """Against the launch without the table: the floor moves exactly the taken-action columns of raised targets (and only while the
    clip leaves room), the calibrated penalty is never below the plain one, and mc_stats NULL is accepted."""
    B = 65
    cpu, G, tie_y, _ = mc_oracle.loss_inputs(B, 7)
    inputs = [t.to(DEV) for t in cpu]
    base = _call(inputs, "cql", alpha=1.0, with_err=True, clip_rect=0)
    fl = _call(inputs, "mc", G=G.to(DEV), flags=FLOOR, alpha=1.0, with_err=True, clip_rect=0, with_stats=False)
    o = mc_oracle.objective(cpu, 1.0, G, FLOOR, clip_rect=0)
    changed = (fl["dq32"][:, :15] != base["dq32"][:, :15]).reshape(B, 5, 3)
    onehot = torch.zeros(B, 5, 3, dtype=torch.bool)
    onehot[torch.arange(B), :, cpu[3]] = True
    want = onehot & (o["raised"] & (cpu[6] > 0)).unsqueeze(2)
    assert torch.equal(changed, want) and changed.any()
    assert torch.equal(fl["pen"], base["pen"]) and fl["stats"].abs().sum().item() == 0.0
    cal = _call(inputs, "mc", G=G.to(DEV), flags=CAL, alpha=1.0, clip_rect=0)
    assert cal["pen"].item() > base["pen"].item()


# ---- 4. the existing entries keep their bits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("per_sample", [False, True], ids=["gamma", "discount"])
@pytest.mark.parametrize("mode", ["plain", "weighted", "cql"])
def test_minus_inf_table_gives_the_existing_entry_bit_for_bit(mode, per_sample, bf16):
    """mc_return = -inf under every legal flag set: loss, dq, dq_f32, err and penalty are the matching existing entry's bits (both
    loss kinds, valid on / off, the deterministic launch; in the atomic launch everything but the order-dependent sums), and
    mc_stats[0] stays 0."""
    B = 65
    alpha, weighted = MODES[mode]["alpha"], MODES[mode]["weighted"]
    cpu = cql_oracle.td_inputs(B, 23)
    inputs = [t.to(DEV) for t in cpu]
    w = _weights(B).to(DEV) if weighted else None
    disc = _discount(B).to(DEV) if per_sample else None
    G = torch.full((B, 5), -float("inf"), device=DEV)
    entry = "nstep" if per_sample else mode
    for loss_kind in (0, 1):
        for use_valid in (False, True):
            for det in (1, 0):
                kw = dict(alpha=alpha, weight=w, with_err=weighted, disc=disc, bf16=bf16, loss_kind=loss_kind, use_valid=use_valid, deterministic=det)
                ref = _call(inputs, entry, **kw)
                for flags in ((FLOOR, CAL, FLOOR | CAL) if mode == "cql" else (FLOOR,)):
                    got = _call(inputs, "mc", G=G, flags=flags, **kw)
                    assert torch.equal(got["dq"], ref["dq"]) and torch.equal(got["dq32"], ref["dq32"]), (flags, loss_kind, use_valid, det)
                    if weighted:
                        assert torch.equal(got["err"], ref["err"])
                    if det:
                        assert torch.equal(got["loss"], ref["loss"]) and torch.equal(got["pen"], ref["pen"])
                    assert got["stats"][0].item() == 0.0


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_ops_td_loss_mc_and_refusals_by_name():
    from video_dqn_amd import _lib, ops
    cpu, G, _, _ = mc_oracle.loss_inputs(5, 2)
    inputs = [t.to(DEV) for t in cpu]
    Gd = G.to(DEV)
    loss, dq, dq32, pen, err, stats = ops.td_loss_mc(*inputs[:6], inputs[6], mc_return=Gd, floor=True, calibrated=True, cql_alpha=1.5, gamma=0.9,
                                                     with_err=True, weights=_weights(5).to(DEV), deterministic=True)
    raw = _call(inputs, "mc", G=Gd, flags=3, alpha=1.5, weight=_weights(5).to(DEV), with_err=True)
    assert torch.equal(loss.cpu(), raw["loss"]) and torch.equal(pen.cpu(), raw["pen"]) and torch.equal(dq32.cpu(), raw["dq32"])
    assert torch.equal(err.cpu(), raw["err"]) and torch.equal(stats.cpu(), raw["stats"]) and torch.equal(dq.cpu(), raw["dq32"])
    for kw, word in ((dict(mc_flags=0), "mc_flags is 0"), (dict(mc_flags=4, cql_alpha=1.0), "unknown bits"),
                     (dict(calibrated=True), "calibrated.*cql_alpha"), (dict(floor=True, linear=True), "linear")):
        with pytest.raises(_lib.VdqnError, match="vdqn_td_loss_mc: .*" + word):
            ops.td_loss_mc(*inputs[:6], mc_return=Gd, **kw)
    with pytest.raises(_lib.VdqnError, match="vdqn_td_loss_mc: mc_return is NULL"):
        ops.td_loss_mc(*inputs[:6], mc_return=None, floor=True)
    with pytest.raises(ValueError, match="mc_return"):
        ops.td_loss_mc(*inputs[:6], mc_return=Gd[:4].contiguous(), floor=True)


# ---- 6. the stepper -------------------------------------------------------------------------------------------------------------------
def test_step_with_a_minus_inf_table_is_the_plain_step():
    """The small f32 extra_capacity net at B = 4, deterministic: two updates of step(mc_return = -inf) with mc_floor leave the
    parameters, moments, loss and gradient of the plain step bit for bit; the same with the penalty on and both switches."""
    from test_gpu_cql import _batch, _stepper
    B = 4
    ninf = torch.full((B, 5), -float("inf"), device=DEV)
    for base, on in ((dict(), dict(mc_floor=True)), (dict(cql_alpha=1.0), dict(cql_alpha=1.0, mc_floor=True, cql_calibrated=True))):
        runs = []
        for kw in (base, on):
            net, stp = _stepper("f32", B, **kw)
            losses = [stp.step(*_batch(300 + s, B), mc_return=(ninf if "mc_floor" in kw else None)).clone() for s in (1, 2)]
            torch.cuda.synchronize()
            runs.append((net.params.cpu(), stp.exp_avg.cpu(), stp.exp_avg_sq.cpu(), torch.cat(losses).cpu(), stp.grads.cpu(), stp.cql_penalty.cpu()))
            assert stp.mc_stats[0].item() == 0.0
        for x, y in zip(*runs):
            assert torch.equal(x, y)


def _table_with_margins(qb, qo, qt, act, rew, term, gamma, seed):
    """G [B, 5] at least 0.02 away from every Q(s, .) of its category and from the unclipped target, about half of them above it:
    the f32 engine and the float64 oracle (Q within 1e-3 relative) then take the same side of every comparison."""
    B = qb.shape[0]
    q3, qo3, qt3 = (t[:, :15].reshape(B, 5, 3).double().cpu() for t in (qb, qo, qt))
    y_pre = rew.double().cpu() + gamma * qt3.gather(2, qo3.argmax(2, keepdim=True)).squeeze(2) * (1 - term.double().cpu())
    g = torch.Generator().manual_seed(seed)
    G = torch.zeros(B, 5, dtype=torch.float64)
    for b in range(B):
        for c in range(5):
            sign = 1.0 if (b + c) % 2 else -1.0
            for _ in range(1000):
                cand = y_pre[b, c] + sign * (0.03 + 0.3 * torch.rand(1, generator=g).item())
                if (q3[b, c] - cand).abs().min().item() >= 0.02:
                    break
            else:
                raise AssertionError("no value with the margins found")
            G[b, c] = cand
    return G.float()


def test_step_with_a_real_table_matches_the_f64_oracles():
    """One update with cql_alpha = 1, both switches and importance weights on the f32 engine at B = 8.  The reported loss, cql_penalty
    and mc_stats against mc_oracle.objective on the step's own Q rows (test_gpu_cql.py's stepper gate, 1e-3 relative), and every
    gradient tensor against the float64 network oracle that takes the engine's ReLU decisions
    (test_weighted_step_gradient_matches_f64_oracle's gates: relative L2 <= 1e-3, max element <= 5e-3 of the tensor's max, more
    than 60 tensors)."""
    from oracle import ref_cpu
    from test_gpu_cql import _qf
    from test_gpu_engine import _EngineReLU, _engine_relu_masks, make_engine
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B, alpha, gamma = 8, 1.0, 0.99
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    batch = (tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV), tup[4].float().to(DEV))
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05

    def build():
        net = make_engine("f32", seed=7, max_batch=2 * B)
        stp = TDStepper(net, B, lr=1e-4, gamma=gamma, clip_rect=True, cql_alpha=alpha, mc_floor=True, cql_calibrated=True)
        make_engine("f32", seed=8, max_batch=2 * B).pack_weights(stp.packed_target)  # a target network of its own
        return net, stp

    # a first stepper shows the engine's Q rows (they do not depend on the table): the table is drawn around them
    net, stp = build()
    stp.step(*batch, weights=w.to(DEV), td_error=torch.zeros(B, device=DEV), mc_return=torch.full((B, 5), -float("inf"), device=DEV))
    torch.cuda.synchronize()
    qb, qo, qt = (t.clone() for t in _qf(net, stp, B))
    G = _table_with_margins(qb, qo, qt, batch[3], batch[4], batch[5], gamma, 5)

    net, stp = build()
    err = torch.zeros(B, device=DEV)
    loss = stp.step(*batch, weights=w.to(DEV), td_error=err, mc_return=G.to(DEV))
    torch.cuda.synchronize()
    qb2, qo2, qt2 = _qf(net, stp, B)
    assert torch.equal(qb2, qb) and torch.equal(stp.q_before, qb[:, :15])
    ones = torch.ones(B, 5)
    o = mc_oracle.objective([qb.cpu(), qo.cpu(), qt.cpu(), batch[3].cpu(), batch[4].cpu(), batch[5].cpu(), ones], alpha, G, FLOOR | CAL,
                            weight=w, use_valid=False, gamma=gamma, clip_rect=1)
    print(f"loss {loss.item():.6f} / {o['loss'].item():.6f}, penalty {stp.cql_penalty.item():.6f} / {o['penalty'].item():.6f}, "
          f"mc_stats {stp.mc_stats.tolist()} / {o['stats'].tolist()}")
    assert 0.25 <= o["raised"].double().mean().item() <= 0.75
    assert _rel(loss.item(), o["loss"].item()) <= 1e-3 and _rel(stp.cql_penalty.item(), o["penalty"].item()) <= 1e-3
    assert _rel(stp.mc_stats[0].item(), o["stats"][0].item()) <= 1e-3 and _rel(stp.mc_stats[1].item(), o["stats"][1].item()) <= 1e-3
    assert (err.cpu().double() - o["err"]).abs().max().item() <= 1e-3 * o["err"].abs().max().item()

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
    Gd, wd = G.double(), w.double().view(B, 1)
    y_pre = tup[3].double() + gamma * d["Q_a"]
    assert bool(((y_pre - Gd).abs() >= 0.01).all()) and bool(((d["before_values"].detach() - Gd.unsqueeze(2)).abs() >= 0.01).all())
    y = torch.maximum(y_pre, Gd).clamp(0, 1).detach()
    bv = d["before_values"]
    pen = torch.logsumexp(torch.where(bv >= Gd.unsqueeze(2), bv, Gd.unsqueeze(2).expand_as(bv)), 2) - d["Q_b"]
    objective = ((0.5 * (d["Q_b"] - y) ** 2) * wd).mean() + alpha * (pen * wd).mean()
    objective.backward()
    assert _rel(loss.item(), objective.item()) <= 1e-3
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


def test_stepper_refusals_by_name():
    from test_gpu_cql import _batch, _stepper
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine, TDStepper
    B = 4
    net = NetEngine(3, 5, 1, True, "f32", 2 * B)
    with pytest.raises(_lib.VdqnError, match="cql_calibrated needs cql_alpha"):
        TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, cql_calibrated=True)
    for kw in (dict(train_on_ground_truth=True), dict(linear=True)):
        with pytest.raises(_lib.VdqnError, match="mc_floor / cql_calibrated"):
            TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, mc_floor=True, **kw)
    _, on = _stepper("f32", B, mc_floor=True)
    _, off = _stepper("f32", B)
    batch = _batch(301, B)
    G = torch.zeros(B, 5, device=DEV)
    with pytest.raises(_lib.VdqnError, match="mc_return is required exactly when"):
        on.step(*batch)
    with pytest.raises(_lib.VdqnError, match="mc_return is required exactly when"):
        off.step(*batch, mc_return=G)
    for bad in (G[:3].contiguous(), G.double(), torch.zeros(B, 4, device=DEV), G.cpu(), torch.zeros(B, 10, device=DEV)[:, ::2]):
        with pytest.raises(_lib.VdqnError, match="mc_return must be"):
            on.step(*batch, mc_return=bad)
    assert on.sample_number == 0 and on.adam_step == 0  # nothing ran


# ---- 7. run_train ---------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def _run(tmp_path, tag, shards, steps, extra="", max_steps=None, tensorboard=False):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    _write_cfg(tmp_path / tag, shards, steps, extra)
    logs = []
    cfg = ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=tensorboard)
    model, stepper, _ = run_train(cfg, max_steps=max_steps, log=lambda *a: logs.append(" ".join(map(str, a))))
    torch.cuda.synchronize()
    return model, stepper, logs, cfg


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    root = str(tmp_path_factory.mktemp("mcreturn") / "shards")
    _synthetic_shards(root, n_samples=96)  # 24 frames, 96 rows, random frame indices: cycles and rows without a successor
    return root


WAYS = {"floor": "MC_RETURN_FLOOR: True\n", "calibrated": "CQL_CALIBRATED: True\nCQL_ALPHA: 1.0\n",
        "both_nstep": "MC_RETURN_FLOOR: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 1.0\nN_STEP: 3\n",
        "both_per": "MC_RETURN_FLOOR: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 1.0\nPRIORITIZED_REPLAY: True\n",
        # weight, discount and G all present at once
        "both_nstep_per": "MC_RETURN_FLOOR: True\nCQL_CALIBRATED: True\nCQL_ALPHA: 1.0\nN_STEP: 3\nPRIORITIZED_REPLAY: True\n"}


@pytest.mark.parametrize("way", list(WAYS))
def test_run_train_equals_a_manual_loop_with_the_host_oracle(tmp_path, shards, way):
    """Six updates of run_train against a manual loop on a second, identically seeded stepper (run_train with zero updates builds
    it): the rows the same seed draws, G built on the host by the float32 oracle and gathered at the SAMPLED rows (with N_STEP 3 the
    chains walked by nstep_oracle, `after` from each chain's last row), TDStepper.step fed with them.  Parameters, moments, loss and,
    with PRIORITIZED_REPLAY, the priority table end bit-identical."""
    from video_dqn_amd.mcreturn import rounds_for
    from video_dqn_amd.nstep import successors
    from video_dqn_amd.shards import DeviceFrameStore
    extra, per, n_step = WAYS[way], "PRIORITIZED" in WAYS[way], 3 if "N_STEP" in WAYS[way] else 1
    model, stepper, logs, _ = _run(tmp_path, "auto", shards, 6, extra)
    assert stepper.adam_step == 6 and stepper.returns is not None and (stepper.nstep is not None) == (n_step > 1)
    line = [l for l in logs if l.startswith("Monte-Carlo returns: 96 rows, 7 rounds")]
    assert len(line) == 1 and "table max" in line[0] and "mean" in line[0]

    m_model, m_stepper, _, _ = _run(tmp_path, "manual", shards, 6, extra, max_steps=0)  # the same start; no update has run
    assert m_stepper.adam_step == 0
    store = DeviceFrameStore(shards, DEV, one_action=True, inverse_actions=True)
    index = np.load(os.path.join(shards, "index.npz"))
    next_row = successors(index["before"][:, 0], index["after"][:, 0])
    rew, term = store.rew.cpu().numpy(), store.term.cpu().numpy()
    assert rounds_for(0.99, 96) == 7
    G = mc_oracle.returns_f32(next_row, rew, term, 0.99, 7)
    assert stepper.returns.G.cpu().numpy().tobytes() == G.tobytes() and (G > rew).any()
    perm = torch.randperm(96, generator=torch.Generator(device="cpu").manual_seed(4))[:96]
    replay = m_stepper.replay
    for t in range(1, 7):
        if per:
            idx_d, weight = replay.sample(t)
            idx = idx_d.cpu().numpy()
        else:
            idx, weight = perm[4 * (t - 1):4 * t].numpy(), None
        idx_t = torch.from_numpy(idx).to(DEV)
        if n_step > 1:
            rew_n, term_n, disc, last, _ = nstep_oracle.walk_f32(idx, next_row, rew, term, n_step, 0.99)
            r_t, t_t, d_t, last_t = (torch.from_numpy(x).to(DEV) for x in (rew_n, term_n, disc, last))
        else:
            r_t, t_t, d_t, last_t = store.rew.index_select(0, idx_t), store.term.index_select(0, idx_t), None, idx_t
        before = store.frames.index_select(0, store.before.index_select(0, idx_t).reshape(-1))
        after = store.frames.index_select(0, store.after.index_select(0, last_t).reshape(-1))
        m_stepper.step(before, after, 0, store.act.index_select(0, idx_t), r_t, t_t, weights=weight, td_error=(replay.err if per else None),
                       discount=d_t, mc_return=torch.from_numpy(G[idx]).to(DEV))
        if per:
            replay.update()
    torch.cuda.synchronize()
    assert torch.equal(model.engine.params, m_model.engine.params)
    assert torch.equal(stepper.exp_avg, m_stepper.exp_avg) and torch.equal(stepper.exp_avg_sq, m_stepper.exp_avg_sq)
    assert torch.equal(stepper.loss, m_stepper.loss) and torch.equal(stepper.q_before, m_stepper.q_before)
    assert torch.equal(stepper.mc_stats, m_stepper.mc_stats) and torch.isfinite(stepper.mc_stats).all()
    if per:
        assert torch.equal(stepper.replay.prio, replay.prio) and not bool((replay.prio == 1.0).all())


def test_default_keys_launch_nothing_new_and_both_scalars_are_logged(tmp_path, shards):
    """A run without the keys and a run with both at False end bit-identical and launch neither mc_returns nor an _mc loss; a run
    with both on launches them, ends elsewhere, and at update 100 writes mc_floor_share/train and q_minus_return/train with the values
    of update 99 (read one update late, like the loss)."""
    from video_dqn_amd import _lib
    from video_dqn_amd.config import JsonlWriter
    finals, names = [], []
    for tag, extra in (("none", ""), ("false", "MC_RETURN_FLOOR: False\nCQL_CALIBRATED: False\n")):
        _lib.profile_enable(True)
        try:
            model, stepper, logs, _ = _run(tmp_path, tag, shards, 6, extra)
            names.append(set(_lib.profile_collect()))
        finally:
            _lib.profile_enable(False)
        assert stepper.returns is None and not any("Monte-Carlo" in l for l in logs)
        finals.append((model.engine.params.cpu(), stepper.exp_avg.cpu(), stepper.exp_avg_sq.cpu(), stepper.loss.cpu()))
    for x, y in zip(*finals):
        assert torch.equal(x, y)
    assert names[0] == names[1] and "td_loss" in names[0] and not any(n == "mc_returns" or n.endswith("_mc") for n in names[0]), names[0]
    _lib.profile_enable(True)
    try:
        model, stepper, logs, cfg = _run(tmp_path, "on", shards, 100, WAYS["both_per"].replace("PRIORITIZED_REPLAY: True\n", ""), tensorboard=True)
        on_names = set(_lib.profile_collect())
    finally:
        _lib.profile_enable(False)
    assert {"mc_returns", "td_loss_cql_mc"} <= on_names and "td_loss_cql" not in on_names, on_names
    if not isinstance(cfg.writer, JsonlWriter):
        pytest.fail("this test reads scalars.jsonl: it needs the JsonlWriter stand-in (no tensorboard package)")
    cfg.writer.close()
    rows = [json.loads(l) for l in open(os.path.join(cfg.log_dir, "scalars.jsonl"))]
    share = [r for r in rows if r["tag"] == "mc_floor_share/train"]
    gap = [r for r in rows if r["tag"] == "q_minus_return/train"]
    assert len(share) == 1 and len(gap) == 1 and share[0]["step"] == 99 and gap[0]["step"] == 99
    print(f"mc_floor_share/train {share[0]['value']:.4f}, q_minus_return/train {gap[0]['value']:.4f}")
    assert 0.0 <= share[0]["value"] <= 1.0 and math.isfinite(gap[0]["value"])
    assert not torch.equal(model.engine.params.cpu(), finals[0][0])
