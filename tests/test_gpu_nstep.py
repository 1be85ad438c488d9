"""n-step returns on the GPU: vdqn_nstep_walk against the numpy float32 oracle (tests/nstep_oracle.py) bit for bit, the TD loss
with a per-sample discount (vdqn_td_loss_nstep) against the scalar-gamma entries bit for bit and against the float64 oracle,
TDStepper.step(discount=) and run_train with N_STEP against a manual loop that walks the chains on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cql_oracle
import nstep_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32


# ---- 1. the walk ---------------------------------------------------------------------------------------------------------------------
def _walk_gpu(idx, next_row, rew, term, n, gamma):
    from video_dqn_amd import ops
    out = ops.nstep_walk(torch.from_numpy(idx).to(DEV), torch.from_numpy(next_row).to(DEV), torch.from_numpy(rew).to(DEV),
                         torch.from_numpy(term).to(DEV), n=n, gamma=gamma)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("fractional", [False, True], ids=["binary", "fractional"])
@pytest.mark.parametrize("n_cat", [1, 5])
@pytest.mark.parametrize("N", [1, 7, 300])
def test_nstep_walk_equals_the_f32_oracle_bit_for_bit(N, n_cat, fractional):
    """All five outputs, over the block edges of the batch, every n and gamma.  The tables (nstep_oracle.tables) hold a self-loop, a
    2-cycle, a row without a successor, successor entries -7, N and 2^31 - 1, chains shorter and longer than n; the indices
    (nstep_oracle.indices) repeat rows and go below 0 and beyond N."""
    next_row, rew, term = nstep_oracle.tables(N, n_cat, 7 + N, fractional)
    seen_steps = set()
    for B in (1, 63, 64, 65, 257):
        idx = nstep_oracle.indices(N, B, B)
        for n in (1, 2, 3, 16):
            for gamma in (0.9, 0.99, 1.0):
                want = nstep_oracle.walk_f32(idx, next_row, rew, term, n, gamma)
                got = _walk_gpu(idx, next_row, rew, term, n, gamma)
                for name, g, w in zip(("rew_n", "term_n", "disc", "last_row", "steps"), got, want):
                    assert g.dtype == w.dtype and g.shape == w.shape, name
                    assert np.array_equal(g.view(np.uint8), w.view(np.uint8)), (name, B, n, gamma)
                assert got[3].min() >= 0 and got[3].max() < N and got[4].min() >= 1 and got[4].max() <= n
                if B == 257:
                    seen_steps.add((n, tuple(sorted(set(got[4].tolist())))))
    if N == 300:  # chains shorter than n and of n rows both occurred
        assert all(len(s) >= 2 for n, s in seen_steps if n > 1), seen_steps


def test_nstep_walk_bad_arguments_fail_by_name_and_write_nothing():
    from video_dqn_amd import _lib, ops
    next_row, rew, term = nstep_oracle.tables(7, 5, 1)
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    nr, r, t = (torch.from_numpy(x).to(DEV) for x in (next_row, rew, term))
    for kw, word in ((dict(n=0), "n 0"), (dict(n=17), "n 17"), (dict(gamma=float("nan")), "gamma"), (dict(gamma=float("-inf")), "gamma")):
        args = dict(n=3, gamma=0.99)
        args.update(kw)
        with pytest.raises(_lib.VdqnError, match="vdqn_nstep_walk.*" + word):
            ops.nstep_walk(idx, nr, r, t, **args)
    with pytest.raises(_lib.VdqnError, match="vdqn_nstep_walk.*n_cat"):
        ops.nstep_walk(idx, nr, torch.zeros(7, 9, device=DEV), torch.zeros(7, 9, device=DEV), n=3, gamma=0.99)
    lib = _lib.load()
    out = torch.full((64,), 7.0, device=DEV)
    rc = lib.vdqn_nstep_walk(idx.data_ptr(), 0, nr.data_ptr(), r.data_ptr(), t.data_ptr(), 7, 5, 3, 0.99, out.data_ptr(), out.data_ptr(),
                             out.data_ptr(), out.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and lib.vdqn_last_error().decode().startswith("vdqn_nstep_walk: batch") and bool((out == 7.0).all())


def test_walker_reuses_its_buffers_and_checks_its_inputs():
    from video_dqn_amd.nstep import NStepWalker
    next_row, rew, term = nstep_oracle.tables(300, 5, 2)
    rew_d, term_d = torch.from_numpy(rew).to(DEV), torch.from_numpy(term).to(DEV)
    wk = NStepWalker(next_row, rew_d, term_d, 65, 3, 0.99)
    for seed in (1, 2):
        idx = np.clip(nstep_oracle.indices(300, 65, seed), 0, 299)
        got = wk.walk(torch.from_numpy(idx).to(DEV))
        torch.cuda.synchronize()
        assert got[0] is wk.rew_n and got[2] is wk.disc
        for g, w in zip(got, nstep_oracle.walk_f32(idx, next_row, rew, term, 3, 0.99)):
            assert np.array_equal(g.cpu().numpy(), w)
    with pytest.raises(ValueError, match="idx"):
        wk.walk(torch.zeros(64, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="N_STEP"):
        NStepWalker(next_row, rew_d, term_d, 65, 17, 0.99)
    with pytest.raises(ValueError, match="successor table"):
        NStepWalker(next_row[:10], rew_d, term_d, 65, 3, 0.99)


# ---- 2. the per-sample discount in the loss launch -------------------------------------------------------------------------------------
MODES = ("plain", "weighted", "cql")
ALPHA = 0.75


def _loss(mode, inputs, dtype, loss_kind, use_valid, clip_rect, weight, gamma=None, disc=None, deterministic=1, linear=0):
    """One of the three scalar-gamma entries (disc None) or vdqn_td_loss_nstep in the same mode (disc given), through the raw ABI.
    -> dict(loss, dq (stored dtype, as f32), dq32, err, pen) on the CPU; err / pen None where the mode has none."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    loss, pen = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    dq = torch.full((B, ldq), 7.0, dtype=torch.bfloat16 if dtype == _lib.VDQN_BF16 else torch.float32, device=DEV)
    dq32 = torch.full((B, ldq), 7.0, device=DEV)
    err = torch.full((B,), -1.0, device=DEV) if mode != "plain" else None
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = qb.data_ptr(), qo.data_ptr(), qt.data_ptr()
    a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
    a.loss, a.dq, a.dq_f32 = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr()
    a.batch, a.n_cat, a.n_act, a.ldq = B, 5, 3, ldq
    a.gamma, a.inv_count = (-123.0 if disc is not None else gamma), 1.0 / (5 * B)  # (with a discount, gamma is not read)
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, linear, int(use_valid), dtype, loss_kind, deterministic
    st = torch.cuda.current_stream().cuda_stream
    w = weight.data_ptr() if mode != "plain" else None  # (CQL runs weighted too: its weight may be NULL, which test_gpu_cql.py covers)
    e = err.data_ptr() if err is not None else None
    if disc is not None:
        _lib.check(lib.vdqn_td_loss_nstep(C.byref(a), w, e, ALPHA if mode == "cql" else 0.0, pen.data_ptr() if mode == "cql" else None,
                                          disc.data_ptr(), st), "vdqn_td_loss_nstep")
    elif mode == "plain":
        _lib.check(lib.vdqn_td_loss(C.byref(a), st), "vdqn_td_loss")
    elif mode == "weighted":
        _lib.check(lib.vdqn_td_loss_weighted(C.byref(a), w, e, st), "vdqn_td_loss_weighted")
    else:
        _lib.check(lib.vdqn_td_loss_cql(C.byref(a), w, e, ALPHA, pen.data_ptr(), st), "vdqn_td_loss_cql")
    torch.cuda.synchronize()
    return dict(loss=loss.cpu(), dq=dq.float().cpu(), dq32=dq32.cpu(), err=None if err is None else err.cpu(),
                pen=pen.cpu() if mode == "cql" else None)


def _same(x, y, keys=("loss", "dq", "dq32", "err", "pen")):
    return all((x[k] is None and y[k] is None) or torch.equal(x[k], y[k]) for k in keys)


@pytest.mark.parametrize("dtype_name", ["f32", "bf16"])
@pytest.mark.parametrize("mode", MODES)
def test_per_sample_discount_in_the_loss_launch(mode, dtype_name):
    """l2 / Huber x valid on / off x rect on / off x batch 1, 5, 64, 257.
    1. A constant discount gamma writes the existing entry's dq, err, penalty and (deterministic mode) loss bit for bit.
    2. Discounts drawn per sample from {g, g*g, g*g*g} (float32 products): every dq row and err[b] is, bit for bit, the row of the
       existing entry run with that sample's value as its scalar gamma; the loss (and penalty) are held against the float64 oracle
       at tests/test_gpu_cql.py's gate for the loss scalar, 1e-5 relative."""
    from video_dqn_amd import _lib
    dtype = _lib.VDQN_BF16 if dtype_name == "bf16" else _lib.VDQN_F32
    g1 = F(0.9)
    values = [g1, F(g1 * g1), F(F(g1 * g1) * g1)]
    for B in (1, 5, 64, 257):
        cpu = cql_oracle.td_inputs(B, 50 + B)
        cpu[0] = cpu[0] * 2.0  # |d| beyond 1 as well: both Huber branches
        cpu[6][0, 0] = 1.0     # at least one valid term
        inputs = [t.to(DEV) for t in cpu]
        w_cpu = torch.rand(B, generator=torch.Generator().manual_seed(B)) * 0.9 + 0.1
        w = w_cpu.to(DEV)
        pick = torch.randint(0, 3, (B,), generator=torch.Generator().manual_seed(100 + B))
        pick[0] = 2 if B == 1 else pick[0]
        disc_cpu = torch.tensor([values[k] for k in pick.tolist()], dtype=torch.float32)
        for loss_kind in (0, 1):
            for use_valid in (False, True):
                for clip_rect in (1, 0):
                    kw = dict(dtype=dtype, loss_kind=loss_kind, use_valid=use_valid, clip_rect=clip_rect, weight=w)
                    tag = (mode, dtype_name, B, loss_kind, use_valid, clip_rect)
                    # 1. constant
                    base = _loss(mode, inputs, gamma=float(g1), **kw)
                    const = _loss(mode, inputs, disc=torch.full((B,), float(g1), device=DEV), **kw)
                    assert _same(base, const), tag
                    free_b = _loss(mode, inputs, gamma=float(g1), deterministic=0, **kw)
                    free_c = _loss(mode, inputs, disc=torch.full((B,), float(g1), device=DEV), deterministic=0, **kw)
                    assert _same(free_b, free_c, ("dq", "dq32", "err")) and _same(base, free_c, ("dq", "dq32", "err")), tag
                    # 2. varying
                    vary = _loss(mode, inputs, disc=disc_cpu.to(DEV), **kw)
                    scalar = [base] + [_loss(mode, inputs, gamma=float(v), **kw) for v in values[1:]]
                    for k in range(3):
                        rows = pick == k
                        for key in ("dq", "dq32") + (("err",) if mode != "plain" else ()):
                            assert torch.equal(vary[key][rows], scalar[k][key][rows]), tag + (key, k)
                    assert torch.all(vary["dq32"][:, 15:] == 0)
                    o = cql_oracle.objective(cpu, ALPHA if mode == "cql" else 0.0, weight=None if mode == "plain" else w_cpu,
                                             use_valid=use_valid, loss_kind=loss_kind, clip_rect=clip_rect, gamma=disc_cpu.double().view(B, 1))
                    e_loss = abs(vary["loss"].item() - o["loss"].item()) / max(abs(o["loss"].item()), 1e-30)
                    assert e_loss <= 1e-5, tag + (e_loss,)
                    if mode == "cql":
                        assert abs(vary["pen"].item() - o["penalty"].item()) <= 1e-5 * abs(o["penalty"].item()), tag
                        assert torch.equal(vary["pen"], base["pen"])  # the penalty does not see the target
                    if B > 1 and not clip_rect:
                        assert not torch.equal(vary["dq32"], base["dq32"]), tag  # (the discount did reach the target)


def test_ops_td_loss_discount_paths():
    from video_dqn_amd import ops
    cpu = cql_oracle.td_inputs(5, 2)
    inputs = [t.to(DEV) for t in cpu]
    disc = torch.full((5,), 0.9, device=DEV)
    w = torch.rand(5, device=DEV) + 0.1
    a = ops.td_loss(*inputs[:6], inputs[6], gamma=0.9)
    b = ops.td_loss(*inputs[:6], inputs[6], discount=disc)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])) and abs(a[0].item() - b[0].item()) <= 1e-6 * abs(a[0].item())
    a = ops.td_loss_cql(*inputs[:6], inputs[6], cql_alpha=1.5, gamma=0.9, weights=w, with_err=True, deterministic=True)
    b = ops.td_loss_cql(*inputs[:6], inputs[6], cql_alpha=1.5, discount=disc, weights=w, with_err=True, deterministic=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = ops.td_loss_nstep(*inputs[:6], inputs[6], discount=disc, weights=w, with_err=True, deterministic=True)
    assert c[3] is None and torch.equal(c[4], a[4])  # the weighted launch: no penalty, the same raw errors
    with pytest.raises(ValueError, match="discount"):
        ops.td_loss_nstep(*inputs[:6], discount=disc[:4].contiguous())


def test_refusals_linear_and_validation():
    """`linear` with a discount fails by name at the operator, at vdqn_net_td_forward and in TDStepper.step; vdqn_net_td_eval with
    sample_gamma fails by name."""
    from video_dqn_amd import _lib, ops
    cpu = cql_oracle.td_inputs(5, 2)
    inputs = [t.to(DEV) for t in cpu]
    disc = torch.full((5,), 0.9, device=DEV)
    with pytest.raises(_lib.VdqnError, match="vdqn_td_loss_nstep: linear"):
        ops.td_loss(*inputs[:6], discount=disc, linear=True)
    B = 4
    net, stp = _stepper("f32", B)
    batch = _batch(301, B)
    d4 = torch.full((B,), 0.99, device=DEV)
    a = stp._args(*batch, stp._ones, None, discount=d4)
    st = torch.cuda.current_stream().cuda_stream
    stp.eval_begin()
    assert net.lib.vdqn_net_td_eval(net.handle, C.byref(a), stp.eval_acc.data_ptr(), st) == -1
    assert net.lib.vdqn_last_error().decode().startswith("vdqn_net_td_eval: sample_gamma")
    a.linear = 1
    assert net.lib.vdqn_net_td_forward(net.handle, C.byref(a), st) == -1
    assert "sample_gamma is given with linear" in net.lib.vdqn_last_error().decode()
    torch.cuda.synchronize()
    assert stp.eval_acc.abs().sum().item() == 0.0
    _, lin = _stepper("f32", B, linear=True)
    with pytest.raises(_lib.VdqnError, match="discount.*LINEAR"):
        lin.step(*batch, discount=d4)
    with pytest.raises(_lib.VdqnError, match="discount must be"):
        stp.step(*batch, discount=d4.double())


# ---- 3. the stepper ------------------------------------------------------------------------------------------------------------------
def _stepper(dtype, B, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, True, dtype, 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7))
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, **kw)


def _batch(seed, B):
    from video_dqn_amd import synth
    (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
    before, after, act, rew, term = tup[:5]
    return (before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))


@pytest.mark.parametrize("options", ["plain", "cql_weighted"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_step_with_a_constant_discount_is_step_without_it(dtype, options):
    """Two updates with step(discount = constant gamma) leave parameters, moments, loss and Q(s) bit-identical to step() without it;
    once more with the conservative penalty and importance weights on (and the per-sample errors compared too)."""
    B = 4
    kw = dict(cql_alpha=1.0) if options == "cql_weighted" else {}
    runs = []
    for with_discount in (False, True):
        net, stp = _stepper(dtype, B, **kw)
        disc = torch.full((B,), 0.99, device=DEV) if with_discount else None
        w = (torch.rand(B, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.1).to(DEV) if kw else None
        err = torch.zeros(B, device=DEV) if kw else None
        losses = []
        for s in (1, 2):
            losses.append(stp.step(*_batch(300 + s, B), weights=w, td_error=err, discount=disc).clone())
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), stp.exp_avg.cpu(), stp.exp_avg_sq.cpu(), torch.cat(losses).cpu(), stp.q_before.cpu(), stp.grads.cpu(),
                     stp.cql_penalty.cpu(), err.cpu() if kw else torch.zeros(1)))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.isfinite(runs[0][3]).all() and not torch.equal(runs[0][0], _stepper(dtype, B)[0].params.cpu())


# ---- 4. run_train ----------------------------------------------------------------------------------------------------------------------
def _write_cfg(folder, shards, steps, dtype, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 96\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        f"COMPUTE_DTYPE: '{dtype}'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def _run(tmp_path, tag, shards, steps, dtype, extra="", max_steps=None):
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    _write_cfg(tmp_path / tag, shards, steps, dtype, extra)
    logs = []
    model, stepper, _ = run_train(ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False), max_steps=max_steps,
                                  log=lambda *a: logs.append(" ".join(map(str, a))))
    torch.cuda.synchronize()
    return model, stepper, logs


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    root = str(tmp_path_factory.mktemp("nstep") / "shards")
    _synthetic_shards(root)  # 24 frames, 37 samples, random frame indices: cycles and rows without a successor
    return root


@pytest.mark.parametrize("per", [False, True], ids=["epochs", "per"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_run_train_n_step_3_equals_a_manual_loop_with_the_host_oracle(tmp_path, shards, dtype, per):
    """Three updates of run_train with N_STEP 3 against a manual loop on a second, identically seeded stepper (run_train with zero
    updates builds it): the rows the same seed draws at N_STEP 1 (the epoch permutation, or the prioritized draws), their chains
    walked by the numpy oracle on the host, `after` gathered from each chain's last row, and TDStepper.step fed the oracle's rew_n,
    term_n and disc.  Parameters, moments and, with PRIORITIZED_REPLAY, the priority table end bit-identical."""
    from video_dqn_amd.nstep import successors
    from video_dqn_amd.shards import DeviceFrameStore
    extra = "N_STEP: 3\n" + ("PRIORITIZED_REPLAY: True\n" if per else "")
    model, stepper, logs = _run(tmp_path, "auto", shards, 3, dtype, extra)
    assert stepper.adam_step == 3 and stepper.nstep is not None and stepper.nstep.n == 3
    line = [l for l in logs if l.startswith("n-step returns: N_STEP 3")]
    assert len(line) == 1 and "chains of 1 row:" in line[0] and "3 rows:" in line[0] and "validation stays one-step" in line[0]

    m_model, m_stepper, _ = _run(tmp_path, "manual", shards, 3, dtype, extra, max_steps=0)  # the same start; no update has run
    assert m_stepper.adam_step == 0
    store = DeviceFrameStore(shards, DEV, one_action=True, inverse_actions=True)
    index = np.load(os.path.join(shards, "index.npz"))
    next_row = successors(index["before"][:, 0], index["after"][:, 0])
    assert np.array_equal(next_row, stepper.nstep.next_row.cpu().numpy())
    assert (next_row == -1).any() and next_row[next_row[next_row[5]]] == 5  # rows without a successor and a cycle (5 -> 36 -> 7 -> 5) are in the data
    rew, term = store.rew.cpu().numpy(), store.term.cpu().numpy()
    perm = torch.randperm(37, generator=torch.Generator(device="cpu").manual_seed(4))[:36]
    replay = m_stepper.replay
    steps_seen = set()
    for t in (1, 2, 3):
        if per:
            idx_d, weight = replay.sample(t)
            idx = idx_d.cpu().numpy()
        else:
            idx, weight = perm[4 * (t - 1):4 * t].numpy(), None
        rew_n, term_n, disc, last, steps = nstep_oracle.walk_f32(idx, next_row, rew, term, 3, 0.99)
        steps_seen |= set(steps.tolist())
        idx_t, last_t = torch.from_numpy(idx).to(DEV), torch.from_numpy(last).to(DEV)
        before = store.frames.index_select(0, store.before.index_select(0, idx_t).reshape(-1))
        after = store.frames.index_select(0, store.after.index_select(0, last_t).reshape(-1))
        m_stepper.step(before, after, 0, store.act.index_select(0, idx_t), torch.from_numpy(rew_n).to(DEV), torch.from_numpy(term_n).to(DEV),
                       weights=weight, td_error=(replay.err if per else None), discount=torch.from_numpy(disc).to(DEV))
        if per:
            replay.update()
    torch.cuda.synchronize()
    assert len(steps_seen) >= 2  # (chains of different lengths were walked)
    assert torch.equal(model.engine.params, m_model.engine.params)
    assert torch.equal(stepper.exp_avg, m_stepper.exp_avg) and torch.equal(stepper.exp_avg_sq, m_stepper.exp_avg_sq)
    assert torch.equal(stepper.loss, m_stepper.loss) and torch.equal(stepper.q_before, m_stepper.q_before)
    if per:
        assert torch.equal(stepper.replay.prio, replay.prio) and not bool((replay.prio == 1.0).all())


def test_n_step_1_is_a_run_without_the_key_and_n_step_3_is_not(tmp_path, shards):
    finals = []
    for tag, extra in (("none", ""), ("one", "N_STEP: 1\n"), ("three", "N_STEP: 3\n")):
        model, stepper, logs = _run(tmp_path, tag, shards, 3, "f32", extra)
        finals.append((model.engine.params.cpu(), stepper.exp_avg.cpu(), stepper.exp_avg_sq.cpu(), stepper.loss.cpu()))
        assert (stepper.nstep is not None) == (tag == "three") and any("n-step" in l for l in logs) == (tag == "three")
    for x, y in zip(finals[0], finals[1]):
        assert torch.equal(x, y)
    assert not torch.equal(finals[0][0], finals[2][0])
