"""Prioritized experience replay on the GPU: the sampling kernel against the numpy oracle (tests/per_oracle.py) index for index,
the draw distribution, the priority update, the weighted TD loss against vdqn_td_loss and float64, TDStepper with weights, and
run_train with PRIORITIZED_REPLAY on a resident shard dataset (determinism, checkpoint, resume)."""
import ctypes as C

import numpy as np
import pytest
import torch

import per_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sample(p, G, seed, step, beta):
    from video_dqn_amd import _lib
    lib = _lib.load()
    p = p.to(DEV).contiguous()
    ws = torch.empty(lib.vdqn_per_workspace_bytes(p.numel()), dtype=torch.uint8, device=DEV)
    idx = torch.empty(G, dtype=torch.int64, device=DEV)
    w = torch.empty(G, dtype=torch.float32, device=DEV)
    _lib.check(lib.vdqn_per_sample(p.data_ptr(), p.numel(), G, seed, step, beta, ws.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "vdqn_per_sample")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), w.cpu().numpy()


def _tables(n, rng):
    yield "uniform", np.ones(n, np.float32)
    yield "loguniform", np.exp(rng.uniform(np.log(1e-6), np.log(1e3), n)).astype(np.float32)
    z = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), n)).astype(np.float32)
    for lo in range(0, n, 700):
        z[lo:lo + 300] = 0.0  # runs of zeros across segment and chunk boundaries
    if z.max() == 0:
        z[-1] = 1.0
    yield "zero_runs", z
    one = np.zeros(n, np.float32)
    one[(n * 7) // 11] = 3.5
    yield "single", one


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003, 1000000])
def test_sample_kernel_matches_oracle(n):
    rng = np.random.default_rng(n)
    for G in (1, 256, 512):
        for name, p in _tables(n, rng):
            step, beta = 1000 + G, 0.4 + 0.1 * (G % 3)
            idx, w = _sample(torch.from_numpy(p), G, 17, step, beta)
            ridx, rw = per_oracle.sample(p, G, 17, step, beta)
            np.testing.assert_array_equal(idx, ridx, err_msg=f"{name} n={n} G={G}")
            np.testing.assert_allclose(w, rw, rtol=1e-6, atol=0, err_msg=f"{name} n={n} G={G}")
            assert np.all(p[idx] > 0)


def test_draw_distribution_chi_square():
    """N = 64 fixed priorities, 400 draws of G = 256 (102400 samples, deterministic seed): the counts against p / sum(p).
    63 degrees of freedom; the 1e-4 upper tail of chi^2(63) is ~117.  Stratification makes the counts tighter than multinomial,
    so a correct sampler sits far below (the statistic is printed)."""
    rng = np.random.default_rng(5)
    p = np.exp(rng.uniform(np.log(0.05), np.log(5.0), 64)).astype(np.float32)
    counts = np.zeros(64)
    for step in range(400):
        idx, _ = _sample(torch.from_numpy(p), 256, 2024, step, 0.4)
        counts += np.bincount(idx, minlength=64)
    exp = counts.sum() * p.astype(np.float64) / p.astype(np.float64).sum()
    chi2 = ((counts - exp) ** 2 / exp).sum()
    print(f"chi2 = {chi2:.2f} (63 dof)")
    assert chi2 < 117.0


def test_priority_update_duplicates_untouched_and_values():
    from video_dqn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(1)
    n, G = 5000, 512
    p0 = rng.uniform(0.1, 2.0, n).astype(np.float32)
    idx = rng.integers(0, 300, G).astype(np.int64)  # many repeats
    err = rng.uniform(0, 3, G).astype(np.float32)
    for alpha in (0.6, 1.0, 0.0):
        p, idx_d, err_d = torch.from_numpy(p0).to(DEV), torch.from_numpy(idx).to(DEV), torch.from_numpy(err).to(DEV)
        _lib.check(lib.vdqn_per_update(p.data_ptr(), n, idx_d.data_ptr(), err_d.data_ptr(), G, alpha, torch.cuda.current_stream().cuda_stream),
                   "vdqn_per_update")
        got = p.cpu().numpy()
        ref = per_oracle.update(p0, idx, err, alpha)
        untouched = np.setdiff1d(np.arange(n), idx)
        assert np.array_equal(got[untouched].view(np.uint32), p0[untouched].view(np.uint32))
        last = {int(i): j for j, i in enumerate(idx)}
        for i, j in last.items():
            exact = (np.float64(err[j]) + 1e-6) ** alpha
            assert abs(got[i] - exact) <= 1e-6 * exact
        np.testing.assert_allclose(got, ref, rtol=1e-6)


def _td_inputs(B, seed, ldq=64, n_cat=5, n_act=3):
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, ldq, generator=g) * 0.7 for _ in range(3)]
    act = torch.randint(0, n_act, (B,), generator=g)
    rew = (torch.rand(B, n_cat, generator=g) < 0.3).float()
    term = (torch.rand(B, n_cat, generator=g) < 0.2).float()
    valid = (torch.rand(B, n_cat, generator=g) < 0.8).float()
    return [t.to(DEV) for t in q + [act, rew, term, valid]]


def _td(inputs, dtype, loss_kind, use_valid, weight=None, with_err=True, linear=0, clip_rect=1, gamma=0.9, deterministic=1, q_copy=False):
    """vdqn_td_loss (weight None) or vdqn_td_loss_weighted through the raw ABI -> (loss, dq as f32, dq_f32, err, q_copy) on the CPU."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    qb, qo, qt, act, rew, term, valid = inputs
    B, ldq = qb.shape
    loss = torch.zeros(1, device=DEV)
    dq = torch.zeros(B, ldq, dtype=torch.bfloat16 if dtype == _lib.VDQN_BF16 else torch.float32, device=DEV)
    dq32 = torch.zeros(B, ldq, device=DEV)
    err = torch.full((B,), -1.0, device=DEV) if with_err else None
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = qb.data_ptr(), qo.data_ptr(), qt.data_ptr()
    a.act, a.rew, a.term, a.valid = act.data_ptr(), rew.data_ptr(), term.data_ptr(), valid.data_ptr() if use_valid else None
    a.loss, a.dq, a.dq_f32 = loss.data_ptr(), dq.data_ptr(), dq32.data_ptr()
    a.batch, a.n_cat, a.n_act, a.ldq = B, 5, 3, ldq
    a.gamma, a.inv_count = gamma, 1.0 / (5 * B)
    a.clip_rect, a.linear, a.use_valid, a.dtype, a.loss_kind, a.deterministic = clip_rect, linear, int(use_valid), dtype, loss_kind, deterministic
    qc = torch.full((B, 15), -7.0, device=DEV) if q_copy else None
    a.q_copy = qc.data_ptr() if q_copy else None
    st = torch.cuda.current_stream().cuda_stream
    if weight is None:
        _lib.check(lib.vdqn_td_loss(C.byref(a), st), "vdqn_td_loss")
    else:
        _lib.check(lib.vdqn_td_loss_weighted(C.byref(a), weight.data_ptr(), err.data_ptr() if with_err else None, st), "vdqn_td_loss_weighted")
    torch.cuda.synchronize()
    return loss.cpu(), dq.float().cpu(), dq32.cpu(), (err.cpu() if with_err else None), (qc.cpu() if q_copy else None)


def _td_f64(inputs, loss_kind, use_valid):
    """float64 per-sample loss terms [B, n_cat], dl [B, n_cat] and d [B, n_cat] (clip 'rect', gamma 0.9)."""
    qb, qo, qt, act, rew, term, valid = [t.cpu().double() if t.is_floating_point() else t.cpu() for t in inputs]
    B = qb.shape[0]
    qb3, qo3, qt3 = (t[:, :15].reshape(B, 5, 3) for t in (qb, qo, qt))
    q_s = qb3.gather(2, act.view(B, 1, 1).expand(B, 5, 1)).squeeze(2)
    best = qo3.float().argmax(2, keepdim=True)
    qa = qt3.gather(2, best).squeeze(2) * (1 - term)
    y = (rew + 0.9 * qa).clamp(0, 1)
    d = q_s - y
    vm = valid if use_valid else torch.ones_like(d)
    if loss_kind == 1:
        l, dl = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5), d.clamp(-1, 1)
    else:
        l, dl = 0.5 * d * d, d
    return l * vm, dl * vm, d, vm


@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
def test_td_loss_weighted(loss_kind, use_valid):
    from video_dqn_amd import _lib
    B = 96
    inputs = _td_inputs(B, 11 + loss_kind + 2 * use_valid)
    for dtype in (_lib.VDQN_F32, _lib.VDQN_BF16):
        ref = _td(inputs, dtype, loss_kind, use_valid)
        ones = _td(inputs, dtype, loss_kind, use_valid, weight=torch.ones(B, device=DEV))
        assert torch.equal(ref[0], ones[0]) and torch.equal(ref[1], ones[1]) and torch.equal(ref[2], ones[2])
    w = torch.rand(B, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.1
    loss, _, dq32, err, _ = _td(inputs, _lib.VDQN_F32, loss_kind, use_valid, weight=w.to(DEV))
    l, dl, d, vm = _td_f64(inputs, loss_kind, use_valid)
    inv = 1.0 / (5 * B)
    wl = w.double().view(B, 1)
    exp_loss = (l * wl).sum() * inv
    assert abs(loss.item() - exp_loss.item()) <= 1e-5 * abs(exp_loss.item())  # (an f32 sum of 5 B terms)
    act = inputs[3].cpu()
    cols = (torch.arange(5).view(1, 5) * 3 + act.view(B, 1))
    got = dq32.double().gather(1, cols)
    exp = dl * wl * inv
    assert (got - exp).abs().max().item() <= 1e-6 * exp.abs().max().item()
    mask = torch.ones(B, 64, dtype=torch.bool)
    mask.scatter_(1, cols, False)
    assert torch.all(dq32[mask] == 0)
    exp_err = (d.abs() * vm).sum(1) / 5
    assert (err.double() - exp_err).abs().max().item() <= 1e-6 * max(exp_err.abs().max().item(), 1e-30)


def test_td_loss_weighted_unit_weights_every_target_option():
    """vdqn_td_loss and vdqn_td_loss_weighted launch two instances of one kernel template (plain and weighted) that share the one
    statement of the Double-DQN target (td_error_of): with w = 1 the two agree bit for bit over every option of the target and the
    loss, in both dtypes."""
    from video_dqn_amd import _lib
    B = 70
    inputs = _td_inputs(B, 29)
    inputs[0] = inputs[0] * 2.5  # |d| beyond 1: both Huber branches
    for dtype in (_lib.VDQN_F32, _lib.VDQN_BF16):
        for loss_kind in (0, 1):
            for use_valid in (False, True):
                for linear, clip_rect, gamma in ((0, 1, 0.9), (1, 1, 0.9), (0, 0, 0.99), (1, 0, 0.5)):
                    kw = dict(linear=linear, clip_rect=clip_rect, gamma=gamma)
                    ref = _td(inputs, dtype, loss_kind, use_valid, **kw)
                    ones = _td(inputs, dtype, loss_kind, use_valid, weight=torch.ones(B, device=DEV), **kw)
                    assert torch.equal(ref[0], ones[0]) and torch.equal(ref[1], ones[1]) and torch.equal(ref[2], ones[2]), (dtype, loss_kind, use_valid, kw)


# The plain and the weighted entry at the shapes where the shared element loop and block sum can go wrong: (B, ldq)
EDGE_SHAPES = [(1, 64),    # one block, one wave, 64 of 256 threads live
               (5, 64),    # two blocks, the second a quarter full
               (17, 15),   # no padding columns; 255 elements, one short of a block
               (16, 16),   # exactly one block, one padding column per row
               (96, 64)]   # the size the other tests use


@pytest.mark.parametrize("B,ldq", EDGE_SHAPES, ids=[f"B{b}_ld{l}" for b, l in EDGE_SHAPES])
@pytest.mark.parametrize("loss_kind", [0, 1], ids=["l2", "huber"])
@pytest.mark.parametrize("use_valid", [False, True], ids=["all", "valid"])
def test_td_loss_plain_and_weighted_edge_shapes(use_valid, loss_kind, B, ldq):
    """Both entries, both dtypes, against the float64 restatement with test_td_loss_weighted's tolerances (loss 1e-5 relative — an
    f32 sum of 5 B terms —, dq and err 1e-6 of their largest element); padding columns and non-taken actions of dq exactly 0;
    q_copy is q_before[:, :15]; a multi-block launch writes the deterministic launch's dq bit for bit and its loss within the same
    1e-5; the two entries agree bit for bit at w = 1."""
    from video_dqn_amd import _lib
    inputs = _td_inputs(B, 11 + loss_kind + 2 * use_valid, ldq=ldq)
    inputs[0] = inputs[0] * 2.5  # |d| beyond 1: both Huber branches
    inputs[6][0, 0] = 1.0  # (B = 1: at least one valid term)
    w = torch.rand(B, generator=torch.Generator().manual_seed(3)) * 0.9 + 0.1
    l, dl, d, vm = _td_f64(inputs, loss_kind, use_valid)
    inv = 1.0 / (5 * B)
    act = inputs[3].cpu()
    cols = (torch.arange(5).view(1, 5) * 3 + act.view(B, 1))
    zero = torch.ones(B, ldq, dtype=torch.bool)
    zero.scatter_(1, cols, False)
    exp_err = (d.abs() * vm).sum(1) / 5
    for dtype in (_lib.VDQN_F32, _lib.VDQN_BF16):
        for weight in (None, torch.ones(B), w):
            wl = torch.ones(B, 1, dtype=torch.float64) if weight is None else weight.double().view(B, 1)
            exp_loss, exp_dq = ((l * wl).sum() * inv).item(), dl * wl * inv
            kw = dict(weight=None if weight is None else weight.to(DEV), q_copy=True)
            det = _td(inputs, dtype, loss_kind, use_valid, deterministic=1, **kw)
            free = _td(inputs, dtype, loss_kind, use_valid, deterministic=0, **kw)
            for name, (loss, dq, dq32, err, qc) in (("deterministic", det), ("multi-block", free)):
                e_loss = abs(loss.item() - exp_loss) / abs(exp_loss)
                e_dq = (dq32.double().gather(1, cols) - exp_dq).abs().max().item() / exp_dq.abs().max().item()
                print(f"dtype {dtype} {name} weight {'none' if weight is None else 'ones' if weight is not w else 'random'}: "
                      f"loss {e_loss:.2e} relative, dq {e_dq:.2e} of the max element")
                assert e_loss <= 1e-5 and e_dq <= 1e-6
                assert torch.all(dq32[zero] == 0) and torch.all(dq[zero] == 0)
                assert torch.equal(dq, dq32.bfloat16().float() if dtype == _lib.VDQN_BF16 else dq32)
                assert torch.equal(qc, inputs[0].cpu()[:, :15])
                if weight is not None:
                    e_err = (err.double() - exp_err).abs().max().item() / max(exp_err.abs().max().item(), 1e-30)
                    print(f"  err {e_err:.2e} of the max element")
                    assert e_err <= 1e-6
            assert torch.equal(free[1], det[1]) and torch.equal(free[2], det[2])  # dq has no sum in it: only the loss may differ
            if weight is not None:
                assert torch.equal(free[3], det[3])
            if weight is None:
                plain = det, free
            elif weight is not w:  # w = 1: the weighted entry is the plain one, bit for bit (the loss where its order is fixed)
                assert torch.equal(plain[0][0], det[0])
                for x, y in zip(plain, (det, free)):
                    assert torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])


def _stepper(dtype, B, deterministic=True):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, True, dtype, 2 * B, deterministic=deterministic)
    net.load_tensors(synth.make_state_dict(7))
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True)


def _batch(seed, B):
    from video_dqn_amd import synth
    (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
    before, after, act, rew, term = tup[:5]
    return (before.contiguous().to(DEV), after.contiguous().to(DEV), 1, act.to(DEV), rew.float().to(DEV), term.float().to(DEV))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stepper_unit_weights_bit_identical(dtype):
    B = 8
    runs = []
    for weighted in (False, True):
        net, stp = _stepper(dtype, B)
        err = torch.zeros(B, device=DEV)
        for s in (1, 2):
            kw = dict(weights=torch.ones(B, device=DEV), td_error=err) if weighted else {}
            stp.step(*_batch(300 + s, B), **kw)
        torch.cuda.synchronize()
        runs.append((net.params.cpu(), stp.loss.cpu(), err.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.all(runs[1][2] > 0)


def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 10\nNUM_STEPS: {steps}\nSEED: 4\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nPRIORITIZED_REPLAY: True\nTARGET_UPDATE_INTERVAL: 1\n" + extra)


def test_run_train_prioritized_replay(tmp_path):
    from test_shards_cpu import _make_dataset
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.model import load_model_number
    from video_dqn_amd.shards import build_shards
    from video_dqn_amd.trainer import run_train
    shards = str(tmp_path / "shards")
    build_shards(_make_dataset(tmp_path, n=21), shards, shard_frames=8, log=lambda *a: None)
    finals = []
    for tag in ("a", "b"):
        _write_cfg(tmp_path / tag, shards, 20)
        logs = []
        model, stepper, running = run_train(ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False),
                                            log=lambda *a: logs.append(" ".join(map(str, a))))
        assert any("prioritized replay over 20 samples" in l for l in logs) and np.isfinite(running)
        snap = torch.load(tmp_path / tag / "models" / "sample20.torch", map_location="cpu")
        finals.append((model.engine.params.cpu(), snap["replay_state"]["priorities"]))
    assert torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1])
    prio = finals[0][1]
    assert prio.dtype == torch.float32 and prio.shape == (20,) and not torch.all(prio == 1.0)
    snap10 = torch.load(tmp_path / "a" / "models" / "sample10.torch", map_location="cpu")
    assert set(snap10) == {"sample_number", "model_state_dict", "optimizer_state_dict", "replay_state"}
    # resume (-r 10).  The reference's loop restarts at resume_from + 1 and increments before its first update (kept:
    # test_gpu_boundary), so the resumed run performs updates 12..20; a second resume from the same checkpoint lands on the
    # same parameters and table, and one from a copy without replay_state starts from the uniform table and does not
    _write_cfg(tmp_path / "r0", shards, 20)
    (tmp_path / "r0" / "models").mkdir()
    torch.save(snap10, tmp_path / "r0" / "models" / "sample10.torch")
    _, stepper, _ = run_train(ExperimentConfig(str(tmp_path / "r0"), device=DEV, tensorboard=False, resume=True), resume_from=10,
                              max_steps=0, log=lambda *a: None)  # (no update: the state as loaded)
    assert stepper.adam_step == 10
    assert torch.equal(stepper.replay.prio.cpu().view(torch.int32), snap10["replay_state"]["priorities"].view(torch.int32))
    resumed = []
    for tag, strip in (("r1", False), ("r2", False), ("r3", True)):
        _write_cfg(tmp_path / tag, shards, 20)
        (tmp_path / tag / "models").mkdir()
        s10 = dict(snap10)
        if strip:
            del s10["replay_state"]
        torch.save(s10, tmp_path / tag / "models" / "sample10.torch")
        logs = []
        model, stepper, _ = run_train(ExperimentConfig(str(tmp_path / tag), device=DEV, tensorboard=False, resume=True), resume_from=10,
                                      log=lambda *a: logs.append(" ".join(map(str, a))))
        assert any(("uniform table" if strip else "restored") in l for l in logs)
        snap = torch.load(tmp_path / tag / "models" / "sample20.torch", map_location="cpu")
        resumed.append((model.engine.params.cpu(), snap["replay_state"]["priorities"]))
        assert stepper.adam_step == 19
    assert torch.equal(resumed[0][0], resumed[1][0]) and torch.equal(resumed[0][1], resumed[1][1])
    assert not torch.equal(resumed[0][1], resumed[2][1])
    m = load_model_number(ExperimentConfig(str(tmp_path / "a"), device=DEV, tensorboard=False), 20)
    sd = m.state_dict()
    saved = torch.load(tmp_path / "a" / "models" / "sample20.torch", map_location="cpu")["model_state_dict"]
    assert all(torch.equal(sd[k].cpu(), v) for k, v in saved.items())
    # a table of the wrong size is an error
    bad = dict(snap10)
    bad["replay_state"] = {"priorities": torch.ones(7)}
    _write_cfg(tmp_path / "bad", shards, 20)
    (tmp_path / "bad" / "models").mkdir()
    torch.save(bad, tmp_path / "bad" / "models" / "sample10.torch")
    with pytest.raises(ValueError, match="7 priorities"):
        run_train(ExperimentConfig(str(tmp_path / "bad"), device=DEV, tensorboard=False, resume=True), resume_from=10, log=lambda *a: None)


def test_alpha_zero_is_the_unweighted_update_on_the_drawn_indices():
    """alpha = 0: every priority stays 1.0, every weight is exactly 1, and the update equals the unweighted one on the same
    sampled indices, bit for bit."""
    from video_dqn_amd.replay import PrioritizedSampler
    B, n = 8, 40
    frames = _batch(400, n)
    ref_net, ref_stp = _stepper("f32", B)
    net, stp = _stepper("f32", B)
    smp = PrioritizedSampler(n, B, DEV, alpha=0.0, beta=0.4, num_steps=10, seed=3)
    for s in (1, 2, 3):
        idx, w = smp.sample(s)
        sel = [frames[0][idx], frames[1][idx], 1] + [t[idx] for t in frames[3:]]
        stp.step(*sel, weights=w, td_error=smp.err)
        smp.update()
        ref_stp.step(*[t.clone() if torch.is_tensor(t) else t for t in sel])
        torch.cuda.synchronize()
        assert torch.all(w == 1.0)
    assert torch.all(smp.prio == 1.0)
    assert torch.equal(net.params, ref_net.params)


def test_weighted_step_gradient_matches_f64_oracle():
    """TDStepper.step with random importance weights, f32 engine at B = 8: every gradient tensor against the float64 oracle that
    takes the engine's ReLU decisions (the strict gate of test_gpu_engine: relative L2 <= 1e-3, max element <= 5e-3 of the tensor's
    max).  The oracle has no weights: the test forms the weighted mean of its per-sample TD losses itself."""
    from oracle import ref_cpu
    from test_gpu_engine import _EngineReLU, _engine_relu_masks, make_engine
    from video_dqn_amd import synth
    from video_dqn_amd.engine import TDStepper
    B = 8
    net = make_engine("f32", seed=7, max_batch=2 * B)
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True)
    make_engine("f32", seed=8, max_batch=2 * B).pack_weights(stp.packed_target)  # a target network of its own
    (tup, _) = synth.make_batch(101, B, 1, structured=True, reward_p=0.3)
    w = torch.rand(B, generator=torch.Generator().manual_seed(12)) * 0.95 + 0.05
    err = torch.zeros(B, device=DEV)
    stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV),
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
    (d["losses"] * w.double().view(B, 1)).mean().backward()
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


# ---- data parallelism: two ranks on one GPU over gloo (the harness of tests/test_gpu_ddp.py) -------------------------------
def _dp_pool(n):
    return _batch(600, n)


def _dp_run(B, world, rank, grad_hook=None, err_hook=None, steps=3, n=40):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    from video_dqn_amd.replay import PrioritizedSampler
    net = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7))
    smp = PrioritizedSampler(n, B, DEV, alpha=0.6, beta=0.4, num_steps=10, seed=5, rank=rank, world_size=world)
    stp = TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, world_size=world, allreduce=grad_hook,
                    allreduce_errors=(lambda: err_hook(smp.err_all)) if err_hook else None)
    pool = _dp_pool(n)
    draws = []
    for s in range(1, steps + 1):
        idx, w = smp.sample(s)
        stp.step(pool[0][idx], pool[1][idx], 1, pool[3][idx], pool[4][idx], pool[5][idx], weights=w, td_error=smp.err)
        smp.update()
        torch.cuda.synchronize()
        draws.append(idx.cpu().clone())
    return net.params.cpu(), smp.prio.cpu(), torch.stack(draws)


def _dp_worker(rank, world, port, out_dir, B):
    import os
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

    params, prio, draws = _dp_run(B, world, rank, through_host, through_host)
    torch.save({"params": params, "prio": prio, "draws": draws}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process_on_the_big_batch(tmp_path):
    """Two ranks x B = 4 on one GPU (gloo) against one process at batch 2B, three prioritized updates: both ranks hold bit-identical
    priority tables, each rank drew its slice of the one-process run's draws at every update, and the parameters meet
    test_gpu_ddp.py's bound against the big batch."""
    import torch.multiprocessing as mp
    from test_gpu_ddp import _free_port
    B, world = 4, 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), B), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    assert torch.equal(ranks[0]["prio"].view(torch.int32), ranks[1]["prio"].view(torch.int32))
    assert torch.equal(ranks[0]["params"], ranks[1]["params"])
    params, prio, draws = _dp_run(B * world, 1, 0)
    for r in range(world):
        assert torch.equal(ranks[r]["draws"], draws[:, r * B:(r + 1) * B]), r
    assert not torch.all(prio == 1.0)
    # the one-process table differs from the ranks' only through the TD errors of updates 2-3, computed with parameters that differ
    # in the summation order of update 1's gradient (measured: 1.8e-5 relative at worst, an entry with a small error)
    torch.testing.assert_close(ranks[0]["prio"], prio, rtol=1e-4, atol=1e-6)
    from video_dqn_amd.engine import NetEngine
    nt = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True).trainable_numel
    delta = (params[:nt] - ranks[0]["params"][:nt]).abs()
    assert delta.max().item() <= 2.5e-4 and delta.mean().item() < 2e-6
