"""Soft (Polyak) target updates on the GPU (csrc/optim.hip vdqn_polyak / vdqn_adam_polyak, TDStepper(target_tau=...), run_train with
TARGET_TAU) against tests/polyak_oracle.py: the operator and the fused launch bit for bit, the averaged weights along a chain of
updates and inside the target pass, the early Adam launches, clipping and decay, ARCHITECTURE='basic', resume, the trainer and
two ranks over gloo on one device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import optim_oracle
import polyak_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 5, 255, 256, 257, 1025, 100003]
PAST_THE_CAP = 4096 * 256 * 4 + 5  # every thread of the 4096-block grid walks its float4 loop a second time; one tail element
POISON = 1e30


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _same(x, y):
    return torch.equal(_bits(x), _bits(y))


def _pair(n, seed):
    """(target, online) as numpy f32: the online values a tenth of a standard deviation away, every seventh one equal."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(n).astype(np.float32)
    p = (t + 0.1 * rng.standard_normal(n)).astype(np.float32)
    p[::7] = t[::7]
    return t, p


def _guarded(x):
    """x (numpy f32) on the device behind a 16-byte boundary with four poison elements on either side -> (buffer, view of x)."""
    n = x.size
    buf = torch.full((n + 8,), POISON, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[4:4 + n] = torch.from_numpy(x).to(DEV)
    return buf, buf[4:4 + n]


def _guards_intact(buf):
    g = torch.cat([buf[:4], buf[-4:]]).cpu()
    return bool((g == np.float32(POISON)).all())


# ---- 1. the operator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_polyak_update_is_lerp_f32_bit_for_bit_and_stays_in_its_range(n):
    from video_dqn_amd import ops
    for tau in (0.005, 0.5, 1.0):
        t, p = _pair(n, 17 * n)
        tbuf, tv = _guarded(t)
        pbuf, pv = _guarded(p)
        ops.polyak_update(tv, pv, tau)
        torch.cuda.synchronize()
        want = torch.from_numpy(polyak_oracle.lerp_f32(t, p, tau))
        assert torch.equal(tv.cpu(), want), (n, tau)
        assert torch.equal(pv.cpu(), torch.from_numpy(p))  # the online values are only read
        assert _guards_intact(tbuf) and _guards_intact(pbuf)
        if tau == 1.0:
            assert _same(tv, pv)
        if n >= 255:
            assert not torch.equal(tv.cpu(), torch.from_numpy(t))


# ---- 2. the fused launch ----------------------------------------------------------------------------------------------------------
def _adam_state(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, n).astype(np.float32)
    g = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    g[::7] = 0.0
    m = rng.uniform(-1e-3, 1e-3, n).astype(np.float32)
    v = rng.uniform(0, 1e-6, n).astype(np.float32)
    t = (p + 0.01 * rng.standard_normal(n)).astype(np.float32)
    return p, g, m, v, t


@pytest.mark.parametrize("n", SIZES + [PAST_THE_CAP])
def test_adam_polyak_equals_adam_scaled_then_polyak_bit_for_bit(n):
    from video_dqn_amd import ops
    host = _adam_state(n, 3 * n + 1)
    coef = torch.full((1,), 0.37, dtype=torch.float32, device=DEV)
    for kw in (dict(weight_decay=0.1, coef=coef), dict(weight_decay=0.0, coef=None)):
        for tau in (0.005, 0.5):
            two = [_guarded(x) for x in host]
            one = [_guarded(x) for x in host]
            plain = [_guarded(x) for x in host[:4]]
            for step in (1, 2):
                ops.adam_scaled(two[0][1], two[1][1], two[2][1], two[3][1], step, 1e-3, **kw)
                ops.polyak_update(two[4][1], two[0][1], tau)
                ops.adam_polyak(one[0][1], one[1][1], one[2][1], one[3][1], one[4][1], tau, step, 1e-3, **kw)
                if kw["coef"] is None:
                    ops.adam(plain[0][1], plain[1][1], plain[2][1], plain[3][1], step, 1e-3)
            torch.cuda.synchronize()
            for name, a, b in zip(("p", "g", "exp_avg", "exp_avg_sq", "target"), two, one):
                assert _same(a[1], b[1]), (name, n, tau, kw["weight_decay"])
                assert _guards_intact(b[0]), name
            assert torch.equal(one[1][1].cpu(), torch.from_numpy(host[1]))  # g is left as it is
            assert not torch.equal(one[4][1].cpu(), torch.from_numpy(host[4]))
            if kw["coef"] is None:  # unit factors: vdqn_adam's bits in p, m, v
                for name, a, b in zip(("p", "g", "exp_avg", "exp_avg_sq"), plain, one):
                    assert _same(a[1], b[1]), (name, n, tau)
            del two, one, plain


# ---- 3. the stepper ---------------------------------------------------------------------------------------------------------------
BASE_LR = 1e-3  # (the reference's rate: an lr-sized step stays well above the f32 spacing of the weights)


def _make(dtype, B, extra_capacity=True, tui=1000, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7, extra_capacity=extra_capacity))
    return net, TDStepper(net, B, lr=BASE_LR, gamma=0.99, clip_rect=True, target_update_interval=tui, **kw)


_BATCHES = {}


def _batch(seed, B):
    from video_dqn_amd import synth
    if (seed, B) not in _BATCHES:
        (tup, _) = synth.make_batch(seed, B, 1, structured=True, reward_p=0.3)
        _BATCHES[(seed, B)] = (tup[0].contiguous(), tup[1].contiguous(), tup[2], tup[3].float(), tup[4].float())
    t = _BATCHES[(seed, B)]
    return [t[0].to(DEV), t[1].to(DEV), 1, t[2].to(DEV), t[3].to(DEV), t[4].to(DEV)]


def _hand_over(dst_net, src_net):
    """dst's online state := src's (parameters, BatchNorm statistics and counters)."""
    dst_net.params.copy_(src_net.params)
    dst_net.bnstats.copy_(src_net.bnstats)
    dst_net.num_batches_tracked.copy_(src_net.num_batches_tracked)
    dst_net.mark_dirty()


def _np(x):
    return x.detach().cpu().numpy()


def test_target_follows_the_lerp_chain_and_the_target_pass_uses_it():
    """f32 deterministic, tau 0.25, target_update_interval 2, three updates.  After each one `target_params` is lerp_f32 applied
    along the stepper's own parameter snapshots, bit for bit (a hard copy at update 2 would break the chain), the frozen resnet.fc
    tail included.  A plain twin that is handed the same parameters, with `packed_target` folded by hand from the first stepper's
    `target_params`, and runs forward_backward only, produces the same gradient and loss bit for bit: the target pass reads the
    averaged weights.  A stepper without the feature sees another loss from update 2 on."""
    B, tau = 8, 0.25
    net, stp = _make("f32", B, tui=2, target_tau=tau)
    twin_net, twin = _make("f32", B)
    off_net, off = _make("f32", B)
    nt = net.trainable_numel
    assert stp.target_params.dtype == torch.float32 and stp.target_params.numel() == net.params_numel > nt
    assert _same(stp.target_params, net.params)
    want = _np(net.params).copy()
    for t in range(1, 4):
        _hand_over(twin_net, net)
        twin_net.pack_weights(twin.packed_target, with_dgrad=False, params=stp.target_params)
        twin.forward_backward(*_batch(300 + t, B))
        stp.step(*_batch(300 + t, B))
        off.step(*_batch(300 + t, B))
        torch.cuda.synchronize()
        assert _same(twin.grads, stp.grads) and _same(twin.loss, stp.loss), t
        if t == 1:
            assert _same(off.loss, stp.loss)  # (both targets are still the initial weights)
        else:
            assert not _same(off.loss, stp.loss), t
        want = polyak_oracle.lerp_f32(want, _np(net.params), tau)
        assert np.array_equal(_np(stp.target_params).view(np.int32), want.view(np.int32)), t
        assert _same(stp.target_params[nt:], net.params[nt:])
        assert not _same(stp.target_params[:nt], net.params[:nt])


@pytest.mark.parametrize("dtype", ["f32", "bf16", "bf16x3"])
def test_tau_one_equals_a_hard_copy_before_every_update(dtype):
    B = 8
    net_a, stp_a = _make(dtype, B, tui=1)
    net_b, stp_b = _make(dtype, B, target_tau=1.0)
    for t in range(1, 4):
        stp_a.step(*_batch(300 + t, B))
        stp_b.step(*_batch(300 + t, B))
        torch.cuda.synchronize()
        assert _same(stp_a.loss, stp_b.loss), t
    for name, x, y in (("params", net_a.params, net_b.params), ("exp_avg", stp_a.exp_avg, stp_b.exp_avg),
                       ("exp_avg_sq", stp_a.exp_avg_sq, stp_b.exp_avg_sq), ("target_params", net_b.params, stp_b.target_params)):
        assert _same(x, y), name


def test_tau_zero_is_the_plain_stepper_and_allocates_nothing():
    B = 8
    net_a, stp_a = _make("f32", B, tui=2)
    net_b, stp_b = _make("f32", B, tui=2, target_tau=0.0)
    assert stp_b.target_params is None and stp_b.target_tau == 0.0
    for t in range(1, 4):
        stp_a.step(*_batch(300 + t, B))
        stp_b.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", net_a.params, net_b.params), ("exp_avg", stp_a.exp_avg, stp_b.exp_avg),
                       ("exp_avg_sq", stp_a.exp_avg_sq, stp_b.exp_avg_sq), ("loss", stp_a.loss, stp_b.loss)):
        assert _same(x, y), name


def test_early_adam_launches_carry_the_target_with_them():
    """step() queues the Adam launches of stage 0 / 1 on the gradient stream by default; a twin driven as forward_backward(
    early_adam=False) + optimizer_step() (one launch behind the backward pass) ends with the same params and target_params."""
    from video_dqn_amd import engine
    assert engine._EARLY_ADAM
    B, tau = 8, 0.25
    net_a, stp_a = _make("f32", B, target_tau=tau)
    net_b, stp_b = _make("f32", B, target_tau=tau)
    ranges = []
    real = engine.TDStepper._adam_range

    def recording(self, b, e, step):
        ranges.append((self is stp_a, b, e))
        return real(self, b, e, step)
    engine.TDStepper._adam_range = recording
    try:
        for t in range(1, 4):
            stp_a.step(*_batch(300 + t, B))
            net_b.pack_weights(stp_b.packed_target, with_dgrad=False, params=stp_b.target_params)  # what step() does in front
            stp_b.sample_number += 1
            stp_b.forward_backward(*_batch(300 + t, B), early_adam=False)
            stp_b.optimizer_step()
            torch.cuda.synchronize()
            assert _same(stp_a.loss, stp_b.loss), t
    finally:
        engine.TDStepper._adam_range = real
    assert sum(1 for a, _, _ in ranges if a) > sum(1 for a, _, _ in ranges if not a) == 3  # several launches against one per update
    for name, x, y in (("params", net_a.params, net_b.params), ("target_params", stp_a.target_params, stp_b.target_params),
                       ("exp_avg_sq", stp_a.exp_avg_sq, stp_b.exp_avg_sq)):
        assert _same(x, y), name


def test_with_clipping_and_decay_the_target_follows_the_clipped_decayed_weights():
    B, tau, wd = 8, 0.25, 0.1
    net0, stp0 = _make("f32", B)
    stp0.forward_backward(*_batch(301, B))
    torch.cuda.synchronize()
    max_norm = 0.5 * optim_oracle.clip_coef(stp0.grads.cpu().numpy(), 1.0)[0]
    net_a, stp_a = _make("f32", B, grad_clip_norm=max_norm, weight_decay=wd, target_tau=tau)
    net_b, stp_b = _make("f32", B, grad_clip_norm=max_norm, weight_decay=wd)
    want = _np(net_a.params).copy()
    for t in range(1, 3):
        stp_a.step(*_batch(300 + t, B))
        torch.cuda.synchronize()
        if t == 1:  # (from update 2 on the two targets, and with them the gradients, differ)
            stp_b.step(*_batch(300 + t, B))
            torch.cuda.synchronize()
            assert _same(net_a.params, net_b.params) and _same(stp_a.exp_avg, stp_b.exp_avg) and _same(stp_a.clip_out, stp_b.clip_out)
            assert stp_a.clip_out[1].item() < 0.51
        want = polyak_oracle.lerp_f32(want, _np(net_a.params), tau)
        assert np.array_equal(_np(stp_a.target_params).view(np.int32), want.view(np.int32)), t
    # update 2 against a plain stepper that is handed update 1's state and the same target: params bit for bit
    net_c, stp_c = _make("f32", B, grad_clip_norm=max_norm, weight_decay=wd)
    net_d, stp_d = _make("f32", B, grad_clip_norm=max_norm, weight_decay=wd, target_tau=tau)
    for stp in (stp_c, stp_d):
        stp.step(*_batch(301, B))
    torch.cuda.synchronize()
    assert _same(net_c.params, net_d.params)
    net_c.pack_weights(stp_c.packed_target, with_dgrad=False, params=stp_d.target_params)
    for stp in (stp_c, stp_d):
        stp.step(*_batch(302, B))
    torch.cuda.synchronize()
    assert _same(net_c.params, net_d.params) and _same(stp_c.exp_avg_sq, stp_d.exp_avg_sq) and _same(stp_c.loss, stp_d.loss)
    assert _same(net_d.params, net_a.params)


def test_basic_architecture_folds_the_target_with_the_online_statistics():
    """ARCHITECTURE='basic' (train-mode BatchNorm), f32 deterministic, two updates: target_params is the chain, and update 2's loss
    equals a plain twin's whose target was folded by hand from (target_params, the online statistics before the update)."""
    B, tau = 8, 0.25
    net, stp = _make("f32", B, extra_capacity=False, target_tau=tau)
    twin_net, twin = _make("f32", B, extra_capacity=False)
    want = _np(net.params).copy()
    for t in range(1, 3):
        _hand_over(twin_net, net)
        twin_net.pack_weights(twin.packed_target, with_dgrad=False, params=stp.target_params, bnstats=net.bnstats)
        twin.forward_backward(*_batch(300 + t, B))
        stats_before = net.bnstats.clone()
        stp.step(*_batch(300 + t, B))
        torch.cuda.synchronize()
        assert torch.isfinite(stp.loss).all()
        assert _same(twin.loss, stp.loss) and _same(twin.grads, stp.grads), t
        assert not _same(stats_before, net.bnstats)  # the statistics move with every update; the target takes them as they stand
        want = polyak_oracle.lerp_f32(want, _np(net.params), tau)
        assert np.array_equal(_np(stp.target_params).view(np.int32), want.view(np.int32)), t


def test_refusals_by_name():
    from video_dqn_amd import _lib, synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    B = 4
    net = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7))
    for bad in (-1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(_lib.VdqnError, match="target_tau"):
            TDStepper(net, B, lr=BASE_LR, gamma=0.99, clip_rect=True, target_tau=bad)
    with pytest.raises(_lib.VdqnError, match="target_tau"):
        TDStepper(net, B, lr=BASE_LR, gamma=0.99, clip_rect=True, train_on_ground_truth=True, target_tau=0.005)
    TDStepper(net, B, lr=BASE_LR, gamma=0.99, clip_rect=True, train_on_ground_truth=True, target_tau=0.0)
    t = torch.zeros(8, device=DEV)
    from video_dqn_amd import ops
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(_lib.VdqnError, match="vdqn_polyak"):
            ops.polyak_update(t, t.clone(), bad)
    with pytest.raises(_lib.VdqnError, match="polyak_update"):
        ops.polyak_update(t, torch.zeros(4, device=DEV), 0.5)
    with pytest.raises(_lib.VdqnError, match="overlap"):
        ops.polyak_update(t, t, 0.5)


def _model(B):
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    m = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="f32", device=DEV, max_batch=2 * B, deterministic=True)
    m.load_state_dict(synth.make_state_dict(7), strict=True)
    return m


def test_resume_through_the_checkpoint_dicts_continues_bit_for_bit():
    """Six updates in one go against three, the trainer's checkpoint dicts (optimiser state and target_state_dict) into a fresh
    stepper, three more: parameters, moments and target_params bit-identical."""
    from video_dqn_amd.engine import TDStepper
    from video_dqn_amd.trainer import load_optimizer_state_dict, load_target_state_dict, optimizer_state_dict, target_state_dict
    B, tau = 4, 0.25

    def fresh():
        m = _model(B)
        return m, TDStepper(m.engine, B, lr=BASE_LR, gamma=0.99, clip_rect=True, target_tau=tau)
    m_u, stp_u = fresh()
    for t in range(1, 7):
        stp_u.step(*_batch(300 + t, B))
    m_i, stp_i = fresh()
    for t in range(1, 4):
        stp_i.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    msd = {k: v.clone() for k, v in m_i.state_dict().items()}
    osd, tsd = optimizer_state_dict(stp_i), target_state_dict(stp_i, m_i)
    assert list(tsd) == list(msd) and all(tsd[k].shape == msd[k].shape for k in msd)
    assert not torch.equal(tsd["top.4.weight"], msd["top.4.weight"])
    m_r, stp_r = fresh()
    m_r.load_state_dict(msd)
    load_optimizer_state_dict(stp_r, osd)
    stp_r.sync_target()
    assert _same(stp_r.target_params, m_r.engine.params)
    load_target_state_dict(stp_r, tsd)
    assert _same(stp_r.target_params, stp_i.target_params)
    stp_r.sample_number = 3
    for t in range(4, 7):
        stp_r.step(*_batch(300 + t, B))
    torch.cuda.synchronize()
    for name, x, y in (("params", m_u.engine.params, m_r.engine.params), ("exp_avg", stp_u.exp_avg, stp_r.exp_avg),
                       ("exp_avg_sq", stp_u.exp_avg_sq, stp_r.exp_avg_sq), ("target_params", stp_u.target_params, stp_r.target_params),
                       ("loss", stp_u.loss, stp_r.loss)):
        assert _same(x, y), name


# ---- 4. run_train -----------------------------------------------------------------------------------------------------------------
SEED = 4


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    root = str(tmp_path_factory.mktemp("polyak_shards") / "shards")
    _synthetic_shards(root)
    return root


def _train(folder, shards, steps, extra, resume_from=-1):
    """-> (stepper, log lines)"""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 4\nNUM_STEPS: {steps}\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)
    logs = []
    cfg = ExperimentConfig(str(folder), device=DEV, tensorboard=False, resume=resume_from > -1)
    model, stepper, running = run_train(cfg, resume_from=resume_from, log=lambda *a: logs.append(" ".join(map(str, a))))
    assert np.isfinite(running)
    return stepper, logs


def _copy_checkpoint(src, dst_folder, drop=None):
    (dst_folder / "models").mkdir(parents=True)
    snap = torch.load(src, map_location="cpu")
    if drop:
        del snap[drop]
    torch.save(snap, dst_folder / "models" / src.name)


STEPS, ON = 8, "TARGET_TAU: 0.25\n"


@pytest.fixture(scope="module")
def trained(tmp_path_factory, shards):
    """One run of eight updates with TARGET_TAU 0.25 and a checkpoint at update 4 -> (stepper, log lines, path of that checkpoint)."""
    folder = tmp_path_factory.mktemp("polyak_run") / "a"
    stepper, logs = _train(folder, shards, STEPS, ON)
    return stepper, logs, folder / "models" / "sample4.torch"


def test_run_train_checkpoints_the_target_in_the_models_names_and_shapes(trained):
    stepper, logs, src = trained
    assert any("soft target updates" in l and "TARGET_UPDATE_INTERVAL is unused" in l for l in logs)
    assert stepper.target_tau == 0.25 and not _same(stepper.target_params, stepper.net.params)
    snap = torch.load(src, map_location="cpu")
    assert list(snap) == ["sample_number", "model_state_dict", "optimizer_state_dict", "target_state_dict"]
    msd, tsd = snap["model_state_dict"], snap["target_state_dict"]
    assert list(tsd) == list(msd) and all(tsd[k].shape == msd[k].shape and tsd[k].dtype == msd[k].dtype for k in msd)
    assert not torch.equal(tsd["top.4.weight"], msd["top.4.weight"])
    assert torch.equal(tsd["resnet.bn1.running_mean"], msd["resnet.bn1.running_mean"])
    assert torch.equal(tsd["resnet.fc.weight"], msd["resnet.fc.weight"])  # the frozen tail: copied once, never moved


def test_run_train_two_resumes_from_one_checkpoint_agree(tmp_path, shards, trained):
    resumed = []
    for tag in ("r0", "r1"):
        _copy_checkpoint(trained[2], tmp_path / tag)
        r_stepper, r_logs = _train(tmp_path / tag, shards, STEPS, ON, resume_from=4)
        assert any("target weights restored from the checkpoint" in l for l in r_logs)
        resumed.append(r_stepper)
    assert _same(resumed[0].net.params, resumed[1].net.params) and _same(resumed[0].target_params, resumed[1].target_params)
    assert not _same(resumed[0].target_params, resumed[0].net.params)


def test_run_train_resumes_without_the_key_and_runs_without_the_feature(tmp_path, shards, trained):
    # the key deleted: the run says so and starts its target from the online weights
    _copy_checkpoint(trained[2], tmp_path / "n", drop="target_state_dict")
    n_stepper, n_logs = _train(tmp_path / "n", shards, STEPS, ON, resume_from=4)
    assert any("no target_state_dict" in l and "online weights" in l for l in n_logs)
    assert not any("restored from the checkpoint" in l for l in n_logs)
    assert n_stepper.target_params is not None
    # the key off: the parent's checkpoint keys, no log line, no allocation
    d_stepper, d_logs = _train(tmp_path / "d", shards, 4, "")
    assert list(torch.load(tmp_path / "d" / "models" / "sample4.torch", map_location="cpu")) == ["sample_number", "model_state_dict",
                                                                                                 "optimizer_state_dict"]
    assert d_stepper.target_params is None and not any("soft target" in l for l in d_logs)


def test_run_train_with_prioritized_replay_augmentation_and_cql(tmp_path, shards):
    extra = "PRIORITIZED_REPLAY: True\nAUG_SHIFT_PAD: 8\nAUG_FLIP: True\nCQL_ALPHA: 1.0\n"
    runs = [_train(tmp_path / tag, shards, 4, extra + "TARGET_TAU: 0.25\n")[0] for tag in ("p0", "p1")]
    assert _same(runs[0].net.params, runs[1].net.params) and _same(runs[0].target_params, runs[1].target_params)
    assert runs[0].replay is not None and runs[0].augmenter is not None and runs[0].cql_alpha == 1.0
    off = _train(tmp_path / "off", shards, 4, extra)[0]
    assert not _same(off.net.params, runs[0].net.params)


# ---- 5. two ranks on one GPU over gloo --------------------------------------------------------------------------------------------
def test_two_ranks_hold_one_target_and_agree_with_the_big_batch(tmp_path):
    """Two ranks x 4 samples (gloo, one device; tests/scripts/polyak_two_ranks.py) against one process on the 8 samples, two updates at
    tau 0.25: the ranks apply the same reduced gradient, so their params and target_params are bit-identical with no collective of
    the target's own; against the big batch both meet the bounds tests/test_gpu_optim.py's two-rank test sets for `params`."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "scripts"))
    import polyak_two_ranks as prog
    from test_gpu_ddp import _free_port
    B, world, tau = 4, 2, 0.25
    port = str(_free_port())
    script = os.path.join(ROOT, "tests", "scripts", "polyak_two_ranks.py")
    procs = [subprocess.Popen([sys.executable, script, str(r), str(world), port, str(tmp_path), str(B), repr(tau)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    try:
        outs = [p.communicate(timeout=240)[0] for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    for key in ("params", "target_params"):
        assert _same(ranks[0][key], ranks[1][key]), key
    big = prog.run(B * world, 1, 0, tau)
    nt = big["trainable"]
    assert not _same(big["target_params"][:nt], big["params"][:nt]) and not _same(big["target_params"], big["start"])
    for key in ("params", "target_params"):
        delta = (big[key][:nt] - ranks[0][key][:nt]).abs()
        print(f"two ranks against the big batch, {key}: max {delta.max().item():.3e}, mean {delta.mean().item():.3e}")
        assert delta.max().item() <= 2.5e-4 and delta.mean().item() < 2e-6
        assert _same(big[key][nt:], ranks[0][key][nt:])
