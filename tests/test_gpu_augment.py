"""Shift / mirror augmentation on the GPU, all exact: the draw and the action exchange against the numpy oracle
(tests/aug_oracle.py), vdqn_pack_input_aug against vdqn_pack_input of host-augmented frames, one TDStepper update with the hook
against a plain update on host-augmented inputs, run_train with AUG_SHIFT_PAD / AUG_FLIP (determinism, the draws of a fresh and
a resumed run, with prioritized replay), and two ranks over gloo against their slices of the one-process draw."""
import ctypes as C

import numpy as np
import pytest
import torch

import aug_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- 5. the draw and the action exchange ------------------------------------------------------------------------------------------
def test_aug_draw_matches_oracle():
    from video_dqn_amd.augment import aug_draw
    n_cases = 0
    for seed in (0, 7, 2**63 + 5):
        for step in (1, 99999):
            for G, first, n in ((8, 0, 8), (8, 3, 5), (256, 0, 256), (256, 128, 128), (4096, 0, 4096), (4096, 4000, 96)):
                for P, flip in ((0, True), (1, False), (8, True), (8, False), (32, True)):
                    got = aug_draw(seed, step, G, first, n, P, flip, DEV).cpu().numpy()
                    ref = aug_oracle.draw(seed, step, G, P, flip, first, n)
                    np.testing.assert_array_equal(got, ref, err_msg=f"seed={seed} step={step} G={G} first={first} P={P} flip={flip}")
                    n_cases += 1
    assert n_cases == 6 * 6 * 5


def test_aug_swap_actions_matches_oracle():
    from video_dqn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(0)
    n = 300
    act = rng.integers(0, 3, n).astype(np.int64)
    drawn = aug_oracle.draw(2, 9, n, 8, True)
    none, every = drawn.copy(), drawn.copy()
    none[:, 2], every[:, 2] = 0, 1
    odd = drawn.copy()
    odd[:, 2] *= 5  # flip != 0 means 1
    for params in (drawn, none, every, odd):
        for a0, a1 in ((1, 2), (2, 1), (0, 2)):
            out = torch.full((n,), -1, dtype=torch.int64, device=DEV)
            act_d, par_d = torch.from_numpy(act).to(DEV), torch.from_numpy(params).to(DEV)
            _lib.check(lib.vdqn_aug_swap_actions(act_d.data_ptr(), par_d.data_ptr(), n, a0, a1, out.data_ptr(), _st()), "vdqn_aug_swap_actions")
            np.testing.assert_array_equal(out.cpu().numpy(), aug_oracle.swap_actions(act, params, a0, a1))
    np.testing.assert_array_equal(aug_oracle.swap_actions(act, none), act)
    assert np.all(aug_oracle.swap_actions(act, every)[act == 1] == 2)


def test_augmenter_draws_its_rank_slice_and_exchanges_actions():
    from video_dqn_amd.augment import Augmenter
    B, world = 4, 3
    whole = aug_oracle.draw(11, 6, B * world, 8, True)
    act = torch.tensor([1, 2, 0, 1], dtype=torch.int64, device=DEV)
    for rank in range(world):
        a = Augmenter(B, DEV, pad=8, flip=True, flip_actions=[1, 2], seed=11, rank=rank, world_size=world)
        p = a.draw(6)
        assert p.dtype == torch.int32 and tuple(p.shape) == (B, 4) and a.last_step == 6
        np.testing.assert_array_equal(p.cpu().numpy(), whole[rank * B:(rank + 1) * B])
        np.testing.assert_array_equal(a.actions(act).cpu().numpy(), aug_oracle.swap_actions(act.cpu().numpy(), whole[rank * B:(rank + 1) * B]))
    a = Augmenter(B, DEV, pad=8, flip=False, seed=11)
    assert a.actions(act) is act and torch.all(a.draw(6)[:, 2] == 0)


# ---- 6. the pack ------------------------------------------------------------------------------------------------------------------
HAND = [(0, 0, 0), (32, 32, 0), (-32, 32, 0), (32, -32, 0), (-32, -32, 0), (0, 0, 1), (5, -3, 1), (1000, -1000, 7)]


def _frames_u8(seed, n, F):
    from video_dqn_amd import synth
    return np.ascontiguousarray(synth.make_frames_uint8(seed, "before", n, F, structured=True)).reshape(n * F, 224, 224, 3)


def _check_pack(frames, params, F, dtype):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    n_img = frames.shape[0]
    src = torch.from_numpy(frames).to(DEV)
    got = pack_input_aug(src, torch.from_numpy(params).to(DEV), F, dtype)
    ref = ops.pack_input(torch.from_numpy(aug_oracle.augment_frames(frames, params, F)).to(DEV), 0, n_img, dtype)
    plain = ops.pack_input(src, 0, n_img, dtype)
    assert got.dtype == dtype and got.shape == ref.shape
    assert torch.equal(got, ref), params.tolist()
    for i in range(n_img // F):
        p = params[i % len(params)]
        same = torch.equal(got[i * F:(i + 1) * F], plain[i * F:(i + 1) * F])
        assert same == (not p[:3].any()), (i, p.tolist())  # a non-zero param must change the operand: no no-op kernel passes


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("F", [1, 4])
def test_pack_input_aug_equals_pack_of_augmented_frames(dtype, F):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    for n in (1, 3, 8):
        frames = _frames_u8(20 + n, n, F)
        for start in range(0, len(HAND), n):
            params = np.array([HAND[(start + k) % len(HAND)] + (0,) for k in range(n)], np.int32)
            _check_pack(frames, params, F, dtype)
        _check_pack(frames, aug_oracle.draw(3, 5, n, 8, True), F, dtype)
        zero = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
        src = torch.from_numpy(frames).to(DEV)
        assert torch.equal(pack_input_aug(src, zero, F, dtype), ops.pack_input(src, 0, n * F, dtype))
    # fewer params than samples: sample i takes params[i % n_params]
    _check_pack(_frames_u8(31, 8, F), np.array([(2, 1, 0, 0), (0, 0, 0, 0), (-4, 7, 1, 0)], np.int32), F, dtype)


def test_one_pixel_shift_changes_almost_every_pixel():
    fr = _frames_u8(28, 2, 1)
    for p in ((1, 0, 0, 0), (0, 1, 0, 0)):
        moved = aug_oracle.augment_frames(fr, np.array([p], np.int32))
        share = (moved != fr).any(axis=-1).mean()
        print(f"{p}: {100 * share:.2f} % of the pixels change")
        assert share > 0.9


# ---- 7. one update with the hook against a plain update on host-augmented inputs --------------------------------------------------
def _u8_batch(seed, B, F=1):
    from video_dqn_amd import synth
    (tup, raw) = synth.make_batch(seed, B, F, structured=True, reward_p=0.3)
    fb = np.ascontiguousarray(raw[0]).reshape(B * F, 224, 224, 3)
    fa = np.ascontiguousarray(raw[1]).reshape(B * F, 224, 224, 3)
    return fb, fa, tup[2].numpy().astype(np.int64), tup[3].float(), tup[4].float()


def _make(dtype, B, extra_capacity=True, gtb=False, **kw):
    from video_dqn_amd import synth
    from video_dqn_amd.engine import NetEngine, TDStepper
    net = NetEngine(3, 5, 1, extra_capacity, dtype, 2 * B, deterministic=True)
    net.load_tensors(synth.make_state_dict(7, extra_capacity=extra_capacity))
    return net, TDStepper(net, B, lr=1e-4, gamma=0.99, clip_rect=True, train_on_ground_truth=gtb, **kw)


def _step(stp, fb, fa, act, rew, term, gtb, augment=None):
    gt = (rew * 0.5 + 0.25).contiguous().to(DEV) if gtb else None
    stp.step(torch.from_numpy(fb).to(DEV), torch.from_numpy(fa).to(DEV), 0, torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV),
             gt=gt, augment=augment)
    torch.cuda.synchronize()
    return stp.loss.cpu().clone(), stp.q_before.cpu().clone(), stp.grads.cpu().clone(), stp.net.params.cpu().clone()


@pytest.mark.parametrize("dtype,extra_capacity,gtb", [("f32", True, False), ("bf16", True, False), ("bf16x3", True, False), ("f32", False, False),
                                                     ("f32", True, True)], ids=["f32", "bf16", "bf16x3", "f32_basic", "f32_ground_truth"])
def test_step_with_hook_equals_plain_step_on_augmented_inputs(dtype, extra_capacity, gtb):
    B = 4
    fb, fa, act, rew, term = _u8_batch(501, B)
    params = np.array([(8, -5, 1, 0), (0, 0, 0, 0), (-3, 2, 0, 0), (0, 6, 1, 0)], np.int32)
    act2 = aug_oracle.swap_actions(act, params, 1, 2)
    net_a, stp_a = _make(dtype, B, extra_capacity, gtb)
    net_r, stp_r = _make(dtype, B, extra_capacity, gtb)
    net_p, stp_p = _make(dtype, B, extra_capacity, gtb)
    par_d = torch.from_numpy(params).to(DEV)
    act_d = torch.empty(B, dtype=torch.int64, device=DEV)
    from video_dqn_amd import _lib
    _lib.check(_lib.load().vdqn_aug_swap_actions(torch.from_numpy(act).to(DEV).data_ptr(), par_d.data_ptr(), B, 1, 2, act_d.data_ptr(), _st()),
               "vdqn_aug_swap_actions")
    np.testing.assert_array_equal(act_d.cpu().numpy(), act2)
    got = _step(stp_a, fb, fa, act_d.cpu().numpy(), rew, term, gtb, augment=par_d)
    ref = _step(stp_r, aug_oracle.augment_frames(fb, params), aug_oracle.augment_frames(fa, params), act2, rew, term, gtb)
    plain = _step(stp_p, fb, fa, act, rew, term, gtb)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got, ref):
        assert torch.equal(g, r), name
    assert not torch.equal(got[2], plain[2])  # the augmentation reached the update
    # augment=None on the next update: the hook was cleared
    fb2, fa2, act_n, rew2, term2 = _u8_batch(502, B)
    got2 = _step(stp_a, fb2, fa2, act_n, rew2, term2, gtb)
    ref2 = _step(stp_r, fb2, fa2, act_n, rew2, term2, gtb)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got2, ref2):
        assert torch.equal(g, r), name


def test_hook_refuses_f32_frames_and_packed_frames():
    from video_dqn_amd import _lib, synth
    lib = _lib.load()
    B = 4
    net, stp = _make("f32", B)
    params = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    (tup, _) = synth.make_batch(503, B, 1, structured=True, reward_p=0.3)
    f32 = [tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, tup[2].to(DEV), tup[3].float().to(DEV), tup[4].float().to(DEV)]
    with pytest.raises(_lib.VdqnError, match="src_kind"):
        stp.step(*f32, augment=params)
    fb, fa, act, rew, term = _u8_batch(503, B)
    before, after = torch.from_numpy(fb).to(DEV), torch.from_numpy(fa).to(DEV)
    a = stp._args(before, after, 0, torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV), stp._ones, None, augment=params)
    a.packed_frames = stp._packed_buffer(0).data_ptr()
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"packed_frames" in lib.vdqn_last_error()
    a.packed_frames = None
    a.aug_params = params.data_ptr() + 4  # not 16-byte aligned: refused before any launch (nothing ever reads the address)
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"aug_params" in lib.vdqn_last_error() and b"aligned" in lib.vdqn_last_error()
    torch.cuda.synchronize()
    for bad in (params[:2], params.to(torch.int64), params.cpu()):
        with pytest.raises(_lib.VdqnError, match="augment must be"):
            stp.step(before, after, 0, torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV), augment=bad)
    with pytest.raises(_lib.VdqnError, match="next_frames"):
        stp.step(before, after, 0, torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV), augment=params, next_frames=(before, after, 0))


# ---- 8. run_train -----------------------------------------------------------------------------------------------------------------
SEED, PAD = 4, 8


def _write_cfg(folder, shards, steps, extra=""):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 4\nNUM_STEPS: {steps}\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


AUG_ON = f"AUG_SHIFT_PAD: {PAD}\nAUG_FLIP: True\n"


def _train(folder, shards, steps, extra, monkeypatch, resume_from=-1):
    """-> (parameters, stepper, [(update number, params of that update)], log lines)"""
    from video_dqn_amd import augment
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.trainer import run_train
    draws = []
    real = augment.Augmenter.draw

    def recording(self, step):
        p = real(self, step)
        draws.append((int(step), p.cpu().numpy().copy()))
        return p
    _write_cfg(folder, shards, steps, extra)
    logs = []
    with monkeypatch.context() as m:
        m.setattr(augment.Augmenter, "draw", recording)
        model, stepper, running = run_train(ExperimentConfig(str(folder), device=DEV, tensorboard=False, resume=resume_from > -1),
                                            resume_from=resume_from, log=lambda *a: logs.append(" ".join(map(str, a))))
    assert np.isfinite(running)
    return model.engine.params.cpu().clone(), stepper, draws, logs


def test_run_train_with_augmentation(tmp_path, monkeypatch):
    from test_shards_cpu import _synthetic_shards
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    steps = 8
    runs = [_train(tmp_path / tag, shards, steps, AUG_ON, monkeypatch) for tag in ("a", "b")]
    assert torch.equal(runs[0][0], runs[1][0])  # bit-identical parameters, run to run
    params, stepper, draws, logs = runs[0]
    assert any("augmentation: random shift of up to 8 pixels, random left-right mirror with actions 1 <-> 2" in l for l in logs)
    assert [s for s, _ in draws] == list(range(1, steps + 1))
    for s, p in draws:
        np.testing.assert_array_equal(p, aug_oracle.draw(SEED, s, 4, PAD, True))
    assert stepper.augmenter.last_step == steps == stepper.sample_number
    np.testing.assert_array_equal(stepper.augmenter.params.cpu().numpy(), aug_oracle.draw(SEED, steps, 4, PAD, True))
    off, off_stepper, off_draws, off_logs = _train(tmp_path / "off", shards, steps, "", monkeypatch)
    assert off_stepper.augmenter is None and not off_draws and not any("augmentation" in l for l in off_logs)
    assert not torch.equal(off, params)
    # resume (-r 4): the reference's loop restarts at resume_from + 1 and increments before its first update (kept), so the
    # resumed run performs updates 6 .. 8 — and draws what the uninterrupted run drew at THOSE updates
    (tmp_path / "r").mkdir()
    (tmp_path / "r" / "models").mkdir()
    snap = torch.load(tmp_path / "a" / "models" / "sample4.torch", map_location="cpu")
    torch.save(snap, tmp_path / "r" / "models" / "sample4.torch")
    _, r_stepper, r_draws, _ = _train(tmp_path / "r", shards, steps, AUG_ON, monkeypatch, resume_from=4)
    assert [s for s, _ in r_draws] == [6, 7, 8]
    for (s, p), (s0, p0) in zip(r_draws, draws[5:]):
        assert s == s0
        np.testing.assert_array_equal(p, p0)
        np.testing.assert_array_equal(p, aug_oracle.draw(SEED, s, 4, PAD, True))
    # with prioritized replay as well: two runs bit-identical, and not the run without the augmentation
    per = [_train(tmp_path / tag, shards, steps, AUG_ON + "PRIORITIZED_REPLAY: True\n", monkeypatch)[0] for tag in ("p0", "p1")]
    assert torch.equal(per[0], per[1])
    per_off = _train(tmp_path / "p_off", shards, steps, "PRIORITIZED_REPLAY: True\n", monkeypatch)[0]
    assert not torch.equal(per[0], per_off)


def test_run_train_synthetic_loader_path_basic_architecture(tmp_path, monkeypatch):
    """The DataLoader + prefetcher input path (SYNTHETIC_DATA), ARCHITECTURE 'basic', bf16, four frames per sample: the draws are
    the oracle's, two runs end bit-identical, and the run differs from the one without the augmentation."""
    base = ("SYNTHETIC_DATA: True\nARCHITECTURE: 'basic'\nCOMPUTE_DTYPE: 'bf16'\nPANORAMA: True\n")
    outs = []
    for tag, extra in (("a", "AUG_SHIFT_PAD: 4\nAUG_FLIP: True\n"), ("b", "AUG_SHIFT_PAD: 4\nAUG_FLIP: True\n"), ("off", "")):
        params, stepper, draws, _ = _train(tmp_path / tag, "none", 3, base + extra, monkeypatch)
        assert stepper.net.num_frames == 4
        if extra:
            assert [s for s, _ in draws] == [1, 2, 3]
            for s, p in draws:
                np.testing.assert_array_equal(p, aug_oracle.draw(SEED, s, 4, 4, True))
        outs.append(params)
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---- 9. two ranks on one GPU over gloo (the harness of tests/test_gpu_replay.py, with uint8 frames) ---------------------------------
def _dp_run(B, world, rank, grad_hook=None, steps=3):
    from video_dqn_amd.augment import Augmenter
    net, stp = _make("f32", B, world_size=world, allreduce=grad_hook)
    aug = Augmenter(B, DEV, pad=8, flip=True, flip_actions=[1, 2], seed=5, rank=rank, world_size=world)
    G = B * world
    lo, hi = rank * B, (rank + 1) * B
    draws = []
    for s in range(1, steps + 1):
        fb, fa, act, rew, term = _u8_batch(700 + s, G)
        params = aug.draw(s)
        act_d = aug.actions(torch.from_numpy(act[lo:hi].copy()).to(DEV))
        stp.step(torch.from_numpy(fb[lo:hi].copy()).to(DEV), torch.from_numpy(fa[lo:hi].copy()).to(DEV), 0, act_d,
                 rew[lo:hi].contiguous().to(DEV), term[lo:hi].contiguous().to(DEV), augment=params)
        torch.cuda.synchronize()
        draws.append(params.cpu().clone())
    return net.params.cpu(), torch.stack(draws)


def _dp_worker(rank, world, port, out_dir, B):
    import os
    import sys
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)

    def through_host(t, stage=None):  # test transport (as test_gpu_ddp.py): whatever gloo's GPU support is
        torch.cuda.synchronize()
        h = t.cpu()
        dist.all_reduce(h)
        t.copy_(h)

    params, draws = _dp_run(B, world, rank, through_host)
    torch.save({"params": params, "draws": draws}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_draw_their_slices_and_equal_the_big_batch(tmp_path):
    """Two ranks x B = 4 on one GPU (gloo) against one process at batch 2B, three augmented updates (f32, deterministic, P = 8,
    mirror on): each rank's params are its slice of the G = 2B draw, the replicas stay bit-identical, and the parameters meet
    test_gpu_ddp.py's bound against the big batch (two lr-sized steps apart at worst, as there)."""
    import torch.multiprocessing as mp
    from test_gpu_ddp import _free_port
    B, world = 4, 2
    mp.spawn(_dp_worker, args=(world, _free_port(), str(tmp_path), B), nprocs=world, join=True)
    ranks = [torch.load(tmp_path / f"rank{r}.pt") for r in range(world)]
    assert torch.equal(ranks[0]["params"], ranks[1]["params"])
    params, draws = _dp_run(B * world, 1, 0)
    for s in range(3):
        ref = aug_oracle.draw(5, s + 1, B * world, 8, True)
        np.testing.assert_array_equal(draws[s].numpy(), ref)
        for r in range(world):
            np.testing.assert_array_equal(ranks[r]["draws"][s].numpy(), ref[r * B:(r + 1) * B])
    from video_dqn_amd.engine import NetEngine
    nt = NetEngine(3, 5, 1, True, "f32", 2 * B, deterministic=True).trainable_numel
    delta = (params[:nt] - ranks[0]["params"][:nt]).abs()
    print(f"two ranks against the big batch: max {delta.max().item():.3e}, mean {delta.mean().item():.3e}")
    assert delta.max().item() <= 2.5e-4 and delta.mean().item() < 2e-6
