"""Colour-jitter augmentation on the GPU, all exact: the draw against the numpy oracle (tests/aug_color_oracle.py),
vdqn_pack_input_aug_color against vdqn_pack_input of host-augmented frames, one TDStepper update with the two hooks against a plain
update on host-augmented inputs, the refusals, run_train with the colour keys, and a rank's slice of the one-process draw."""
import ctypes as C

import numpy as np
import pytest
import torch

import aug_color_oracle as oracle
import aug_oracle
from test_gpu_augment import _make, _u8_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ID = (256, 256, 256, 0)


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_aug_draw_color_matches_oracle():
    from video_dqn_amd.augment import aug_draw_color
    n_cases = 0
    for seed in (0, 7, 2**63 + 5):
        for step in (1, 99999):
            for G, first, n in ((256, 0, 256), (16, 5, 7)):
                for jqs in ((0, 0, 0), (8, 102, 256)):
                    got = aug_draw_color(seed, step, G, first, n, *jqs, device=DEV)
                    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
                    ref = oracle.draw(seed, step, G, *jqs, first=first, n=n)
                    np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"seed={seed} step={step} G={G} first={first} jq={jqs}")
                    n_cases += 1
    assert n_cases == 3 * 2 * 2 * 2
    assert np.all(oracle.draw(7, 1, 256, 0, 0, 0)[:, :3] == 256) and len(np.unique(oracle.draw(7, 1, 256, 8, 102, 256)[:, 2])) > 100


def test_augmenter_draws_its_rank_slice_and_leaves_the_shift_draw_alone():
    from video_dqn_amd.augment import Augmenter, jq
    B, world = 4, 2
    jqs = (jq(0.4), jq(0.03), jq(1.0))
    assert jqs == (102, 8, 256)
    one = Augmenter(B * world, DEV, pad=8, flip=True, seed=11, brightness=0.4, contrast=0.03, saturation=1.0)
    one.draw(6)
    whole = one.color.cpu().numpy()
    np.testing.assert_array_equal(whole, oracle.draw(11, 6, B * world, *jqs))
    np.testing.assert_array_equal(one.params.cpu().numpy(), aug_oracle.draw(11, 6, B * world, 8, True))  # the shift stream did not move
    for rank in range(world):
        a = Augmenter(B, DEV, pad=8, flip=True, seed=11, rank=rank, world_size=world, brightness=0.4, contrast=0.03, saturation=1.0)
        p = a.draw(6)
        assert p is a.params and a.color.dtype == torch.int32 and tuple(a.color.shape) == (B, 4) and a.last_step == 6
        np.testing.assert_array_equal(a.color.cpu().numpy(), whole[rank * B:(rank + 1) * B])
        np.testing.assert_array_equal(p.cpu().numpy(), aug_oracle.draw(11, 6, B * world, 8, True)[rank * B:(rank + 1) * B])
    assert Augmenter(B, DEV, pad=8, flip=True, seed=11).color is None
    only = Augmenter(B, DEV, seed=11, saturation=0.4)  # colour alone: the shift params are the zeros vdqn_aug_draw gives for pad 0
    assert not only.draw(3).any() and not aug_oracle.draw(11, 3, B, 0, False).any()
    np.testing.assert_array_equal(only.color.cpu().numpy(), oracle.draw(11, 3, B, 0, 0, jq(0.4)))
    with pytest.raises(ValueError, match="AUG_CONTRAST"):
        Augmenter(B, DEV, contrast=1.5)


# ---- the pack ------------------------------------------------------------------------------------------------------------------------
def _frames(F, seed=40):
    """3 samples of F frames: seeded random bytes, with one frame of all 0 and one of all 255."""
    fr = np.random.default_rng(seed + F).integers(0, 256, (3 * F, 224, 224, 3), dtype=np.uint8)
    fr[3 * F - 2], fr[3 * F - 1] = 0, 255
    return fr


def _rows(*rows):
    return np.array(rows, np.int64).astype(np.int32)  # (2**31 - 1 fits; negative values stay)


CASES = {
    # identity factors under the largest shifts and the mirror
    "identity_shifted": (_rows((32, -32, 0, 0), (-32, 32, 1, 0), (0, 0, 1, 0)), _rows(ID, ID, ID)),
    # the extremes of the clamped range, and values outside it: these must equal the clamped factors
    "extremes": (_rows((0, 0, 0, 0), (5, -3, 1, 0), (-8, 8, 0, 0)), _rows((0, 0, 0, 0), (512, 512, 512, 0), (-7, 100000, 2**31 - 1, 0))),
    "one_factor_each": (_rows((0, 0, 0, 0), (3, 1, 0, 0), (0, 0, 1, 0)), _rows((300, 256, 256, 0), (256, 200, 256, 0), (256, 256, 40, 5))),
    # fewer rows than samples: sample i takes row i % 2; the second row is a draw
    "wrap": (np.concatenate([_rows((2, 1, 0, 0)), aug_oracle.draw(3, 5, 8, 8, True)[6:7]]),
             np.concatenate([_rows((300, 200, 128, 0)), oracle.draw(3, 5, 8, 102, 102, 102)[6:7]])),
    "drawn": (aug_oracle.draw(9, 2, 3, 8, True), oracle.draw(9, 2, 3, 8, 102, 256)),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_pack_input_aug_color_equals_pack_of_augmented_frames(dtype, F, case):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(F)
    n_img = 3 * F
    assert not frames[n_img - 2].any() and frames[n_img - 1].min() == 255
    src = torch.from_numpy(frames).to(DEV)
    params, color = CASES[case]
    # F = 1: the three frames are random, all 0 and all 255, so the rows are rotated over them; F = 4: nine random frames already
    for roll in (range(len(params)) if F == 1 else (0,)):
        par, col = np.roll(params, roll, 0), np.roll(color, roll, 0)
        got = pack_input_aug(src, torch.from_numpy(par).to(DEV), F, dtype, color=torch.from_numpy(col).to(DEV))
        host = oracle.color(aug_oracle.augment_frames(frames, par, F), col, F)
        ref = ops.pack_input(torch.from_numpy(host).to(DEV), 0, n_img, dtype)
        assert got.dtype == dtype and got.shape == ref.shape == (n_img, 115, 115, 16)
        assert torch.equal(got, ref), (case, roll)
        plain = pack_input_aug(src, torch.from_numpy(par).to(DEV), F, dtype)
        clamped = np.clip(col.astype(np.int64), 0, 512)
        for i in range(3):
            is_id = tuple(clamped[i % len(col)][:3]) == ID[:3]
            same = torch.equal(got[i * F:(i + 1) * F], plain[i * F:(i + 1) * F])
            if is_id:
                assert same, (case, roll, i)
            elif i == 0:  # (a sample with random frames: a factor that is not 1.0 must change the operand — no no-op kernel passes)
                assert not same, (case, roll, i)
        assert not got[:, :2].any() and not got[:, :, :2].any() and not got[..., 12:].any()  # the zero border and the padding channels


def test_out_of_range_factors_equal_the_clamped_ones():
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(1, seed=50)
    src = torch.from_numpy(frames).to(DEV)
    par = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    wild = _rows((-7, 100000, 2**31 - 1, -1), (-2**31, 513, -1, 2**31 - 1), (2**31 - 1, -2**31, 100000, 3))
    tame = _rows((0, 512, 512, 0), (0, 512, 0, 0), (512, 0, 512, 0))
    for dtype in (torch.bfloat16, torch.float32):
        a = pack_input_aug(src, par, 1, dtype, color=torch.from_numpy(wild).to(DEV))
        b = pack_input_aug(src, par, 1, dtype, color=torch.from_numpy(tame).to(DEV))
        assert torch.equal(a, b)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_identity_factors_equal_the_pack_without_colour(dtype):
    from video_dqn_amd.augment import pack_input_aug
    for F in (1, 4):
        src = torch.from_numpy(_frames(F, seed=60)).to(DEV)
        par = torch.from_numpy(aug_oracle.draw(3, 5, 3, 32, True)).to(DEV)
        ident = torch.tensor([ID] * 3, dtype=torch.int32, device=DEV)
        assert torch.equal(pack_input_aug(src, par, F, dtype, color=ident), pack_input_aug(src, par, F, dtype))


# ---- one update with the two hooks against a plain update on host-augmented inputs ------------------------------------------------------
def _step(stp, fb, fa, act, rew, term, gtb, **kw):
    gt = (rew * 0.5 + 0.25).contiguous().to(DEV) if gtb else None
    stp.step(torch.from_numpy(fb).to(DEV), torch.from_numpy(fa).to(DEV), 0, torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV),
             gt=gt, **kw)
    torch.cuda.synchronize()
    return stp.loss.cpu().clone(), stp.q_before.cpu().clone(), stp.grads.cpu().clone(), stp.net.params.cpu().clone()


@pytest.mark.parametrize("dtype,gtb", [("f32", False), ("bf16", False), ("bf16x3", False), ("f32", True)],
                         ids=["f32", "bf16", "bf16x3", "f32_ground_truth"])
def test_step_with_colour_equals_plain_step_on_augmented_inputs(dtype, gtb):
    B = 4
    fb, fa, act, rew, term = _u8_batch(501, B)
    params = np.array([(8, -5, 1, 0), (0, 0, 0, 0), (-3, 2, 0, 0), (0, 6, 1, 0)], np.int32)
    color = np.array([(300, 200, 128, 0), (256, 256, 256, 0), (180, 330, 400, 0), (256, 256, 0, 0)], np.int32)
    act2 = aug_oracle.swap_actions(act, params, 1, 2)
    _, stp_a = _make(dtype, B, True, gtb)
    _, stp_r = _make(dtype, B, True, gtb)
    _, stp_s = _make(dtype, B, True, gtb)
    par_d, col_d = torch.from_numpy(params).to(DEV), torch.from_numpy(color).to(DEV)
    got = _step(stp_a, fb, fa, act2, rew, term, gtb, augment=par_d, augment_color=col_d)
    host_b = oracle.color(aug_oracle.augment_frames(fb, params), color)
    host_a = oracle.color(aug_oracle.augment_frames(fa, params), color)
    ref = _step(stp_r, host_b, host_a, act2, rew, term, gtb)
    shift_only = _step(stp_s, fb, fa, act2, rew, term, gtb, augment=par_d)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got, ref):
        assert torch.equal(g, r), name
    assert not torch.equal(got[2], shift_only[2])  # the colour factors reached the update
    # augment_color=None on the next update: the hook was cleared
    fb2, fa2, act_n, rew2, term2 = _u8_batch(502, B)
    got2 = _step(stp_a, fb2, fa2, act_n, rew2, term2, gtb)
    ref2 = _step(stp_r, fb2, fa2, act_n, rew2, term2, gtb)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got2, ref2):
        assert torch.equal(g, r), name


def test_refusals():
    from video_dqn_amd import _lib, synth
    lib = _lib.load()
    B = 4
    net, stp = _make("f32", B)
    params = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    color = torch.full((B, 4), 256, dtype=torch.int32, device=DEV)
    fb, fa, act, rew, term = _u8_batch(503, B)
    before, after = torch.from_numpy(fb).to(DEV), torch.from_numpy(fa).to(DEV)
    rest = (torch.from_numpy(act).to(DEV), rew.to(DEV), term.to(DEV))
    with pytest.raises(_lib.VdqnError, match="augment_color needs augment"):
        stp.step(before, after, 0, *rest, augment_color=color)
    for bad in (color[:2], color.to(torch.int64), color.cpu(), color[:, :3], color.t().contiguous().t()):
        with pytest.raises(_lib.VdqnError, match="augment_color must be"):
            stp.step(before, after, 0, *rest, augment=params, augment_color=bad)
    with pytest.raises(_lib.VdqnError, match="next_frames"):
        stp.step(before, after, 0, *rest, augment=params, augment_color=color, next_frames=(before, after, 0))
    (tup, _) = synth.make_batch(503, B, 1, structured=True, reward_p=0.3)
    with pytest.raises(_lib.VdqnError, match="src_kind"):
        stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, *rest, augment=params, augment_color=color)
    assert stp.sample_number == 1  # (only the f32-frame call got as far as the engine, which refused it before any launch)
    # the engine's own checks, through the C entry: every call fails before a launch, nothing reads the addresses
    a = stp._args(before, after, 0, *rest, stp._ones, None, augment=params, augment_color=color)
    assert a.aug_color == color.data_ptr() and a.aug_params == params.data_ptr()
    a.aug_params = None
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"vdqn_net_td_forward: aug_color is given without aug_params" in lib.vdqn_last_error()
    assert lib.vdqn_net_td_forward_cql(net.handle, C.byref(a), 0.5, None, _st()) != 0
    assert b"aug_color is given without aug_params" in lib.vdqn_last_error()
    a.aug_params = params.data_ptr()
    a.aug_color = color.data_ptr() + 4
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"aug_color" in lib.vdqn_last_error() and b"aligned" in lib.vdqn_last_error()
    a.aug_color = color.data_ptr()
    a.packed_frames = stp._packed_buffer(0).data_ptr()
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"packed_frames" in lib.vdqn_last_error()
    a.packed_frames = None
    # validation frames are not augmented
    stp.eval_begin()
    a.aug_params = None
    assert lib.vdqn_net_td_eval(net.handle, C.byref(a), stp.eval_acc.data_ptr(), _st()) != 0
    assert b"vdqn_net_td_eval: aug_color" in lib.vdqn_last_error()
    a.aug_params = params.data_ptr()
    assert lib.vdqn_net_td_eval(net.handle, C.byref(a), stp.eval_acc.data_ptr(), _st()) != 0
    assert b"vdqn_net_td_eval: aug_params" in lib.vdqn_last_error()
    with pytest.raises(TypeError, match="augment_color"):
        stp.eval_batch(before, after, 0, *rest, augment_color=color)
    torch.cuda.synchronize()
    assert not stp.eval_acc.any()  # no refused call added anything


# ---- run_train -----------------------------------------------------------------------------------------------------------------------
SEED = 4
BASE = ("SYNTHETIC_DATA: True\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\nGAMMA: 0.99\nCHECKPOINT_INTERVAL: 100\n"
        f"NUM_STEPS: 3\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\nCOMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nTARGET_UPDATE_INTERVAL: 3\n")


def _train(folder, extra, monkeypatch):
    """-> (stepper, [(update number, augment, augment_color) as the stepper's step() received them], log lines, running loss)"""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.engine import TDStepper
    from video_dqn_amd.trainer import run_train
    seen = []
    real = TDStepper.step

    def recording(self, *a, **kw):
        seen.append((self.sample_number + 1,) + tuple(None if kw.get(k) is None else kw[k].cpu().numpy().copy() for k in ("augment", "augment_color")))
        return real(self, *a, **kw)
    folder.mkdir()
    (folder / "config.yml").write_text(BASE + extra)
    logs = []
    with monkeypatch.context() as m:
        m.setattr(TDStepper, "step", recording)
        _, stepper, running = run_train(ExperimentConfig(str(folder), device=DEV, tensorboard=False), log=lambda *a: logs.append(" ".join(map(str, a))))
    return stepper, seen, logs, running


@pytest.mark.parametrize("extra,pad,flip,jqs", [
    ("AUG_SATURATION: 0.4\n", 0, False, (0, 0, 102)),
    ("AUG_SHIFT_PAD: 8\nAUG_FLIP: True\nAUG_BRIGHTNESS: 0.4\nAUG_CONTRAST: 0.4\nAUG_SATURATION: 0.4\n", 8, True, (102, 102, 102)),
], ids=["saturation_alone", "all_five_keys"])
def test_run_train_with_colour_keys(tmp_path, monkeypatch, extra, pad, flip, jqs):
    stepper, seen, logs, running = _train(tmp_path / "run", extra, monkeypatch)
    assert np.isfinite(running)
    assert [s for s, _, _ in seen] == [1, 2, 3]
    for s, par, col in seen:
        np.testing.assert_array_equal(col, oracle.draw(SEED, s, 4, *jqs))
        np.testing.assert_array_equal(par, aug_oracle.draw(SEED, s, 4, pad, flip))
    assert stepper.augmenter is not None and stepper.augmenter.last_step == 3 and stepper.augmenter.jq == jqs
    line = [l for l in logs if l.startswith("augmentation:")]
    assert len(line) == 1 and "colour jitter" in line[0] and "saturation x [0.6, 1.4]" in line[0]
    assert ("brightness" in line[0]) == (jqs[0] > 0) and ("random shift of up to 8 pixels, random left-right mirror" in line[0]) == flip
    assert ("shift" in line[0]) == (pad > 0)


@pytest.mark.parametrize("extra,has_augmenter", [("", False), ("AUG_BRIGHTNESS: 0.0\nAUG_SHIFT_PAD: 8\n", True)], ids=["all_off", "shift_only"])
def test_run_train_with_colour_keys_at_zero(tmp_path, monkeypatch, extra, has_augmenter):
    stepper, seen, logs, running = _train(tmp_path / "run", extra, monkeypatch)
    assert np.isfinite(running) and [s for s, _, _ in seen] == [1, 2, 3]
    assert all(col is None for _, _, col in seen)
    assert (stepper.augmenter is not None) == has_augmenter and all((par is not None) == has_augmenter for _, par, _ in seen)
    assert not any("colour" in l for l in logs) and any("augmentation:" in l for l in logs) == has_augmenter
    if has_augmenter:
        assert stepper.augmenter.color is None
