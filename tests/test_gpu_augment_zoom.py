"""Random-zoom augmentation on the GPU, all exact: the draw against the numpy oracle (tests/aug_zoom_oracle.py),
vdqn_pack_input_aug_zoom against vdqn_pack_input of host-augmented frames, one TDStepper update with the hooks against a plain update
on host-zoomed inputs, the refusals, run_train with the zoom keys, and a rank's slice of the one-process draw."""
import ctypes as C

import numpy as np
import pytest
import torch

import aug_color_oracle
import aug_oracle
import aug_zoom_oracle as oracle
from test_gpu_augment import _make, _u8_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = 65536
ID = oracle.IDENTITY
MAXO = oracle.MAX_ORIGIN
NEAR, FAR = oracle.origin(32768, 0), oracle.origin(32768, 0xFFFF)  # a 2 x zoom's origin with the window at the frame's two ends
ZERO = (0, 0, 0, 0)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _rows(*rows):
    return np.array(rows, np.int64).astype(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_aug_draw_zoom_matches_oracle():
    from video_dqn_amd.augment import aug_draw_zoom
    n_cases = 0
    for seed in (0, 7, 2**63 + 5):
        for step in (1, 99999):
            for G, first, n in ((256, 0, 256), (16, 5, 7)):
                for jz, aspect in ((0, False), (16384, False), (32768, True), (1, True)):
                    got = aug_draw_zoom(seed, step, G, first, n, jz, aspect, device=DEV)
                    assert got.dtype == torch.int32 and tuple(got.shape) == (n, 4)
                    ref = oracle.draw(seed, step, G, jz, aspect, first=first, n=n)
                    np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"seed={seed} step={step} G={G} first={first} jz={jz}")
                    n_cases += 1
    assert n_cases == 3 * 2 * 2 * 4
    d = oracle.draw(7, 1, 256, 32768, True)
    assert np.all(oracle.draw(7, 1, 256, 0, True) == np.array(ID)) and len(np.unique(d[:, 0])) > 200 and np.any(d[:, 0] != d[:, 1])


def test_augmenter_draws_its_rank_slice_and_leaves_the_other_draws_alone():
    from video_dqn_amd.augment import Augmenter, jq, jz
    B, world = 4, 2
    kw = dict(pad=8, flip=True, seed=11, brightness=0.4, saturation=1.0, zoom=0.25, zoom_aspect=True)
    assert jz(0.25) == 16384
    one = Augmenter(B * world, DEV, **kw)
    one.draw(6)
    whole = one.zoom.cpu().numpy()
    np.testing.assert_array_equal(whole, oracle.draw(11, 6, B * world, 16384, True))
    np.testing.assert_array_equal(one.params.cpu().numpy(), aug_oracle.draw(11, 6, B * world, 8, True))  # the shift stream did not move
    np.testing.assert_array_equal(one.color.cpu().numpy(), aug_color_oracle.draw(11, 6, B * world, jq(0.4), 0, jq(1.0)))  # nor the colour stream
    for rank in range(world):
        a = Augmenter(B, DEV, rank=rank, world_size=world, **kw)
        p = a.draw(6)
        assert p is a.params and a.zoom.dtype == torch.int32 and tuple(a.zoom.shape) == (B, 4) and a.last_step == 6
        np.testing.assert_array_equal(a.zoom.cpu().numpy(), whole[rank * B:(rank + 1) * B])
    assert Augmenter(B, DEV, pad=8, flip=True, seed=11, saturation=0.4).zoom is None
    only = Augmenter(B, DEV, seed=11, zoom=0.5)  # zoom alone: the shift params are the zeros vdqn_aug_draw gives for pad 0, no colour array
    assert not only.draw(3).any() and only.color is None
    np.testing.assert_array_equal(only.zoom.cpu().numpy(), oracle.draw(11, 3, B, 32768, False))
    # a resumed run draws what the uninterrupted run draws: the draw depends on the update number alone
    again = Augmenter(B, DEV, seed=11, zoom=0.5)
    only.draw(4), only.draw(5), again.draw(5)
    assert torch.equal(only.zoom, again.zoom)
    with pytest.raises(ValueError, match="AUG_ZOOM "):
        Augmenter(B, DEV, zoom=0.6)
    with pytest.raises(ValueError, match="AUG_ZOOM_ASPECT "):
        Augmenter(B, DEV, zoom_aspect=True)


# ---- the pack ------------------------------------------------------------------------------------------------------------------------
def _frames(F, seed=40):
    """3 samples of F frames: seeded random bytes, with one frame of all 0 and one of all 255."""
    fr = np.random.default_rng(seed + F).integers(0, 256, (3 * F, 224, 224, 3), dtype=np.uint8)
    fr[3 * F - 2], fr[3 * F - 1] = 0, 255
    return fr


CID = (256, 256, 256, 0)
# name -> (params, zoom rows, colour rows or None)
CASES = {
    "identity": (_rows(ZERO, ZERO, ZERO), _rows(ID, ID, ID), None),
    # 2 x zoom with the window at the frame's origin (the first tap clamps at 0) and at its far corner (the second at 223), and mixed
    "zoom2_corners": (_rows(ZERO, ZERO, ZERO), _rows((32768, 32768, NEAR, NEAR), (32768, 32768, FAR, FAR), (32768, 32768, FAR, NEAR)), None),
    "anisotropic": (_rows(ZERO, ZERO, ZERO), _rows((ONE, 32768, 0, FAR), (32768, ONE, NEAR, 0), (ONE, 32768, 0, NEAR)), None),
    # the largest shifts and the mirror under a zoom: the taps go through both clamps
    "shift_mirror": (_rows((32, -32, 0, 0), (-32, 32, 1, 0), (0, 0, 1, 0)),
                     _rows((32768, 32768, FAR, NEAR), (40000, 60000, oracle.origin(40000, 0x8000), oracle.origin(60000, 0xFFFF)), (32768, 32768, NEAR, FAR)), None),
    "colour": (_rows((5, -3, 1, 0), ZERO, (-8, 8, 0, 0)), _rows((45000, 45000, 700000, 2000000), (32768, 50000, FAR, 12345), ID),
               _rows((300, 200, 128, 0), (256, 256, 40, 0), (180, 330, 400, 0))),
    "colour_identity": (_rows((2, 1, 0, 0), ZERO, (0, 0, 1, 0)), _rows((50000, 36000, 99999, 3000000), (ONE, ONE, 32768, 32768), (33000, 65000, 7000000, 300)),
                        _rows(CID, CID, CID)),
    # fewer rows than samples: sample i takes row i % 2
    "wrap": (aug_oracle.draw(3, 5, 8, 8, True)[5:7], oracle.draw(3, 5, 8, 32768, True)[5:7], aug_color_oracle.draw(3, 5, 8, 102, 102, 102)[5:7]),
    "drawn": (aug_oracle.draw(9, 2, 3, 8, True), oracle.draw(9, 2, 3, 16384, True), None),
    "drawn_isotropic": (aug_oracle.draw(9, 3, 3, 0, False), oracle.draw(9, 3, 3, 32768, False), None),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_pack_input_aug_zoom_equals_pack_of_augmented_frames(dtype, F, case):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(F)
    n_img = 3 * F
    src = _dev(frames)
    params, zoom, color = CASES[case]
    # F = 1: the three frames are random, all 0 and all 255, so the rows are rotated over them; F = 4: nine random frames already
    for roll in (range(len(params)) if F == 1 else (0,)):
        par, zr = np.roll(params, roll, 0), np.roll(zoom, roll, 0)
        col = None if color is None else np.roll(color, roll, 0)
        got = pack_input_aug(src, _dev(par), F, dtype, color=None if col is None else _dev(col), zoom=_dev(zr))
        host = oracle.augment(frames, par, zr, col, F)
        ref = ops.pack_input(_dev(host), 0, n_img, dtype)
        assert got.dtype == dtype and got.shape == ref.shape == (n_img, 115, 115, 16)
        assert torch.equal(got, ref), (case, roll)
        plain = pack_input_aug(src, _dev(par), F, dtype, color=None if col is None else _dev(col))
        for i in range(3):
            same = torch.equal(got[i * F:(i + 1) * F], plain[i * F:(i + 1) * F])
            if tuple(zr[i % len(zr)]) == ID:
                assert same, (case, roll, i)
            elif i == 0:  # (a sample with random frames: a window that is not the frame must change the operand — no no-op kernel passes)
                assert not same, (case, roll, i)
        assert not got[:, :2].any() and not got[:, :, :2].any() and not got[..., 12:].any()  # the zero border and the padding channels


def test_out_of_range_rows_equal_the_clamped_ones():
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(1, seed=50)
    frames[1], frames[2] = frames[0][::-1], frames[0][:, ::-1]  # three frames with content
    src = _dev(frames)
    i32 = (-2**31, 2**31 - 1)
    wild = _rows((-5, 70000, i32[0], i32[1]), (i32[1], i32[0], -MAXO - 1, MAXO + 1), (0, ONE + 1, 12345, -77777))
    tame = _rows((0, ONE, -MAXO, MAXO), (ONE, 0, -MAXO, MAXO), (0, ONE, 12345, -77777))
    for par in (torch.zeros((3, 4), dtype=torch.int32, device=DEV), _dev(_rows((32, -32, 1, 0), (i32[0], i32[1], 7, 0), (-224, 224, 0, 0)))):
        for dtype in (torch.bfloat16, torch.float32):
            a = pack_input_aug(src, par, 1, dtype, zoom=_dev(wild))
            b = pack_input_aug(src, par, 1, dtype, zoom=_dev(tame))
            assert torch.equal(a, b)
    from video_dqn_amd import ops
    ref = ops.pack_input(_dev(oracle.zoom(frames, wild)), 0, 3, torch.float32)
    assert torch.equal(pack_input_aug(src, torch.zeros((3, 4), dtype=torch.int32, device=DEV), 1, torch.float32, zoom=_dev(wild)), ref)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_identity_zoom_equals_the_pack_without_zoom(dtype):
    from video_dqn_amd.augment import pack_input_aug
    for F in (1, 4):
        src = _dev(_frames(F, seed=60))
        par = _dev(aug_oracle.draw(3, 5, 3, 32, True))
        col = _dev(aug_color_oracle.draw(3, 5, 3, 102, 102, 102))
        ident = torch.tensor([ID] * 3, dtype=torch.int32, device=DEV)
        assert torch.equal(pack_input_aug(src, par, F, dtype, zoom=ident), pack_input_aug(src, par, F, dtype))
        assert torch.equal(pack_input_aug(src, par, F, dtype, color=col, zoom=ident), pack_input_aug(src, par, F, dtype, color=col))


# ---- the launcher's choice of one of the eight instances ------------------------------------------------------------------------------
# two samples of two frames; rows under which every shared piece of the pack matters: a shift beyond the frame under a mirror, a zoom
# row at a step of 1.0 with a fractional origin (its pairs stage all five rows), colour factors that are neither 1.0 nor clamped
DISPATCH_PARAMS = _rows((-260, 9, 1, 0), (11, -6, 1, 0))
DISPATCH_ZOOM = _rows((45000, ONE, 700000, 3 * ONE + 21845), (32768, 50000, FAR, 12345))
DISPATCH_COLOR = _rows((300, 200, 128, 0), (180, 330, 400, 0))
_dispatch_host = {}


def _dispatch_reference(with_zoom, with_color, first_row):
    """(the four frames, the rows from `first_row` on, the frames augmented on the host), computed once for both dtypes"""
    key = (with_zoom, with_color, first_row)
    if key not in _dispatch_host:
        frames = np.random.default_rng(77).integers(0, 256, (4, 224, 224, 3), dtype=np.uint8)
        par, zr, col = DISPATCH_PARAMS[first_row:], DISPATCH_ZOOM[first_row:], DISPATCH_COLOR[first_row:]
        host = aug_oracle.augment_frames(frames, par, 2)
        if with_zoom:
            host = oracle.zoom(host, zr, 2)
        if with_color:
            host = aug_color_oracle.color(host, col, 2)
        _dispatch_host[key] = (frames, par, zr, col, host)
    return _dispatch_host[key]


@pytest.mark.parametrize("with_color", [False, True], ids=["no_colour", "colour"])
@pytest.mark.parametrize("with_zoom", [False, True], ids=["no_zoom", "zoom"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_pack_entries_launch_the_instance_for_dtype_zoom_and_colour(dtype, with_zoom, with_color):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    assert any(len(oracle.source_rows(DISPATCH_ZOOM[0], DISPATCH_PARAMS[0][1], Y0)) == 5 for Y0 in range(0, 224, 4))
    for first_row in (0, 1):  # two rows, then one: both samples take it (% n_params)
        frames, par, zr, col, host = _dispatch_reference(with_zoom, with_color, first_row)
        got = pack_input_aug(_dev(frames), _dev(par), 2, dtype, color=_dev(col) if with_color else None, zoom=_dev(zr) if with_zoom else None)
        ref = ops.pack_input(_dev(host), 0, 4, dtype)
        assert got.dtype == dtype and got.shape == ref.shape == (4, 115, 115, 16)
        assert torch.equal(got, ref), first_row


# ---- one update with the hooks against a plain update on host-zoomed inputs -----------------------------------------------------------
def _step(stp, fb, fa, act, rew, term, gtb, **kw):
    gt = (rew * 0.5 + 0.25).contiguous().to(DEV) if gtb else None
    stp.step(_dev(fb), _dev(fa), 0, _dev(act), rew.to(DEV), term.to(DEV), gt=gt, **kw)
    torch.cuda.synchronize()
    return stp.loss.cpu().clone(), stp.q_before.cpu().clone(), stp.grads.cpu().clone(), stp.net.params.cpu().clone()


@pytest.mark.parametrize("dtype,gtb", [("f32", False), ("bf16", False), ("bf16x3", False), ("f32", True)],
                         ids=["f32", "bf16", "bf16x3", "f32_ground_truth"])
def test_step_with_zoom_equals_plain_step_on_zoomed_inputs(dtype, gtb):
    B = 4
    fb, fa, act, rew, term = _u8_batch(501, B)
    params = np.array([(8, -5, 1, 0), (0, 0, 0, 0), (-3, 2, 0, 0), (0, 6, 1, 0)], np.int32)
    zoom = _rows((40000, 52000, 1500000, 900000), (32768, 32768, FAR, NEAR), ID, (ONE, 33000, 0, 5000000))
    color = np.array([(300, 200, 128, 0), (256, 256, 256, 0), (180, 330, 400, 0), (256, 256, 0, 0)], np.int32)
    act2 = aug_oracle.swap_actions(act, params, 1, 2)
    _, stp_a = _make(dtype, B, True, gtb)
    _, stp_r = _make(dtype, B, True, gtb)
    _, stp_s = _make(dtype, B, True, gtb)
    par_d, zoom_d, col_d = _dev(params), _dev(zoom), _dev(color)
    got = _step(stp_a, fb, fa, act2, rew, term, gtb, augment=par_d, augment_zoom=zoom_d)
    ref = _step(stp_r, oracle.augment(fb, params, zoom), oracle.augment(fa, params, zoom), act2, rew, term, gtb)
    shift_only = _step(stp_s, fb, fa, act2, rew, term, gtb, augment=par_d)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got, ref):
        assert torch.equal(g, r), name
    assert not torch.equal(got[2], shift_only[2])  # the zoom rows reached the update
    # the second update: zoom together with colour
    fb2, fa2, act_n, rew2, term2 = _u8_batch(502, B)
    got2 = _step(stp_a, fb2, fa2, act_n, rew2, term2, gtb, augment=par_d, augment_color=col_d, augment_zoom=zoom_d)
    ref2 = _step(stp_r, oracle.augment(fb2, params, zoom, color), oracle.augment(fa2, params, zoom, color), act_n, rew2, term2, gtb)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got2, ref2):
        assert torch.equal(g, r), name
    # augment_zoom=None on the third: the hook was cleared
    fb3, fa3, act3, rew3, term3 = _u8_batch(503, B)
    got3 = _step(stp_a, fb3, fa3, act3, rew3, term3, gtb)
    ref3 = _step(stp_r, fb3, fa3, act3, rew3, term3, gtb)
    for name, g, r in zip(("loss", "Q(s)", "gradient", "parameters"), got3, ref3):
        assert torch.equal(g, r), name


def test_refusals():
    from video_dqn_amd import _lib, synth
    lib = _lib.load()
    B = 4
    net, stp = _make("f32", B)
    params = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    zoom = torch.tensor([ID] * B, dtype=torch.int32, device=DEV)
    fb, fa, act, rew, term = _u8_batch(503, B)
    before, after = _dev(fb), _dev(fa)
    rest = (_dev(act), rew.to(DEV), term.to(DEV))
    with pytest.raises(_lib.VdqnError, match="augment_zoom needs augment"):
        stp.step(before, after, 0, *rest, augment_zoom=zoom)
    for bad in (zoom[:2], zoom.to(torch.int64), zoom.cpu(), zoom[:, :3], zoom.t().contiguous().t()):
        with pytest.raises(_lib.VdqnError, match="augment_zoom must be"):
            stp.step(before, after, 0, *rest, augment=params, augment_zoom=bad)
    with pytest.raises(_lib.VdqnError, match="next_frames"):
        stp.step(before, after, 0, *rest, augment=params, augment_zoom=zoom, next_frames=(before, after, 0))
    (tup, _) = synth.make_batch(503, B, 1, structured=True, reward_p=0.3)
    with pytest.raises(_lib.VdqnError, match="src_kind"):  # f32 NCHW frames
        stp.step(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, *rest, augment=params, augment_zoom=zoom)
    assert stp.sample_number == 1  # (only the f32-frame call got as far as the engine, which refused it before any launch)
    # the engine's own checks, through the C entries: every call fails before a launch, nothing reads the addresses
    a = stp._args(before, after, 0, *rest, stp._ones, None, augment=params, augment_zoom=zoom)
    assert a.aug_zoom == zoom.data_ptr() and a.aug_params == params.data_ptr() and a.aug_color is None
    a.aug_params = None
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"vdqn_net_td_forward: aug_zoom is given without aug_params" in lib.vdqn_last_error()
    assert lib.vdqn_net_td_forward_cql(net.handle, C.byref(a), 0.5, None, _st()) != 0
    assert b"aug_zoom is given without aug_params" in lib.vdqn_last_error()
    assert lib.vdqn_net_td_forward_mc(net.handle, C.byref(a), 0.0, None, None, 0, None, _st()) != 0
    assert b"aug_zoom is given without aug_params" in lib.vdqn_last_error()
    a.aug_params = params.data_ptr()
    a.aug_zoom = zoom.data_ptr() + 4
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"aug_zoom" in lib.vdqn_last_error() and b"aligned" in lib.vdqn_last_error()
    a.aug_zoom = zoom.data_ptr()
    a.src_kind = 1
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"src_kind" in lib.vdqn_last_error()
    a.src_kind = 0
    a.packed_frames = stp._packed_buffer(0).data_ptr()
    assert lib.vdqn_net_td_forward(net.handle, C.byref(a), _st()) != 0
    assert b"packed_frames" in lib.vdqn_last_error()
    a.packed_frames = None
    # validation frames are not augmented
    stp.eval_begin()
    a.aug_params = None
    assert lib.vdqn_net_td_eval(net.handle, C.byref(a), stp.eval_acc.data_ptr(), _st()) != 0
    assert b"vdqn_net_td_eval: aug_zoom" in lib.vdqn_last_error()
    with pytest.raises(TypeError, match="augment_zoom"):
        stp.eval_batch(before, after, 0, *rest, augment_zoom=zoom)
    torch.cuda.synchronize()
    assert not stp.eval_acc.any()  # no refused call added anything


# ---- run_train -----------------------------------------------------------------------------------------------------------------------
SEED = 4
BASE = ("SYNTHETIC_DATA: True\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\nGAMMA: 0.99\nCHECKPOINT_INTERVAL: 100\n"
        f"NUM_STEPS: 4\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\nCOMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nTARGET_UPDATE_INTERVAL: 3\n")
HOOKS = ("augment", "augment_color", "augment_zoom")


def _train(folder, extra, monkeypatch):
    """-> (stepper, [(update number, augment, augment_color, augment_zoom) as the stepper's step() received them], log lines, running loss)"""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.engine import TDStepper
    from video_dqn_amd.trainer import run_train
    seen = []
    real = TDStepper.step

    def recording(self, *a, **kw):
        seen.append((self.sample_number + 1,) + tuple(None if kw.get(k) is None else kw[k].cpu().numpy().copy() for k in HOOKS))
        return real(self, *a, **kw)
    folder.mkdir()
    (folder / "config.yml").write_text(BASE + extra)
    logs = []
    with monkeypatch.context() as m:
        m.setattr(TDStepper, "step", recording)
        _, stepper, running = run_train(ExperimentConfig(str(folder), device=DEV, tensorboard=False), log=lambda *a: logs.append(" ".join(map(str, a))))
    return stepper, seen, logs, running


@pytest.mark.parametrize("extra,pad,flip,jqs,jz,aspect", [
    ("AUG_ZOOM: 0.25\n", 0, False, None, 16384, False),
    ("AUG_SHIFT_PAD: 8\nAUG_FLIP: True\nAUG_BRIGHTNESS: 0.4\nAUG_CONTRAST: 0.4\nAUG_SATURATION: 0.4\nAUG_ZOOM: 0.5\nAUG_ZOOM_ASPECT: True\n",
     8, True, (102, 102, 102), 32768, True),
], ids=["zoom_alone", "all_keys"])
def test_run_train_with_zoom_keys(tmp_path, monkeypatch, extra, pad, flip, jqs, jz, aspect):
    stepper, seen, logs, running = _train(tmp_path / "run", extra, monkeypatch)
    assert np.isfinite(running)
    assert [s[0] for s in seen] == [1, 2, 3, 4]
    for s, par, col, zr in seen:
        np.testing.assert_array_equal(zr, oracle.draw(SEED, s, 4, jz, aspect))
        np.testing.assert_array_equal(par, aug_oracle.draw(SEED, s, 4, pad, flip))
        if jqs is None:
            assert col is None
        else:
            np.testing.assert_array_equal(col, aug_color_oracle.draw(SEED, s, 4, *jqs))
    aug = stepper.augmenter
    assert aug is not None and aug.last_step == 4 and aug.jz == jz and aug.zoom_aspect == aspect
    line = [l for l in logs if l.startswith("augmentation:")]
    assert len(line) == 1 and f"random zoom to a window of [{1 - jz / 65536:g}, 1] of the frame" in line[0]
    assert ("independently" in line[0]) == aspect and ("shift" in line[0]) == (pad > 0) and ("colour" in line[0]) == (jqs is not None)


@pytest.mark.parametrize("extra,has_augmenter", [("", False), ("AUG_ZOOM: 0.0\nAUG_SHIFT_PAD: 8\n", True)], ids=["all_off", "shift_only"])
def test_run_train_with_zoom_off_builds_no_zoom_array(tmp_path, monkeypatch, extra, has_augmenter):
    stepper, seen, logs, running = _train(tmp_path / "run", extra, monkeypatch)
    assert np.isfinite(running) and [s[0] for s in seen] == [1, 2, 3, 4]
    assert all(zr is None and col is None for _, _, col, zr in seen)
    assert (stepper.augmenter is not None) == has_augmenter and all((par is not None) == has_augmenter for _, par, _, _ in seen)
    assert not any("random zoom" in l for l in logs) and any("augmentation:" in l for l in logs) == has_augmenter
    if has_augmenter:
        assert stepper.augmenter.zoom is None
