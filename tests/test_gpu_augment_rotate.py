"""Random-rotation augmentation on the GPU, all exact: the draw against the numpy oracle (tests/aug_rotate_oracle.py),
vdqn_pack_input_aug_affine against vdqn_pack_input of host-augmented frames, one TDStepper update with affine rows against a plain
update on host-rotated inputs (every compute mode, the ground-truth branch, CQL, IQL), the refusals, and run_train with AUG_ROTATE
(determinism, the draws of a fresh and a resumed run, with zoom and mirror, with prioritized replay, and switched off)."""
import numpy as np
import pytest
import torch

import aug_color_oracle
import aug_oracle
import aug_rotate_oracle as oracle
import aug_zoom_oracle
from test_gpu_augment import _make, _u8_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE = 65536
ID = oracle.IDENTITY
ZID = aug_zoom_oracle.IDENTITY
MAXO = oracle.MAX_ORIGIN
NEAR, FAR = aug_zoom_oracle.origin(32768, 0), aug_zoom_oracle.origin(32768, 0xFFFF)
ZERO = (0, 0, 0, 0)
CID = (256, 256, 256, 0)


def _rows(*rows):
    return np.array(rows, np.int64).astype(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _as_affine(zoom_rows):
    """Zoom rows {ax, ay, bx, by} as affine rows without cross terms."""
    z = np.asarray(zoom_rows).reshape(-1, 4)
    out = np.zeros((len(z), 8), np.int32)
    out[:, [0, 5, 2, 6]] = z
    return out


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_aug_draw_rotate_matches_oracle():
    from video_dqn_amd.augment import aug_draw_rotate
    n_cases = 0
    for seed in (0, 7, 2**63 + 5):
        for step in (1, 99999):
            for G, first, n in ((256, 0, 256), (16, 5, 7)):
                zr = aug_zoom_oracle.draw(seed, step, G, 32768, True, first=first, n=n)
                for jr in (0, 1, 640, 1920):
                    for zoom in (None, zr):
                        got = aug_draw_rotate(seed, step, G, first, n, jr, zoom=None if zoom is None else _dev(zoom), device=DEV)
                        assert got.dtype == torch.int32 and tuple(got.shape) == (n, 8)
                        ref = oracle.draw(seed, step, G, jr, zoom=zoom, first=first, n=n)
                        np.testing.assert_array_equal(got.cpu().numpy(), ref, err_msg=f"seed={seed} step={step} G={G} first={first} jr={jr}")
                        n_cases += 1
    assert n_cases == 3 * 2 * 2 * 4 * 2
    d = oracle.draw(7, 1, 256, 1920)
    assert len(np.unique(d[:, 1])) > 200 and d[:, 1].min() < -30000 and d[:, 1].max() > 30000 and np.all(d[:, 4] == -d[:, 1])


def test_augmenter_with_rotation_leaves_the_other_draws_alone():
    from video_dqn_amd.augment import Augmenter, jq
    B, world = 4, 2
    kw = dict(pad=8, flip=True, seed=11, brightness=0.4, saturation=1.0, zoom=0.25, zoom_aspect=True)
    off = Augmenter(B * world, DEV, **kw)
    on = Augmenter(B * world, DEV, rotate=10.0, **kw)
    assert off.affine is None and Augmenter(B, DEV, rotate=0.0, **kw).affine is None and on.jr == 640
    off.draw(6), on.draw(6)
    for name in ("params", "color", "zoom"):
        assert torch.equal(getattr(on, name), getattr(off, name)), name
    np.testing.assert_array_equal(on.params.cpu().numpy(), aug_oracle.draw(11, 6, B * world, 8, True))
    np.testing.assert_array_equal(on.color.cpu().numpy(), aug_color_oracle.draw(11, 6, B * world, jq(0.4), 0, jq(1.0)))
    zr = aug_zoom_oracle.draw(11, 6, B * world, 16384, True)
    np.testing.assert_array_equal(on.zoom.cpu().numpy(), zr)
    whole = on.affine.cpu().numpy()
    assert on.affine.dtype == torch.int32 and whole.shape == (B * world, 8)
    np.testing.assert_array_equal(whole, oracle.draw(11, 6, B * world, 640, zoom=zr))
    for rank in range(world):  # a rank draws its slice of the one global draw
        a = Augmenter(B, DEV, rank=rank, world_size=world, rotate=10.0, **kw)
        a.draw(6)
        np.testing.assert_array_equal(a.affine.cpu().numpy(), whole[rank * B:(rank + 1) * B])
    only = Augmenter(B, DEV, seed=11, rotate=30.0)  # rotation alone: zero shift params, no colour and no zoom array
    assert not only.draw(3).any() and only.color is None and only.zoom is None
    np.testing.assert_array_equal(only.affine.cpu().numpy(), oracle.draw(11, 3, B, 1920))
    again = Augmenter(B, DEV, seed=11, rotate=30.0)  # the draw depends on the update number alone
    only.draw(4), only.draw(5), again.draw(5)
    assert torch.equal(only.affine, again.affine)
    with pytest.raises(ValueError, match="AUG_ROTATE "):
        Augmenter(B, DEV, rotate=30.5)


# ---- the pack ------------------------------------------------------------------------------------------------------------------------
def _frames(F, seed=40):
    """3 samples of F frames: seeded random bytes, with one frame of all 0 and one of all 255."""
    fr = np.random.default_rng(seed + F).integers(0, 256, (3 * F, 224, 224, 3), dtype=np.uint8)
    fr[3 * F - 2], fr[3 * F - 1] = 0, 255
    return fr


Z2 = ((32768, 32768, NEAR, NEAR), (32768, 32768, FAR, FAR), (32768, 32768, FAR, NEAR))
# name -> (params, affine rows, colour rows or None)
CASES = {
    "identity": (_rows(ZERO, ZERO, ZERO), _rows(ID, ID, ID), None),
    "zoom_rows": (_rows((5, -3, 1, 0), ZERO, (-8, 8, 0, 0)), _as_affine(_rows((45000, 45000, 700000, 2000000), (32768, 50000, FAR, 12345), Z2[1])), None),
    # the largest angle at step 1.0: the largest tile footprint
    "largest_angle": (_rows(ZERO, ZERO, ZERO), _rows(oracle.compose(1920), oracle.compose(-1920), oracle.compose(1919)), None),
    "largest_angle_zoom2_corners": (_rows(ZERO, ZERO, ZERO), _rows(oracle.compose(1920, Z2[0]), oracle.compose(-1920, Z2[1]), oracle.compose(1920, Z2[2])), None),
    # the largest shifts and the mirror under a rotation: the taps go through both clamps
    "shift_mirror": (_rows((32, -32, 0, 0), (-32, 32, 1, 0), (0, 0, 1, 0)),
                     _rows(oracle.compose(-1920, Z2[2]), oracle.compose(700, (40000, 60000, 1234567, 345678)), oracle.compose(1920)), None),
    "colour": (_rows((5, -3, 1, 0), ZERO, (-8, 8, 0, 0)), _rows(oracle.compose(333, (45000, 45000, 700000, 2000000)), oracle.compose(-1920), oracle.compose(5)),
               _rows((300, 200, 128, 0), (256, 256, 40, 0), (180, 330, 400, 0))),
    "colour_identity": (_rows((2, 1, 0, 0), ZERO, (0, 0, 1, 0)), _rows(oracle.compose(1920), oracle.compose(-640, Z2[1]), oracle.compose(64)),
                        _rows(CID, CID, CID)),
    # fewer rows than samples: sample i takes row i % 2
    "wrap": (aug_oracle.draw(3, 5, 8, 8, True)[5:7], oracle.draw(3, 5, 8, 1920, zoom=aug_zoom_oracle.draw(3, 5, 8, 32768, True))[5:7],
             aug_color_oracle.draw(3, 5, 8, 102, 102, 102)[5:7]),
    "drawn": (aug_oracle.draw(9, 2, 3, 8, True), oracle.draw(9, 2, 3, 640, zoom=aug_zoom_oracle.draw(9, 2, 3, 16384, True)), None),
    "drawn_rotation_alone": (aug_oracle.draw(9, 3, 3, 0, False), oracle.draw(9, 3, 3, 1920), None),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("F", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_pack_input_aug_affine_equals_pack_of_augmented_frames(dtype, F, case):
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(F)
    n_img = 3 * F
    src = _dev(frames)
    params, affine, color = CASES[case]
    # F = 1: the three frames are random, all 0 and all 255, so the rows are rotated over them; F = 4: nine random frames already
    for roll in (range(len(params)) if F == 1 else (0,)):
        par, ar = np.roll(params, roll, 0), np.roll(affine, roll, 0)
        col = None if color is None else np.roll(color, roll, 0)
        col_d = None if col is None else _dev(col)
        got = pack_input_aug(src, _dev(par), F, dtype, color=col_d, affine=_dev(ar))
        host = oracle.augment(frames, par, ar, col, F)
        ref = ops.pack_input(_dev(host), 0, n_img, dtype)
        assert got.dtype == dtype and got.shape == ref.shape == (n_img, 115, 115, 16)
        assert torch.equal(got, ref), (case, roll)
        plain = pack_input_aug(src, _dev(par), F, dtype, color=col_d)
        for i in range(3):
            same = torch.equal(got[i * F:(i + 1) * F], plain[i * F:(i + 1) * F])
            if tuple(ar[i % len(ar)]) == ID:
                assert same, (case, roll, i)  # the identity equals the pack without rows
            elif i == 0:  # (a sample with random frames: a map that is not the identity must change the operand — no no-op kernel passes)
                assert not same, (case, roll, i)
        if not ar[:, [1, 4]].any():  # rows without cross terms: the zoom entry's bits
            assert torch.equal(got, pack_input_aug(src, _dev(par), F, dtype, color=col_d, zoom=_dev(ar[:, [0, 5, 2, 6]])))
        assert not got[:, :2].any() and not got[:, :, :2].any() and not got[:, 114].any() and not got[:, :, 114].any()  # the zero border
        assert not got[..., 12:].any()  # the padding channels


def test_wild_rows_equal_the_clamped_ones():
    from video_dqn_amd import ops
    from video_dqn_amd.augment import pack_input_aug
    frames = _frames(1, seed=50)
    frames[1], frames[2] = frames[0][::-1], frames[0][:, ::-1]  # three frames with content
    src = _dev(frames)
    i32 = (-2**31, 2**31 - 1)
    wild = _rows((-5, 70000, i32[0], 99, i32[1], 70000, i32[1], -1), (i32[1], i32[0], -MAXO - 1, 5, i32[0], i32[1], MAXO + 1, 6),
                 (ONE + 1, -ONE - 1, 12345, i32[0], ONE + 7, 3 * ONE, -77777, i32[1]))
    tame = _rows((0, ONE, -MAXO, 0, ONE, ONE, MAXO, 0), (ONE, -ONE, -MAXO, 0, -ONE, ONE, MAXO, 0), (ONE, -ONE, 12345, 0, ONE, ONE, -77777, 0))
    np.testing.assert_array_equal(oracle.clamp_rows(wild), tame)
    zero = torch.zeros((3, 4), dtype=torch.int32, device=DEV)
    for par in (zero, _dev(_rows((32, -32, 1, 0), (i32[0], i32[1], 7, 0), (-224, 224, 0, 0)))):
        for dtype in (torch.bfloat16, torch.float32):
            assert torch.equal(pack_input_aug(src, par, 1, dtype, affine=_dev(wild)), pack_input_aug(src, par, 1, dtype, affine=_dev(tame)))
    ref = ops.pack_input(_dev(oracle.affine(frames, wild)), 0, 3, torch.float32)
    assert torch.equal(pack_input_aug(src, zero, 1, torch.float32, affine=_dev(wild)), ref)
    # the largest footprint the clamps allow, step 1.0 on every term, at both signs of the cross terms and from inside the frame
    big = _rows((ONE, ONE, -100 * ONE, 0, -ONE, ONE, 120 * ONE, 0), (ONE, -ONE, 111 * ONE + 4321, 0, ONE, ONE, -111 * ONE + 99, 0), (ONE, ONE, 0, 0, ONE, ONE, 0, 0))
    ref = ops.pack_input(_dev(oracle.affine(frames, big)), 0, 3, torch.bfloat16)
    assert torch.equal(pack_input_aug(src, zero, 1, torch.bfloat16, affine=_dev(big)), ref)


# ---- one update with affine rows against a plain update on host-rotated inputs ----------------------------------------------------------
def _step(stp, fb, fa, act, rew, term, gtb=False, **kw):
    gt = (rew * 0.5 + 0.25).contiguous().to(DEV) if gtb else None
    stp.step(_dev(fb), _dev(fa), 0, _dev(act), rew.to(DEV), term.to(DEV), gt=gt, **kw)
    torch.cuda.synchronize()
    return stp.loss.cpu().clone(), stp.q_before.cpu().clone(), stp.grads.cpu().clone(), stp.net.params.cpu().clone()


B = 4
PARAMS = np.array([(8, -5, 1, 0), (0, 0, 0, 0), (-3, 2, 0, 0), (0, 6, 1, 0)], np.int32)
AFFINE = _rows(oracle.compose(1920, (40000, 52000, 1500000, 900000)), oracle.compose(-1920, (32768, 32768, FAR, NEAR)), ID, oracle.compose(640))
COLOR = np.array([(300, 200, 128, 0), (256, 256, 256, 0), (180, 330, 400, 0), (256, 256, 0, 0)], np.int32)
NAMES = ("loss", "Q(s)", "gradient", "parameters")
_host = {}


def _batch(seed, color=False):
    """(frames of s, of s', those rotated on the host, actions with the mirrored samples' exchanged, rewards, terminals), made once"""
    key = (seed, color)
    if key not in _host:
        fb, fa, act, rew, term = _u8_batch(seed, B)
        col = COLOR if color else None
        _host[key] = (fb, fa, oracle.augment(fb, PARAMS, AFFINE, col), oracle.augment(fa, PARAMS, AFFINE, col),
                      aug_oracle.swap_actions(act, PARAMS, 1, 2), rew, term)
    return _host[key]


@pytest.mark.parametrize("dtype,gtb", [("f32", False), ("bf16", False), ("bf16x3", False), ("f32", True)],
                         ids=["f32", "bf16", "bf16x3", "f32_ground_truth"])
def test_step_with_affine_rows_equals_plain_step_on_rotated_inputs(dtype, gtb):
    _, stp_a = _make(dtype, B, True, gtb)
    _, stp_r = _make(dtype, B, True, gtb)
    _, stp_s = _make(dtype, B, True, gtb)
    par_d, aff_d, col_d = _dev(PARAMS), _dev(AFFINE), _dev(COLOR)
    fb, fa, hb, ha, act, rew, term = _batch(501)
    got = _step(stp_a, fb, fa, act, rew, term, gtb, augment=par_d, augment_affine=aff_d)
    ref = _step(stp_r, hb, ha, act, rew, term, gtb)
    shift_only = _step(stp_s, fb, fa, act, rew, term, gtb, augment=par_d)
    for name, g, r in zip(NAMES, got, ref):
        assert torch.equal(g, r), name
    assert not torch.equal(got[2], shift_only[2])  # the rows reached the update
    nbytes = 2 * B * 115 * 115 * 16 * (2 if dtype == "bf16" else 4)
    assert stp_a._packed_bufs[0].numel() == nbytes and stp_a._packed_bufs[1] is None and stp_r._packed_bufs == [None, None]
    # the second update: rotation together with colour
    fb2, fa2, hb2, ha2, act2, rew2, term2 = _batch(502, color=True)
    got2 = _step(stp_a, fb2, fa2, act2, rew2, term2, gtb, augment=par_d, augment_color=col_d, augment_affine=aff_d)
    ref2 = _step(stp_r, hb2, ha2, act2, rew2, term2, gtb)
    for name, g, r in zip(NAMES, got2, ref2):
        assert torch.equal(g, r), name
    # no affine rows on the third: a stepper that took some earlier performs the plain step
    fb3, fa3, act3, rew3, term3 = _u8_batch(503, B)
    got3 = _step(stp_a, fb3, fa3, act3, rew3, term3, gtb)
    ref3 = _step(stp_r, fb3, fa3, act3, rew3, term3, gtb)
    for name, g, r in zip(NAMES, got3, ref3):
        assert torch.equal(g, r), name


def test_step_with_affine_rows_under_cql():
    _, stp_a = _make("f32", B, cql_alpha=0.5)
    _, stp_r = _make("f32", B, cql_alpha=0.5)
    fb, fa, hb, ha, act, rew, term = _batch(501)
    got = _step(stp_a, fb, fa, act, rew, term, augment=_dev(PARAMS), augment_affine=_dev(AFFINE))
    ref = _step(stp_r, hb, ha, act, rew, term)
    for name, g, r in zip(NAMES, got, ref):
        assert torch.equal(g, r), name
    assert torch.equal(stp_a.cql_penalty, stp_r.cql_penalty) and float(stp_a.cql_penalty) > 0


def test_step_with_affine_rows_under_iql():
    """The IQL target pass reads the `before` half of the packed frames."""
    from test_gpu_iql import _stepper
    _, stp_a = _stepper("f32", B, iql_expectile=0.7)
    _, stp_r = _stepper("f32", B, iql_expectile=0.7)
    fb, fa, hb, ha, act, rew, term = _batch(501)
    got = _step(stp_a, fb, fa, act, rew, term, augment=_dev(PARAMS), augment_affine=_dev(AFFINE))
    ref = _step(stp_r, hb, ha, act, rew, term)
    for name, g, r in zip(NAMES, got, ref):
        assert torch.equal(g, r), name
    assert torch.equal(stp_a.iql_stats, stp_r.iql_stats)


def test_refusals():
    from video_dqn_amd import _lib, synth
    _, stp = _make("f32", B)
    params = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
    aff = torch.tensor([ID] * B, dtype=torch.int32, device=DEV)
    zoom = torch.tensor([ZID] * B, dtype=torch.int32, device=DEV)
    fb, fa, act, rew, term = _u8_batch(503, B)
    before, after = _dev(fb), _dev(fa)
    rest = (_dev(act), rew.to(DEV), term.to(DEV))
    for call in (stp.step, stp.forward_backward):
        with pytest.raises(_lib.VdqnError, match="augment_affine needs augment"):
            call(before, after, 0, *rest, augment_affine=aff)
        with pytest.raises(_lib.VdqnError, match="augment_affine and augment_zoom are both given"):
            call(before, after, 0, *rest, augment=params, augment_zoom=zoom, augment_affine=aff)
        for bad in (aff[:2], aff.to(torch.int64), aff.cpu(), aff[:, :4].contiguous(), aff.t().contiguous().t()):
            with pytest.raises(_lib.VdqnError, match="augment_affine must be"):
                call(before, after, 0, *rest, augment=params, augment_affine=bad)
        with pytest.raises(_lib.VdqnError, match="next_frames"):
            call(before, after, 0, *rest, augment=params, augment_affine=aff, next_frames=(before, after, 0))
        (tup, _) = synth.make_batch(503, B, 1, structured=True, reward_p=0.3)
        with pytest.raises(_lib.VdqnError, match="augment_affine takes uint8 NHWC frames .src_kind 0., not src_kind 1"):  # f32 NCHW frames
            call(tup[0].contiguous().to(DEV), tup[1].contiguous().to(DEV), 1, *rest, augment=params, augment_affine=aff)
    assert stp.sample_number == 0 and stp._packed_bufs == [None, None]  # every call was refused before anything was counted or allocated
    with pytest.raises(TypeError, match="augment_affine"):  # validation frames are never augmented
        stp.eval_batch(before, after, 0, *rest, augment_affine=aff)


def test_affine_rows_discard_a_pending_pack_ahead():
    _, stp_a = _make("f32", B)
    _, stp_r = _make("f32", B)
    fb, fa, hb, ha, act, rew, term = _batch(501)
    fb0, fa0, act0, rew0, term0 = _u8_batch(503, B)
    nb, na = _dev(fb), _dev(fa)
    stp_a.step(_dev(fb0), _dev(fa0), 0, _dev(act0), rew0.to(DEV), term0.to(DEV), next_frames=(nb, na, 0))
    assert stp_a._ahead is not None
    stp_a.step(nb, na, 0, _dev(act), rew.to(DEV), term.to(DEV), augment=_dev(PARAMS), augment_affine=_dev(AFFINE))
    assert stp_a._ahead is None
    _step(stp_r, fb0, fa0, act0, rew0, term0)
    ref = _step(stp_r, hb, ha, act, rew, term)
    torch.cuda.synchronize()
    assert torch.equal(stp_a.net.params.cpu(), ref[3]) and torch.equal(stp_a.grads.cpu(), ref[2])


# ---- run_train -----------------------------------------------------------------------------------------------------------------------
SEED = 4
HOOKS = ("augment", "augment_color", "augment_zoom", "augment_affine")


def _write_cfg(folder, shards, steps, extra):
    folder.mkdir(exist_ok=True)
    (folder / "config.yml").write_text(
        f"DATASET: '{shards}'\nPANORAMA: False\nLOSS_CLIP: 'rect'\nARCHITECTURE: 'extra_capacity'\nLEARNING_RATE: 0.0001\n"
        f"GAMMA: 0.99\nUSE_INVERSE_ACTIONS: True\nCHECKPOINT_INTERVAL: 4\nNUM_STEPS: {steps}\nSEED: {SEED}\nBATCH_SIZE: 4\nNUM_WORKERS: 0\n"
        "COMPUTE_DTYPE: 'f32'\nDETERMINISTIC: True\nDEVICE_RESIDENT_DATA: 'on'\nTARGET_UPDATE_INTERVAL: 3\n" + extra)


def _train(folder, shards, steps, extra, monkeypatch, resume_from=-1):
    """-> (parameters, stepper, [(update number, augment, augment_color, augment_zoom, augment_affine) as step() received them], log lines)"""
    from video_dqn_amd.config import ExperimentConfig
    from video_dqn_amd.engine import TDStepper
    from video_dqn_amd.trainer import run_train
    seen = []
    real = TDStepper.step

    def recording(self, *a, **kw):
        seen.append((self.sample_number + 1,) + tuple(None if kw.get(k) is None else kw[k].cpu().numpy().copy() for k in HOOKS))
        return real(self, *a, **kw)
    _write_cfg(folder, shards, steps, extra)
    logs = []
    with monkeypatch.context() as m:
        m.setattr(TDStepper, "step", recording)
        model, stepper, running = run_train(ExperimentConfig(str(folder), device=DEV, tensorboard=False, resume=resume_from > -1),
                                            resume_from=resume_from, log=lambda *a: logs.append(" ".join(map(str, a))))
    assert np.isfinite(running)
    return model.engine.params.cpu().clone(), stepper, seen, logs


@pytest.fixture(scope="module")
def shards(tmp_path_factory):
    from test_shards_cpu import _synthetic_shards
    path = str(tmp_path_factory.mktemp("rotate") / "shards")
    _synthetic_shards(path)
    return path


@pytest.fixture(scope="module")
def unaugmented(shards, tmp_path_factory):
    """The parameters after 8 updates without augmentation, without and with prioritized replay."""
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for tag, extra in (("off", ""), ("per_off", "PRIORITIZED_REPLAY: True\n")):
            out[tag] = _train(tmp_path_factory.mktemp(tag) / "run", shards, 8, extra, mp)[0]
    return out


def test_run_train_with_rotation_alone_and_resumed(tmp_path, monkeypatch, shards, unaugmented):
    steps = 8
    runs = [_train(tmp_path / tag, shards, steps, "AUG_ROTATE: 10\n", monkeypatch) for tag in ("a", "b")]
    assert torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], unaugmented["off"])
    params, stepper, seen, logs = runs[0]
    line = [l for l in logs if l.startswith("augmentation:")]
    assert len(line) == 1 and "random rotation by up to ±10°" in line[0] and "zoom" not in line[0] and "shift" not in line[0]
    assert [s[0] for s in seen] == list(range(1, steps + 1))
    for s, par, col, zr, ar in seen:
        assert not par.any() and col is None and zr is None
        np.testing.assert_array_equal(ar, oracle.draw(SEED, s, 4, 640))
    assert stepper.augmenter.jr == 640 and stepper.augmenter.last_step == steps and stepper._packed_bufs[0] is not None
    # resume (-r 4) performs updates 6 .. 8 and draws what the oracle gives for THOSE update numbers
    (tmp_path / "r" / "models").mkdir(parents=True)
    torch.save(torch.load(tmp_path / "a" / "models" / "sample4.torch", map_location="cpu"), tmp_path / "r" / "models" / "sample4.torch")
    _, _, r_seen, _ = _train(tmp_path / "r", shards, steps, "AUG_ROTATE: 10\n", monkeypatch, resume_from=4)
    assert [s[0] for s in r_seen] == [6, 7, 8]
    for s, _, _, _, ar in r_seen:
        np.testing.assert_array_equal(ar, oracle.draw(SEED, s, 4, 640))


def test_run_train_with_rotation_zoom_and_mirror(tmp_path, monkeypatch, shards, unaugmented):
    extra = "AUG_ROTATE: 10\nAUG_ZOOM: 0.25\nAUG_FLIP: True\n"
    runs = [_train(tmp_path / tag, shards, 8, extra, monkeypatch) for tag in ("a", "b")]
    assert torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], unaugmented["off"])
    params, stepper, seen, logs = runs[0]
    line = [l for l in logs if l.startswith("augmentation:")]
    assert len(line) == 1 and all(t in line[0] for t in ("random rotation by up to ±10°", "random zoom", "mirror"))
    for s, par, col, zr, ar in seen:
        np.testing.assert_array_equal(par, aug_oracle.draw(SEED, s, 4, 0, True))
        assert col is None and zr is None  # the affine rows contain the zoom: the update takes them instead
        np.testing.assert_array_equal(ar, oracle.draw(SEED, s, 4, 640, zoom=aug_zoom_oracle.draw(SEED, s, 4, 16384, False)))
    np.testing.assert_array_equal(stepper.augmenter.zoom.cpu().numpy(), aug_zoom_oracle.draw(SEED, 8, 4, 16384, False))


def test_run_train_with_rotation_under_prioritized_replay(tmp_path, monkeypatch, shards, unaugmented):
    extra = "AUG_ROTATE: 10\nPRIORITIZED_REPLAY: True\n"
    runs = [_train(tmp_path / tag, shards, 8, extra, monkeypatch) for tag in ("a", "b")]
    assert torch.equal(runs[0][0], runs[1][0]) and not torch.equal(runs[0][0], unaugmented["per_off"])
    assert any("random rotation by up to ±10°" in l for l in runs[0][3])
    for s, _, _, _, ar in runs[0][2]:
        np.testing.assert_array_equal(ar, oracle.draw(SEED, s, 4, 640))


def test_run_train_with_rotation_off_is_the_shift_path(tmp_path, monkeypatch, shards):
    """AUG_ROTATE: 0.0 beside AUG_SHIFT_PAD: 8: no affine array, no packed slot, the update takes the shift rows through aug_params as
    before, and the run ends on the bits of the run without the key."""
    p_off, stepper, seen, logs = _train(tmp_path / "zero", shards, 4, "AUG_ROTATE: 0.0\nAUG_SHIFT_PAD: 8\n", monkeypatch)
    p_shift, _, seen_shift, _ = _train(tmp_path / "shift", shards, 4, "AUG_SHIFT_PAD: 8\n", monkeypatch)
    assert torch.equal(p_off, p_shift)
    assert stepper.augmenter.affine is None and stepper._packed_bufs == [None, None] and not any("rotation" in l for l in logs)
    for (s, par, col, zr, ar), other in zip(seen, seen_shift):
        assert col is None and zr is None and ar is None
        np.testing.assert_array_equal(par, aug_oracle.draw(SEED, s, 4, 8, False))
        np.testing.assert_array_equal(par, other[1])
