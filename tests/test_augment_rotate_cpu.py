"""Random-rotation augmentation without a GPU: the integer sine and cosine against float64 for every angle, the composed affine row
against the float64 map, the resample (tests/aug_rotate_oracle.py) against the zoom's and against a float64 bilinear, a linear ramp
rotated by hand (which pins the centre, the sense of the angle and its unit without the oracle's formulas), the config key and
run_train's refusals (raised before any device work), and the argument checks of the two C entries."""
import ctypes as C
import math

import numpy as np
import pytest

import aug_color_oracle
import aug_oracle
import aug_rotate_oracle as oracle
import aug_zoom_oracle

ONE = 65536
I32 = (-2**31, 2**31 - 1)
MAXO = oracle.MAX_ORIGIN
NEAR, FAR = aug_zoom_oracle.origin(32768, 0), aug_zoom_oracle.origin(32768, 0xFFFF)
ZOOM_ROWS = [aug_zoom_oracle.IDENTITY, (32768, 32768, NEAR, NEAR), (32768, 32768, FAR, FAR), (32768, 32768, FAR, NEAR)] + \
    [tuple(int(v) for v in r) for r in aug_zoom_oracle.draw(7, 3, 12, 32768, True)]


def _noise(n=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


# ---- sine and cosine -----------------------------------------------------------------------------------------------------------------
def test_sincos_every_angle_against_float64():
    assert oracle.sincos(0) == (0, ONE)
    worst_s = worst_c = 0.0
    for k in range(-oracle.MAX_JR, oracle.MAX_JR + 1):
        S, Cq = oracle.sincos(k)
        assert oracle.sincos(-k) == (-S, Cq), k
        rad = math.radians(k / 64)
        worst_s, worst_c = max(worst_s, abs(S / ONE - math.sin(rad))), max(worst_c, abs(Cq / ONE - math.cos(rad)))
    print(f"worst sine error {worst_s * ONE:.3f} * 2^-16, worst cosine error {worst_c * ONE:.3f} * 2^-16")
    assert worst_s <= 2.0**-16 and worst_c <= 2.0**-16
    assert oracle.sincos(1920) == (32768, 56756)  # sin 30 = 1 / 2 exactly; cos 30 * 65536 = 56755.84
    assert oracle.jr(30.0) == 1920 and oracle.jr(10) == 640 and oracle.jr(0.0) == 0 and oracle.jr(0.01) == 1 and oracle.jr(0.007) == 0


def test_row_at_angle_zero_is_the_zoom_row():
    for z in ZOOM_ROWS:
        ax, ay, bx, by = z
        assert oracle.compose(0, z) == (ax, 0, bx, 0, 0, ay, by, 0)
    assert oracle.compose(0) == oracle.IDENTITY
    np.testing.assert_array_equal(oracle.draw(3, 9, 8, 0), np.array([oracle.IDENTITY] * 8, np.int32))
    zr = aug_zoom_oracle.draw(3, 9, 8, 16384, True)
    d = oracle.draw(3, 9, 8, 0, zoom=zr)
    np.testing.assert_array_equal(d[:, [0, 5, 2, 6]], zr)
    assert not d[:, [1, 3, 4, 7]].any()


def test_source_coordinates_against_the_float64_map():
    """Bound: 2 * 111.5 * (2^-16 + 2^-17) + 2^-16 pixel — per coefficient the trig error (2^-16) and one product rounding (2^-17), over at
    most half a frame on each of the two axes, plus the origin's halving."""
    bound = 2 * 111.5 * (2.0**-16 + 2.0**-17) + 2.0**-16
    assert 0.0051 < bound < 0.0052
    Y, X = np.mgrid[0:224, 0:224].astype(np.float64)
    worst = 0.0
    ks = sorted(set(list(range(-1920, 1921, 37)) + [-1920, -640, -1, 0, 1, 640, 1920]))
    for z in ZOOM_ROWS[:4] + ZOOM_ROWS[4::4]:
        ax, ay, bxz, byz = z
        for k in ks:
            row = oracle.compose(k, z)
            assert all(I32[0] <= w <= I32[1] for w in row)
            np.testing.assert_array_equal(oracle.clamp_rows(np.array([row]))[0], row)  # a drawn row is inside the kernel's clamps
            u, v = oracle.coords(np.array([row]))  # (asserts that no int32 overflows)
            th = math.radians(k / 64)
            xr = 111.5 + math.cos(th) * (X - 111.5) - math.sin(th) * (Y - 111.5)
            yr = 111.5 + math.sin(th) * (X - 111.5) + math.cos(th) * (Y - 111.5)
            uf, vf = (bxz + ax * xr) / 65536.0, (byz + ay * yr) / 65536.0
            worst = max(worst, np.abs(u / 65536.0 - uf).max(), np.abs(v / 65536.0 - vf).max())
    print(f"worst source-coordinate error {worst:.5f} pixel (bound {bound:.5f})")
    assert worst <= bound


# ---- the resample --------------------------------------------------------------------------------------------------------------------
def test_rows_without_cross_terms_resample_as_the_zoom_does():
    fr = _noise(1, seed=1)[0]
    for z in ZOOM_ROWS[:6] + [(0, ONE, 5, -9), (ONE, ONE, -3 * ONE, 7 * ONE)]:
        ax, ay, bx, by = z
        np.testing.assert_array_equal(oracle.resample(fr, (ax, 0, bx, 0, 0, ay, by, 0)), aug_zoom_oracle.resample(fr, np.array([z])))
    np.testing.assert_array_equal(oracle.resample(fr, oracle.IDENTITY), fr)
    # the zoom clamps its origins at 224, the affine row at 448: beyond either every tap sits on the edge
    far = aug_zoom_oracle.MAX_ORIGIN
    np.testing.assert_array_equal(oracle.resample(fr, (ONE, 0, MAXO, 0, 0, ONE, -MAXO, 0)), aug_zoom_oracle.resample(fr, np.array([(ONE, ONE, far, -far)])))


def _float_bilinear(frame, row):
    u, v = oracle.coords(np.array([row]))
    u, v = u / 65536.0, v / 65536.0
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = (u - x0)[..., None], (v - y0)[..., None]
    xa, xb, ya, yb = np.clip(x0, 0, 223), np.clip(x0 + 1, 0, 223), np.clip(y0, 0, 223), np.clip(y0 + 1, 0, 223)
    z = frame.astype(np.float64)
    return (z[ya, xa] * (1 - fx) + z[ya, xb] * fx) * (1 - fy) + (z[yb, xa] * (1 - fx) + z[yb, xb] * fx) * fy


def test_integer_resample_against_float64():
    """The zoom's bound: the Q8 weight is the Q16 fraction truncated (< 1 grey level per axis), the final rounding adds at most 0.5."""
    fr = _noise(1, seed=2)[0]
    worst = 0.0
    for k, z in ((1920, ZOOM_ROWS[0]), (-1920, ZOOM_ROWS[1]), (640, ZOOM_ROWS[2]), (-77, ZOOM_ROWS[5]), (1001, ZOOM_ROWS[7])):
        row = oracle.compose(k, z)
        worst = max(worst, np.abs(oracle.resample(fr, row).astype(np.float64) - _float_bilinear(fr, row)).max())
    print(f"max deviation from float64 bilinear: {worst:.4f}")
    assert worst < 2.5


@pytest.mark.parametrize("k", [640, -640, 1920, -1920])
def test_rotated_ramp_by_hand(k):
    """A linear ramp a x + b y + c is reproduced exactly by a bilinear filter, so the rotated frame is the ramp at the rotated
    coordinates — computed here in float64 from the angle in degrees, the centre (111.5, 111.5) and the sense (a positive angle turns
    the output pixel's offset from the centre counter-clockwise in (x right, y down) index space before the lookup), none of it through
    the oracle's formulas.  2 grey levels: the ramp's byte rounding (0.5), the integer bilinear (< 1.5 on a ramp whose neighbours differ
    by less than 1) and the coordinate error (0.0052 pixel * slope, negligible)."""
    a, b, c = 0.55, 0.35, 20.0
    yy, xx = np.mgrid[0:224, 0:224].astype(np.float64)
    ramp = np.rint(a * xx + b * yy + c)
    assert ramp.min() >= 0 and ramp.max() <= 255
    frame = np.repeat(ramp[..., None], 3, 2).astype(np.uint8)
    got = oracle.resample(frame, oracle.compose(k)).astype(np.float64)[..., 0]
    th = math.radians(k / 64.0)
    xs = 111.5 + math.cos(th) * (xx - 111.5) - math.sin(th) * (yy - 111.5)
    ys = 111.5 + math.sin(th) * (xx - 111.5) + math.cos(th) * (yy - 111.5)
    inside = (xs >= 0.01) & (xs <= 222.99) & (ys >= 0.01) & (ys <= 222.99)  # all four taps in the frame
    assert inside.mean() > 0.6
    err = np.abs(got - (a * xs + b * ys + c))[inside]
    print(f"k = {k}: worst deviation from the rotated ramp {err.max():.3f} grey levels over {inside.sum()} pixels")
    assert err.max() <= 2.0
    # the sense and the unit matter: the opposite angle, or k taken as 1 / 32 degree, is far off
    for wrong in (-th, 2 * th):
        xw = 111.5 + math.cos(wrong) * (xx - 111.5) - math.sin(wrong) * (yy - 111.5)
        yw = 111.5 + math.sin(wrong) * (xx - 111.5) + math.cos(wrong) * (yy - 111.5)
        assert np.abs(got - (a * xw + b * yw + c))[inside].max() > 10
    # and so does the centre: about (112, 112) the corner pixels move by more than the tolerance allows at 30 degrees only; pin it directly
    assert np.abs(got[111:113, 111:113] - (a * 111.5 + b * 111.5 + c)).max() <= 2.0


def test_out_of_frame_taps_replicate_the_edge_and_wild_rows_are_clamped():
    fr = _noise(2, seed=4)
    row = oracle.compose(1920)
    assert (row[2] >> 16, row[6] >> 16) == (70, -41)  # output pixel (0, 0) comes from above the frame: both row taps clamp to row 0
    wx = (row[2] >> 8) & 255
    z = fr[0].astype(int)
    want = [((z[0, 70, c] * (256 - wx) + z[0, 71, c] * wx) * 256 + 32768) >> 16 for c in range(3)]
    assert oracle.resample(fr[0], row)[0, 0].tolist() == want
    wild = np.array([(-5, 70000, I32[0], 99, I32[1], 70000, I32[1], -1), (I32[1], I32[0], -MAXO - 1, 5, I32[0], I32[1], MAXO + 1, 6)], np.int64).astype(np.int32)
    tame = np.array([(0, ONE, -MAXO, 0, ONE, ONE, MAXO, 0), (ONE, -ONE, -MAXO, 0, -ONE, ONE, MAXO, 0)], np.int32)
    np.testing.assert_array_equal(oracle.clamp_rows(wild), tame)
    np.testing.assert_array_equal(oracle.affine(fr, wild), oracle.affine(fr, tame))
    # origins at the bound: every tap on one edge, whatever the cross terms
    for cross in (-ONE, 0, ONE):
        hi = oracle.resample(fr[0], (ONE, cross, MAXO, 0, cross, 0, -MAXO, 0))
        np.testing.assert_array_equal(hi, np.broadcast_to(fr[0][0, 223], hi.shape))
    const = np.full((224, 224, 3), 77, np.uint8)
    np.testing.assert_array_equal(oracle.resample(const, oracle.compose(-1920, ZOOM_ROWS[3])), const)


def test_composition_with_shift_mirror_and_colour():
    fr = _noise(4, seed=5)
    par, col = aug_oracle.draw(3, 5, 2, 32, True), aug_color_oracle.draw(3, 5, 2, 102, 102, 102)
    rows = oracle.draw(3, 5, 2, 1920, zoom=aug_zoom_oracle.draw(3, 5, 2, 32768, True))
    zs = aug_oracle.augment_frames(fr, par, 2)
    np.testing.assert_array_equal(oracle.augment(fr, par, rows, None, 2), oracle.affine(zs, rows, 2))
    np.testing.assert_array_equal(oracle.augment(fr, par, rows, col, 2), aug_color_oracle.color(oracle.affine(zs, rows, 2), col, 2))
    for i in range(4):
        np.testing.assert_array_equal(oracle.affine(fr, rows, 2)[i], oracle.resample(fr[i], rows[i // 2]))


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_draw_range_slices_and_stream():
    assert oracle.ROTATE_STREAM == int.from_bytes(b"AUGROTA1", "big")
    keys = {aug_oracle.splitmix64(4 ^ s) for s in (oracle.ROTATE_STREAM, aug_zoom_oracle.ZOOM_STREAM, aug_oracle.AUG_STREAM, aug_color_oracle.COLOR_STREAM)}
    assert len(keys) == 4
    ks = np.array([oracle.angle(0, step, 256, 1920, j) for step in range(1, 9) for j in range(256)])
    assert ks.min() >= -1920 and ks.max() <= 1920 and ks.min() < -1880 and ks.max() > 1880 and abs(ks.mean()) < 100
    assert sorted({oracle.angle(1, step, 64, 1, j) for step in range(1, 3) for j in range(64)}) == [-1, 0, 1]
    key = aug_oracle.splitmix64(4 ^ oracle.ROTATE_STREAM)
    assert [oracle.angle(4, 12, 32, 640, j) for j in range(32)] == \
        [(((aug_oracle.splitmix64(key ^ (12 * 32 + j)) & 0xFFFF) * 1281) >> 16) - 640 for j in range(32)]
    zr = aug_zoom_oracle.draw(4, 12, 32, 16384, True)
    whole = oracle.draw(4, 12, 32, 640, zoom=zr)
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 640, zoom=zr[16:], first=16, n=16), whole[16:])
    for j in (0, 31):
        assert tuple(whole[j]) == oracle.compose(oracle.angle(4, 12, 32, 640, j), zr[j])


# ---- config key and refusals -----------------------------------------------------------------------------------------------------------
BAD_ROTATE = [-0.1, 30.5, True, "10", float("nan")]


def test_config_key_default_and_merge(tmp_path):
    from video_dqn_amd.augment import MAX_ROTATE, jr
    from video_dqn_amd.config import ExperimentConfig, get_cfg_defaults
    c = get_cfg_defaults()
    assert c.AUG_ROTATE == 0.0 and isinstance(c.AUG_ROTATE, float) and MAX_ROTATE == 30.0
    (tmp_path / "config.yml").write_text("AUG_ROTATE: 10.0\n")
    assert ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False).AUG_ROTATE == 10.0
    (tmp_path / "config.yml").write_text("AUG_ROTATE: 'wide'\n")
    with pytest.raises(ValueError, match="AUG_ROTATE"):
        ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)
    for f in (oracle.jr, jr):
        assert f(30.0) == 1920 and f(10) == 640 and f(0.0) == 0 and f(0) == 0 and f(0.007) == 0 and f(0.008) == 1


def test_check_config_names_the_key():
    from video_dqn_amd.augment import check_config
    from video_dqn_amd.trainer import check_augment
    for fn in (check_config, check_augment):
        for ok in (0.0, 0, 10, 12.5, 30.0):
            fn(0, False, [1, 2], 0.0, 0.0, 0.0, 0.0, False, ok)
            fn(8, True, [1, 2], 0.4, 0.4, 0.4, 0.25, True, rotate=ok)
        fn(8, True, [1, 2], 0.4, 0.4, 0.4, 0.25, True)  # the eight-argument call of before
        for bad in BAD_ROTATE:
            with pytest.raises(ValueError, match="AUG_ROTATE must"):
                fn(0, False, [1, 2], rotate=bad)


@pytest.mark.parametrize("bad", BAD_ROTATE, ids=["negative", "above_30", "bool", "string", "nan"])
def test_run_train_refuses_before_device_work(tmp_path, monkeypatch, bad):
    import torch
    from video_dqn_amd import trainer
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.SYNTHETIC_DATA = True
    c["AUG_ROTATE"] = bad
    c.folder, c.device = str(tmp_path), "cuda"

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    monkeypatch.setattr(torch, "manual_seed", no_device)
    monkeypatch.setattr(trainer, "build_model", no_device)
    with pytest.raises(ValueError, match="AUG_ROTATE "):
        trainer.run_train(c, log=lambda *a: None)


def test_python_entries_refuse_by_name():
    """pack_input_aug's and aug_draw_rotate's own checks come before any device call."""
    import torch
    from video_dqn_amd import _lib
    from video_dqn_amd.augment import aug_draw_rotate, pack_input_aug
    src = torch.zeros((1, 224, 224, 3), dtype=torch.uint8)
    par, zoom, aff = torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32), torch.zeros((1, 8), dtype=torch.int32)
    with pytest.raises(_lib.VdqnError, match="zoom and affine are both given"):
        pack_input_aug(src, par, 1, torch.float32, zoom=zoom, affine=aff)
    for bad in (aff[:, :4].contiguous(), aff.to(torch.int64), torch.zeros((2, 8), dtype=torch.int32)):
        with pytest.raises(_lib.VdqnError, match=r"affine must be contiguous int32 \[\*\]\[8\]"):
            pack_input_aug(src, par, 1, torch.float32, affine=bad)
    with pytest.raises(_lib.VdqnError, match="aug_draw_rotate: zoom must be"):
        aug_draw_rotate(0, 1, 4, 0, 4, 640, zoom=torch.zeros((3, 4), dtype=torch.int32), device="cpu")


# ---- the C entries refuse bad arguments before any device call -----------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * 64)()  # host memory, 16-byte aligned below: never dereferenced, every call fails its argument check
    p = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(seed=0, step=1, G=8, first=0, n=8, jr=640, zoom=p, affine=p)

    def draw(**kw):
        a = dict(ok, **kw)
        return lib.vdqn_aug_draw_rotate(a["seed"], a["step"], a["G"], a["first"], a["n"], a["jr"], a["zoom"], a["affine"], None)
    for kw in (dict(affine=None), dict(n=0), dict(n=-3), dict(jr=-1), dict(jr=1921), dict(jr=2**31 - 1), dict(first=4), dict(first=-1),
               dict(G=0), dict(first=2**31 - 1, n=2**31 - 1, G=2**31 - 1), dict(affine=p + 4), dict(zoom=p + 8), dict(zoom=None, jr=1921)):
        assert draw(**kw) != 0, kw
        assert b"vdqn_aug_draw_rotate" in lib.vdqn_last_error(), kw
    assert draw(affine=None) != 0 and b"null affine" in lib.vdqn_last_error()
    assert draw(affine=p + 4) != 0 and b"affine must be 16-byte aligned" in lib.vdqn_last_error()
    assert draw(zoom=p + 8) != 0 and b"zoom must be 16-byte aligned" in lib.vdqn_last_error()
    assert draw(jr=1921) != 0 and b"range 1921 outside [0, 1920]" in lib.vdqn_last_error()
    assert draw(first=4) != 0 and b"outside the global batch" in lib.vdqn_last_error()

    def pack(src=p, dst=p, n_img=4, F=1, params=p, color=p, affine=p, n_params=4, dtype=_lib.VDQN_BF16):
        return lib.vdqn_pack_input_aug_affine(src, dst, n_img, F, params, color, affine, n_params, dtype, None)
    for kw in (dict(src=None), dict(dst=None), dict(params=None), dict(affine=None), dict(n_img=0), dict(F=0), dict(n_params=0),
               dict(n_img=-1), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7), dict(src=p + 4), dict(dst=p + 8), dict(params=p + 4),
               dict(color=p + 4), dict(affine=p + 4), dict(color=None, affine=p + 8), dict(color=None, dtype=7)):
        assert pack(**kw) != 0, kw
        assert b"vdqn_pack_input_aug_affine" in lib.vdqn_last_error(), kw
    assert pack(affine=None) != 0 and b"null arg" in lib.vdqn_last_error()
    assert pack(n_img=0) != 0 and b"n_img 0" in lib.vdqn_last_error()
    assert pack(affine=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert pack(dtype=_lib.VDQN_F32X3) != 0 and b"dtype" in lib.vdqn_last_error()


def test_abi_version_and_step_args_are_the_parents():
    from video_dqn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_aug_draw_rotate", "vdqn_pack_input_aug_affine"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.vdqn_abi_struct_size(6) == C.sizeof(_lib.StepArgs)
    names = [f[0] for f in _lib.StepArgs._fields_]
    assert names == ["params", "bnstats", "packed_online", "packed_target", "before", "after", "src_kind", "batch", "act", "rew", "term", "valid",
                     "gt", "gamma", "inv_count", "clip_rect", "linear", "use_valid", "train_on_ground_truth", "value_learning", "acts_online",
                     "acts_target", "bwd", "grads", "loss", "q_before", "loss_kind", "packed_frames", "acts_samples", "sample_weight",
                     "sample_err", "aug_params", "aug_color", "aug_zoom", "sample_gamma"]
    assert not any("affine" in n or "rotate" in n for n in names)
