"""Random-zoom augmentation without a GPU: the properties of the integer bilinear resample (tests/aug_zoom_oracle.py) and its distance
from a float64 bilinear at the same coordinates, the invariants of the draw, the five-row staging window the kernel relies on, the
config keys and run_train's refusals (raised before any device work), and the argument checks of the two C entries."""
import ctypes as C

import numpy as np
import pytest

import aug_color_oracle
import aug_oracle
import aug_zoom_oracle as oracle

ONE = 65536
I32 = (-2**31, 2**31 - 1)
MAXO = oracle.MAX_ORIGIN
# the far corner of a 2 x zoom: the window's edge at its largest value, R << 8 with R = (224 * 65536 - 224 * 32768) >> 8
FAR = oracle.origin(32768, 0xFFFF)
CORNER_ROWS = [oracle.IDENTITY, (32768, 32768, oracle.origin(32768, 0), oracle.origin(32768, 0)), (32768, 32768, FAR, FAR),
               (ONE, 32768, 0, FAR), (32768, ONE, FAR, 0), (49152, 40000, oracle.origin(49152, 0x8000), oracle.origin(40000, 0x1234))]


def _noise(n=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _drawn(aspect=True):
    return np.concatenate([oracle.draw(seed, step, 64, jz, aspect) for seed, step, jz in ((0, 1, 32768), (7, 99999, 16384), (2**63 + 5, 3, 1000))])


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def test_far_corner_constant():
    assert FAR == (((224 * ONE - 224 * 32768) >> 8) << 8) + 16384 - 32768 == 112 * ONE - 16384
    assert FAR + 223 * 32768 < 224 * ONE and (FAR + 223 * 32768) >> 16 == 223  # the last output pixel's second tap is clamped


def test_identity_row_reproduces_every_byte():
    fr = _noise(2, seed=1)
    fr[1, :, :112], fr[1, :, 112:] = 0, 255
    got = oracle.zoom(fr, np.array([oracle.IDENTITY], np.int32))
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, fr)
    np.testing.assert_array_equal(oracle.draw(3, 9, 8, 0, False), np.array([oracle.IDENTITY] * 8, np.int32))
    np.testing.assert_array_equal(oracle.draw(3, 9, 8, 0, True), np.array([oracle.IDENTITY] * 8, np.int32))
    par = aug_oracle.draw(3, 5, 2, 32, True)
    np.testing.assert_array_equal(oracle.augment(fr, par, np.array([oracle.IDENTITY], np.int32)), aug_oracle.augment_frames(fr, par))


def test_output_range_and_constant_frames():
    rows = np.concatenate([_drawn()[::16], np.array(CORNER_ROWS, np.int64).astype(np.int32)])
    ext = np.zeros((2, 224, 224, 3), np.uint8)
    ext[1] = 255
    chk = np.zeros((1, 224, 224, 3), np.uint8)
    chk[0, ::2, 1::2], chk[0, 1::2, ::2] = 255, 255  # a checkerboard of the two extremes: every weight pair meets 0 and 255
    for row in rows:
        out = oracle.zoom(chk, row[None])  # (resample asserts 0 <= out <= 255 before it narrows to uint8)
        assert out.dtype == np.uint8
        np.testing.assert_array_equal(oracle.zoom(ext, row[None]), ext)
        for c in (1, 127, 200):
            const = np.full((1, 224, 224, 3), c, np.uint8)
            np.testing.assert_array_equal(oracle.zoom(const, row[None]), const)


def _float_bilinear(frame, row):
    ax, ay, bx, by = (int(v) for v in oracle.clamp_rows(row)[0])
    z = frame.astype(np.float64)
    u = (bx + np.arange(224) * ax) / 65536.0
    v = (by + np.arange(224) * ay) / 65536.0
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fx, fy = (u - x0)[None, :, None], (v - y0)[:, None, None]
    xa, xb, ya, yb = np.clip(x0, 0, 223), np.clip(x0 + 1, 0, 223), np.clip(y0, 0, 223), np.clip(y0 + 1, 0, 223)
    top = z[ya][:, xa] * (1 - fx) + z[ya][:, xb] * fx
    bot = z[yb][:, xa] * (1 - fx) + z[yb][:, xb] * fx
    return top * (1 - fy) + bot * fy


def test_integer_resample_against_float64():
    """The Q8 weight is the Q16 fraction truncated: less than 1 / 256 below it, times a tap difference of at most 255, is less than 1
    grey level per axis; the final round-half-up adds at most 0.5: less than 2.5 in all."""
    fr = _noise(1, seed=2)[0]
    rows = np.concatenate([_drawn()[::8], np.array(CORNER_ROWS, np.int64).astype(np.int32)])
    worst = 0.0
    for row in rows:
        worst = max(worst, np.abs(oracle.resample(fr, row).astype(np.float64) - _float_bilinear(fr, row)).max())
    print(f"max deviation from float64 bilinear over {len(rows)} rows: {worst:.4f}")
    assert worst < 2.5


def test_one_pixel_by_hand():
    fr = _noise(1, seed=3)
    row = np.array([(40000, 50000, 1234567, 2345678)], np.int32)
    Y, X = 100, 57
    u, v = 1234567 + X * 40000, 2345678 + Y * 50000
    x0, wx, y0, wy = u >> 16, (u >> 8) & 255, v >> 16, (v >> 8) & 255
    assert (x0, wx, y0, wy) == (53, 160, 112, 22)  # u = 3514567 = 53 * 65536 + 41159, v = 7345678 = 112 * 65536 + 5646
    z = fr[0].astype(int)
    want = [((z[y0, x0, c] * (256 - wx) + z[y0, x0 + 1, c] * wx) * (256 - wy) + (z[y0 + 1, x0, c] * (256 - wx) + z[y0 + 1, x0 + 1, c] * wx) * wy
             + 32768) >> 16 for c in range(3)]
    assert oracle.zoom(fr, row)[0, Y, X].tolist() == want
    # composition: the taps go through the shift / mirror remap, the colour transform works on the resampled bytes
    par, col = np.array([(5, -3, 1, 0)], np.int32), np.array([(300, 200, 128, 0)], np.int32)
    zs = aug_oracle.augment_frames(fr, par)
    assert zs[0, y0, x0].tolist() == fr[0, y0 - 3, 223 - (x0 + 5)].tolist()
    np.testing.assert_array_equal(oracle.augment(fr, par, row, col), aug_color_oracle.color(oracle.zoom(zs, row), col))
    np.testing.assert_array_equal(oracle.augment(fr, par, row), oracle.zoom(zs, row))


def test_rows_per_sample_wrap_and_clamp():
    fr = _noise(8, seed=4)
    rows = np.array([(32768, 32768, FAR, 0), oracle.IDENTITY, (50000, 60000, 100000, 900000)], np.int32)
    got = oracle.zoom(fr, rows, frames_per_sample=2)
    for i in range(8):
        np.testing.assert_array_equal(got[i], oracle.resample(fr[i], rows[(i // 2) % 3]))
    np.testing.assert_array_equal(got[2:4], fr[2:4])
    wild = np.array([(-5, 70000, I32[0], I32[1]), (I32[1], I32[0], -MAXO - 1, MAXO + 1)], np.int64).astype(np.int32)
    tame = np.array([(0, ONE, -MAXO, MAXO), (ONE, 0, -MAXO, MAXO)], np.int32)
    np.testing.assert_array_equal(oracle.zoom(fr[:2], wild), oracle.zoom(fr[:2], tame))
    # step 0: every output pixel of an axis reads the same source coordinate; an origin beyond the frame reads the edge pixel
    out = oracle.zoom(fr[:1], np.array([(0, ONE, MAXO, 0)], np.int32))
    np.testing.assert_array_equal(out[0], np.repeat(fr[0, :, 223:224], 224, 1))


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def test_jz():
    from video_dqn_amd.augment import jz
    for f in (oracle.jz, jz):
        assert f(0.5) == 32768 and f(0.25) == 16384 and f(0.0) == 0 and f(0) == 0 and f(0.000001) == 0 and f(0.00001) == 1


def test_drawn_rows_stay_inside_the_frame():
    for jz in (0, 1, 1000, 16384, 32768):
        for aspect in (False, True):
            for seed, step in ((0, 1), (7, 99999), (2**63 + 5, 3)):
                d = oracle.draw(seed, step, 256, jz, aspect).astype(np.int64)
                assert d.shape == (256, 4)
                ax, ay, bx, by = d.T
                assert np.all((ONE - jz <= ax) & (ax <= ONE)) and np.all((ONE - jz <= ay) & (ay <= ONE))
                assert np.all(bx + 223 * ax < 224 * ONE) and np.all(by + 223 * ay < 224 * ONE)
                assert np.all(bx >= (ax >> 1) - 32768) and np.all(by >= (ay >> 1) - 32768)  # the window's edge is at 0 or inside
                if not aspect:
                    assert np.all(ax == ay)
    # every 16-bit draw, both extremes of the width: the bound does not lean on the hash
    hk = np.arange(65536, dtype=np.int64)
    for a in (32768, 32769, 40000, 65535, 65536):
        r = (224 * ONE - 224 * a) >> 8
        b = (((hk * (r + 1)) >> 16) << 8) + (a >> 1) - 32768
        assert b.max() + 223 * a < 224 * ONE and b.min() == (a >> 1) - 32768
        assert b.max() == (r << 8) + (a >> 1) - 32768


def test_draw_covers_both_ends_of_its_range():
    d = np.concatenate([oracle.draw(0, step, 256, 32768, True) for step in range(1, 17)]).astype(np.int64)
    for k in (0, 1):
        assert d[:, k].min() < ONE - 32768 + 300 and d[:, k].max() > ONE - 300
        assert abs(d[:, k].mean() - (ONE - 16384)) < 600  # uniform over 32769 values: sigma / sqrt(4096) = 148
    assert abs(np.corrcoef(d[:, 0], d[:, 1])[0, 1]) < 0.05
    few = np.concatenate([oracle.draw(1, step, 256, 8, False) for step in range(1, 5)])
    assert sorted(np.unique(few[:, 0])) == list(range(ONE - 8, ONE + 1))
    # the position: from the frame's near edge to its far edge
    tight = d[d[:, 0] < 40000]
    edge = tight[:, 2] - (tight[:, 0] >> 1) + 32768  # the window's edge o, Q16
    room = 224 * (ONE - tight[:, 0])                    # 224 * 65536 - 224 * ax: where it fits
    assert len(tight) > 200 and edge.min() >= 0 and np.all(edge <= room)
    assert (edge / room).min() < 0.02 and (edge / room).max() > 0.98


def test_draw_slices_and_stream():
    whole = oracle.draw(4, 12, 32, 16384, True)
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 16384, True, first=16, n=16), whole[16:32])
    np.testing.assert_array_equal(oracle.draw(4, 12, 16, 16384, True, first=5, n=7), oracle.draw(4, 12, 16, 16384, True)[5:12])
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 16384, False)[:, 0], whole[:, 0])  # ax does not depend on `aspect`
    # a stream of its own: neither the shift / mirror hash nor the colour hash at the same seed, update and batch
    assert oracle.ZOOM_STREAM == int.from_bytes(b"AUGZOOM1", "big") == 0x4155475A4F4F4D31
    keys = {aug_oracle.splitmix64(4 ^ s) for s in (oracle.ZOOM_STREAM, aug_oracle.AUG_STREAM, aug_color_oracle.COLOR_STREAM)}
    assert len(keys) == 3
    key = aug_oracle.splitmix64(4 ^ oracle.ZOOM_STREAM)
    hs = [aug_oracle.splitmix64(key ^ (12 * 32 + j)) for j in range(32)]
    np.testing.assert_array_equal(whole[:, 0], [ONE - (((h & 0xFFFF) * 16385) >> 16) for h in hs])
    np.testing.assert_array_equal(whole[:, 1], [ONE - ((((h >> 16) & 0xFFFF) * 16385) >> 16) for h in hs])
    # the other draws are what they were: restated from their own keys
    k_aug = aug_oracle.splitmix64(4 ^ aug_oracle.AUG_STREAM)
    np.testing.assert_array_equal(aug_oracle.draw(4, 12, 32, 8, True)[:, 0],
                                  [(((aug_oracle.splitmix64(k_aug ^ (12 * 32 + j)) & 0xFFFF) * 17) >> 16) - 8 for j in range(32)])
    k_col = aug_oracle.splitmix64(4 ^ aug_color_oracle.COLOR_STREAM)
    np.testing.assert_array_equal(aug_color_oracle.draw(4, 12, 32, 8, 0, 0)[:, 0],
                                  [256 - 8 + (((aug_oracle.splitmix64(k_col ^ (12 * 32 + j)) & 0xFFFF) * 17) >> 16) for j in range(32)])
    h16 = np.array([h & 0xFFFF for h in hs])
    assert not np.array_equal(h16, [aug_oracle.splitmix64(k_aug ^ (12 * 32 + j)) & 0xFFFF for j in range(32)])


# ---- the staging window --------------------------------------------------------------------------------------------------------------
ADVERSARIAL = [(32768, ONE, 0, 0), (ONE, ONE, 0, 0), (ONE, ONE, 65535, 65535), (ONE, ONE, -1, -1), (ONE, ONE, -ONE, -ONE),
               (0, 0, 0, 0), (ONE, ONE, MAXO, MAXO), (ONE, ONE, -MAXO, -MAXO), (ONE, 65535, 0, 1), (ONE, 65535, 0, 65535),
               (I32[1], I32[1], I32[1], I32[1]), (I32[0], I32[0], I32[0], I32[0]), (I32[1], I32[1], I32[0], I32[0]),
               (ONE + 1, ONE + 1, 7, 7), (3 * ONE, 3 * ONE, 0, 0), (ONE, ONE, 0, -3 * ONE + 1), (ONE, 49152, 0, 12345)]


def test_a_pair_of_packed_rows_needs_at_most_five_source_rows():
    rows = np.concatenate([_drawn(), _drawn(aspect=False)[::4], np.array(ADVERSARIAL, np.int64).astype(np.int32)])
    worst = 0
    for row in rows:
        for sy in (0, -32, 32, 5, -224, 224, I32[0], I32[1]):
            for Y0 in range(0, 224, 4):
                src = oracle.source_rows(row, sy, Y0)
                assert 1 <= len(src) <= 5 and src[0] >= 0 and src[-1] <= 223
                assert src[-1] - src[0] == len(src) - 1, (row, sy, Y0, src)  # consecutive: slot = row - first
                worst = max(worst, len(src))
    assert worst == 5  # and five are needed: rows[4][42] would not do
    assert len(oracle.source_rows((ONE, ONE, 0, 1), 0, 8)) == 5 and len(oracle.source_rows(oracle.IDENTITY, 0, 8)) == 5
    assert len(oracle.source_rows((ONE, 32768, 0, 0), 0, 8)) == 3


def test_any_int32_row_indexes_inside_the_frame():
    for row in ADVERSARIAL + CORNER_ROWS:
        ax, ay, bx, by = (int(v) for v in oracle.clamp_rows(np.array([row], np.int64))[0])
        for a, b in ((ax, bx), (ay, by)):
            u = b + np.arange(224, dtype=np.int64) * a
            assert np.abs(u).max() < 2**25  # (and the kernel's int32 arithmetic does not wrap)
            i0, i1, w = oracle.taps(a, b)
            assert i0.min() >= 0 and i1.max() <= 223 and w.min() >= 0 and w.max() <= 255


# ---- config keys and refusals ----------------------------------------------------------------------------------------------------------
BAD_ZOOM = [-0.1, 0.6, True, "0.25", float("nan")]
BAD_ASPECT = [1, "yes", 0.5]


def test_config_keys_defaults_and_merge(tmp_path):
    from video_dqn_amd.config import ExperimentConfig, get_cfg_defaults
    c = get_cfg_defaults()
    assert c.AUG_ZOOM == 0.0 and isinstance(c.AUG_ZOOM, float) and c.AUG_ZOOM_ASPECT is False
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\n")
    e = ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)
    assert (e.AUG_ZOOM, e.AUG_ZOOM_ASPECT) == (0.0, False)
    (tmp_path / "config.yml").write_text("AUG_ZOOM: 0.25\nAUG_ZOOM_ASPECT: True\n")
    e = ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)
    assert (e.AUG_ZOOM, e.AUG_ZOOM_ASPECT) == (0.25, True)
    (tmp_path / "config.yml").write_text("AUG_ZOOM: 'wide'\n")
    with pytest.raises(ValueError, match="AUG_ZOOM"):
        ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)


def test_check_config_names_the_key():
    from video_dqn_amd.augment import check_config
    from video_dqn_amd.trainer import check_augment
    for fn in (check_config, check_augment):
        for ok in (0.0, 0, 0.25, 0.5):
            fn(0, False, [1, 2], 0.0, 0.0, 0.0, ok, False)
            fn(8, True, [1, 2], 0.4, 0.4, 0.4, zoom=ok)
        fn(0, False, [1, 2], zoom=0.25, zoom_aspect=True)
        fn(8, True, [1, 2], 0.4, 0.4, 0.4)  # the six-argument call of before
        for bad in BAD_ZOOM:
            with pytest.raises(ValueError, match="AUG_ZOOM must"):
                fn(0, False, [1, 2], zoom=bad)
        for bad in BAD_ASPECT:
            with pytest.raises(ValueError, match="AUG_ZOOM_ASPECT must"):
                fn(0, False, [1, 2], zoom=0.25, zoom_aspect=bad)
        for off in (0.0, 0, 0.000001):
            with pytest.raises(ValueError, match="AUG_ZOOM_ASPECT is True, but AUG_ZOOM"):
                fn(0, False, [1, 2], zoom=off, zoom_aspect=True)


@pytest.mark.parametrize("key,bad,zoom", [("AUG_ZOOM", b, None) for b in BAD_ZOOM] + [("AUG_ZOOM_ASPECT", b, 0.25) for b in BAD_ASPECT]
                         + [("AUG_ZOOM_ASPECT", True, 0.0)],
                         ids=["negative", "above_half", "bool", "string", "nan", "aspect_int", "aspect_string", "aspect_float", "aspect_without_zoom"])
def test_run_train_refuses_before_device_work(tmp_path, monkeypatch, key, bad, zoom):
    import torch
    from video_dqn_amd import trainer
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.SYNTHETIC_DATA = True
    if zoom is not None:
        c.AUG_ZOOM = zoom
    c[key] = bad
    c.folder, c.device = str(tmp_path), "cuda"

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    monkeypatch.setattr(torch, "manual_seed", no_device)
    monkeypatch.setattr(trainer, "build_model", no_device)
    with pytest.raises(ValueError, match=key + " "):
        trainer.run_train(c, log=lambda *a: None)


# ---- the C entries refuse bad arguments before any device call -----------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * 64)()  # host memory, 16-byte aligned below: never dereferenced, every call fails its argument check
    p = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(seed=0, step=1, G=8, first=0, n=8, jz=16384, aspect=1, zoom=p)

    def draw(**kw):
        a = dict(ok, **kw)
        return lib.vdqn_aug_draw_zoom(a["seed"], a["step"], a["G"], a["first"], a["n"], a["jz"], a["aspect"], a["zoom"], None)
    for kw in (dict(zoom=None), dict(n=0), dict(n=-3), dict(jz=-1), dict(jz=32769), dict(jz=2**31 - 1), dict(first=4), dict(first=-1),
               dict(G=0), dict(first=2**31 - 1, n=2**31 - 1, G=2**31 - 1), dict(zoom=p + 4)):
        assert draw(**kw) != 0, kw
        assert b"vdqn_aug_draw_zoom" in lib.vdqn_last_error(), kw
    assert draw(zoom=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert draw(jz=32769) != 0 and b"width" in lib.vdqn_last_error()
    assert draw(first=4) != 0 and b"outside the global batch" in lib.vdqn_last_error()

    def pack(src=p, dst=p, n_img=4, F=1, params=p, color=p, zoom=p, n_params=4, dtype=_lib.VDQN_BF16):
        return lib.vdqn_pack_input_aug_zoom(src, dst, n_img, F, params, color, zoom, n_params, dtype, None)
    for kw in (dict(src=None), dict(dst=None), dict(params=None), dict(zoom=None), dict(n_img=0), dict(F=0), dict(n_params=0),
               dict(n_img=-1), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7), dict(src=p + 4), dict(dst=p + 8), dict(params=p + 4),
               dict(color=p + 4), dict(zoom=p + 4), dict(color=None, zoom=p + 8), dict(color=None, dtype=7)):
        assert pack(**kw) != 0, kw
        assert b"vdqn_pack_input_aug_zoom" in lib.vdqn_last_error(), kw
    assert pack(zoom=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert pack(dtype=_lib.VDQN_F32X3) != 0 and b"dtype" in lib.vdqn_last_error()


def test_abi_the_struct_grew_and_the_version_did_not():
    from video_dqn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_aug_draw_zoom", "vdqn_pack_input_aug_zoom"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    lib = _lib.load()  # (compares sizeof(vdqn_step_args), which gained aug_zoom, with the binding's)
    assert lib.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.vdqn_abi_struct_size(6) == C.sizeof(_lib.StepArgs)
    assert lib.vdqn_abi_struct_size(7) == -1  # no new argument struct
    names = [f[0] for f in _lib.StepArgs._fields_]
    assert names.index("aug_zoom") == names.index("aug_color") + 1 == names.index("aug_params") + 2
    assert _lib.StepArgs.aug_zoom.offset == _lib.StepArgs.aug_color.offset + 8
    assert names[-1] == "sample_gamma" and _lib.StepArgs.sample_gamma.offset == _lib.StepArgs.aug_zoom.offset + 8
    a = _lib.StepArgs()
    assert a.aug_zoom is None  # zero-initialised: callers that never heard of it pass NULL
    assert lib.vdqn_net_td_forward(None, C.byref(a), None) != 0  # (null net: refused before anything is read)
