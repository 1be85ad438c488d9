"""Colour-jitter augmentation without a GPU: the properties of the integer arithmetic (tests/aug_color_oracle.py) and its distance from
the real-valued formulas, the invariants of the draw, the config keys and run_train's refusals (raised before any device work), and
the argument checks of the two C entries."""
import ctypes as C
import math

import numpy as np
import pytest

import aug_color_oracle as oracle
import aug_oracle

FACTORS = (0, 128, 256, 300, 512)


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def _pixels(n=4096, seed=0):
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, 3))
    px[:8] = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    return px


def test_factor_256_is_the_identity_on_every_byte():
    t = np.arange(256)
    np.testing.assert_array_equal(oracle.brightness(t, 256), t)
    np.testing.assert_array_equal(oracle.contrast(t, 256), t)
    np.testing.assert_array_equal(oracle.bc(256, 256), t)
    px = _pixels()
    np.testing.assert_array_equal(oracle.saturation(px, 256), px)
    # every (R, G) pair with every 5th B: the identity does not lean on the random sample
    grid = np.stack(np.meshgrid(t, t, t[::5], indexing="ij"), -1).reshape(-1, 3)
    np.testing.assert_array_equal(oracle.saturation(grid, 256), grid)
    fr = np.random.default_rng(1).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)
    got = oracle.color(fr, np.array([[256, 256, 256, 0]], np.int32))
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, fr)


def test_grey_is_a_fixed_point_of_saturation_and_factor_0_gives_grey():
    grey = np.repeat(np.arange(256)[:, None], 3, 1)
    for fs in range(0, 513):
        np.testing.assert_array_equal(oracle.saturation(grey, fs), grey)
    out = oracle.saturation(_pixels(), 0)
    assert np.all(out[:, 0] == out[:, 1]) and np.all(out[:, 1] == out[:, 2])
    px = _pixels()
    np.testing.assert_array_equal(out[:, 0], (77 * px[:, 0] + 150 * px[:, 1] + 29 * px[:, 2] + 128) // 256)


def test_brightness_then_contrast_is_monotone_in_the_byte():
    for fb in FACTORS:
        for fc in FACTORS:
            m = oracle.bc(fb, fc)
            assert m.shape == (256,) and m.min() >= 0 and m.max() <= 255
            assert np.all(np.diff(m) >= 0), (fb, fc)
    np.testing.assert_array_equal(oracle.bc(0, 256), np.zeros(256))
    np.testing.assert_array_equal(oracle.bc(256, 0), np.full(256, 128))
    assert oracle.bc(512, 256)[128] == 255 and oracle.bc(256, 512)[64] == 0 and oracle.bc(256, 512)[192] == 255


def test_integer_stages_against_float64():
    """Exhaustive over 256 bytes x factors 0 .. 512 for brightness and contrast (round half up of the real value: at most 0.5 away),
    seeded random pixels x every factor for saturation (the rounded grey, at most 0.5 away and weighted by |1 - f / 256| <= 1, plus
    one more rounding; the two extremes cannot coincide: less than 1.0 away)."""
    v = np.arange(256, dtype=np.float64)[None, :]
    f = np.arange(513, dtype=np.float64)[:, None]
    fi = np.arange(513)[:, None]
    vi = np.arange(256)[None, :]
    b_int = np.minimum(255, (vi * fi + 128) // 256)
    b_real = np.minimum(255.0, v * f / 256.0)
    c_int = np.clip(128 + ((vi - 128) * fi + 128) // 256, 0, 255)
    c_real = np.clip(128.0 + (v - 128.0) * f / 256.0, 0.0, 255.0)
    for fac in (0, 1, 255, 256, 257, 300, 512):  # the vectorised restatement above is the oracle's
        np.testing.assert_array_equal(oracle.brightness(np.arange(256), fac), b_int[fac])
        np.testing.assert_array_equal(oracle.contrast(np.arange(256), fac), c_int[fac])
    db, dc = np.abs(b_int - b_real).max(), np.abs(c_int - c_real).max()
    px = _pixels(2048, seed=3)
    pf = px.astype(np.float64)
    g_real = ((77 * pf[:, 0] + 150 * pf[:, 1] + 29 * pf[:, 2]) / 256.0)[:, None]
    ds = 0.0
    for fs in range(513):
        s_real = np.clip(g_real + (pf - g_real) * fs / 256.0, 0.0, 255.0)
        ds = max(ds, np.abs(oracle.saturation(px, fs) - s_real).max())
    print(f"max deviation from float64: brightness {db}, contrast {dc}, saturation {ds:.4f}")
    assert db <= 0.5 and dc <= 0.5 and ds < 1.0


def test_color_takes_factors_per_sample_and_clamps_them():
    fr = np.random.default_rng(2).integers(0, 256, (8, 224, 224, 3), dtype=np.uint8)
    fac = np.array([[300, 200, 0, 0], [256, 256, 256, 9], [100, 512, 400, 0]], np.int32)
    got = oracle.color(fr, fac, frames_per_sample=2)
    for i in range(8):
        fb, fc, fs = fac[(i // 2) % 3][:3]
        ref = oracle.contrast(oracle.brightness(oracle.saturation(fr[i], fs), fb), fc)
        np.testing.assert_array_equal(got[i], ref)
    np.testing.assert_array_equal(got[2:4], fr[2:4])  # word 3 is ignored
    wild = np.array([[-7, 100000, 2**31 - 1, 0]], np.int32)
    np.testing.assert_array_equal(oracle.color(fr[:2], wild), oracle.color(fr[:2], np.array([[0, 512, 512, 0]], np.int32)))
    # an independent statement on one pixel, by hand: (200, 100, 50), f_s = 128, f_b = 300, f_c = 200
    one = np.zeros((1, 224, 224, 3), np.uint8)
    one[...] = (200, 100, 50)
    g = (77 * 200 + 150 * 100 + 29 * 50 + 128) // 256
    assert g == 124
    sat = [g + ((v - g) * 128 + 128) // 256 for v in (200, 100, 50)]
    assert sat == [162, 112, 87]
    bri = [min(255, (v * 300 + 128) // 256) for v in sat]
    assert bri == [190, 131, 102]
    con = [min(255, max(0, 128 + ((v - 128) * 200 + 128) // 256)) for v in bri]
    assert con == [176, 130, 108]
    assert oracle.color(one, np.array([[300, 200, 128, 0]], np.int32))[0, 5, 7].tolist() == con


# ---- the draw ----------------------------------------------------------------------------------------------------------------------
def test_jq():
    from video_dqn_amd.augment import jq
    for f in (oracle.jq, jq):
        assert f(0.4) == 102 and f(1.0) == 256 and f(0.0) == 0 and f(0.5) == 128 and f(0.001) == 0 and f(0.002) == 1
        assert f(1) == 256 and f(0) == 0


def test_draw_range_and_coverage():
    for jqs in ((0, 0, 0), (1, 8, 256), (8, 102, 256), (256, 0, 37)):
        for seed, step in ((0, 1), (7, 99999), (2**63 + 5, 3)):
            d = oracle.draw(seed, step, 256, *jqs)
            assert d.dtype == np.int32 and d.shape == (256, 4) and np.all(d[:, 3] == 0)
            for k, j in enumerate(jqs):
                assert d[:, k].min() >= 256 - j and d[:, k].max() <= 256 + j
    assert np.all(oracle.draw(0, 1, 256, 0, 0, 0)[:, :3] == 256)
    d = oracle.draw(0, 1, 256, 8, 8, 8)
    for k in range(3):
        assert len(np.unique(d[:, k])) == 17, k


def test_draw_independence():
    d = np.concatenate([oracle.draw(0, step, 256, 102, 102, 102) for step in range(1, 17)])
    assert len(d) == 4096
    for a, b in ((0, 1), (0, 2), (1, 2)):
        corr = np.corrcoef(d[:, a], d[:, b])[0, 1]
        print(f"corr(f{a}, f{b}) {corr:.2e}")
        assert abs(corr) < 0.05
    for k in range(3):  # and each factor is spread over its range: mean near 256, the spread of a uniform draw over 205 values
        assert abs(d[:, k].mean() - 256) < 4 and abs(d[:, k].std() - math.sqrt((205 ** 2 - 1) / 12)) < 3


def test_draw_slices_and_stream():
    whole = oracle.draw(4, 12, 32, 8, 102, 256)
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 8, 102, 256, first=16, n=16), whole[16:32])
    np.testing.assert_array_equal(oracle.draw(4, 12, 16, 8, 102, 256, first=5, n=7), oracle.draw(4, 12, 16, 8, 102, 256)[5:12])
    # one factor's value does not depend on the other half-widths
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 8, 0, 0)[:, 0], whole[:, 0])
    np.testing.assert_array_equal(oracle.draw(4, 12, 32, 0, 0, 256)[:, 2], whole[:, 2])
    # a stream of its own: not the hash the shift / mirror draw uses at the same seed, update and batch, which is what it was
    assert oracle.COLOR_STREAM == int.from_bytes(b"AUGCOLR1", "big") == 0x415547434F4C5231
    assert aug_oracle.AUG_STREAM == int.from_bytes(b"AUGMENT1", "big") != oracle.COLOR_STREAM
    key_aug, key_col = aug_oracle.splitmix64(4 ^ aug_oracle.AUG_STREAM), aug_oracle.splitmix64(4 ^ oracle.COLOR_STREAM)
    assert key_aug != key_col
    shift = aug_oracle.draw(4, 12, 32, 8, True)
    h_aug = [aug_oracle.splitmix64(key_aug ^ (12 * 32 + j)) for j in range(32)]
    np.testing.assert_array_equal(shift[:, 0], [(((h & 0xFFFF) * 17) >> 16) - 8 for h in h_aug])  # aug_oracle.draw is unaffected
    h_col = [aug_oracle.splitmix64(key_col ^ (12 * 32 + j)) for j in range(32)]
    np.testing.assert_array_equal(whole[:, 0], [256 - 8 + (((h & 0xFFFF) * 17) >> 16) for h in h_col])
    assert not np.array_equal(whole[:, 0] - 256, shift[:, 0])


# ---- config keys and refusals ----------------------------------------------------------------------------------------------------------
KEYS = ("AUG_BRIGHTNESS", "AUG_CONTRAST", "AUG_SATURATION")
BAD = [-0.1, 1.5, True, "0.4", float("nan")]


def test_config_keys_defaults_and_merge(tmp_path):
    from video_dqn_amd.config import ExperimentConfig, get_cfg_defaults
    c = get_cfg_defaults()
    for k in KEYS:
        assert c[k] == 0.0 and isinstance(c[k], float)
    (tmp_path / "config.yml").write_text("SYNTHETIC_DATA: True\n")
    e = ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)
    assert (e.AUG_BRIGHTNESS, e.AUG_CONTRAST, e.AUG_SATURATION) == (0.0, 0.0, 0.0)
    (tmp_path / "config.yml").write_text("AUG_BRIGHTNESS: 0.4\nAUG_CONTRAST: 1\nAUG_SATURATION: 0.25\n")
    e = ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)
    assert (e.AUG_BRIGHTNESS, e.AUG_CONTRAST, e.AUG_SATURATION) == (0.4, 1.0, 0.25)
    (tmp_path / "config.yml").write_text("AUG_SATURATION: 'strong'\n")
    with pytest.raises(ValueError, match="AUG_SATURATION"):
        ExperimentConfig(str(tmp_path), device="cpu", tensorboard=False)


@pytest.mark.parametrize("which", range(3), ids=KEYS)
def test_check_config_names_the_key(which):
    from video_dqn_amd.augment import check_config
    from video_dqn_amd.trainer import check_augment
    for ok in (0.0, 0, 0.4, 1.0, 1):
        v = [0.0, 0.0, 0.0]
        v[which] = ok
        check_config(0, False, [1, 2], *v)
        check_augment(8, True, [1, 2], *v)
    for bad in BAD:
        v = [0.2, 0.2, 0.2]
        v[which] = bad
        for fn in (check_config, check_augment):
            with pytest.raises(ValueError, match=KEYS[which] + " "):
                fn(0, False, [1, 2], *v)
    check_config(8, True, [1, 2])  # the three-argument call of before


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("bad", BAD, ids=["negative", "above_1", "bool", "string", "nan"])
def test_run_train_refuses_before_device_work(tmp_path, monkeypatch, key, bad):
    import torch
    from video_dqn_amd import trainer
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    c.SYNTHETIC_DATA = True
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
    ok = dict(seed=0, step=1, G=8, first=0, n=8, jb=8, jc=102, js=256, color=p)

    def draw(**kw):
        a = dict(ok, **kw)
        return lib.vdqn_aug_draw_color(a["seed"], a["step"], a["G"], a["first"], a["n"], a["jb"], a["jc"], a["js"], a["color"], None)
    for kw in (dict(color=None), dict(n=0), dict(n=-3), dict(jb=-1), dict(jb=257), dict(jc=-1), dict(jc=257), dict(js=-1), dict(js=257),
               dict(js=2**31 - 1), dict(first=4), dict(first=-1), dict(G=0), dict(first=2**31 - 1, n=2**31 - 1, G=2**31 - 1), dict(color=p + 4)):
        assert draw(**kw) != 0, kw
        assert b"vdqn_aug_draw_color" in lib.vdqn_last_error(), kw
    assert draw(color=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert draw(js=257) != 0 and b"half-widths" in lib.vdqn_last_error()
    assert draw(first=4) != 0 and b"outside the global batch" in lib.vdqn_last_error()

    def pack(src=p, dst=p, n_img=4, F=1, params=p, color=p, n_params=4, dtype=_lib.VDQN_BF16):
        return lib.vdqn_pack_input_aug_color(src, dst, n_img, F, params, color, n_params, dtype, None)
    for kw in (dict(src=None), dict(dst=None), dict(params=None), dict(color=None), dict(n_img=0), dict(F=0), dict(n_params=0),
               dict(n_img=-1), dict(dtype=_lib.VDQN_F32X3), dict(dtype=7), dict(src=p + 4), dict(dst=p + 8), dict(params=p + 4),
               dict(color=p + 4)):
        assert pack(**kw) != 0, kw
        assert b"vdqn_pack_input_aug_color" in lib.vdqn_last_error(), kw
    assert pack(color=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert pack(dtype=_lib.VDQN_F32X3) != 0 and b"dtype" in lib.vdqn_last_error()


def test_abi_the_struct_grew_and_the_version_did_not():
    from video_dqn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_aug_draw_color", "vdqn_pack_input_aug_color"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    lib = _lib.load()  # (compares sizeof(vdqn_step_args), which gained aug_color, with the binding's)
    assert lib.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.vdqn_abi_struct_size(6) == C.sizeof(_lib.StepArgs)
    assert lib.vdqn_abi_struct_size(7) == -1  # no new argument struct
    names = [f[0] for f in _lib.StepArgs._fields_]
    assert names.index("aug_color") == names.index("aug_params") + 1
    assert _lib.StepArgs.aug_color.offset == _lib.StepArgs.aug_params.offset + 8
    a = _lib.StepArgs()
    assert a.aug_color is None  # zero-initialised: callers that never heard of it pass NULL
    assert lib.vdqn_net_td_forward(None, C.byref(a), None) != 0  # (null net: refused before anything is read)
