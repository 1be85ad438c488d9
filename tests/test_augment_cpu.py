"""Shift / mirror augmentation without a GPU: the config keys, run_train's refusals (raised before any device work), the numpy
oracle (tests/aug_oracle.py) against an independent statement of the transform, the invariants of the draw, and the argument
checks of the C entries."""
import ctypes as C

import numpy as np
import pytest

import aug_oracle
import per_oracle


def test_config_keys_defaults_merge_and_types(tmp_path):
    from video_dqn_amd.config import get_cfg_defaults
    c = get_cfg_defaults()
    assert c.AUG_SHIFT_PAD == 0 and c.AUG_FLIP is False and c.AUG_FLIP_ACTIONS == [1, 2]
    f = tmp_path / "config.yml"
    f.write_text("AUG_SHIFT_PAD: 8\nAUG_FLIP: True\nAUG_FLIP_ACTIONS: [0, 2]\n")
    c.merge_from_file(str(f))
    assert c.AUG_SHIFT_PAD == 8 and isinstance(c.AUG_SHIFT_PAD, int) and c.AUG_FLIP is True and c.AUG_FLIP_ACTIONS == [0, 2]
    for bad in ("AUG_SHIFT_PAD: 'wide'\n", "AUG_SHIFT_PAD: 2.5\n", "AUG_FLIP: 1\n", "AUG_FLIP_ACTIONS: 12\n"):
        f.write_text(bad)
        with pytest.raises(ValueError, match="Type mismatch"):
            get_cfg_defaults().merge_from_file(str(f))


@pytest.mark.parametrize("keys,reason", [
    (dict(AUG_SHIFT_PAD=-1), "AUG_SHIFT_PAD"),
    (dict(AUG_SHIFT_PAD=33), "AUG_SHIFT_PAD"),
    (dict(AUG_FLIP=True, AUG_FLIP_ACTIONS=[1, 1]), "AUG_FLIP_ACTIONS"),
    (dict(AUG_FLIP=True, AUG_FLIP_ACTIONS=[0, 3]), "AUG_FLIP_ACTIONS"),
    (dict(AUG_FLIP=True, AUG_FLIP_ACTIONS=[0, 1, 2]), "AUG_FLIP_ACTIONS"),
], ids=["pad_negative", "pad_33", "same_actions", "action_3", "three_actions"])
def test_run_train_refuses_before_device_work(tmp_path, monkeypatch, keys, reason):
    import torch
    from test_shards_cpu import _synthetic_shards
    from video_dqn_amd import trainer
    from video_dqn_amd.config import get_cfg_defaults
    shards = str(tmp_path / "shards")
    _synthetic_shards(shards)
    c = get_cfg_defaults()
    c.DATASET = shards
    for k, v in keys.items():
        c[k] = v
    c.folder, c.device = str(tmp_path), "cuda"

    def no_device(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(torch.cuda, "mem_get_info", no_device)
    monkeypatch.setattr(torch.cuda, "current_stream", no_device)
    monkeypatch.setattr(torch, "manual_seed", no_device)
    monkeypatch.setattr(trainer, "build_model", no_device)
    with pytest.raises(ValueError, match=reason):
        trainer.run_train(c, log=lambda *a: None)


def test_check_config_accepts_the_range():
    from video_dqn_amd.augment import check_config
    for pad in (0, 1, 32):
        for fa in ([1, 2], [2, 1], (0, 2), [0, 1]):
            check_config(pad, True, fa)
    for bad in (True, 1.0, "8"):
        with pytest.raises(ValueError, match="AUG_SHIFT_PAD"):
            check_config(bad, False, [1, 2])
    with pytest.raises(ValueError, match="AUG_FLIP "):
        check_config(0, 1, [1, 2])
    with pytest.raises(ValueError, match="AUG_FLIP_ACTIONS"):
        check_config(0, True, [1, 2.0])


# ---- the oracle against an independent statement: mirror the source, pad by edge replication, crop at the drawn offset ----------
def _frames(n=2, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)


def _pad_crop(frame, sx, sy, flip, P):
    src = frame[:, ::-1] if flip else frame
    padded = np.pad(src, ((P, P), (P, P), (0, 0)), mode="edge")
    return padded[P + sy:P + sy + 224, P + sx:P + sx + 224]


@pytest.mark.parametrize("sx,sy,flip", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-8, 8, 1)])
def test_oracle_equals_mirror_pad_crop(sx, sy, flip):
    fr = _frames()
    got = aug_oracle.augment_frames(fr, np.array([[sx, sy, flip, 0]], np.int32))
    for i in range(len(fr)):
        np.testing.assert_array_equal(got[i], _pad_crop(fr[i], sx, sy, flip, 8))
    assert not np.array_equal(got, fr)


def test_oracle_identity_double_mirror_and_far_shift():
    fr = _frames(3, seed=1)
    np.testing.assert_array_equal(aug_oracle.augment_frames(fr, np.zeros((1, 4), np.int32)), fr)
    mirror = np.array([[0, 0, 1, 0]], np.int32)
    once = aug_oracle.augment_frames(fr, mirror)
    np.testing.assert_array_equal(once, fr[:, :, ::-1])
    np.testing.assert_array_equal(aug_oracle.augment_frames(once, mirror), fr)
    far = aug_oracle.augment_frames(fr, np.array([[1000, -1000, 0, 0]], np.int32))
    far_m = aug_oracle.augment_frames(fr, np.array([[1000, -1000, 7, 0]], np.int32))  # flip != 0 means 1
    for i in range(len(fr)):
        assert np.all(far[i] == fr[i][0][223]) and np.all(far_m[i] == fr[i][0][0])
    # extreme int32 values stay inside the frame
    ext = aug_oracle.augment_frames(fr[:1], np.array([[-2**31, 2**31 - 1, 0, 0]], np.int32))
    assert np.all(ext[0] == fr[0][223][0])


def test_oracle_params_per_sample_shared_by_its_frames():
    fr = _frames(8, seed=2)
    params = np.array([[3, -2, 0, 0], [0, 5, 1, 0]], np.int32)
    got = aug_oracle.augment_frames(fr, params, frames_per_sample=4)
    for i in range(8):
        np.testing.assert_array_equal(got[i], aug_oracle.augment_frames(fr[i:i + 1], params[i // 4:i // 4 + 1])[0])


def test_oracle_swap_actions():
    params = np.array([[0, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0]], np.int32)
    act = np.array([1, 1, 2, 0, 2], np.int64)
    np.testing.assert_array_equal(aug_oracle.swap_actions(act, params), [2, 1, 1, 0, 2])
    np.testing.assert_array_equal(aug_oracle.swap_actions(act, params, 0, 2), [1, 1, 0, 2, 2])
    np.testing.assert_array_equal(act, [1, 1, 2, 0, 2])


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def test_draw_range_and_coverage():
    for P in (0, 1, 8, 32):
        for seed, step in ((0, 1), (7, 99999), (2**63 + 5, 3)):
            d = aug_oracle.draw(seed, step, 256, P, True)
            assert d.dtype == np.int32 and d.shape == (256, 4)
            assert d[:, :2].min() >= -P and d[:, :2].max() <= P and set(np.unique(d[:, 2])) <= {0, 1} and np.all(d[:, 3] == 0)
    d = aug_oracle.draw(0, 1, 256, 8, True)
    assert len(np.unique(d[:, 0])) == 17 and len(np.unique(d[:, 1])) == 17 and len(np.unique(d[:, 2])) == 2


def test_draw_flip_share_and_independence():
    d = np.concatenate([aug_oracle.draw(0, step, 256, 8, True) for step in range(1, 17)])
    assert len(d) == 4096
    share = d[:, 2].mean()
    corr = np.corrcoef(d[:, 0], d[:, 1])[0, 1]
    print(f"flip share {share:.4f}, corr(sx, sy) {corr:.2e}")
    assert abs(share - 0.5) <= 0.03 and abs(corr) < 0.05


def test_draw_slices_stream_and_flip_off():
    whole = aug_oracle.draw(4, 12, 32, 8, True)
    np.testing.assert_array_equal(aug_oracle.draw(4, 12, 32, 8, True, first=16, n=16), whole[16:32])
    off = aug_oracle.draw(4, 12, 32, 8, False)
    assert np.all(off[:, 2] == 0)
    np.testing.assert_array_equal(off[:, :2], whole[:, :2])
    # a stream of its own: not the hash prioritized replay draws from at the same seed, update and batch
    key_per = per_oracle.splitmix64(4)
    h_per = [per_oracle.splitmix64(key_per ^ (12 * 32 + j)) for j in range(32)]
    np.testing.assert_array_equal(per_oracle.uniforms(4, 12, 32), np.array([(h >> 11) * 2.0 ** -53 for h in h_per]))
    sx_from_per = np.array([(((h & 0xFFFF) * 17) >> 16) - 8 for h in h_per])
    assert not np.array_equal(sx_from_per, whole[:, 0])
    assert aug_oracle.splitmix64(4 ^ aug_oracle.AUG_STREAM) != key_per
    assert aug_oracle.AUG_STREAM == int.from_bytes(b"AUGMENT1", "big")


# ---- the C entries refuse bad arguments before any device call -------------------------------------------------------------------
def test_c_entries_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()
    buf = (C.c_int32 * 64)()  # host memory, 16-byte aligned below: never dereferenced, every call fails its argument check
    p = (C.addressof(buf) + 15) // 16 * 16
    ok = dict(seed=0, step=1, G=8, first=0, n=8, pad=8, flip=1, params=p)

    def draw(**kw):
        a = dict(ok, **kw)
        return lib.vdqn_aug_draw(a["seed"], a["step"], a["G"], a["first"], a["n"], a["pad"], a["flip"], a["params"], None)
    for kw in (dict(params=None), dict(n=0), dict(n=-3), dict(pad=-1), dict(pad=33), dict(first=4), dict(first=-1), dict(G=0)):
        assert draw(**kw) != 0, kw
        assert b"vdqn_aug_draw" in lib.vdqn_last_error()

    def swap(act=p, params=p, n=4, a0=1, a1=2, out=p):
        return lib.vdqn_aug_swap_actions(act, params, n, a0, a1, out, None)
    for kw in (dict(act=None), dict(params=None), dict(out=None), dict(n=0), dict(a0=1, a1=1), dict(a0=0, a1=3), dict(a0=-1, a1=2)):
        assert swap(**kw) != 0, kw
        assert b"vdqn_aug_swap_actions" in lib.vdqn_last_error()

    def pack(src=p, dst=p, n_img=4, F=1, params=p, n_params=4, dtype=_lib.VDQN_BF16):
        return lib.vdqn_pack_input_aug(src, dst, n_img, F, params, n_params, dtype, None)
    for kw in (dict(src=None), dict(dst=None), dict(params=None), dict(n_img=0), dict(F=0), dict(n_params=0), dict(dtype=_lib.VDQN_F32X3),
               dict(dtype=7)):
        assert pack(**kw) != 0, kw
        assert b"vdqn_pack_input_aug" in lib.vdqn_last_error()
    assert lib.vdqn_net_td_forward(None, C.byref(_lib.StepArgs()), None) != 0  # (null net: refused before anything is read)
    assert lib.vdqn_abi_version() == 16
