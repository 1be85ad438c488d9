"""The frame-gradient oracle (tests/input_grad_oracle.py) against itself, and the C entries' argument checks (no GPU: every call
fails before it reaches the device)."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_grad_oracle as IO


def _w7(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((64, 3, 7, 7), generator=g, dtype=torch.float64) * 2 - 1) * 0.2


def _both(g_c1, w7):
    a = IO.input_grad_packed(g_c1, IO.operand_from_7x7(w7))
    b = IO.input_grad_conv_transpose(g_c1, w7)
    return a, b


def test_two_formulations_agree_on_random_data():
    g = torch.Generator().manual_seed(1)
    g_c1 = torch.rand((1, 112, 112, 64), generator=g, dtype=torch.float64) * 2 - 1
    a, b = _both(g_c1, _w7(2))
    assert a.shape == b.shape == (1, 3, 224, 224)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize("pos", [(0, 0), (0, 111), (111, 0), (111, 111), (0, 57), (111, 40), (63, 0), (18, 111), (50, 61)])
def test_two_formulations_agree_on_impulses(pos):
    """One non-zero element of conv1's output gradient at the four corners, on each edge and inside: the patch it spreads into is
    the 7 x 7 x 3 kernel of its channel, clipped by the frame."""
    w7 = _w7(3)
    h, w = pos
    co = (7 * h + 3 * w) % 64
    g_c1 = torch.zeros((1, 112, 112, 64), dtype=torch.float64)
    g_c1[0, h, w, co] = 1.5
    a, b = _both(g_c1, w7)
    assert torch.equal(a, b)  # one product per element, every other addend an exact zero
    ref = torch.zeros((3, 224 + 7, 224 + 7), dtype=torch.float64)
    ref[:, 2 * h:2 * h + 7, 2 * w:2 * w + 7] = 1.5 * w7[co]  # input row 2 h - 3 + r7, at index + 3
    assert torch.equal(a[0], ref[:, 3:227, 3:227])


def test_operand_and_7x7_weights_are_inverse():
    w7 = _w7(4)
    w = IO.operand_from_7x7(w7)
    assert torch.equal(IO.w7_from_operand(w), w7)
    assert int((w != 0).sum()) == 64 * 147


def test_unpack_inverts_the_space_to_depth_pack():
    """An index-valued frame through the pack and back: every frame pixel is hit exactly once, border and pad channels never."""
    frame = (torch.arange(2 * 3 * 224 * 224, dtype=torch.float64) + 1).reshape(2, 3, 224, 224)
    t = IO.pack_s2d(frame)
    assert torch.equal(IO.unpack_s2d(t), frame)
    vals = t[t != 0]
    assert vals.numel() == frame.numel() and torch.equal(vals.sort().values, frame.reshape(-1))
    for b in (0, 1, 114):
        assert float(t[:, b].abs().max()) == 0 and float(t[:, :, b].abs().max()) == 0
    assert float(t[..., 12:].abs().max()) == 0
    # the other direction: a packed tensor that is non-zero ONLY at border pixels and pad channels unpacks to nothing
    junk = torch.ones((1, 115, 115, 16), dtype=torch.float64)
    junk[:, 2:114, 2:114, :12] = 0
    assert float(IO.unpack_s2d(junk).abs().max()) == 0
    # spot values straight from pack_input_kernel's comment: packed (y, x) holds source (2 (y - 2) + bh, 2 (x - 2) + bw)
    assert t[1, 7, 9, (1 * 2 + 0) * 3 + 2] == frame[1, 2, 2 * 5 + 1, 2 * 7 + 0]


def test_maxpool_backward_routes_by_code_and_rounds_once():
    rng = np.random.default_rng(5)
    idx = IO.random_codes(rng, 1)
    for oh, ow in ((0, 0), (0, 30), (30, 0), (55, 55)):
        assert set(np.unique(idx[0, oh, ow].numpy())) <= set(IO.valid_codes(oh, ow))
    assert len(IO.valid_codes(0, 0)) == 4 and len(IO.valid_codes(0, 9)) == 6 and len(IO.valid_codes(55, 55)) == 9
    g = torch.from_numpy(rng.standard_normal((1, 56, 56, 64)).astype(np.float32)).to(torch.bfloat16).float()
    full = IO.maxpool_bwd(g, idx, round_bf16=False)
    np.testing.assert_allclose(full.double().sum((1, 2)).numpy(), g.double().sum((1, 2)).numpy(), rtol=0, atol=1e-3)  # nothing lost
    rounded = IO.maxpool_bwd(g, idx)
    assert torch.equal(rounded, full.to(torch.bfloat16).float())
    # pixel (1, 1) lies in the windows of pooled (0, 0) [code 8], (0, 1) [6], (1, 0) [2], (1, 1) [0]
    idx2 = torch.full((1, 56, 56, 64), 4, dtype=torch.uint8)
    idx2[0, 0, 0], idx2[0, 0, 1], idx2[0, 1, 0], idx2[0, 1, 1] = 8, 6, 2, 0
    got = IO.maxpool_bwd(g, idx2, round_bf16=False)[0, 1, 1]
    want = ((g[0, 0, 0] + g[0, 0, 1]) + g[0, 1, 0]) + g[0, 1, 1]
    assert torch.equal(got, want)


def test_library_exports_the_input_grad_symbols_and_refuses_bad_arguments():
    from video_dqn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("vdqn_stem_input_grad", "vdqn_stem_input_grad_workspace_bytes", "vdqn_net_input_grad"):
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS
    lib = _lib.load()
    assert lib.vdqn_abi_version() == 16
    assert lib.vdqn_stem_input_grad_workspace_bytes(3, _lib.VDQN_BF16) == 0
    assert lib.vdqn_stem_input_grad_workspace_bytes(3, _lib.VDQN_F32) == 3 * 112 * 112 * 64 * 4
    assert lib.vdqn_stem_input_grad_workspace_bytes(0, _lib.VDQN_BF16) == -1
    assert lib.vdqn_stem_input_grad_workspace_bytes(3, 7) == -1
    p = 4096

    def call(g=p, idx=p, wt=p, out=p, n=1, dtype=_lib.VDQN_BF16, ws=None, ws_bytes=0):
        return lib.vdqn_stem_input_grad(g, idx, wt, None, out, n, dtype, ws, ws_bytes, None)
    for kw in (dict(g=None), dict(idx=None), dict(wt=None), dict(out=None), dict(n=0), dict(n=-2), dict(dtype=7), dict(g=p + 8), dict(out=p + 4),
               dict(idx=p + 1), dict(wt=p + 2), dict(n=5350), dict(dtype=_lib.VDQN_F32), dict(dtype=_lib.VDQN_F32, ws=p, ws_bytes=64)):
        assert call(**kw) != 0, kw
        assert b"vdqn_stem_input_grad" in lib.vdqn_last_error(), kw
    assert call(n=5350) != 0 and b"split the batch" in lib.vdqn_last_error()
    assert call(out=p + 4) != 0 and b"aligned" in lib.vdqn_last_error()
    assert lib.vdqn_net_input_grad(None, C.byref(_lib.StepArgs()), p, 0, None) != 0 and b"vdqn_net_input_grad" in lib.vdqn_last_error()


def test_the_basic_architecture_is_refused_by_name():
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, 1, extra_capacity=False, dtype="bf16", max_batch=2, device="cpu")
    a = _lib.StepArgs()
    a.batch = a.acts_samples = 1
    a.packed_online = a.acts_online = a.bwd = 4096
    assert net.lib.vdqn_net_input_grad(net.handle, C.byref(a), 4096, 0, None) != 0
    assert b"basic" in net.lib.vdqn_last_error()
    ext = NetEngine(3, 5, 1, extra_capacity=True, dtype="bf16", max_batch=2, device="cpu")
    assert ext.lib.vdqn_net_input_grad(ext.handle, C.byref(a), 4096, 2, None) != 0 and b"scale_kind" in ext.lib.vdqn_last_error()
    assert ext.lib.vdqn_net_input_grad(ext.handle, C.byref(a), 4100, 0, None) != 0 and b"aligned" in ext.lib.vdqn_last_error()
    assert ext.lib.vdqn_net_input_grad(ext.handle, C.byref(a), None, 0, None) != 0
