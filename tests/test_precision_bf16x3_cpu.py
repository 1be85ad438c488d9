"""CPU-side tests of the bf16x3 compute mode (VDQN_F32X3: f32 storage, GEMMs as split bf16 x 3): the ABI constant, the engine's
storage layout (identical to f32), the dtype checks of the C entry points, the config key and checkpoint compatibility."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_f32x3_constant_matches_header():
    from video_dqn_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vdqn.h")).read()
    m = re.search(r"#define\s+VDQN_F32X3\s+(\d+)", hdr)
    assert m is not None, "VDQN_F32X3 missing from include/vdqn.h"
    assert int(m.group(1)) == _lib.VDQN_F32X3 == 2
    assert _lib.load().vdqn_abi_version() == _lib.ABI_VERSION == 16


@pytest.mark.parametrize("extra_capacity,frames", [(True, 1), (True, 4), (False, 4)])
def test_storage_layout_same_as_f32(extra_capacity, frames):
    """A bf16x3 engine keeps the f32 layout: parameter table, params / BN statistics / packed weights, activations and the
    backward workspace have the f32 sizes; dtype_name stays "f32" (what callers use to pick torch dtypes)."""
    from video_dqn_amd.engine import NetEngine
    a = NetEngine(3, 5, frames, extra_capacity, "f32", 16, device="cpu")
    b = NetEngine(3, 5, frames, extra_capacity, "bf16x3", 16, device="cpu")
    assert (b.dtype_name, b.compute_dtype) == ("f32", "bf16x3")
    assert (a.dtype_name, a.compute_dtype) == ("f32", "f32")
    assert list(a.slots.values()) == list(b.slots.values())
    assert (a.params_numel, a.trainable_numel, a.bnstats_numel, a.packed_bytes) == \
           (b.params_numel, b.trainable_numel, b.bnstats_numel, b.packed_bytes)
    for n in (1, 3, 8):
        assert a.acts_bytes(n) == b.acts_bytes(n)
        assert a.bwd_bytes(n) == b.bwd_bytes(n)
    assert b.params.dtype == torch.float32 and b.bnstats.dtype == torch.float32


def test_net_create_rejects_unknown_dtype():
    from video_dqn_amd import _lib
    lib = _lib.load()
    for dt, ok in ((_lib.VDQN_F32X3, True), (3, False), (-1, False)):
        cfg = _lib.NetConfig(3, 5, 1, 1, dt, 8, 0)
        h = ctypes.c_void_p()
        rc = lib.vdqn_net_create(ctypes.byref(cfg), ctypes.byref(h))
        assert (rc == 0) == ok, (dt, rc)
        if rc == 0:
            lib.vdqn_net_destroy(h)
        else:
            assert b"bad dtype" in lib.vdqn_last_error()


def test_pointwise_entries_reject_f32x3():
    """Only the GEMM entries take VDQN_F32X3; the pointwise ones (called by the engine with VDQN_F32) refuse it at their dtype
    check.  The pointers are non-null placeholders that get the calls past the argument checks up to the dtype check, which
    returns before anything is dereferenced or launched, so no GPU is needed here."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    fake = 256  # never dereferenced: the dtype check returns first
    assert lib.vdqn_pack_input(fake, 0, fake, 1, _lib.VDQN_F32X3, None) != 0
    assert b"bad dtype" in lib.vdqn_last_error()
    assert lib.vdqn_maxpool_fwd(fake, fake, fake, 1, 112, 112, 64, _lib.VDQN_F32X3, None) != 0
    assert b"bad dtype" in lib.vdqn_last_error()


def test_conv_entries_accept_f32x3_dtype():
    """vdqn_conv2d / vdqn_conv2d_wgrad get past the dtype check with VDQN_F32X3 (they then fail on the null tensors) and reject
    dtype 3 at the dtype check itself; the weight-gradient workspace query plans an f32x3 call like an f32 one."""
    from video_dqn_amd import _lib
    lib = _lib.load()
    a = _lib.ConvArgs()
    a.dtype = _lib.VDQN_F32X3
    assert lib.vdqn_conv2d(ctypes.byref(a), None) != 0
    assert b"bad dtype" not in lib.vdqn_last_error()
    a.dtype = 3
    assert lib.vdqn_conv2d(ctypes.byref(a), None) != 0
    assert b"bad dtype" in lib.vdqn_last_error()
    w = _lib.WgradArgs()
    w.n_img, w.hi, w.wi, w.ci, w.pix_stride, w.ho, w.wo, w.co, w.ldg, w.r, w.s, w.stride, w.pad = 4, 14, 14, 128, 128, 14, 14, 128, 128, 3, 3, 1, 1
    sizes = {}
    for dt in (_lib.VDQN_F32, _lib.VDQN_F32X3, 3):
        w.dtype = dt
        sizes[dt] = lib.vdqn_conv2d_wgrad_workspace_bytes(ctypes.byref(w))
    assert sizes[_lib.VDQN_F32X3] == sizes[_lib.VDQN_F32] > 0 and sizes[3] == -1


def test_ops_precision_keyword_checks_operands():
    from video_dqn_amd import _lib, ops
    x32, x16 = torch.zeros(1), torch.zeros(1, dtype=torch.bfloat16)
    assert ops.gemm_dtype_code(x32, None) == _lib.VDQN_F32
    assert ops.gemm_dtype_code(x16, None) == _lib.VDQN_BF16
    assert ops.gemm_dtype_code(x32, "bf16x3") == _lib.VDQN_F32X3
    with pytest.raises(TypeError):
        ops.gemm_dtype_code(x16, "bf16x3")
    with pytest.raises(ValueError):
        ops.gemm_dtype_code(x32, "tf32")


def test_compute_dtype_merges_from_config(tmp_path):
    from video_dqn_amd.config import ExperimentConfig
    folder = tmp_path / "exp"
    folder.mkdir()
    (folder / "config.yml").write_text("COMPUTE_DTYPE: 'bf16x3'\nARCHITECTURE: 'extra_capacity'\n")
    c = ExperimentConfig(str(folder), device="cpu", tensorboard=False)
    assert c.COMPUTE_DTYPE == "bf16x3"
    from video_dqn_amd.model import HabitatDQNMultiAction
    m = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype=c.COMPUTE_DTYPE, device="cpu")
    assert (m.engine.dtype_name, m.engine.compute_dtype) == ("f32", "bf16x3")


def test_state_dict_roundtrip_between_bf16x3_and_f32():
    """Checkpoints hold the f32 master weights whatever the compute mode: a bf16x3 state_dict loads into an f32 / bf16 model and
    back, bit for bit."""
    from video_dqn_amd import synth
    from video_dqn_amd.model import HabitatDQNMultiAction
    sd = synth.make_state_dict(7)
    x3 = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="bf16x3", device="cpu")
    x3.load_state_dict(sd, strict=False)
    for other in ("f32", "bf16"):
        m = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype=other, device="cpu")
        m.load_state_dict(x3.state_dict())
        back = HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, dtype="bf16x3", device="cpu")
        back.load_state_dict(m.state_dict())
        a, b = x3.state_dict(), back.state_dict()
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(x3.engine.params, back.engine.params)
