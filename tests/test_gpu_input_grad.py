"""The gradient of a frame on the GPU: the fused stem data-gradient operator (video_dqn_amd/csrc/stem_dgrad.hip) against
tests/input_grad_oracle.py, the engine's use of it, `x.grad` through the module against torch on the CPU (oracle/ref_cpu.py) at the
G3 gate's numbers (tests/test_gpu_autograd.py), and the public methods `input_gradient` / `saliency`."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import input_grad_oracle as IO  # noqa: E402
from helpers import relerr  # noqa: E402
from video_dqn_amd import synth  # noqa: E402

DEV = "cuda"
GATE = {"bf16": 2e-4, "bf16x3": 5e-6, "f32": 1e-3}  # of the output's maximum (tests/test_gpu_ops.py: TOL_F32OUT; the bf16x3 gate)


def _bf16_values(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=None)
def _w7_bf16():
    """conv1's 7x7 weights with bf16 values (f32 storage)."""
    return _bf16_values(torch.from_numpy(synth.uniform(41, "w7", (64, 3, 7, 7), -0.2, 0.2)))


def _operand(dtype):
    return IO.operand_from_7x7(_w7_bf16()).reshape(64, 4, 1, 64).to(dtype).to(DEV)


# ---- operator: impulses, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos", [(0, 0), (0, 55), (55, 0), (55, 55), (0, 27), (30, 20)])
def test_operator_impulses_are_exact(pos):
    """One non-zero bf16 element of g_pool, for every arg-max code that is valid at its position: the output is exactly g * w on
    the (clipped) 7 x 7 x 3 patch of its channel and zero elsewhere — a bf16 x bf16 product is exact in f32 and every other addend
    is zero.  Pins the index mapping, the border drop and the routing by code."""
    from video_dqn_amd import ops
    oh, ow = pos
    w7 = _w7_bf16()
    wt = _operand(torch.bfloat16)
    codes = IO.valid_codes(oh, ow)
    assert len(codes) == (2 if oh == 0 else 3) * (2 if ow == 0 else 3)
    for code in codes:
        co = (11 * code + oh + 3 * ow) % 64
        gval = _bf16_values(torch.tensor(-1.0 - code / 8.0)).item()
        g_pool = torch.zeros((1, 56, 56, 64), dtype=torch.bfloat16)
        g_pool[0, oh, ow, co] = gval
        idx = torch.full((1, 56, 56, 64), 4, dtype=torch.uint8)
        idx[0, oh, ow, co] = code
        got = ops.stem_input_grad(g_pool.to(DEV), idx.to(DEV), wt).cpu()
        h, w = 2 * oh - 1 + code // 3, 2 * ow - 1 + code % 3
        ref = torch.zeros((3, 224 + 7, 224 + 7), dtype=torch.float32)
        ref[:, 2 * h:2 * h + 7, 2 * w:2 * w + 7] = gval * w7[co]  # frame row 2 h - 3 + r7, stored at + 3
        ref = ref[:, 3:227, 3:227]
        assert int((ref != 0).sum()) > 0
        assert torch.equal(got[0], ref), (pos, code, int((got[0] != ref).sum()))


# ---- operator: random --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _random_case(n):
    rng = np.random.default_rng(100 + n)
    g = torch.from_numpy(rng.standard_normal((n, 56, 56, 64)).astype(np.float32))
    g = _bf16_values(g * torch.from_numpy(rng.integers(0, 2, size=g.shape).astype(np.float32)))  # about half of it zero
    idx = IO.random_codes(rng, n)
    w = IO.operand_from_7x7(_w7_bf16())
    return g, idx, IO.stem_input_grad(g, idx, w, round_bf16=True), IO.stem_input_grad(g, idx, w, round_bf16=False)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "f32"])
def test_operator_random_matches_the_oracle(n, mode):
    """Random gradient (half of it zero) and random valid codes on the identical bf16 operands; an odd image count exercises the
    block-to-image split.  bf16: the max-pool backward tiles are rounded to bf16 as vdqn_maxpool_bwd rounds them; f32 / bf16x3: they
    stay f32."""
    from video_dqn_amd import ops
    g, idx, ref_bf16, ref_f32 = _random_case(n)
    dtype = torch.bfloat16 if mode == "bf16" else torch.float32
    got = ops.stem_input_grad(g.to(dtype).to(DEV), idx.to(DEV), _operand(dtype), precision="bf16x3" if mode == "bf16x3" else None)
    ref = ref_bf16 if mode == "bf16" else ref_f32
    assert got.shape == (n, 3, 224, 224) and got.dtype == torch.float32
    err = relerr(got.double().cpu(), ref)
    print(f"\nstem_input_grad {mode} n={n}: max error {err:.3e} of the maximum")
    assert err < GATE[mode]


def test_operator_is_deterministic_and_scales_by_channel():
    from video_dqn_amd import ops
    g, idx, _, _ = _random_case(3)
    gd, idd, wt = g.to(torch.bfloat16).to(DEV), idx.to(DEV), _operand(torch.bfloat16)
    a = ops.stem_input_grad(gd, idd, wt)
    b = ops.stem_input_grad(gd, idd, wt)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    px = ops.stem_input_grad(gd, idd, wt, pixel_units=True)
    scale = torch.from_numpy(ops.stem_pixel_scale()).to(DEV).view(1, 3, 1, 1)
    assert torch.equal(px.view(torch.int32), (a * scale).view(torch.int32))
    np.testing.assert_allclose(ops.stem_pixel_scale(), 1.0 / (255.0 * np.array([0.229, 0.224, 0.225])), rtol=1e-6)


def test_oracle_pack_is_the_pack_kernel():
    from video_dqn_amd import ops
    x = torch.from_numpy(synth.uniform(43, "x", (2, 3, 224, 224), -2.0, 2.0))
    got = ops.pack_input(x.to(DEV), 1, 2, torch.float32).cpu()
    assert torch.equal(got, IO.pack_s2d(x))


# ---- engine == operator ------------------------------------------------------------------------------------------------------
def _module(dtype, seed=7, max_batch=4, num_frames=1, extra_capacity=True, sd=None):
    from video_dqn_amd.model import HabitatDQNMultiAction
    m = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, num_frames=num_frames, dtype=dtype, device=DEV,
                              max_batch=max_batch, deterministic=True)
    m.load_state_dict(sd if sd is not None else synth.make_state_dict(seed, extra_capacity=extra_capacity, num_frames=num_frames))
    return m


def _frames(seed, B, F=1):
    x = synth.normalise_frames(synth.make_frames_uint8(seed, "f", B, F, structured=True))
    return x.view(B, F, 3, 224, 224).contiguous()


def _dq(seed, B):
    return torch.from_numpy(synth.uniform(seed, "dq", (B, 5, 3), -1.0, 1.0))


def test_engine_input_gradient_is_the_operator_on_its_own_tensors():
    """bf16 engine, B = 2: gx of backward_from_dq(want_input_grad=True) == ops.stem_input_grad on the engine's own g_pool, idx and
    conv1 operand (read through the debug-tensor offsets), bit for bit."""
    from video_dqn_amd import ops
    m = _module("bf16")
    eng, B = m.engine, 2
    packed = m._packed_with_dgrad()
    _, acts = eng.forward_saved(_frames(3, B).to(DEV), 1, B, packed)
    grads, gx = eng.backward_from_dq(acts, packed, _dq(5, B).reshape(B, 15).to(DEV), B, want_input_grad=True)
    assert gx.shape == (B, 3, 224, 224) and grads.shape == (eng.trainable_numel,)
    off_g = eng.lib.vdqn_net_bwd_offset(eng.handle, B, b"g_pool")
    off_i = eng.lib.vdqn_net_act_offset(eng.handle, B, b"idx")
    off_w = eng.lib.vdqn_net_packed_offset(eng.handle, b"wf:resnet.conv1")
    assert min(off_g, off_i, off_w) >= 0
    nel = B * 56 * 56 * 64
    g_pool = eng._bwd_ws[1][off_g:off_g + 2 * nel].view(torch.bfloat16).view(B, 56, 56, 64)
    idx = acts[off_i:off_i + nel].view(B, 56, 56, 64)
    wt = packed[off_w:off_w + 64 * 256 * 2].view(torch.bfloat16).view(64, 4, 1, 64)
    assert float(g_pool.float().abs().max()) > 0
    ref = ops.stem_input_grad(g_pool, idx, wt)
    assert torch.equal(gx.view(torch.int32), ref.view(torch.int32))
    assert float(gx.abs().max()) > 0


# ---- autograd, f32, against torch on the CPU ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cpu_case(F=1, zero_frame=None):
    """(state dict, frames [2 or 1, F, ..], dq, x.grad of oracle.ref_cpu's module on the CPU)."""
    from oracle import ref_cpu
    B = 2 if F == 1 else 1
    sd = synth.make_state_dict(7, num_frames=F)
    if zero_frame is not None:  # this frame's 1600 features reach nothing
        sd["top.0.weight"] = sd["top.0.weight"].clone()
        sd["top.0.weight"][:, 1600 * zero_frame:1600 * (zero_frame + 1)] = 0
    ref = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, num_frames=F)
    ref.load_state_dict(sd)
    ref.eval()
    x = _frames(11, B, F).clone().requires_grad_(True)
    dq = _dq(12, B)
    (ref(x) * dq).sum().backward()
    return sd, x.detach(), dq, x.grad.detach()


def _g3_gate(got, ref, what):
    """The G3 gate's numbers (tests/test_gpu_autograd.py): every element within 3e-3 of the tensor's maximum, the L2 norm within 1e-3."""
    got, ref = got.double().cpu(), ref.double()
    amax = ref.abs().max().item()
    worst = (got - ref).abs().max().item()
    nrm = abs(got.norm().item() / ref.norm().item() - 1.0)
    print(f"\n{what}: worst element {worst / amax:.3e} of the maximum, norm off by {nrm:.3e}")
    assert amax > 0
    assert worst <= 3e-3 * amax
    assert nrm <= 1e-3


def _hip_grad(m, x, dq, requires=True):
    xd = x.to(DEV).clone().requires_grad_(requires)
    m.zero_grad(set_to_none=True)
    (m(xd) * dq.to(DEV)).sum().backward()
    return xd.grad


@pytest.fixture(scope="module")
def f32_module():
    return _module("f32")


def test_autograd_input_gradient_matches_torch_cpu(f32_module):
    """x.grad of (q * dq).sum() through the f32 module against oracle.ref_cpu's module on the CPU at the G3 gate's numbers.
    Measured on an MI355X: worst element 2.76e-3 of the maximum (gate 3e-3), norm off by 4.0e-6 (gate 1e-3) — the worst element is a
    handful of pixels behind an activation whose ReLU or arg-max falls the other way in the two f32 evaluation orders (frame 0 of
    the two-frame case below, where none does, agrees to 1e-6).  Then: the parameters' gradients do not depend on whether the
    frames asked for one, and a frozen network still gives the same x.grad."""
    m = f32_module
    _, x, dq, ref = _cpu_case()
    g = _hip_grad(m, x, dq)
    assert g.shape == (2, 1, 3, 224, 224)
    _g3_gate(g, ref, "x.grad, f32 engine vs torch CPU")
    pgrads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    assert len(pgrads) == 68
    # the parameters' gradients do not depend on whether the frames asked for one
    _hip_grad(m, x, dq, requires=False)
    for n, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad.view(torch.int32), pgrads[n].view(torch.int32)), n
    # a frozen network: the graph is built because the input asks for it
    m.requires_grad_(False)
    try:
        g2 = _hip_grad(m, x, dq)
        assert all(p.grad is None for p in m.parameters())
    finally:
        m.requires_grad_(True)
    assert torch.equal(g2.view(torch.int32), g.view(torch.int32))


def test_four_dimensional_input_and_batches_above_max_batch(f32_module):
    m = f32_module
    _, x, dq, _ = _cpu_case()
    g5 = _hip_grad(m, x, dq)
    g4 = _hip_grad(m, x[:, 0], dq)
    assert g4.shape == (2, 3, 224, 224) and torch.equal(g4, g5[:, 0])
    x6, dq6 = torch.cat([x, x.flip(0), x]), torch.cat([dq, dq * 0.5, -dq])  # B = 6 > max_batch = 4: splits as forward does
    g6 = _hip_grad(m, x6, dq6)
    parts = torch.cat([_hip_grad(m, x6[:4], dq6[:4]), _hip_grad(m, x6[4:], dq6[4:])])
    assert g6.shape == (6, 1, 3, 224, 224) and torch.equal(g6.view(torch.int32), parts.view(torch.int32))
    assert relerr(g6[:2], g5) < 1e-3  # (another batch size may pick other tiles: not bit for bit)


def test_two_frames_keep_their_order():
    """num_frames = 2, B = 1: the gradient comes back as [1, 2, 3, 224, 224] in the frames' order — against the CPU module, whose
    top.0 sees frame f's features at columns 1600 f ..; with frame 1's columns zeroed its gradient is exactly zero and frame 0's is
    not; a zero dq gives a zero gradient."""
    sd, x, dq, ref = _cpu_case(F=2, zero_frame=1)
    m = _module("f32", num_frames=2, sd=sd)
    g = _hip_grad(m, x, dq)
    assert g.shape == (1, 2, 3, 224, 224)
    assert float(ref[0, 1].abs().max()) == 0 and float(g[0, 1].abs().max()) == 0
    _g3_gate(g[0, 0], ref[0, 0], "frame 0 of 2")
    assert float(_hip_grad(m, x, dq * 0).abs().max()) == 0
    sd, x, dq, ref = _cpu_case(F=2)
    m.load_state_dict(sd)
    g = _hip_grad(m, x, dq)
    for f in range(2):
        _g3_gate(g[0, f], ref[0, f], f"frame {f} of 2, full weights")


# ---- public methods ----------------------------------------------------------------------------------------------------------
def test_input_gradient_and_saliency(f32_module):
    from oracle import ref_cpu
    m = f32_module
    u8 = torch.from_numpy(synth.make_frames_uint8(21, "f", 2, 1, structured=True)).to(DEV)  # [2, 1, 224, 224, 3]
    dq = _dq(22, 2)
    xn = ref_cpu.to_imgnet(u8[:, 0].cpu()).view(2, 1, 3, 224, 224)
    want = _hip_grad(m, xn, dq)
    m.train()
    try:
        got = m.input_gradient(u8, dq.to(DEV))
        assert m.training
        assert got.shape == (2, 1, 3, 224, 224) and torch.equal(got, want)
        assert torch.equal(m.input_gradient(xn.to(DEV), dq.to(DEV)), want)
        assert torch.equal(m.input_gradient(u8[:, 0], dq.to(DEV)), want)  # [B, 224, 224, 3] with num_frames == 1
        px = m.input_gradient(u8, dq.to(DEV), pixel_units=True)
        from video_dqn_amd import ops
        assert torch.equal(px, want * torch.from_numpy(ops.stem_pixel_scale()).to(DEV).view(1, 1, 3, 1, 1))
        # saliency: three lines of torch on top of input_gradient
        with torch.no_grad():
            q = m(u8)
        for action in (None, 1):
            act = q[:, 3].argmax(-1) if action is None else torch.full((2,), action, device=DEV)
            onehot = torch.zeros_like(q)
            onehot[torch.arange(2, device=DEV), 3, act] = 1.0
            sal = m.saliency(u8, 3, action)
            assert sal.shape == (2, 1, 224, 224)
            assert torch.equal(sal, m.input_gradient(u8, onehot, pixel_units=True).abs().amax(2))
            assert float(sal.max()) > 0
        assert m.training
    finally:
        m.eval()
    m.saliency(u8, 0)
    assert not m.training


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from video_dqn_amd import _lib, ops
    basic = _module("f32", extra_capacity=False)
    basic.eval()
    x = _frames(3, 1).to(DEV)
    with pytest.raises(NotImplementedError, match="basic"):
        basic(x.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="basic"):
        basic.input_gradient(x, _dq(1, 1).to(DEV))
    with pytest.raises(NotImplementedError, match="basic"):
        basic.saliency(x, 0)
    with pytest.raises(_lib.VdqnError, match="basic"):
        basic.engine.backward_from_dq(None, None, None, 1, want_input_grad=True)
    lib = _lib.load()
    good = torch.zeros(4096, dtype=torch.uint8, device=DEV).data_ptr()
    with pytest.raises(_lib.VdqnError, match="null"):
        _lib.check(lib.vdqn_stem_input_grad(None, good, good, None, good, 1, _lib.VDQN_BF16, None, 0, None), "vdqn_stem_input_grad")
    with pytest.raises(_lib.VdqnError, match="n_img"):
        _lib.check(lib.vdqn_stem_input_grad(good, good, good, None, good, 0, _lib.VDQN_BF16, None, 0, None), "vdqn_stem_input_grad")
    with pytest.raises(TypeError):
        ops.stem_input_grad(torch.zeros((1, 56, 56, 64), dtype=torch.bfloat16, device=DEV), torch.zeros((1, 56, 56, 64), dtype=torch.uint8, device=DEV),
                            _operand(torch.float32))
    with pytest.raises(_lib.VdqnError, match="null"):
        _lib.check(lib.vdqn_net_input_grad(None, C.byref(_lib.StepArgs()), good, 0, None), "vdqn_net_input_grad")
    torch.cuda.synchronize()
