"""Attribution on the GPU: the data-gradient-only backward (vdqn_net_backward_data) against the full backward's frame gradient, the
three kernels of video_dqn_amd/csrc/attrib.hip against tests/attrib_oracle.py bit for bit, `integrated_gradients` / `smoothgrad`
end to end, and integrated gradients against torch autograd on the CPU (oracle/ref_cpu.py).  Every case runs at max_batch <= 8."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import attrib_oracle as AO  # noqa: E402
from helpers import relerr  # noqa: E402
from video_dqn_amd import synth  # noqa: E402

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _module(dtype, max_batch=8, num_frames=1, extra_capacity=True):
    from video_dqn_amd.model import HabitatDQNMultiAction
    m = HabitatDQNMultiAction(3, 5, extra_capacity=extra_capacity, panorama=False, num_frames=num_frames, dtype=dtype, device=DEV,
                              max_batch=max_batch, deterministic=True)
    m.load_state_dict(synth.make_state_dict(7, extra_capacity=extra_capacity, num_frames=num_frames))
    return m


def _u8(seed, n):
    return synth.make_frames_uint8(seed, "f", n, 1, structured=True).reshape(n, 224, 224, 3)


def _frames(seed, B, F=1):
    return torch.from_numpy(AO.normalise(_u8(seed, B * F))).view(B, F, 3, 224, 224).contiguous()


@pytest.fixture(scope="module")
def f32_module():
    return _module("f32")


# ---- 1. the data-only backward is the full backward's frame gradient ------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1), (1, 2)], ids=["B2F1", "B1F2"])
@pytest.mark.parametrize("mode", ["bf16", "f32", "bf16x3"])
def test_backward_data_is_the_full_backwards_frame_gradient(mode, shape):
    """backward_data == the gx of backward_from_dq(want_input_grad=True) on the same saved activations, as int32 bits, with and
    without pixel_units; a second call gives the same bits; no gradient buffer is handed over (vdqn_step_args.grads is NULL)."""
    B, F = shape
    m = _module(mode, max_batch=4, num_frames=F)
    eng = m.engine
    packed = m._packed_with_dgrad()
    _, acts = eng.forward_saved(_frames(3, B, F).to(DEV), 1, B, packed)
    dq = torch.from_numpy(synth.uniform(5, "dq", (B, 15), -1.0, 1.0)).to(DEV)
    for px in (False, True):
        _, want = eng.backward_from_dq(acts, packed, dq, B, want_input_grad=True, pixel_units=px)
        want = want.clone()
        eng._bwd_ws[1].fill_(0x7F)  # nothing the full backward left behind may be what the data-only walk reads
        got = eng.backward_data(acts, packed, dq, B, pixel_units=px)
        assert got.shape == (B * F, 3, 224, 224) and got.dtype == torch.float32
        assert float(got.abs().max()) > 0
        assert torch.equal(_bits(got), _bits(want)), (mode, shape, px, int((_bits(got) != _bits(want)).sum()))
        again = eng.backward_data(acts, packed, dq, B, pixel_units=px)
        assert torch.equal(_bits(again), _bits(got))


# ---- 2. the pack ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pack_case(source, mode, n, S):
    """(src tensor, kwargs of ops.attrib_pack without the device, the oracle's perturbed float frames [S * n, 3, 224, 224])."""
    u8 = _u8(31, n)
    x = AO.normalise(u8)
    if source == "float":  # values no uint8 frame has
        x = (x * np.float32(1.01) + np.float32(0.003)).astype(np.float32)
    src = torch.from_numpy(u8 if source == "uint8" else x)
    coef = (np.arange(S, dtype=np.float32) + np.float32(0.37)) / np.float32(S + 0.11)
    if mode == "const":
        b = AO.norm_pixel([12.0, 100.0, 250.0])
        return src, dict(coef=coef, baseline=[float(v) for v in b]), AO.path_frames(x, b, coef)
    if mode == "image":
        bu8 = _u8(32, n)
        bx = AO.normalise(bu8)
        if source == "float":
            bx = (bx * np.float32(0.5)).astype(np.float32)
        return src, dict(coef=coef, baseline=torch.from_numpy(bu8 if source == "uint8" else bx)), AO.path_frames(x, bx, coef)
    sigma = np.float32(0.15) / AO.STD
    return src, dict(sigma=[float(v) for v in sigma], seed=1234, s0=5, i0=2), AO.noise_frames(x, sigma, 1234, S, s0=5, i0=2)


def _dev_kwargs(kw):
    out = dict(kw)
    if "coef" in out:
        out["coef"] = torch.from_numpy(np.ascontiguousarray(out["coef"])).to(DEV)
    if isinstance(out.get("baseline"), torch.Tensor):
        out["baseline"] = out["baseline"].to(DEV)
    return out


@pytest.mark.parametrize("n,S", [(1, 3), (3, 1), (3, 3)])
@pytest.mark.parametrize("mode", ["const", "image", "noise"])
@pytest.mark.parametrize("source", ["uint8", "float"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_pack_is_the_plain_pack_of_the_oracles_frames(dtype, source, mode, n, S):
    from video_dqn_amd import ops
    src, kw, frames = _pack_case(source, mode, n, S)
    got = ops.attrib_pack(src.to(DEV), S, dtype, **_dev_kwargs(kw))
    want = ops.pack_input(torch.from_numpy(frames).to(DEV), 1, S * n, dtype)
    assert got.shape == want.shape == (S * n, 115, 115, 16)
    gb, wb = got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), want.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(gb, wb), int((gb != wb).sum())
    assert float(got[:, 2:114, 2:114, :12].float().abs().max()) > 0


def test_pack_noise_does_not_depend_on_the_chunking_and_depends_on_the_seed():
    from video_dqn_amd import ops
    src = torch.from_numpy(_u8(33, 2)).to(DEV)
    sg = [0.5, 0.6, 0.7]
    whole = ops.attrib_pack(src, 4, torch.float32, sigma=sg, seed=9)
    halves = torch.cat([ops.attrib_pack(src, 2, torch.float32, sigma=sg, seed=9, s0=s0) for s0 in (0, 2)])
    assert torch.equal(_bits(whole), _bits(halves))
    # images: the second image alone at i0 = 1 is the second image of the pair
    second = ops.attrib_pack(src[1:], 4, torch.float32, sigma=sg, seed=9, i0=1)
    assert torch.equal(_bits(second), _bits(whole.view(4, 2, 115, 115, 16)[:, 1]))
    other = ops.attrib_pack(src, 4, torch.float32, sigma=sg, seed=10)
    assert not torch.equal(_bits(whole), _bits(other))
    assert not torch.equal(_bits(whole[:2]), _bits(whole[2:4]))  # the copies differ


# ---- 3. reduce and finish ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squared", [False, True])
def test_reduce_matches_the_oracle(squared):
    from video_dqn_amd import ops
    rng = np.random.default_rng(41)
    S, n = 5, 3
    g = rng.standard_normal((S * n, 3, 224, 224)).astype(np.float32)
    w = (rng.random(S) / 3 + 0.01).astype(np.float32)  # no powers of two
    gd, wd = torch.from_numpy(g).to(DEV), torch.from_numpy(w).to(DEV)
    want = AO.reduce(g, w, squared=squared)
    got = ops.attrib_reduce(gd, wd, squared=squared)
    assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(want)))
    # continue: two chunks give one call's bits
    acc = ops.attrib_reduce(gd[:2 * n], wd[:2], squared=squared)
    out = ops.attrib_reduce(gd[2 * n:], wd[2:], acc, squared=squared)
    assert out.data_ptr() == acc.data_ptr() and torch.equal(_bits(out.cpu()), _bits(torch.from_numpy(want)))
    assert torch.equal(_bits(ops.attrib_reduce(gd, wd, squared=squared)), _bits(got))  # run to run
    # overwrite: what the buffer held is gone, NaNs included
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import _stream
    held = torch.full((n, 3, 224, 224), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(_lib.load().vdqn_attrib_reduce(gd.data_ptr(), wd.data_ptr(), held.data_ptr(), n, S, int(squared), 0, _stream()), "vdqn_attrib_reduce")
    assert torch.equal(_bits(held.cpu()), _bits(torch.from_numpy(want)))


@pytest.mark.parametrize("source", ["uint8", "float"])
def test_finish_matches_the_oracle(source):
    from video_dqn_amd import ops
    rng = np.random.default_rng(43)
    n = 3
    acc = rng.standard_normal((n, 3, 224, 224)).astype(np.float32)
    accd = torch.from_numpy(acc).to(DEV)
    u8, bu8 = _u8(44, n), _u8(45, n)
    x, bx = AO.normalise(u8), AO.normalise(bu8)
    src, base = (torch.from_numpy(u8), torch.from_numpy(bu8)) if source == "uint8" else (torch.from_numpy(x), torch.from_numpy(bx))
    const = AO.norm_pixel([0.0, 0.0, 0.0])
    for b_arg, b_ref in (([float(v) for v in const], const), (base.to(DEV), bx)):
        for px in (False, True):
            got = ops.attrib_finish(accd, src.to(DEV), b_arg, pixel_units=px)
            want = AO.finish_ig(acc, x, b_ref, ops.stem_pixel_scale() if px else None)
            assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(want))), (source, px)
    got = ops.attrib_finish(accd)
    assert got.shape == (n, 224, 224)
    assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(AO.finish_max(acc))))
    assert torch.equal(_bits(got), _bits(accd.abs().amax(1)))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------
def _target(m, x, category, action=None):
    with torch.no_grad():
        q = m(x)
    act = q[:, category].argmax(-1) if action is None else torch.full((q.shape[0],), action, device=DEV)
    dq = torch.zeros_like(q)
    dq[torch.arange(q.shape[0], device=DEV), category, act] = 1.0
    return dq


def test_integrated_gradients_is_the_oracle_over_input_gradient(f32_module):
    """f32 module, B = 2, steps = 4, max_batch = 8: the method runs one forward / backward pair over 8 samples; `input_gradient` of the
    oracle's eight perturbed float frames in one call runs the same launches on the same operand (the pack test), so the oracle's
    reduce and finish over its result are the method's bits.  A uint8 input with three baseline pixel values goes the same way."""
    m = f32_module
    x = _frames(51, 2).to(DEV)
    black = AO.norm_pixel([0, 0, 0])
    coef = np.array([(k + 0.5) / 4 for k in range(4)], dtype=np.float32)
    w = np.full(4, 1.0 / 4, dtype=np.float32)
    m.train()
    try:
        got = m.integrated_gradients(x, 3, steps=4)
        assert m.training
    finally:
        m.eval()
    assert got.shape == (2, 1, 3, 224, 224) and got.dtype == torch.float32 and float(got.abs().max()) > 0
    xs = AO.path_frames(x.cpu().numpy().reshape(2, 3, 224, 224), black, coef)
    g = m.input_gradient(torch.from_numpy(xs).to(DEV), _target(m, x, 3).repeat(4, 1, 1))
    want = AO.finish_ig(AO.reduce(g.cpu().numpy().reshape(8, 3, 224, 224), w), x.cpu().numpy().reshape(2, 3, 224, 224), black)
    assert torch.equal(_bits(got.cpu().view(2, 3, 224, 224)), _bits(torch.from_numpy(want)))
    # uint8 frames, a grey baseline, a fixed action, pixel units
    u8 = torch.from_numpy(_u8(52, 2)).to(DEV)
    got = m.integrated_gradients(u8, 1, action=2, steps=4, baseline=(128, 128, 128), pixel_units=True)
    from video_dqn_amd import ops
    xn, grey = AO.normalise(u8.cpu().numpy()), AO.norm_pixel([128, 128, 128])
    g = m.input_gradient(torch.from_numpy(AO.path_frames(xn, grey, coef)).to(DEV), _target(m, u8, 1, 2).repeat(4, 1, 1))
    want = AO.finish_ig(AO.reduce(g.cpu().numpy().reshape(8, 3, 224, 224), w), xn, grey, ops.stem_pixel_scale())
    assert got.shape == (2, 3, 224, 224)  # a 4-D input gives a 4-D result
    assert torch.equal(_bits(got.cpu()), _bits(torch.from_numpy(want)))


def test_smoothgrad_without_noise_is_saliency_on_the_tiled_batch(f32_module):
    """sigma = 0, samples = 4, B = 2, max_batch = 8: the four copies are the clean frames, so the method is the oracle's reduce and
    max read-out over `input_gradient` of the four-fold tiled batch, bit for bit (same batch size, same launches).  Against
    `saliency` of the tiled batch itself the bound is relerr < 1e-3, the number test_four_dimensional_input_and_batches_above_max_batch
    uses where tiles may differ: a sample's gradient may depend on its position in the batch in the last bits, and the mean of four
    such gradients is then not any one of them."""
    m = f32_module
    x = _frames(53, 2).to(DEV)
    m.train()
    try:
        got = m.smoothgrad(x, 2, samples=4, sigma=0.0)
        assert m.training
    finally:
        m.eval()
    assert got.shape == (2, 1, 224, 224)
    tiled = x.repeat(4, 1, 1, 1, 1)
    g = m.input_gradient(tiled, _target(m, x, 2).repeat(4, 1, 1))
    want = AO.finish_max(AO.reduce(g.cpu().numpy().reshape(8, 3, 224, 224), np.full(4, 0.25, dtype=np.float32)))
    assert torch.equal(_bits(got.cpu().view(2, 224, 224)), _bits(torch.from_numpy(want)))
    sal = m.saliency(tiled, 2)
    assert relerr(got, sal[:2]) < 1e-3
    # squared: the mean of the squares of four equal gradients
    sq = m.smoothgrad(x, 2, samples=4, sigma=0.0, squared=True)
    assert relerr(sq, got * got) < 1e-3


def test_smoothgrad_noise_chunks_batches_and_shapes():
    """max_batch = 4: B = 2 runs samples = 3 in chunks of 2 + 1 copies, B = 5 splits into 4 + 1 samples; neither changes the noise
    a frame receives (the global copy and image indices), so a frame's map does not depend on its neighbours beyond the last bits."""
    m = _module("f32", max_batch=4)
    u8 = torch.from_numpy(_u8(54, 5)).to(DEV)
    a = m.smoothgrad(u8, 0, action=1, samples=3, sigma=0.1, seed=3)
    assert a.shape == (5, 224, 224) and a.dtype == torch.float32 and float(a.min()) >= 0 and float(a.max()) > 0
    assert torch.equal(_bits(a), _bits(m.smoothgrad(u8, 0, action=1, samples=3, sigma=0.1, seed=3)))
    b = m.smoothgrad(u8[:2].unsqueeze(1), 0, action=1, samples=3, sigma=0.1, seed=3)
    assert b.shape == (2, 1, 224, 224)
    assert relerr(b[:, 0], a[:2]) < 1e-3  # (another batch size may pick other tiles: not bit for bit)
    assert not torch.equal(m.smoothgrad(u8[:2], 0, action=1, samples=3, sigma=0.1, seed=4), b[:, 0])  # another seed, other noise
    # integrated gradients above max_batch and in chunks: steps = 3 at B = 5 -> 4 + 1 samples, one copy per pair
    ig = m.integrated_gradients(u8, 0, action=1, steps=3)
    assert ig.shape == (5, 3, 224, 224)
    parts = torch.cat([m.integrated_gradients(u8[:4], 0, action=1, steps=3), m.integrated_gradients(u8[4:], 0, action=1, steps=3)])
    assert torch.equal(_bits(ig), _bits(parts))


def test_two_frame_samples_keep_their_frames():
    """num_frames = 2, B = 2, bf16, max_batch = 4, steps = 2: copy s of sample b is sample s * B + b and a sample's two frames stay
    together, so the method is again the oracle over `input_gradient` of the four perturbed two-frame samples, bit for bit."""
    m = _module("bf16", max_batch=4, num_frames=2)
    x = _frames(57, 2, 2).to(DEV)
    got = m.integrated_gradients(x, 4, action=0, steps=2)
    assert got.shape == (2, 2, 3, 224, 224)
    black, coef = AO.norm_pixel([0, 0, 0]), np.array([0.25, 0.75], dtype=np.float32)
    xn = x.cpu().numpy().reshape(4, 3, 224, 224)
    xs = torch.from_numpy(AO.path_frames(xn, black, coef)).view(4, 2, 3, 224, 224)
    g = m.input_gradient(xs.to(DEV), _target(m, x, 4, 0).repeat(2, 1, 1))
    want = AO.finish_ig(AO.reduce(g.cpu().numpy().reshape(8, 3, 224, 224), np.full(2, 0.5, dtype=np.float32)), xn, black)
    assert torch.equal(_bits(got.cpu().view(4, 3, 224, 224)), _bits(torch.from_numpy(want)))
    assert float(got[:, 1].abs().max()) > 0
    assert m.smoothgrad(x, 4, action=0, samples=2, sigma=0.05).shape == (2, 2, 224, 224)


# ---- 5. integrated gradients against torch autograd on the CPU --------------------------------------------------------------------
def test_integrated_gradients_match_torch_cpu(f32_module):
    """f32 module, B = 1, steps = 4, black baseline, against oracle.ref_cpu's module differentiated by torch autograd at the same four
    midpoints.  The attribution is a fixed linear combination of four frame gradients times (x - b), so the gate started from the one
    x.grad itself is held to (tests/test_gpu_input_grad.py): every element within 3e-3 of the maximum, the norm within 1e-3.
    Measured on an MI355X: worst element 6.32e-3 of the maximum, norm off by 6.1e-6.  The norm says the tensors agree; the worst
    element is a handful of pixels behind an activation whose ReLU or arg-max falls the other way in the two f32 evaluation orders
    (the docstring of test_autograd_input_gradient_matches_torch_cpu: 2.76e-3 for one gradient; here four gradients at four inputs,
    each with its own, measured against the maximum of a product with (x - b)).  The element gate is therefore twice the measured
    error rounded up to one digit, 2e-2; the norm gate stays 1e-3.
    The completeness gap sum(attr) - (Q(x) - Q(b)) is held to the reference's own gap at the same four steps: within 3e-3 of the
    larger of the two scalars it is the difference of, the element number applied to a scalar.  Measured: -3.980e-3 against
    -3.961e-3, off by 1.6e-4 of 0.122."""
    from oracle import ref_cpu
    m = f32_module
    ref = ref_cpu.HabitatDQNMultiAction(3, 5, extra_capacity=True, panorama=False, num_frames=1)
    ref.load_state_dict(synth.make_state_dict(7))
    ref.eval()
    x = _frames(55, 1)
    cat, act = 3, 1
    b = torch.from_numpy(AO.norm_pixel([0, 0, 0])).view(1, 1, 3, 1, 1).expand_as(x).contiguous()
    total = torch.zeros_like(x, dtype=torch.float64)
    for k in range(4):
        xk = (b + np.float32((k + 0.5) / 4) * (x - b)).clone().requires_grad_(True)
        ref(xk)[0, cat, act].backward()
        total += 0.25 * xk.grad.double()
    want = (x - b).double() * total
    with torch.no_grad():
        dq_ref = float(ref(x)[0, cat, act]) - float(ref(b)[0, cat, act])
    want_delta = float(want.sum()) - dq_ref
    got, delta = m.integrated_gradients(x.to(DEV), cat, action=act, steps=4, return_delta=True)
    assert got.shape == (1, 1, 3, 224, 224) and delta.shape == (1,)
    got = got.double().cpu()
    amax = want.abs().max().item()
    worst = (got - want).abs().max().item()
    nrm = abs(got.norm().item() / want.norm().item() - 1.0)
    scale = max(abs(float(want.sum())), abs(dq_ref))
    print(f"\nintegrated gradients, f32 engine vs torch CPU: worst element {worst / amax:.3e} of the maximum, norm off by {nrm:.3e}; "
          f"completeness gap {float(delta):.6e} against {want_delta:.6e} (off by {abs(float(delta) - want_delta) / scale:.3e} of {scale:.3e})")
    assert amax > 0
    assert worst <= 2e-2 * amax
    assert nrm <= 1e-3
    assert abs(float(delta) - want_delta) <= 3e-3 * scale


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(f32_module):
    from video_dqn_amd import _lib, ops
    m = f32_module
    x = _frames(56, 1).to(DEV)
    basic = _module("f32", max_batch=2, extra_capacity=False)
    basic.eval()
    with pytest.raises(NotImplementedError, match="integrated_gradients: ARCHITECTURE='basic'"):
        basic.integrated_gradients(x, 0)
    with pytest.raises(NotImplementedError, match="smoothgrad: ARCHITECTURE='basic'"):
        basic.smoothgrad(x, 0)
    with pytest.raises(_lib.VdqnError, match="backward_data: ARCHITECTURE='basic'"):
        basic.engine.backward_data(None, None, None, 1)
    with pytest.raises(_lib.VdqnError, match="forward_attrib: ARCHITECTURE='basic'"):
        basic.engine.forward_attrib(x.view(1, 3, 224, 224), 1, None, sigma=[0, 0, 0])
    for steps in (0, -1, 2.5):
        with pytest.raises(ValueError, match="steps"):
            m.integrated_gradients(x, 0, steps=steps)
    for samples in (0, -3):
        with pytest.raises(ValueError, match="samples"):
            m.smoothgrad(x, 0, samples=samples)
    for sigma in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            m.smoothgrad(x, 0, sigma=sigma)
    for baseline in ((1, 2), (0, 0, 300), 7, torch.zeros((2, 1, 3, 224, 224), device=DEV), torch.zeros((1, 1, 224, 224, 3), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="baseline"):
            m.integrated_gradients(x, 0, baseline=baseline)
    with pytest.raises(Exception, match="bad shape"):
        m.smoothgrad(torch.zeros((1, 2, 3, 224, 224), device=DEV), 0)
    with pytest.raises(ValueError, match="coef .* or sigma"):
        ops.attrib_pack(x.view(1, 3, 224, 224), 1, torch.float32)
    with pytest.raises(ValueError, match="source must be"):
        ops.attrib_pack(torch.zeros((1, 3, 224, 225), device=DEV), 1, torch.float32, sigma=[0, 0, 0])
    with pytest.raises(_lib.VdqnError, match="sigma"):
        ops.attrib_pack(x.view(1, 3, 224, 224), 1, torch.float32, sigma=[0.1, -1.0, 0.1])
    with pytest.raises(_lib.VdqnError, match="n_copies"):
        ops.attrib_pack(x.view(1, 3, 224, 224), 0, torch.float32, sigma=[0, 0, 0])
    with pytest.raises(ValueError, match="attrib_reduce"):
        ops.attrib_reduce(torch.zeros((3, 3, 224, 224), device=DEV), torch.ones(2, device=DEV))
    lib = _lib.load()
    with pytest.raises(_lib.VdqnError, match="null"):
        _lib.check(lib.vdqn_net_backward_data(None, C.byref(_lib.StepArgs()), None, None, 0, None), "vdqn_net_backward_data")
    torch.cuda.synchronize()
