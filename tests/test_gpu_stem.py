"""The stem's forward chain, the standalone pools and the input pack element by element (tests/stem_oracle.py).

vdqn_stem_conv_pool / _n on the flat packed operand with EVERY element filled (borders, pad channels, the weight entries a 7 x 7
kernel has not), for the (n, n_idx) of CASES: fewer tiles than workgroups; both tile loops; ranges that are no multiple of the grid;
and 17 images, where 64 workgroups walk three tiles, reuse both window buffers and change epilogue on an odd k (the grid is
min(64 n, 2 CUs): the cases are written for 256 CUs and skip elsewhere).  Each case runs the two integer draws (stem_oracle.check_int:
non-zero pooled values bit for bit, zeros by ==, every arg-max byte equal) and the real draw (check_real: the derived bounds), into
caller buffers pre-filled with 0xA5 and followed by a 4 KiB guard: the rows of idx from n_idx on and both guards must keep their
bytes, and the launch is asserted by its profiler tag.  f32 and bf16x3 (csrc/igemm.hip MODE 3) run three of the cases;
test_rerun_persistent_off repeats the bf16 tests in a child process under VDQN_STEM_PERSISTENT=0, the only test of MODE 3's bf16
pooling.  The unfused chain (vdqn_conv2d + vdqn_maxpool_fwd) is held against the same reference; the standalone pools run at odd and
even sizes (generic and row-pair backward kernels: the row-pair condition of vdqn_maxpool_bwd, even hi and wi and 2 (wi / 2) c
(esz + 1) <= 64 KiB, cannot be missed by shape at 112 x 112 x 64, so the generic kernel is shown at the odd sizes and the row-pair
one also at 6 x 8); the pack runs from uint8 (both kernels: an unaligned source takes the generic one) and f32 sources.

Record (MI355X, 256 CUs, not thresholds; each test prints its own with pytest -s).  Integer draws: every path bit-equal to the
reference in pooled values and arg-max bytes on the kernels as they are — the persistent kernel's arg-max and plain epilogues (narrow
and wide, all nine cases), MODE 3 bf16 (the same under VDQN_STEM_PERSISTENT=0), MODE 3 f32 and bf16x3 (narrow), the unfused chain,
the pools and the pack; no case failed, nothing here was tuned on the kernels.  Real draw, largest error as a share of its bound:
  stem_conv_pool<bf16>, persistent     pool 0.959 (n = 1, 3) .. 0.970 (n = 17) of the window's largest b, named tap 0.959 .. 0.970 of b
  stem_conv_pool<bf16>, MODE 3         the same figures (the same bits)
  vdqn_conv2d + vdqn_maxpool_fwd       conv 0.959 of b, pool 0.959, named tap 0.959
    (a bf16 store's b is 2^-8 (|ref| + B) + B: round to nearest uses all of the half-ulp term just above a power of two, so these
    figures measure the rounding, not the accumulation; the f32 path shows what the sums use of B)
  stem_conv_pool<f32>                  pool 7.3e-3 (1,1), 8.3e-3 (3,1), 1.0e-2 (9,4) of B; named tap 7.6e-3 .. 9.0e-3
  stem_conv_pool<bf16x3>               3.3e-6 .. 3.4e-6 of the output's max (gate 1e-4; one bf16 pass 1.8e-3)
The slowest tests: test_rerun_persistent_off 6.3 s (a child process that imports torch and repeats ten tests, 4.6 s of it inside the
child's pytest), test_fused_stem_bf16[17-9] 1.1 s (it computes the 17-image references the other two n = 17 cases share), [1-1] 0.5 s
(the first launch), [9-4] 0.4 s, f32 / x3 [9-4] 0.3 s, everything else under 0.2 s; the file 11.8 s."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import stem_oracle as S  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
FILL = 0xA5
CASES = [(1, 1), (1, 0), (3, 1), (3, 3), (3, 0), (9, 4), (17, 9), (17, 17), (17, 0)]
OTHER_CASES = [(1, 1), (3, 1), (9, 4)]
TAG = {"bf16": "stem_conv_pool<bf16>", "f32": "stem_conv_pool<f32>", "x3": "stem_conv_pool<bf16x3>"}
POOL_SHAPES = [(2, 7, 5, 8), (1, 6, 9, 16), (3, 1, 1, 8), (2, 6, 8, 16), (1, 112, 112, 64)]


@pytest.fixture(autouse=True)
def _profiler():
    from video_dqn_amd import _lib
    _lib.profile_enable(True)
    _lib.profile_collect()
    yield
    _lib.profile_enable(False)


def _launches():
    from video_dqn_amd import _lib
    torch.cuda.synchronize()
    return {k: v["launches"] for k, v in _lib.profile_collect().items()}


def _need_256_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"the (n, n_idx) cases are laid out for a grid of 2 x 256 workgroups; this device has {cus} CUs")


def _dev(t, dtype):
    return t.to(S.STORE_DTYPE[dtype]).to(DEV).contiguous()


def _guarded(shape, dtype):
    """A tensor of `shape` whose bytes are all 0xA5, followed by GUARD bytes of the same -> (raw uint8 buffer, the tensor, its bytes)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return raw, raw[:nbytes].view(dtype).view(shape), nbytes


def _stem(o, n_idx, dtype, fails, what):
    """One vdqn_stem_conv_pool_n into guarded 0xA5 buffers -> (pool, idx) on the CPU; guards, untouched idx rows and the tag checked."""
    from video_dqn_amd import ops
    n = o["t_in"].shape[0]
    st = S.STORE_DTYPE[dtype]
    raw_p, pool, nb_p = _guarded((n, 56, 56, 64), st)
    raw_i, idx, nb_i = _guarded((n, 56, 56, 64), torch.uint8)
    p2, i2 = ops.stem_conv_pool(_dev(o["t_in"], dtype), _dev(o["wt"], dtype), o["bias"].to(DEV), n_idx=n_idx,
                                precision="bf16x3" if dtype == "x3" else None, pool=pool, idx=idx)
    ran = _launches()
    assert p2 is pool and i2 is idx
    if ran != {TAG[dtype]: 1}:
        fails.append(f"{what}: ran {ran}, expected one {TAG[dtype]}")
    if not bool((raw_p[nb_p:] == FILL).all()) or not bool((raw_i[nb_i:] == FILL).all()):
        fails.append(f"{what}: the guard behind pool or idx was written")
    if n_idx < n and not bool((idx[n_idx:] == FILL).all()):
        fails.append(f"{what}: {int((idx[n_idx:] != FILL).sum())} arg-max bytes of the images >= n_idx were written")
    return pool.cpu(), idx.cpu()


def _check_draws(n, n_idx, dtype, kinds):
    fails, notes = [], []
    for kind in kinds:
        what = f"{dtype}/{kind}/({n},{n_idx})"
        if kind == "real":
            o, ref = S.cached_real(n, dtype)
            pool, idx = _stem(o, n_idx, dtype, fails, what)
            if dtype == "x3":
                e3, e1, ok = S.x3_gate(pool, ref["pool"], ref["pool_bf16"])
                notes.append(f"bf16x3 error {e3:.3g} of max (gate {S.X3_ERR_MAX}), one bf16 pass {e1:.3g}")
                if not ok or not bool(torch.isfinite(pool).all()):
                    fails.append(f"{what}: bf16x3 gate: error {e3:.3g} of max, one bf16 pass {e1:.3g}")
                if n_idx:
                    okc = S.valid_mask(idx[:n_idx], 112, 112)
                    named = S.gather_tap(ref["ref"][:n_idx], idx[:n_idx], 0.0)
                    off = (pool[:n_idx].double() - named).abs() > S.X3_ERR_MAX * float(ref["pool"].abs().max())
                    if not bool(okc.all()) or bool((off & okc).any()):
                        fails.append(f"{what}: {int((~okc).sum())} invalid codes, {int((off & okc).sum())} pooled values that are not the named tap's")
            else:
                f, r_pool, r_idx = S.check_real(what, pool, idx, ref, n_idx)
                fails += f
                notes.append(f"real: pool error {r_pool:.3g} x its bound, named tap {r_idx:.3g} x b")
        else:
            o, ref = S.cached_int(kind, n, dtype)
            pool, idx = _stem(o, n_idx, dtype, fails, what)
            fails += S.check_int(what, pool, idx, ref, n_idx)
    print(f"\n[stem] {dtype} ({n},{n_idx}): " + "; ".join(notes))
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("n,n_idx", CASES, ids=lambda v: str(v))
def test_fused_stem_bf16(n, n_idx):
    _need_256_cus()
    _check_draws(n, n_idx, "bf16", ("narrow", "wide", "real"))


def test_plain_and_argmax_tiles_agree_bf16():
    """(3, 1) with image 2 a copy of image 0: the arg-max epilogue (image 0) and the plain one (image 2) give the same pooled bits."""
    _need_256_cus()
    fails = []
    for kind in ("narrow", "wide", "real"):
        o = dict(S.make_operands(kind, 3, "bf16"))
        o["t_in"] = o["t_in"].clone()
        o["t_in"][2] = o["t_in"][0]
        pool, _ = _stem(o, 1, "bf16", fails, kind)
        if not torch.equal(S._bits(pool[2]), S._bits(pool[0])):
            fails.append(f"{kind}: {int((S._bits(pool[2]) != S._bits(pool[0])).sum())} pooled values of the plain image differ in bits from the arg-max image")
        if torch.equal(pool[1], pool[0]):
            fails.append(f"{kind}: image 1 equals image 0")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("n,n_idx", OTHER_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", ["f32", "x3"])
def test_fused_stem_f32_and_bf16x3(dtype, n, n_idx):
    """MODE 3 of csrc/igemm.hip with f32 tensors: integers of bf16 range have a zero low part, so both types are bit-exact."""
    _need_256_cus()
    _check_draws(n, n_idx, dtype, ("narrow", "real"))


@pytest.mark.parametrize("n", [1, 3])
def test_unfused_chain_bf16(n):
    """vdqn_conv2d (bias, ReLU, ci = 64 of pix_stride 16) + vdqn_maxpool_fwd on the same operands, against the same reference."""
    from video_dqn_amd import ops
    fails = []
    for kind in ("narrow", "wide", "real"):
        o = S.make_operands(kind, n, "bf16")
        c1 = ops.conv2d(_dev(o["t_in"], "bf16"), _dev(o["wt"], "bf16"), ho=112, wo=112, co=64, r=4, s=1, stride=1, pad=0,
                        bias=o["bias"].to(DEV), relu=True, ci=64, pix_stride=16)
        pool, idx = ops.maxpool_fwd(c1)
        ran = _launches()
        if ran.get("maxpool_fwd") != 1 or len(ran) != 2:
            fails.append(f"{kind}: ran {ran}")
        c1, pool, idx = c1.cpu(), pool.cpu(), idx.cpu()
        if kind == "real":
            ref = S.reference_real(o)
            err = (c1.double() - ref["ref"]).abs()
            if bool((err > ref["b"]).any()):
                fails.append(f"{kind}: {int((err > ref['b']).sum())} conv values outside b")
            f, r_pool, r_idx = S.check_real(kind, pool, idx, ref)
            fails += f
            print(f"\n[unfused] n = {n}: conv {S._worst(err, ref['b']):.3g} x b, pool {r_pool:.3g} x its bound, named tap {r_idx:.3g} x b")
        else:
            ref = S.reference_int(o, keep_c1=True)
            fails += S.check_values_exact(f"{kind} c1", c1, ref["stored"]) + S.check_int(kind, pool, idx, ref)
    assert not fails, "\n".join(fails[:40])


# ---- the bf16 tests once more on the MODE 3 kernel (the switch is read once per process: a child process) ----
def test_rerun_persistent_off():
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", "test_fused_stem_bf16 or test_plain_and_argmax"],
                       env=dict(os.environ, VDQN_STEM_PERSISTENT="0"), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-6000:]
    print("\n[persistent off]\n" + "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("[stem]") or " passed" in ln))


# ---- standalone pools ----
def _pool_operand(shape, dtype, seed):
    """Integers in [-3, 2] (ties, all-negative windows), a third of the zeros negative."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 3, shape, generator=g).float()
    neg0 = (x == 0) & (torch.rand(shape, generator=g) < 1 / 3)
    return torch.where(neg0, torch.full_like(x, -0.0), x)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_standalone_pools(shape, dtype):
    from video_dqn_amd import ops
    n, hi, wi, c = shape
    st = S.STORE_DTYPE[dtype]
    fails = []
    x = _pool_operand(shape, dtype, 21)
    has_neg0 = bool(((x == 0) & torch.signbit(x)).any())
    dx = _dev(x, dtype)
    assert bool(torch.signbit(dx.float().cpu())[x == 0].any()) == has_neg0
    pool, idx = ops.maxpool_fwd(dx)
    if _launches() != {"maxpool_fwd": 1}:
        fails.append("forward: not one maxpool_fwd launch")
    fails += S.check_pool_fwd("forward", pool.cpu(), idx.cpu(), x)
    if hi * wi > 1:
        ref_pool = S.pool_fwd_reference(x)[0]
        assert bool((ref_pool < 0).any()) and bool((ref_pool == 0).any())   # all-negative windows and zero maxima are there
    g = torch.Generator().manual_seed(22)
    codes = {"random": S.random_codes(g, n, hi, wi, c), "forward": idx.cpu()}
    if not bool(S.valid_mask(codes["forward"], hi, wi).all()):
        fails.append("forward: invalid codes")
        codes.pop("forward")
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    gys = {"int": torch.randint(-2, 3, (n, ho, wo, c), generator=g).float(), "real": (torch.rand((n, ho, wo, c), generator=g) * 2 - 1).to(st).float()}
    for cname, cd in codes.items():
        for gname, gy in gys.items():
            for with_x in (False, True):
                got = ops.maxpool_bwd(_dev(gy, dtype), cd.to(DEV), dx if with_x else None, (hi, wi))
                if _launches() != {"maxpool_bwd": 1}:
                    fails.append("backward: not one maxpool_bwd launch")
                ref = S.pool_bwd_reference(gy, cd, x if with_x else None, (hi, wi), st)
                fails += S.check_values_exact(f"backward {cname} codes / {gname} gy / x {with_x}", got.cpu(), ref)
    assert not fails, "\n".join(fails[:40])


# ---- pack ----
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("source", ["u8-1", "u8-3", "u8-3-unaligned", "f32-2"])
def test_pack_every_element(source, dtype):
    """Every element of [n, 115, 115, 16] has the reference's bits; the border rows / columns and the channels 12..15 are +0.0 over a
    0xA5 pre-fill; nothing is written behind the tensor."""
    from video_dqn_amd import ops
    kind, n = source.split("-")[0], int(source.split("-")[1])
    if kind == "u8":
        frames = np.stack([S.byte_frame(101 * i) for i in range(n)])
        assert len({f.tobytes() for f in frames}) == n
        raw_s = torch.zeros((frames.size + 16,), dtype=torch.uint8, device=DEV)
        off = 1 if source.endswith("unaligned") else 0     # an unaligned uint8 source takes pack_input_kernel, an aligned one the row kernel
        src = raw_s[off:off + frames.size]
        src.copy_(torch.from_numpy(frames).reshape(-1).to(DEV))
        assert src.data_ptr() % 16 == off
        ref = S.pack_reference(frames, dtype)
    else:
        x = S.special_f32_frames(n)
        src = x.to(DEV)
        ref = S.pack_reference(x, dtype)
    raw, out, nbytes = _guarded((n, 115, 115, 16), dtype)
    got = ops.pack_input(src, 0 if kind == "u8" else 1, n, dtype, out=out)
    ran = _launches()
    assert got is out and ran == {"pack_input": 1}, ran
    assert bool((raw[nbytes:] == FILL).all()), "the guard behind the packed tensor was written"
    got = got.cpu()
    bad = S._bits(got) != S._bits(ref)
    first = tuple(int(v) for v in bad.nonzero()[0]) if bool(bad.any()) else None
    assert first is None, f"{int(bad.sum())} of {bad.numel()} elements differ in bits, first at {first}: got {float(got[first])}, expected {float(ref[first])}"
    border = torch.cat([got[:, [0, 1, 114]].reshape(-1), got[:, :, [0, 1, 114]].reshape(-1), got[..., 12:].reshape(-1)])
    assert int(S._bits(border).abs().max()) == 0


def test_wrappers_refuse_wrong_caller_buffers():
    from video_dqn_amd import ops
    o = S.make_operands("narrow", 1)
    t, w, b = _dev(o["t_in"], "bf16"), _dev(o["wt"], "bf16"), o["bias"].to(DEV)
    with pytest.raises(ValueError, match="pool must be"):
        ops.stem_conv_pool(t, w, b, pool=torch.empty((1, 56, 56, 64), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="idx must be"):
        ops.stem_conv_pool(t, w, b, idx=torch.empty((2, 56, 56, 64), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="want_idx=False"):
        ops.stem_conv_pool(t, w, b, want_idx=False, idx=torch.empty((1, 56, 56, 64), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        ops.pack_input(torch.zeros((224 * 224 * 3,), dtype=torch.uint8, device=DEV), 0, 1, torch.bfloat16,
                       out=torch.empty((1, 115, 115, 16), dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
