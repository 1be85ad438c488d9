"""The stem oracle (tests/stem_oracle.py) checked on the CPU, without a GPU: the integer reference equals torch's own f32 chain
(conv2d + relu + one rounding + max_pool2d with indices) bit for bit, torch's f32 on real operands lies inside every derived bound,
the integer draws hold the edges they exist for, the flat operand is tied to the real 7 x 7 / stride-2 convolution, the standalone
pool references equal torch at odd sizes, and every injected fault fails the check aimed at it.

Records (CPU, not thresholds; each test prints its own with pytest -s):
  torch-CPU f32 against float64 on the real draw uses 9e-3 of the pool bound and of the named-tap bound as an f32 store (what the
  accumulation bound B alone leaves a plain f32 sum), 0.96 of both as a bf16 store (the 2^-8 half-ulp term is tight just above a
  power of two).
  Injectors on INTEGER operands: every one fails bit for bit on both draws (pooled values or arg-max bytes changed, of 200704:
  last maximum 0 / 40913 narrow, 0 / 28752 wide; outside-as-zero 0 / 1493; no +0 floor 26668 / -; a kernel row at the seams about
  21000 / 10700; stale window 88255 / 81928; next wave's row 23288 / -), except bf16 truncation on the narrow draw, whose small
  integers are exact in bf16 (0 / 0; the wide draw: 23587 / 110).
  Injectors on REAL operands (share of the touched elements the bounds flag; test_injectors_on_real_operands):
    kernel row dropped at a tile seam      caught, 48 % of the pooled pixels whose window holds a seam row (where that row held the maximum)
    stale window (tile t - 2 G)            caught, 95 %
    next wave's row missing                caught, 29 % of pooled rows 7 ty + {1, 3, 5} (where the lost row held the maximum)
    signed maximum without the +0 floor    caught, every all-negative window (12 % of all windows)
    out-of-image taps counted as 0         caught only as invalid codes, in the 17 % of the border windows that are all zero
    bf16 truncation                        caught on 18 % of the elements (the truncation errors above half an ulp, less what B and
                                           the 2^-8 |ref| term leave)
    last maximum wins                      NOT visible: real operands have no ties at a non-zero maximum (0 of 200704 windows flagged)
  The last line is why the integer pass exists: on the narrow integer draw the same injector changes 20 % of the arg-max bytes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import input_grad_oracle as IG
import stem_oracle as S

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _torch_chain(o, store):
    """torch-CPU f32: the flat operand as a 4 x 4 / 1 convolution with 16 input channels, ReLU, one rounding, max-pool with indices
    -> (pool NHWC of `store`, codes uint8, stored NHWC f32)."""
    x = o["t_in"].permute(0, 3, 1, 2).contiguous()
    w = o["wt"].reshape(64, 4, 4, 16).permute(0, 3, 1, 2).contiguous()       # [co][k][kr][kx]
    c1 = F.relu(F.conv2d(x, w, o["bias"])).to(store).float()
    pool, ind = F.max_pool2d(c1, 3, 2, 1, return_indices=True)
    h, wcol = ind // 112, ind % 112
    oh, ow = torch.arange(56).view(1, 1, 56, 1), torch.arange(56).view(1, 1, 1, 56)
    code = (h - (2 * oh - 1)) * 3 + (wcol - (2 * ow - 1))
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()   # noqa: E731
    return nhwc(pool).to(store), nhwc(code).to(torch.uint8), nhwc(c1)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_integer_reference_equals_torch_f32_bit_for_bit(kind, dtype):
    o = S.make_operands(kind, 2, dtype)
    ref = S.reference_int(o, keep_c1=True)       # (asserts the 2^24 limit)
    pool, code, stored = _torch_chain(o, S.STORE_DTYPE[dtype])
    assert torch.equal(stored, ref["stored"]) and torch.equal(ref["c1"], ref["c1"].round())
    assert S.check_int("torch", pool, code, ref) == []
    assert torch.equal(code, ref["idx"])          # ties included: torch's CPU rule is "first" too (next test)
    assert float(o["t_in"][:, [0, 1, 114]].abs().sum()) > 0 and float(o["t_in"][:, :, [0, 1, 114]].abs().sum()) > 0
    assert float(o["t_in"][..., 12:].abs().sum()) > 0 and float(o["wt"].reshape(64, 4, 4, 16)[:, 0, 0].abs().sum()) > 0


def test_torch_cpu_takes_the_first_maximum():
    x = torch.zeros((1, 1, 4, 4))
    x[0, 0, 1, 2] = x[0, 0, 2, 1] = x[0, 0, 2, 2] = 5.0     # window (1, 1) covers rows / columns 1..3: taps 1, 3 and 4 tie
    _, ind = F.max_pool2d(x, 3, 2, 1, return_indices=True)
    assert int(ind[0, 0, 1, 1]) == 1 * 4 + 2
    pool, idx = S.pool_fwd_reference(x.permute(0, 2, 3, 1))
    assert int(idx[0, 1, 1, 0]) == 1 and float(pool[0, 1, 1, 0]) == 5.0
    assert int(S.inject_last_max(x.permute(0, 2, 3, 1))[1][0, 1, 1, 0]) == 4


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_real_reference_holds_torch_f32_inside_every_bound(dtype):
    o = S.make_operands("real", 2, dtype)
    ref = S.reference_real(o)
    pool, code, _ = _torch_chain(o, S.STORE_DTYPE[dtype])
    fails, r_pool, r_idx = S.check_real("torch", pool, code, ref)
    print(f"\n[ratio] torch f32 / {dtype} store against float64: pool {r_pool:.3g} x its bound, named tap {r_idx:.3g} x b")
    assert fails == []
    assert (r_pool < 0.05 and r_idx < 0.05) if dtype == "f32" else (r_pool <= 1.0 and r_idx <= 1.0)


@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_operand_conditions(kind):
    st = S.operand_conditions(kind, 1)            # (asserts them)
    print(f"\n[operands] {kind}: " + ", ".join(f"{k} {v}" for k, v in st.items() if k != "codes") + f", codes {min(st['codes']):.3f} .. {max(st['codes']):.3f}")
    assert st["zero_low"] > 0.5 and min(st["codes"]) >= 0.08
    o = S.make_operands(kind, 3)
    assert torch.equal(o["t_in"][0], S.make_operands(kind, 1)["t_in"][0]) and not torch.equal(o["t_in"][0], o["t_in"][2])


def test_flat_operand_is_the_7x7_convolution():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((2, 3, 224, 224), generator=g, dtype=F64) * 2 - 1
    w7 = torch.rand((64, 3, 7, 7), generator=g, dtype=F64) * 0.4 - 0.2
    b = torch.rand((64,), generator=g, dtype=F64) * 2 - 1
    got = S.conv_flat(IG.pack_s2d(x), IG.operand_from_7x7(w7).reshape(64, 4, 1, 64), b, F64)
    ref = F.conv2d(x, w7, b, 2, 3).permute(0, 2, 3, 1)
    assert tuple(got.shape) == tuple(ref.shape) == (2, 112, 112, 64)
    assert float((got - ref).abs().max()) < 1e-12


@pytest.mark.parametrize("shape", [(2, 7, 5, 8), (1, 6, 9, 16), (3, 1, 1, 8), (2, 6, 8, 16)])
def test_pool_references_equal_torch(shape):
    n, hi, wi, c = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-3, 4, shape, generator=g).float()
    pool, idx = S.pool_fwd_reference(x)
    xn = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    tp = F.max_pool2d(xn, 3, 2, 1)
    assert torch.equal(tp.detach().permute(0, 2, 3, 1), pool) and bool(S.valid_mask(idx, hi, wi).all())
    assert torch.equal(S.gather_tap(x, idx), pool)
    gy = torch.randint(-2, 3, tuple(pool.shape), generator=g).float()
    tp.backward(gy.permute(0, 3, 1, 2))
    assert torch.equal(S.pool_bwd_reference(gy, idx, None, (hi, wi)), xn.grad.permute(0, 2, 3, 1))
    assert torch.equal(S.pool_bwd_reference(gy, idx, x), (xn.grad * (xn.detach() > 0)).permute(0, 2, 3, 1))
    codes = S.random_codes(g, n, hi, wi, c)
    assert tuple(codes.shape) == tuple(idx.shape)
    # a +-0 tie: only the value and "the code names a zero" are asked
    z = torch.zeros(shape)
    z[:, 0::2, 1::2] = -0.0     # a checkerboard of signs: every window of two or more taps holds both
    z[:, 1::2, 0::2] = -0.0
    p0, i0 = S.pool_fwd_reference(z)
    assert S.check_pool_fwd("zeros", p0, i0, z) == []
    last = S.pool_fwd_reference(z, last_wins=True)[1]
    assert S.check_pool_fwd("zeros", p0, last, z) == [] or hi == wi == 1   # mixed-sign windows accept any zero tap
    assert S.check_pool_fwd("ints", pool, S.inject_last_max(x)[1], x) != [] or hi == wi == 1


def test_pool_bwd_reference_is_the_stem_oracle_at_112():
    g = torch.Generator().manual_seed(12)
    gy = torch.randint(-2, 3, (1, 56, 56, 64), generator=g).float()
    codes = S.random_codes(g, 1, 112, 112, 64)
    assert torch.equal(S.pool_bwd_reference(gy, codes, None, (112, 112), BF16), IG.maxpool_bwd(gy, codes, True))


def test_pack_reference_and_frames():
    f = S.byte_frame()
    assert f.dtype == np.uint8 and {int(f[0, 0, 0]), int(f[0, 223, 0]), int(f[223, 0, 0]), int(f[223, 223, 0])} == {0, 255}
    for edge in (f[0], f[223], f[:, 0], f[:, 223]):
        assert set(np.unique(edge)) == {0, 255}
    from video_dqn_amd import synth
    frames = np.stack([f, S.byte_frame(101)])
    assert torch.equal(S.normalise_u8(frames), synth.normalise_frames(frames[:, None]))   # the loader's expression, same bits
    for dt in (F32, BF16):
        p = S.pack_reference(frames, dt)
        assert tuple(p.shape) == (2, 115, 115, 16) and p.dtype == dt
        border = torch.cat([p[:, [0, 1, 114]].reshape(-1), p[:, :, [0, 1, 114]].reshape(-1), p[..., 12:].reshape(-1)])
        assert int(S._bits(border).abs().max()) == 0
        assert not torch.equal(S.pack_reference(frames, dt, pack=S.pack_swapped), p)
        assert int((S._bits(S.pack_reference(frames, dt, pack=S.pack_swapped)) != S._bits(p)).sum()) > 0.3 * p.numel()
    x = S.special_f32_frames()
    bits = x.view(-1).view(torch.int32)
    assert int(((x == 0) & torch.signbit(x)).sum()) > 100 and int(((x != 0) & (x.abs() < 1.1754944e-38)).sum()) > 100
    tie = (bits & 0xFFFF) == 0x8000
    assert int((tie & ((bits >> 16) & 1 == 0)).sum()) > 100 and int((tie & ((bits >> 16) & 1 == 1)).sum()) > 100
    assert bool(torch.isfinite(x).all())


# ---- every injector fails the check it is aimed at ----
@pytest.fixture(scope="module")
def ints():
    out = {}
    for kind in ("narrow", "wide"):
        o = S.make_operands(kind, 1)
        out[kind] = (o, S.reference_int(o, keep_c1=True))
    return out


def _changed(pool, idx, ref):
    return int((pool != ref["pool"]).sum()), (0 if idx is None else int((idx != ref["idx"]).sum()))


@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_injectors_fail_bit_for_bit_on_integers(ints, kind):
    o, ref = ints[kind]
    st = S.STORE_DTYPE["bf16"]
    q = lambda t: t.to(st)   # noqa: E731
    assert S.check_int("ref", q(ref["pool"]), ref["idx"], ref) == []
    seen = {}
    # last maximum wins: arg-max bytes only
    p, i = S.inject_last_max(ref["stored"])
    assert S.check_values_exact("last", q(p), ref["pool"]) == [] and S.check_idx_exact("last", i, ref["idx"]) != []
    seen["last"] = _changed(p, i, ref)
    # out-of-image taps counted as 0 with their code: arg-max bytes of the all-zero border windows
    p, i = S.inject_outside_zero(ref["stored"])
    assert S.check_values_exact("outside", q(p), ref["pool"]) == [] and S.check_idx_exact("outside", i, ref["idx"]) != []
    assert not bool(S.valid_mask(i, 112, 112).all())
    seen["outside"] = _changed(p, i, ref)
    # signed maxima without the +0 floor
    p = S.inject_signed_no_floor(ref["c1"].to(st).float())
    assert S.check_values_exact("floor", q(p), ref["pool"]) != [] and float(p.min()) < 0
    seen["floor"] = _changed(p, None, ref)
    # one kernel row dropped at the tile seams
    for kr in range(4):
        c1, rows = S.inject_drop_kr_at_seams(o, kr, F32)
        assert rows == [13, 14, 27, 28, 41, 42, 55, 56, 69, 70, 83, 84, 97, 98]
        p, i = S.pool_fwd_reference(c1.clamp_min(0).to(st).float())
        assert S.check_int(f"kr{kr}", q(p), i, ref) != []
        seen[f"kr{kr}"] = _changed(p, i, ref)
    # a stale window buffer (one image: G = 16 puts tile t - 32, four tile rows up, under tile t)
    p, i, touched = S.inject_stale_window(ref["pool"], ref["idx"], 16)
    assert S.check_values_exact("stale", q(p), ref["pool"]) != [] and S.check_idx_exact("stale", i, ref["idx"]) != []
    assert not bool(((p != ref["pool"]) & ~touched).any()) and int(touched.sum()) == touched.numel() // 2
    seen["stale"] = _changed(p, i, ref)
    # pooled rows 2 wave + 1 without the next wave's row
    p, touched = S.inject_missing_next_wave_row(ref["stored"])
    assert S.check_values_exact("wave", q(p), ref["pool"]) != [] and not bool(((p != ref["pool"]) & ~touched).any())
    seen["wave"] = _changed(p, None, ref)
    # truncation instead of round to nearest even: only where the store rounds at all (the wide draw)
    p, i = S.pool_fwd_reference(S.truncate_bf16(ref["c1"].clamp_min(0)))
    if kind == "wide":
        assert S.check_values_exact("trunc", q(p), ref["pool"]) != []
    else:
        assert S.check_int("trunc", q(p), i, ref) == []   # small integers are exact in bf16: this draw cannot see it
    seen["trunc"] = _changed(p, i, ref)
    print(f"\n[injectors] {kind}: (pooled values, arg-max bytes) changed of {ref['pool'].numel()}: {seen}")


def test_injectors_on_real_operands():
    """Which injectors the derived bounds catch on real operands and on what share of the touched elements (module docstring)."""
    o = S.make_operands("real", 1, "bf16")
    ref = S.reference_real(o)
    st = BF16
    stored = ref["ref"].float().to(st).float()
    c1 = S.conv_flat(o["t_in"], o["wt"], o["bias"], F64)
    pool, idx = S.pool_fwd_reference(stored)
    assert S.check_real("clean", pool.to(st), idx, ref)[0] == []

    def flagged(v, touched=None):
        m = v["pool"].clone()
        for k in ("invalid", "named", "beaten"):
            if k in v:
                m |= v[k]
        return int(m.sum()) if touched is None else int((m & touched).sum()) / max(int(touched.sum()), 1)

    share = {}
    # kernel row dropped at the seams: the pooled pixels whose window holds a seam row
    c1x, rows = S.inject_drop_kr_at_seams(o, 1)
    p, i = S.pool_fwd_reference(c1x.clamp_min(0).float().to(st).float())
    touched = torch.zeros((1, 56, 56, 64), dtype=torch.bool)
    for oh in range(56):
        if any(2 * oh - 1 + kh in rows for kh in range(3)):
            touched[:, oh] = True
    share["seam"] = flagged(S.real_violations(p.to(st), i, ref), touched)
    p, i, touched = S.inject_stale_window(pool, idx, 16)
    share["stale"] = flagged(S.real_violations(p.to(st), i, ref), touched)
    p, touched = S.inject_missing_next_wave_row(stored)
    share["wave"] = flagged(S.real_violations(p.to(st), None, ref, 0), touched)
    p = S.inject_signed_no_floor(c1.float().to(st).float())
    allneg = S.pool_fwd_reference(c1)[0] < 0
    share["floor"] = flagged(S.real_violations(p.to(st), None, ref, 0), allneg & (p < 0))
    share["floor_windows"] = int(allneg.sum()) / allneg.numel()
    p, i = S.inject_outside_zero(stored)
    border = torch.zeros((1, 56, 56, 64), dtype=torch.bool)
    border[:, 0] = True
    border[:, :, 0] = True
    v = S.real_violations(p.to(st), i, ref)
    share["outside"] = flagged(v, border)
    assert not bool(v["pool"].any()) and bool(v["invalid"].any())
    p, i = S.pool_fwd_reference(S.truncate_bf16(ref["ref"].float()))
    share["trunc"] = flagged(S.real_violations(p.to(st), i, ref)) / p.numel()
    p, i = S.inject_last_max(stored)
    share["last"] = flagged(S.real_violations(p.to(st), i, ref))
    print(f"\n[injectors] real operands: share of the touched elements flagged: {share}")
    assert share["seam"] > 0.3 and share["stale"] > 0.9 and share["wave"] > 0.2 and share["floor"] > 0.95 and share["floor_windows"] > 0.01
    assert share["outside"] > 0.01 and share["trunc"] > 0.05
    # legitimate: real operands cannot see a wrong tie rule: the integer pass exists for it
    assert share["last"] <= 5
