"""CPU oracle of the stem's forward chain (tests/test_stem_cpu.py, tests/test_gpu_stem.py): vdqn_stem_conv_pool (csrc/stem.hip, the
persistent bf16 kernel with its arg-max and plain epilogues; csrc/igemm.hip MODE 3 for f32, bf16x3 and bf16 under
VDQN_STEM_PERSISTENT=0), vdqn_maxpool_fwd / vdqn_maxpool_bwd at any size and vdqn_pack_input (csrc/pointwise.hip).

The stem reference is defined on the FLAT packed operand, as wgrad_oracle._stem_dw is for the gradient:
    c1[n, y, x, co] = bias[co] + sum_{kr < 4, j < 64} t_flat[((n * 115 + y + kr) * 115 + x) * 16 + j] * wt[co][kr][0][j]
for y, x < 112, with EVERY element of t_in [n, 115, 115, 16] and wt [64, 4, 1, 64] filled (border rows / columns 0, 1, 114, the pad
channels 12..15 and the weight entries of r7 < 0 / s7 < 0 included): the kernels are plain convolutions over that operand and may
assume nothing about it.  Then ReLU, one rounding to the store type, and MaxPool2d(3, 2, 1) with the first maximum in kh * 3 + kw
order over the in-image taps, taken on the STORED values.

Two operand kinds (make_operands):
  integer  "narrow": t_in, wt in {-1, 0, 1}, bias in [-4, 4]: many windows tie at a non-zero maximum and every code is the answer
           somewhere.  "wide": t_in in [-8, 8], wt in [-4, 4], bias in [-100, 100]: conv values reach about 1000, so the bf16 store
           rounds (exact round-to-even ties included) and rounding itself creates maxima that tie.  In both a quarter of the
           channels (LOW_CHANNELS) carry LOW_BIAS, chosen here on the CPU so that most of their windows are all zero.  reference()
           asserts sum |products| + |bias| < 2^24 per pixel: any summation order gives the integer, acc + bias is exact, and the one
           rounding is torch.Tensor.to(bfloat16).  The check is check_int: every non-zero pooled value bit for bit, a pooled zero by
           == (either sign passes), every arg-max byte equal.
  "real"   uniform draws as conv_epilogue_oracle.make_operands (bf16 values for bf16).  B = 256 * 2^-23 * S is that oracle's
           accumulation bound with K = 256 (S: sum of the absolute products + |bias|); the stored conv value is within
           b = B (f32) or 2^-8 (|ref| + B) + B (bf16) of ref = relu(c1).  check_real, for every element:
             pool  |got - ref_pool| <= max of b over the window's in-image taps (the maximum is 1-Lipschitz);
             idx   a valid code for the position, |got_pool - ref[tap named by idx]| <= b(tap), and no in-image tap of the window has
                   ref - b above got_pool + b(named tap).
           bf16x3 keeps the gate of tests/test_gpu_bf16x3.py (conv_epilogue_oracle.x3_gate).

operand_conditions() asserts on the oracle's OWN operands that the edges are there (ties, all-zero windows, every code, rounding
ties both ways): they are no measurements of a kernel.

pool_fwd_reference / pool_bwd_reference: the standalone pools at any hi, wi, c (the backward: an f32 sum in pooled-row then
window-column order with one rounding, input_grad_oracle.maxpool_bwd generalised).  pack_reference: input_grad_oracle.pack_s2d of the
numpy-f32 (u / 255 - mean) / std — the expression of pack_input_kernel.

The fault injectors at the end return what a wrong kernel would (tests/test_stem_cpu.py applies each)."""
from functools import lru_cache

import numpy as np
import torch

import input_grad_oracle as IG
from conv_epilogue_oracle import BF16, F32, F64, STORE_DTYPE, X3_ERR_MAX, x3_gate  # noqa: F401 (re-exported)

INT_LIMIT = 2 ** 24
K_STEM = 256
LOW_CHANNELS = tuple(range(3, 64, 4))       # one channel of every group of four: every lane group / fragment of the kernels has one
LOW_BIAS = {"narrow": -16.0, "wide": -300.0}  # about -1.5 sigma of the conv sums (sigma 10.7 / 202): P(window all <= 0) is about 0.55
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
NEG_INF = float("-inf")


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def make_operands(kind: str, n: int, dtype: str = "bf16", seed: int = 1):
    """CPU f32 tensors holding values of the storage type: t_in [n, 115, 115, 16], wt [64, 4, 1, 64], bias [64] (f32 for every type),
    every element drawn.  Image i of a draw does not depend on n (one generator per image)."""
    g = torch.Generator().manual_seed(7919 * seed + {"narrow": 1, "wide": 2, "real": 3}[kind])
    if kind == "real":
        rt = (lambda t: t.to(BF16).float()) if dtype == "bf16" else (lambda t: t)
        wt = rt(torch.rand((64, 4, 1, 64), generator=g) * 0.2 - 0.1)
        bias = torch.rand((64,), generator=g) * 2 - 1
    else:
        lw, lb = (1, 4) if kind == "narrow" else (4, 100)
        wt = torch.randint(-lw, lw + 1, (64, 4, 1, 64), generator=g).float()
        bias = torch.randint(-lb, lb + 1, (64,), generator=g).float()
        bias[list(LOW_CHANNELS)] = LOW_BIAS[kind]
    t_in = torch.empty((n, 115, 115, 16))
    for i in range(n):
        gi = torch.Generator().manual_seed(104729 * seed + 31 * i + {"narrow": 1, "wide": 2, "real": 3}[kind])
        if kind == "real":
            t_in[i] = rt(torch.rand((115, 115, 16), generator=gi) * 2 - 1)
        else:
            lt = 1 if kind == "narrow" else 8
            t_in[i] = torch.randint(-lt, lt + 1, (115, 115, 16), generator=gi).float()
    return {"kind": kind, "dtype": dtype, "t_in": t_in, "wt": wt, "bias": bias}


# ---------------------------------------------------------------------------------------------------------------------------------
# the flat convolution, the pools
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_flat(t_in, wt, bias, dtype=F64):
    """c1 [n, 112, 112, 64] in `dtype` arithmetic on the flat operand (module docstring); bias None: without."""
    n = t_in.shape[0]
    x = t_in.to(dtype).contiguous()
    w = wt.to(dtype).reshape(64, 4, 64)
    c1 = torch.zeros((n * 12544, 64), dtype=dtype)
    for kr in range(4):
        win = torch.as_strided(x, (n, 112, 112, 64), (115 * 115 * 16, 115 * 16, 16, 1), kr * 115 * 16)
        c1 += win.reshape(n * 12544, 64) @ w[:, kr, :].t()
    if bias is not None:
        c1 += bias.to(dtype)
    return c1.reshape(n, 112, 112, 64)


def _padded(x, fill):
    """[n, hi, wi, c] -> [n, 2 ho + 1, 2 wo + 1, c], index = pixel + 1, `fill` outside the image."""
    n, hi, wi, c = x.shape
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    p = torch.full((n, 2 * ho + 1, 2 * wo + 1, c), fill, dtype=x.dtype)
    p[:, 1:1 + hi, 1:1 + wi] = x
    return p, ho, wo


def _tap(p, ho, wo, kh, kw):
    return p[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2]


def pool_fwd_reference(x, last_wins=False, outside=NEG_INF):
    """MaxPool2d(3, 2, 1) of x [n, hi, wi, c] (any float type, no ReLU) -> (pool [n, ho, wo, c], idx uint8): the first maximum in
    kh * 3 + kw order over the in-image taps (-0.0 == +0.0: the earlier tap keeps the window).  last_wins / outside: the faults of
    inject_last_max / inject_outside_zero."""
    p, ho, wo = _padded(x, outside)
    best = torch.full_like(_tap(p, ho, wo, 0, 0), NEG_INF)
    code = torch.zeros(best.shape, dtype=torch.uint8)
    for kh in range(3):
        for kw in range(3):
            v = _tap(p, ho, wo, kh, kw)
            upd = (v >= best) if last_wins else (v > best)
            best = torch.where(upd, v, best)
            code = torch.where(upd, torch.full_like(code, kh * 3 + kw), code)
    return best, code


def valid_mask(idx, hi, wi):
    """True where the code of idx [n, ho, wo, c] names a tap inside hi x wi (IG.valid_codes at any size)."""
    _, ho, wo, _ = idx.shape
    i = idx.long()
    kh, kw = i // 3, i % 3
    h = 2 * torch.arange(ho).view(1, ho, 1, 1) - 1 + kh
    w = 2 * torch.arange(wo).view(1, 1, wo, 1) - 1 + kw
    return (i <= 8) & (h >= 0) & (h < hi) & (w >= 0) & (w < wi)


def gather_tap(x, idx, fill=float("nan")):
    """The value of x [n, hi, wi, c] at the tap each code of idx names; `fill` where the code is none of 0..8 or leaves the image."""
    p, ho, wo = _padded(x, fill)
    out = torch.full_like(_tap(p, ho, wo, 0, 0), fill)
    for kh in range(3):
        for kw in range(3):
            out = torch.where(idx == kh * 3 + kw, _tap(p, ho, wo, kh, kw), out)
    return out


def random_codes(g, n, hi, wi, c):
    """uint8 [n, ho, wo, c]: uniformly random valid codes at any size."""
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    kh = torch.randint(0, 3, (n, ho, wo, c), generator=g)
    kw = torch.randint(0, 3, (n, ho, wo, c), generator=g)
    oh, ow = torch.arange(ho).view(1, ho, 1, 1), torch.arange(wo).view(1, 1, wo, 1)
    kh = torch.minimum(torch.maximum(kh, (oh == 0).long()), hi - 2 * oh)
    kw = torch.minimum(torch.maximum(kw, (ow == 0).long()), wi - 2 * ow)
    idx = (kh * 3 + kw).to(torch.uint8)
    assert bool(valid_mask(idx, hi, wi).all())
    return idx


def pool_bwd_reference(gy, idx, x=None, hw=None, dtype=F32):
    """gy [n, ho, wo, c], idx uint8 -> gx [n, hi, wi, c] f32 holding values of `dtype`: every pixel the f32 sum of the <= 4 windows whose
    arg-max it is, in pooled-row then window-column order (maxpool_bwd_kernel, maxpool_bwd_rows_kernel), masked by x > 0 when x is
    given, rounded once."""
    n, ho, wo, c = gy.shape
    hi, wi = (x.shape[1], x.shape[2]) if x is not None else hw
    g = gy.float()
    out = torch.zeros((n, 2 * ho + 1, 2 * wo + 1, c), dtype=F32)
    for kh in (2, 1, 0):       # for a fixed pixel the pooled row grows as kh falls, the window column as kw falls
        for kw in (2, 1, 0):
            out[:, kh:kh + 2 * ho:2, kw:kw + 2 * wo:2] += torch.where(idx == kh * 3 + kw, g, torch.zeros_like(g))
    inside = torch.zeros(out.shape[1:3], dtype=torch.bool)
    inside[1:1 + hi, 1:1 + wi] = True
    assert float(out[:, ~inside].abs().max() if (~inside).any() else 0.0) == 0.0, "a code points outside the image"
    out = out[:, 1:1 + hi, 1:1 + wi].contiguous()
    if x is not None:
        out = torch.where(x.float() > 0, out, torch.zeros_like(out))
    return out.to(dtype).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def reference_int(o, keep_c1=False):
    """Integer operands -> dict(pool f32, idx uint8[, c1 f32 pre-ReLU exact, stored f32]) for the operands' store type.  Asserts
    sum |products| + |bias| < 2^24 at every pixel, which makes the f32 arithmetic used here (and any other order) exact."""
    assert o["kind"] in ("narrow", "wide")
    S = conv_flat(o["t_in"].abs(), o["wt"].abs(), o["bias"].abs(), F32)
    assert float(S.max()) < INT_LIMIT, float(S.max())
    c1 = conv_flat(o["t_in"], o["wt"], o["bias"], F32)
    stored = c1.clamp_min(0).to(STORE_DTYPE[o["dtype"]]).float()
    pool, idx = pool_fwd_reference(stored)
    r = {"pool": pool, "idx": idx}
    if keep_c1:
        r["c1"], r["stored"] = c1, stored
    return r


def stored_bound(ref, B, dtype):
    """b: the bound of a stored conv value against ref = relu(c1) (module docstring)."""
    return B if dtype != "bf16" else 2.0 ** -8 * (ref.abs() + B) + B


def reference_real(o, want_x3=False):
    """Real operands -> dict(ref [n, 112, 112, 64] float64 = relu(c1), b the stored-value bound, pool float64[, pool_bf16: the pooled
    result of the operands rounded to bf16, for the bf16x3 gate])."""
    c1 = conv_flat(o["t_in"], o["wt"], o["bias"], F64)
    S = conv_flat(o["t_in"].abs(), o["wt"].abs(), o["bias"].abs(), F64)
    ref = c1.clamp_min(0)
    r = {"ref": ref, "b": stored_bound(ref, K_STEM * 2.0 ** -23 * S, o["dtype"]), "pool": pool_fwd_reference(ref)[0]}
    if want_x3:
        cb = conv_flat(o["t_in"].to(BF16), o["wt"].to(BF16), o["bias"], F64)
        r["pool_bf16"] = pool_fwd_reference(cb.clamp_min(0))[0]
    return r


@lru_cache(maxsize=None)
def cached_int(kind, n, dtype="bf16"):
    """(operands, reference) of an integer draw, computed once per process and shared: callers must leave both unchanged."""
    o = make_operands(kind, n, dtype)
    return o, reference_int(o)


@lru_cache(maxsize=4)
def cached_real(n, dtype="bf16"):
    o = make_operands("real", n, dtype)
    return o, reference_real(o, want_x3=dtype == "x3")


# ---------------------------------------------------------------------------------------------------------------------------------
# conditions on the oracle's own operands
# ---------------------------------------------------------------------------------------------------------------------------------
def window_stats(stored, pool, idx):
    """Shares over all windows: non-zero ties (a maximum > 0 held by two or more in-image taps), all-zero windows, and per code."""
    p, ho, wo = _padded(stored, NEG_INF)
    hits = torch.zeros(pool.shape, dtype=torch.int32)
    for kh in range(3):
        for kw in range(3):
            hits += (_tap(p, ho, wo, kh, kw) == pool).int()
    total = pool.numel()
    return {"ties": int(((hits >= 2) & (pool > 0)).sum()) / total, "zero": int((pool == 0).sum()) / total,
            "codes": [int((idx == k).sum()) / total for k in range(9)],
            "zero_low": int((pool[..., list(LOW_CHANNELS)] == 0).sum()) / pool[..., list(LOW_CHANNELS)].numel()}


def rounding_stats(c1, stored):
    """Of the post-ReLU integers v and their bf16 stores: the share that differ, and the numbers of exact half-way cases that went
    down and up (round to nearest even does both)."""
    v = c1.clamp_min(0)
    diff = stored != v
    _, e = torch.frexp(v)                       # v = m * 2^e, m in [0.5, 1): a bf16 ulp is 2^(e - 8)
    half = torch.ldexp(torch.ones_like(v), e - 9)
    tie = diff & ((stored - v).abs() == half)
    return {"rounded": int(diff.sum()) / v.numel(), "ties_down": int((tie & (stored < v)).sum()), "ties_up": int((tie & (stored > v)).sum())}


def operand_conditions(kind, n=1):
    """Asserts what the issue asks of the integer draws, on the reference alone -> the figures."""
    o = make_operands(kind, n, "bf16")
    r = reference_int(o, keep_c1=True)
    st = window_stats(r["stored"], r["pool"], r["idx"])
    st.update(rounding_stats(r["c1"], r["stored"]))
    assert st["zero"] >= 0.01, st
    assert min(st["codes"]) > 0, st
    assert st["zero_low"] > 0.5, st
    if kind == "narrow":
        assert st["ties"] >= 0.02, st
    else:
        assert st["rounded"] >= 0.01 and st["ties_down"] >= 1 and st["ties_up"] >= 1, st
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# checks: each returns a list of failure lines (empty: passed); nothing is left out of any of them
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def check_values_exact(what, got, expected):
    """got (a tensor of the store type) against expected (f32 holding values of that type): every non-zero expected value bit for
    bit, a zero by == (either sign)."""
    exp = expected.to(got.dtype)
    if got.shape != exp.shape:
        return [f"{what}: shape {tuple(got.shape)}, expected {tuple(exp.shape)}"]
    bad = torch.where(exp == 0, got != 0, _bits(got) != _bits(exp))
    if not bool(bad.any()):
        return []
    first = tuple(int(v) for v in bad.nonzero()[0])
    return [f"{what}: {int(bad.sum())} of {bad.numel()} values differ, first at {first}: got {float(got[first])}, expected {float(exp[first])}"]


def check_idx_exact(what, got, expected):
    bad = got != expected
    if not bool(bad.any()):
        return []
    first = tuple(int(v) for v in bad.nonzero()[0])
    return [f"{what}: {int(bad.sum())} of {bad.numel()} arg-max bytes differ, first at {first}: got {int(got[first])}, expected {int(expected[first])}"]


def check_int(what, got_pool, got_idx, ref, n_idx=None):
    """The integer pass: pooled values of all images, arg-max bytes of the first n_idx (None: all)."""
    n_idx = got_pool.shape[0] if n_idx is None else n_idx
    fails = check_values_exact(f"{what} pool", got_pool, ref["pool"])
    if n_idx > 0:
        fails += check_idx_exact(f"{what} idx", got_idx[:n_idx], ref["idx"][:n_idx])
    return fails


def _worst(err, bound):
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def real_violations(got_pool, got_idx, ref, n_idx=None):
    """The real-valued pass (module docstring) -> dict of boolean masks of the offending elements (pool: outside the window's largest
    b or not finite; invalid: a code that names no in-image tap; named: the pooled value is not the named tap's within b; beaten: a
    tap of the window certainly beats the named one; the last three over the first n_idx images) and the largest error / bound of the
    pool and of the named-tap check."""
    n = got_pool.shape[0]
    n_idx = n if n_idx is None else n_idx
    got = got_pool.double()
    bp, ho, wo = _padded(ref["b"], 0.0)             # b >= 0: the padding never raises a window's largest b
    bmax = _tap(bp, ho, wo, 0, 0).clone()
    for kh in range(3):
        for kw in range(3):
            bmax = torch.maximum(bmax, _tap(bp, ho, wo, kh, kw))
    err = (got - ref["pool"]).abs()
    v = {"pool": ~(err <= bmax) | ~torch.isfinite(got), "r_pool": _worst(err, bmax), "r_idx": 0.0}
    if n_idx > 0:
        idx, gp = got_idx[:n_idx], got[:n_idx]
        ok = valid_mask(idx, 112, 112)
        named = gather_tap(ref["ref"][:n_idx], idx, 0.0)
        named_b = gather_tap(ref["b"][:n_idx], idx, 0.0)
        e2 = torch.where(ok, (gp - named).abs(), torch.zeros_like(gp))
        low, _, _ = _padded(ref["ref"][:n_idx] - ref["b"][:n_idx], NEG_INF)
        beaten = torch.zeros_like(ok)
        for kh in range(3):
            for kw in range(3):
                beaten |= _tap(low, ho, wo, kh, kw) > gp + named_b
        v.update(invalid=~ok, named=~(e2 <= named_b), beaten=beaten & ok, r_idx=_worst(e2, named_b))
    return v


def check_real(what, got_pool, got_idx, ref, n_idx=None):
    """-> (failure lines, largest pool error / its bound, largest named-tap error / b)."""
    v = real_violations(got_pool, got_idx, ref, n_idx)
    text = {"pool": "pooled values outside the window's largest b (or not finite)", "invalid": "codes name no in-image tap",
            "named": "pooled values are not the named tap's within b", "beaten": "windows hold a tap that certainly beats the named one"}
    fails = []
    for k, t in text.items():
        if k in v and bool(v[k].any()):
            first = tuple(int(i) for i in v[k].nonzero()[0])
            fails.append(f"{what}: {int(v[k].sum())} of {v[k].numel()} {t}, first at {first} (worst pool {v['r_pool']:.3g} x, named {v['r_idx']:.3g} x)")
    return fails, v["r_pool"], v["r_idx"]


def check_pool_fwd(what, got_pool, got_idx, x):
    """The standalone forward on x (f32 holding values of got_pool's type): values as check_values_exact; codes equal to the
    reference's, except in a window whose maximum is a zero and which holds zeros of both signs: there the code must name an in-image
    tap that holds a zero."""
    pool, idx = pool_fwd_reference(x)
    fails = check_values_exact(f"{what} pool", got_pool, pool)
    neg = torch.signbit(x) & (x == 0)
    has_neg = pool_fwd_reference(neg.float())[0] > 0
    has_pos = pool_fwd_reference(((x == 0) & ~neg).float())[0] > 0
    mixed = (pool == 0) & has_neg & has_pos
    named = gather_tap(x, got_idx)
    bad = torch.where(mixed, ~(named == 0), got_idx != idx)
    if bool(bad.any()):
        first = tuple(int(v) for v in bad.nonzero()[0])
        fails.append(f"{what} idx: {int(bad.sum())} of {bad.numel()} codes wrong, first at {first}: got {int(got_idx[first])}, expected {int(idx[first])}")
    return fails


# ---------------------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------------------
def normalise_u8(frames_u8):
    """uint8 [n, 224, 224, 3] -> f32 [n, 3, 224, 224]: (u / 255 - mean) / std in numpy float32, operation by operation."""
    u = np.asarray(frames_u8).astype(np.float32)
    v = ((u / np.float32(255.0)) - MEAN) / STD
    assert v.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


def pack_reference(frames, dtype, pack=IG.pack_s2d):
    """frames uint8 [n, 224, 224, 3] (numpy or torch) or f32 [n, 3, 224, 224] -> [n, 115, 115, 16] of `dtype` (a torch dtype)."""
    if isinstance(frames, torch.Tensor) and frames.dtype == F32:
        x = frames
    else:
        x = normalise_u8(frames.numpy() if isinstance(frames, torch.Tensor) else frames)
    return pack(x).to(dtype)


def byte_frame(shift=0):
    """uint8 [224, 224, 3]: every byte value in every colour at every (bh, bw) slot (source pixel (y, x) holds (x // 2 + 7 * (y // 2)
    + 64 * (2 (y % 2) + x % 2) + 85 c + shift) mod 256: the 112 even columns of one row walk 112 values, the rows shift them by 7,
    so each slot sees all 256), then 0 / 255 at the four corners and alternating along the four edges."""
    y, x, c = np.meshgrid(np.arange(224), np.arange(224), np.arange(3), indexing="ij")
    f = ((x // 2 + 7 * (y // 2) + 64 * (2 * (y % 2) + x % 2) + 85 * c + shift) % 256).astype(np.uint8)
    edge = np.where((np.arange(224) // 2) % 2 == 0, 0, 255).astype(np.uint8)[:, None]   # both values in both slots of an edge
    f[0], f[223], f[:, 0], f[:, 223] = edge, 255 - edge, 255 - edge, edge
    f[0, 0], f[0, 223], f[223, 0], f[223, 223] = 0, 255, 255, 0
    for bh in range(2):
        for bw in range(2):
            for ch in range(3):   # the interior alone holds all 256 values of the slot
                assert len(np.unique(f[2 + bh:222:2, 2 + bw:222:2, ch])) == 256
    return f


def special_f32_frames(n=1, seed=5):
    """f32 [n, 3, 224, 224]: uniform values with -0.0, +0.0, denormals (both signs, the smallest and the largest), and values exactly
    half-way between two bf16 neighbours (ties to the even and to the odd side, both signs) scattered in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, 224, 224), generator=g) * 4 - 2
    flat = x.view(-1)
    bits = flat.view(torch.int32)
    special = torch.tensor([-0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 5e-40, -3e-41])
    tie = bits[50::89].clone()
    bits[50::89] = (tie & ~0xFFFF) | 0x8000                 # exactly half-way: the kept mantissa's last bit is even or odd as drawn
    for k in range(special.numel()):
        flat[k + 3::97] = special[k]
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# fault injectors: what a wrong kernel would return
# ---------------------------------------------------------------------------------------------------------------------------------
def inject_last_max(stored):
    """(pool, idx) with the LAST maximum of a window winning."""
    return pool_fwd_reference(stored, last_wins=True)


def inject_outside_zero(stored):
    """(pool, idx) with the out-of-image taps counted as 0.0, code and all (not masked, not skipped)."""
    return pool_fwd_reference(stored, outside=0.0)


def inject_signed_no_floor(c1_rounded):
    """pool of the plain epilogue without its +0.0 floor: the maximum of the UNCLAMPED rounded values as signed 16-bit patterns (among
    negative values the most negative has the largest pattern), so an all-negative window gives a negative number."""
    pos = pool_fwd_reference(c1_rounded)[0]
    neg = -pool_fwd_reference(-c1_rounded)[0]          # the window's minimum
    return torch.where(pos >= 0, pos.clamp_min(0), neg)


def seam_rows():
    """The conv rows at the top and bottom of a tile's patch (14 ty - 1 + {0, 15}) that exist."""
    return sorted({y for ty in range(8) for y in (14 * ty - 1, 14 * ty + 14) if 0 <= y < 112})


def inject_drop_kr_at_seams(o, kr, dtype=F64):
    """c1 with kernel row kr missing at the tile-seam conv rows -> (c1 [n, 112, 112, 64], the rows touched)."""
    c1 = conv_flat(o["t_in"], o["wt"], o["bias"], dtype)
    w = o["wt"].clone()
    w[:, [k for k in range(4) if k != kr]] = 0
    part = conv_flat(o["t_in"], w, None, dtype)
    rows = seam_rows()
    c1[:, rows] -= part[:, rows]
    return c1, rows


def inject_stale_window(pool, idx, G):
    """Tile t (id img * 64 + ty * 8 + tx) pooled from the window of tile t - 2 G: the buffer a workgroup reuses for its third tile
    still holding its first -> (pool, idx, mask of the touched elements)."""
    n = pool.shape[0]
    tiles = lambda t: t.reshape(n, 8, 7, 8, 7, 64).permute(0, 1, 3, 2, 4, 5).reshape(n * 64, 7, 7, 64)   # noqa: E731
    back = lambda t: t.reshape(n, 8, 8, 7, 7, 64).permute(0, 1, 3, 2, 4, 5).reshape(n, 56, 56, 64)       # noqa: E731
    tp, ti = tiles(pool).clone(), tiles(idx).clone()
    assert n * 64 > 2 * G
    tp[2 * G:], ti[2 * G:] = tiles(pool)[:n * 64 - 2 * G], tiles(idx)[:n * 64 - 2 * G]
    touched = torch.zeros((n * 64, 7, 7, 64), dtype=torch.bool)
    touched[2 * G:] = True
    return back(tp), back(ti), back(touched)


def inject_missing_next_wave_row(stored):
    """pool of the plain epilogue with pooled rows 2 wave + 1 of a tile (7 ty + {1, 3, 5}) missing the row the next wave sends: their
    kh = 2 taps -> (pool, mask of the touched rows)."""
    p, ho, wo = _padded(stored, NEG_INF)
    rows = torch.tensor([oh % 7 in (1, 3, 5) for oh in range(ho)])
    best = torch.full_like(_tap(p, ho, wo, 0, 0), NEG_INF)
    for kh in range(3):
        for kw in range(3):
            v = _tap(p, ho, wo, kh, kw)
            if kh == 2:
                v = torch.where(rows.view(1, ho, 1, 1), torch.full_like(v, NEG_INF), v)
            best = torch.maximum(best, v)
    touched = torch.zeros(best.shape, dtype=torch.bool)
    touched[:, rows] = True
    return best, touched


def truncate_bf16(x):
    """f32 -> the bf16 value below it in magnitude (the low 16 bits dropped), as f32."""
    return (x.float().contiguous().view(torch.int32) & ~0xFFFF).view(F32)


def pack_swapped(frame):
    """IG.pack_s2d with bh / bw swapped in the channel index."""
    n = frame.shape[0]
    t = torch.zeros((n, 115, 115, 16), dtype=frame.dtype)
    for bh in range(2):
        for bw in range(2):
            for c in range(3):
                t[:, 2:114, 2:114, (bw * 2 + bh) * 3 + c] = frame[:, c, bh::2, bw::2]
    return t
