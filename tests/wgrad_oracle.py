"""CPU oracle of the weight-gradient entries of the C ABI: vdqn_conv2d_wgrad (wgrad_kernel in six instances, wgrad_win_kernel,
stem_wgrad_kernel, wgrad_reduce_kernel, colsum_kernel), vdqn_conv2d_wgrad_workspace_bytes and vdqn_stem_wgrad_pool
(tests/test_wgrad_cpu.py, tests/test_gpu_wgrad.py).  Everything is NHWC, as the ABI sees it.

Two operand kinds (make_operands):
  "int"   x in [-3, 3], gy and g_pool in [-2, 2], integers.  They are exact in bf16, every product and every partial sum in any order
          is an integer below 2^24 (reference() asserts it per case on the sum of the absolute products), so an f32 accumulation is
          exact whatever the tile shape, split, atomic order or reduction order; so are the f32 MFMA and bf16x3 (the low part of a
          small integer is zero) and a max-pool backward tile (at most four windows, at most 8 in magnitude).  The check is
          check_exact: equality with the integer reference, element by element, no tolerance.
  "real"  uniform [-1, 1] rounded to the storage type: integers cannot see a rounding that is skipped or done twice.  The check is
          check_bound: per element |got - ref64| <= B = (M + 2) * 2^-23 * S, S the same gradient of the absolute operands and
          M = n * ho * wo the reduction length: conv_epilogue_oracle.py's any-order bound (M * 2^-24 * S for an f32 sum of M terms in
          any order, the factor 2 for the roundings inside an MFMA and of f32 products) with the additions of the split partials and
          of the atomics counted in (+ 2).  bf16x3 keeps conv_epilogue_oracle.x3_gate.  dbias: the same bound on sum |gy|.

reference(): ordinary geometries through F.grad.conv2d_weight in float64 on the first `ci` channels of x and the first `co` columns
of gy; the stem geometry (r = 4, s = 1, ci = 64 of pix_stride 16, 115 -> 112) directly on the flat operand,
    dw[co][ky][k] = sum gy[n, y, x, co] * xflat[((n * 115 + y + ky) * 115 + x) * 16 + k],  k < 64,
so that any integer "packed" tensor is a valid input and no 7 x 7 remapping is needed.  dbias sums the columns 0 .. co_pad - 1 of gy
(what colsum_kernel sums).  stem_pool_reference() is input_grad_oracle.maxpool_bwd followed by the stem reference.

plan(): a restatement of plan_wgrad (csrc/wgrad.hip): kernel variant / profiler tag, tile, splitk, kchunk, the copies of dw the
ordered mode stores and the workspace bytes, under the same environment switches; stem_pool_grid() likewise.

The fault injectors at the end produce the wrong results the checks must catch (tests/test_wgrad_cpu.py applies each)."""
import os
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import input_grad_oracle as IG
from conv_epilogue_oracle import BF16, F32, F64, STORE_DTYPE, x3_gate  # noqa: F401 (x3_gate re-exported)

SENTINEL = 768.0          # exact in bf16 and f32, far from every result: the padding rows of dw
INT_LIMIT = 2 ** 24
KIND = {"bf16": "bf16", "f32": "f32", "x3": "bf16x3"}
CODE_TABLE_BYTES = 3200   # kWgCodeBytes: the window kernel's border-code table


@dataclass(frozen=True)
class Case:
    name: str
    dtype: str        # "bf16", "f32", "x3" (f32 tensors, split-bf16 MFMAs)
    n: int
    hi: int
    wi: int
    ci: int
    pix_stride: int
    ho: int
    wo: int
    co: int
    ldg: int
    r: int
    s: int
    stride: int
    pad: int
    splitk: int = 0   # 0: the library's own split

    @property
    def M(self):
        return self.n * self.ho * self.wo

    @property
    def co_pad(self):
        return (self.co + 63) // 64 * 64

    @property
    def is_stem(self):
        return (self.r, self.s, self.ci, self.pix_stride, self.hi, self.wi, self.ho, self.wo, self.stride, self.pad) == \
            (4, 1, 64, 16, 115, 115, 112, 112, 1, 0)


def geo(name, dtype, n, hi, wi, ci, co, k, stride, pad, *, ldg=None, pix_stride=None, splitk=0):
    ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
    return Case(name, dtype, n, hi, wi, ci, ci if pix_stride is None else pix_stride, ho, wo, co, (co + 63) // 64 * 64 if ldg is None else ldg,
                k, k, stride, pad, splitk)


def stem(name, dtype, n, splitk=0):
    return Case(name, dtype, n, 115, 115, 64, 16, 112, 112, 64, 64, 4, 1, 1, 0, splitk)


def _dtypes(name, dtypes, *a, **kw):
    return [geo(f"{name}-{d}", d, *a, **kw) for d in dtypes]


ALL3 = ("bf16", "f32", "x3")
CASES = (
    # ---- window kernel (bf16, 3x3 / 1 / 1), wgrad_win<bf16,64> ----
    [geo("win-2x2", "bf16", 7, 2, 2, 128, 64, 3, 1, 1),          # every pixel a border of every kind; 32 images per K tile
     geo("win-3x3", "bf16", 40, 3, 3, 64, 64, 3, 1, 1),          # rem wraps 14 times per tile (128 % 9); automatic split of 2
     geo("win-5x17", "bf16", 3, 5, 17, 64, 128, 3, 1, 1),        # non-square, wide
     geo("win-10x6", "bf16", 5, 10, 6, 64, 64, 3, 1, 1),         # non-square, tall
     geo("win-10x6-k3", "bf16", 5, 10, 6, 64, 64, 3, 1, 1, splitk=3),   # a split that starts inside an image
     geo("win-10x6-k5", "bf16", 5, 10, 6, 64, 64, 3, 1, 1, splitk=5),   # (VDQN_WGRAD_WINDOW=0: splits with an empty range)
     geo("win-8x8", "bf16", 4, 8, 8, 64, 64, 3, 1, 1),           # M = 256: kchunk and tile ends coincide with M
     geo("win-57x56", "bf16", 1, 57, 56, 64, 64, 3, 1, 1),       # 3192 of the 3200 code-table bytes, non-square, 13 splits
     geo("win-co100", "bf16", 3, 9, 9, 64, 100, 3, 1, 1, ldg=128),      # ragged co, gy columns 100..127 non-zero
     geo("win-ldg192", "bf16", 2, 6, 10, 64, 64, 3, 1, 1, ldg=192)]     # gy rows wider than co_pad
    # ---- routing edges beside the window kernel (bf16) ----
    + [geo("gen-58x56", "bf16", 1, 58, 56, 128, 128, 3, 1, 1),          # 3248 > 3200 table bytes: wgrad<bf16,128>
       geo("gen-pix128", "bf16", 3, 5, 17, 64, 64, 3, 1, 1, pix_stride=128),   # pix_stride != ci: wgrad<bf16,64>
       geo("gen-w1", "bf16", 5, 4, 1, 64, 64, 3, 1, 1)]                 # wo = 1
    # ---- generic kernel ----
    + _dtypes("s2-odd", ALL3, 3, 9, 9, 64, 128, 3, 2, 1)                # hi < 2 ho: car_oh negative modulo 2^32
    + _dtypes("s2-14x9", ALL3, 3, 14, 9, 128, 256, 3, 2, 1)             # 128-wide tiles, non-square
    + _dtypes("ds", ALL3, 2, 14, 10, 128, 256, 1, 2, 0)                 # bf16: 64-wide tiles by VDQN_WGRAD_DS64; f32 / x3: 128
    + [geo("ds-odd-bf16", "bf16", 3, 9, 7, 64, 128, 1, 2, 0)]
    + _dtypes("valid", ALL3, 3, 7, 9, 128, 64, 3, 1, 0)
    + _dtypes("linear", ALL3, 37, 1, 1, 256, 15, 1, 1, 0)
    + _dtypes("co130", ("bf16", "f32"), 2, 6, 6, 64, 130, 3, 1, 0, ldg=192)    # 24 / 48 column groups in colsum_kernel
    + _dtypes("5x17", ("f32", "x3"), 3, 5, 17, 64, 128, 3, 1, 1)        # the window geometries on the f32 kernels (KP = 64)
    + _dtypes("10x6", ("f32", "x3"), 5, 10, 6, 64, 64, 3, 1, 1)
    + [geo("10x6-k5-f32", "f32", 5, 10, 6, 64, 64, 3, 1, 1, splitk=5)]  # splits 3 and 4 have no pixels
    # the bf16 64-wide tiles stage 128 pixels per K-step: the cases above with M <= 128 compute the slot advances (adv_*, car_ow, car_oh)
    # but never use them there.  The same geometries with a second K-step:
    + [geo("s2-odd-n8-bf16", "bf16", 8, 9, 9, 64, 128, 3, 2, 1),        # M = 200: 128 = 5 images + 3 pixels, car_oh negative
       geo("ds-odd-n8-bf16", "bf16", 8, 9, 7, 64, 128, 1, 2, 0),        # M = 160
       geo("valid-n8-bf16", "bf16", 8, 7, 9, 128, 64, 3, 1, 0),         # M = 280: two splits, the first of two K-steps
       geo("gen-w1-5x1", "bf16", 30, 5, 1, 64, 64, 3, 1, 1)]            # wo = 1, M = 150: 128 = 25 images + 3 rows
    + _dtypes("l4", ("f32", "x3"), 2, 7, 7, 512, 512, 3, 1, 1)          # 128-wide f32 tiles (KP = 32)
    # ---- stem: rows per block 1, 2, 3 (the last: blocks that cross images, a one-row last block) ----
    + [stem("stem-1", "bf16", 1), stem("stem-5", "bf16", 5), stem("stem-10", "bf16", 10),
       stem("stem-1-k1", "bf16", 1, splitk=1),                          # the same geometry on wgrad<bf16,64>: overlapping 64-wide "channels"
       stem("stem-1-f32", "f32", 1), stem("stem-1-x3", "x3", 1)]
)
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
POOL_N = (1, 10, 19)   # pooled-row pairs per block 1, 2, 3; 19 is the smallest n with a short last block


# ---------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(name, seed, kind):
    return torch.Generator().manual_seed(1000 * seed + sum(map(ord, name)) + (0 if kind == "int" else 500))


def _draw(g, shape, lim, kind, dtype):
    if kind == "int":
        return torch.randint(-lim, lim + 1, shape, generator=g).float()
    t = torch.rand(shape, generator=g) * 2 - 1
    return t.to(BF16).float() if dtype == "bf16" else t


def make_operands(c: Case, seed: int = 1, kind: str = "int"):
    """CPU f32 tensors holding values of the case's storage type: x [n, hi, wi, pix_stride] (EVERY channel filled, those past ci
    included), gy [n, ho, wo, ldg] (EVERY column filled, the padding included), and for the integer kind the starting values
    dw0 [co_pad, r, s, ci] (integers in [-50, 50] in rows < co, SENTINEL in rows >= co) and dbias0 [co_pad] (integers)."""
    g = _gen(c.name, seed, kind)
    o = {"kind": kind,
         "x": _draw(g, (c.n, c.hi, c.wi, c.pix_stride), 3, kind, c.dtype),
         "gy": _draw(g, (c.n, c.ho, c.wo, c.ldg), 2, kind, c.dtype)}
    if kind == "int":
        dw0 = torch.randint(-50, 51, (c.co_pad, c.r, c.s, c.ci), generator=g).float()
        dw0[c.co:] = SENTINEL
        o["dw0"], o["dbias0"] = dw0, torch.randint(-50, 51, (c.co_pad,), generator=g).float()
    return o


def make_pool_operands(n: int, seed: int = 1, kind: str = "int"):
    """g_pool [n, 56, 56, 64] (f32 holding bf16 values), idx uint8 valid arg-max codes, packed [n, 115, 115, 16], dw0 [64, 4, 1, 64]."""
    g = _gen(f"pool-{n}", seed, kind)
    rng = np.random.default_rng(7000 * seed + n)
    o = {"kind": kind, "g_pool": _draw(g, (n, 56, 56, 64), 2, kind, "bf16"), "idx": IG.random_codes(rng, n),
         "packed": _draw(g, (n, 115, 115, 16), 3, kind, "bf16")}
    if kind == "int":
        o["dw0"] = torch.randint(-50, 51, (64, 4, 1, 64), generator=g).float()
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------------------
def _stem_dw(gy, xflat, dtype=F64):
    """gy [n, 112, 112, >= 64], x [n, 115, 115, 16] -> dw [64, 4, 1, 64] on the flat operand (module docstring)."""
    n = gy.shape[0]
    x = xflat.to(dtype).contiguous()
    g = gy[..., :64].to(dtype).reshape(n * 12544, 64)
    dw = torch.zeros((64, 4, 1, 64), dtype=dtype)
    for ky in range(4):
        win = torch.as_strided(x, (n, 112, 112, 64), (115 * 115 * 16, 115 * 16, 16, 1), ky * 115 * 16)
        dw[:, ky, 0, :] = g.t() @ win.reshape(n * 12544, 64)
    return dw


def _dw(c: Case, gy, x, dtype=F64):
    """dw [co, r, s, ci] of the case in `dtype` arithmetic."""
    if c.is_stem:
        return _stem_dw(gy, x, dtype)[:c.co]
    xn = x[..., :c.ci].to(dtype).permute(0, 3, 1, 2)
    gn = gy[..., :c.co].to(dtype).permute(0, 3, 1, 2)
    dw = F.grad.conv2d_weight(xn, (c.co, c.ci, c.r, c.s), gn, c.stride, c.pad)
    assert tuple(dw.shape) == (c.co, c.ci, c.r, c.s)
    return dw.permute(0, 2, 3, 1).contiguous()


def reference(c: Case, o, dtype=F64):
    """-> dict(dw [co, r, s, ci], dbias [co_pad], S, Sb: the same of the absolute operands, B, Bb: the bounds) in `dtype` (float64:
    the reference; float32: torch's own f32, which tests/test_wgrad_cpu.py holds against it).  Integer operands: asserts that every
    partial sum in any order stays below 2^24 (S, plus the starting value's 50)."""
    gy, x = o["gy"], o["x"]
    dw, S = _dw(c, gy, x, dtype), _dw(c, gy.abs(), x.abs(), F64)
    flat = gy.reshape(c.M, c.ldg)[:, :c.co_pad]
    dbias, Sb = flat.to(dtype).sum(0), flat.abs().double().sum(0)
    if o["kind"] == "int":
        assert float(S.max()) + 50 < INT_LIMIT and float(Sb.max()) + 50 < INT_LIMIT, (c.name, float(S.max()))
    k = (c.M + 2) * 2.0 ** -23
    return dict(dw=dw, dbias=dbias, S=S, Sb=Sb, B=k * S, Bb=k * Sb)


def stem_pool_reference(g_pool, idx, packed, dtype=F64, kind="int", bwd=None):
    """max-pool backward (rounded once to bf16, as the kernel builds its tiles) then the stem reference -> dict(dw [64, 4, 1, 64], S, B)."""
    bwd = IG.maxpool_bwd if bwd is None else bwd
    g_c1 = bwd(g_pool, idx, True)
    n = g_pool.shape[0]
    dw, S = _stem_dw(g_c1, packed, dtype), _stem_dw(g_c1.abs(), packed.abs(), F64)
    if kind == "int":
        assert float(g_c1.abs().max()) <= 8 and float(S.max()) + 50 < INT_LIMIT and float(S.max()) <= n * 12544 * 24
    return dict(dw=dw, S=S, B=(n * 12544 + 2) * 2.0 ** -23 * S)


# ---------------------------------------------------------------------------------------------------------------------------------
# plan_wgrad, restated
# ---------------------------------------------------------------------------------------------------------------------------------
def _env_int(env, key, default):
    v = env.get(key)
    return default if v is None else int(v)


def refusal(c: Case):
    """The field the library's plan refuses the case for (None: accepted), in the library's order."""
    if c.ci % 64 or c.ldg % 64:
        return "multiples of 64"
    if c.stride not in (1, 2):
        return "stride"
    if not 0 < c.M < 2 ** 24:
        return "output pixels"
    if c.ho * c.wo >= 65536:
        return "ho*wo"
    if c.ldg < c.co_pad:
        return "ldg"
    return None


def plan(c: Case, env=None):
    """-> dict(variant "stem" | "win" | "gen", tag, bt, tiles, splitk, kchunk, copies, copy_elems, bytes)."""
    env = os.environ if env is None else env
    assert refusal(c) is None, (c.name, refusal(c))
    bf = c.dtype == "bf16"
    M, taps, co_pad = c.M, c.r * c.s, c.co_pad
    copy_elems = co_pad * taps * c.ci
    ds64 = _env_int(env, "VDQN_WGRAD_DS64", 1)
    bt = 128 if (co_pad % 128 == 0 and c.ci % 128 == 0 and not (ds64 and taps == 1 and bf)) else 64
    tiles = (co_pad // bt) * taps * (c.ci // bt)
    max_split = (M + 255) // 256
    splitk = c.splitk
    if splitk <= 0:
        splitk = max(1, min(_env_int(env, "VDQN_WGRAD_BLOCKS", 512) // tiles, max_split))
    if _env_int(env, "VDQN_WGRAD_STEM", 1) and bf and c.is_stem and c.co == 64 and c.ldg == 64 and c.splitk <= 0:
        total_rows = c.n * 112
        grid = min(total_rows, 512)
        rpb = (total_rows + grid - 1) // grid
        copies = (total_rows + rpb - 1) // rpb
        return dict(variant="stem", tag="wgrad_stem<bf16>", bt=64, tiles=copies, splitk=1, kchunk=M, copies=copies, copy_elems=64 * 256,
                    bytes=copies * 64 * 256 * 4, rows_per_block=rpb)
    win_geom = (bf and c.r == 3 and c.s == 3 and c.stride == 1 and c.pad == 1 and c.pix_stride == c.ci and c.wo >= 2 and c.hi == c.ho
                and c.wi == c.wo and c.ho * c.wo <= CODE_TABLE_BYTES)
    variant, tag = "gen", f"wgrad<{KIND[c.dtype]},{bt}>"
    if _env_int(env, "VDQN_WGRAD_WINDOW", 1) and win_geom:
        variant, tag, bt = "win", "wgrad_win<bf16,64>", 64
        tiles = (co_pad // 64) * 3 * (c.ci // 64)
        splitk = c.splitk if c.splitk > 0 else _env_int(env, "VDQN_WGRAD_WIN_BLOCKS", 448) // tiles
        splitk = max(1, min(splitk, max_split))
    kchunk = ((M + splitk - 1) // splitk + 127) // 128 * 128
    copies = (M + kchunk - 1) // kchunk
    return dict(variant=variant, tag=tag, bt=bt, tiles=tiles, splitk=splitk, kchunk=kchunk, copies=copies, copy_elems=copy_elems,
                bytes=copies * copy_elems * 4)


def stem_pool_grid(n: int):
    """-> (pooled-row pairs per block, blocks per image, workspace bytes) of vdqn_stem_wgrad_pool."""
    bpi = min(max(512 // n, 1), 56)
    ppb = (56 + bpi - 1) // bpi
    bpi = (56 + ppb - 1) // ppb
    return ppb, bpi, n * bpi * 64 * 256 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# checks: each returns (number of offending elements, a figure for the message)
# ---------------------------------------------------------------------------------------------------------------------------------
def check_exact(got, expected):
    """Element-by-element equality (by value), nothing left out -> (number of differing elements, index of the first)."""
    got, expected = got.double(), expected.double()
    if got.shape != expected.shape:
        return max(got.numel(), expected.numel()), ("shape", tuple(got.shape), tuple(expected.shape))
    if torch.equal(got, expected):
        return 0, None
    bad = ~(got == expected)   # a NaN differs
    first = tuple(int(v) for v in bad.nonzero()[0])
    return int(bad.sum()), first


def check_bound(got, ref, B):
    """|got - ref| <= B on every element -> (number outside or not finite, largest error / B)."""
    got = got.double()
    err = (got - ref).abs()
    ratio = torch.where(B > 0, err / B.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return int((err > B).sum()) + int((~torch.isfinite(got)).sum()), float(ratio.max()) if ratio.numel() else 0.0


def check_padding_rows(dw_full, co):
    """Rows co .. co_pad - 1 of a dw that started as make_operands' dw0 still hold the sentinel -> number of elements that do not."""
    return int((dw_full[co:] != SENTINEL).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# fault injectors: what a wrong kernel would return.  Each takes the operands and gives a float64 dw / dbias / workspace figure.
# ---------------------------------------------------------------------------------------------------------------------------------
def window_emulation(c: Case, o, swap_ho_wo=False, dtype=F64):
    """dw [co, 3, 3, ci] the way wgrad_win_kernel addresses it: the x pixel of output pixel pm and tap (kr, ks) is pixel
    pm + (kr - 1) * wo + (ks - 1) of the flat tensor (images laid end to end), zero where the border code of pm's position puts the
    tap outside its image or the index leaves the tensor.  swap_ho_wo: the shift taken with ho for wo (the fault)."""
    assert c.r == c.s == 3 and c.stride == 1 and c.pad == 1 and c.hi == c.ho and c.wi == c.wo and c.pix_stride == c.ci
    M, howo = c.M, c.ho * c.wo
    x = o["x"].to(dtype).reshape(M, c.ci)
    gy = o["gy"].to(dtype).reshape(M, c.ldg)[:, :c.co]
    pm = torch.arange(M)
    rem = pm % howo
    oh, ow = rem // c.wo, rem % c.wo
    shift_w = c.ho if swap_ho_wo else c.wo
    dw = torch.zeros((c.co, 3, 3, c.ci), dtype=dtype)
    for kr in range(3):
        for ks in range(3):
            out = ((kr == 0) & (oh == 0)) | ((kr == 2) & (oh == c.ho - 1)) | ((ks == 0) & (ow == 0)) | ((ks == 2) & (ow == c.wo - 1))
            src = pm + (kr - 1) * shift_w + (ks - 1)
            ok = ~out & (src >= 0) & (src < M)
            xs = torch.where(ok[:, None], x[src.clamp(0, M - 1)], torch.zeros((), dtype=dtype))
            dw[:, kr, ks, :] = gy.t() @ xs
    return dw


def drop_border_column(c: Case, o, kr, ks, ow=None, dtype=F64):
    """dw with the terms of ONE output column (default: the last) missing from tap (kr, ks) -> (dw, mask of the touched elements)."""
    ow = c.wo - 1 if ow is None else ow
    dw = _dw(c, o["gy"], o["x"], dtype)
    iw = ow * c.stride - c.pad + ks
    part = torch.zeros((c.co, c.ci), dtype=dtype)
    for oh in range(c.ho):
        ih = oh * c.stride - c.pad + kr
        if 0 <= ih < c.hi and 0 <= iw < c.wi:
            part += o["gy"][:, oh, ow, :c.co].to(dtype).t() @ o["x"][:, ih, iw, :c.ci].to(dtype)
    dw[:, kr, ks, :] -= part
    touched = torch.zeros(dw.shape, dtype=torch.bool)
    touched[:, kr, ks, :] = True
    return dw, touched


def drop_split(c: Case, o, split, pl=None, dtype=F64):
    """dw without the pixels [split * kchunk, (split + 1) * kchunk) of the plan's split."""
    pl = plan(c, {}) if pl is None else pl
    k0, k1 = split * pl["kchunk"], min(c.M, (split + 1) * pl["kchunk"])
    assert k0 < k1, "the split has no pixels"
    gy = o["gy"].clone()
    gy.view(c.M, c.ldg)[k0:k1] = 0
    return _dw(c, gy, o["x"], dtype)


def write_padding_row(dw_full, c: Case):
    """A dw in which the kernel's `co < p.co` test is missing for one element of the first padding row."""
    assert c.co < c.co_pad
    out = dw_full.clone()
    out[c.co, 0, 0, 0] = 0.0
    return out


def add_twice(dw0, ref_dw, co):
    """dw0 + 2 ref in rows < co: a partial that reaches dw twice (or a chunk loop that does not accumulate but overwrites: dw0 lost)."""
    out = dw0.double().clone()
    out[:co] += 2 * ref_dw
    return out


def dbias_over_co(c: Case, o, dtype=F64):
    """dbias summed over the first co columns only (the padding columns' sums missing)."""
    db = torch.zeros(c.co_pad, dtype=dtype)
    db[:c.co] = o["gy"].reshape(c.M, c.ldg)[:, :c.co].to(dtype).sum(0)
    return db


def maxpool_bwd_lost_window(g_pool, idx, round_bf16=True):
    """input_grad_oracle.maxpool_bwd without the windows whose arg-max code is 0 (pooled row k + 1, window column j + 1: the fourth
    candidate of an odd pixel of an odd row)."""
    g = torch.where(idx == 0, torch.zeros_like(g_pool), g_pool)
    return IG.maxpool_bwd(g, idx, round_bf16)
