"""CPU oracle of one vdqn_conv2d call with an epilogue operand set (tests/test_conv_epilogue_cpu.py, tests/test_gpu_conv_epilogue.py).

Everything is NHWC, as the C ABI sees it.  A call (`Call`) is what the kernel is handed: `ci` input channels over hi x wi pixels, `co`
output channels over ho x wo, mode 0 (forward) or 1 (data gradient: the kernel's input is the gradient of a forward convolution's
output, its weights are [co][r][s][ci] = that convolution's weights with the channel roles swapped).

reference(): the float64 result `ref`, the per-element sum of absolute products `S` (+ |bias| + |resid|) and the accumulation bound
    B = K * 2^-23 * S,   K = r * s * ci (+ ci2 of a fused sibling).
Products of bf16 operands are exact in f32; K * 2^-24 * S bounds the error of an f32 sum of K terms in ANY order (each of the at
most K - 1 additions rounds a partial sum that is at most S in magnitude, relative error 2^-24; (1 + u)^K - 1 < 2 K u for K u < 0.1,
K <= 4608 here), the factor 2 covers the roundings inside an MFMA, the f32 operands' product roundings (one more 2^-24 S) and the
epilogue's two additions.  The bound is derived, not tuned: torch-CPU f32 against float64 sits below 1e-3 of it, one dropped tap at a
pixel is tens of times above it (test_conv_epilogue_cpu.py shows both).

Bounds per element: f32 copy and f32 stores |got - ref| <= B; a bf16 store |got - ref| <= 2^-8 (|ref| + B) + B (round to nearest:
half an ulp is at most 2^-8 of the rounded value's magnitude, which is within B of |ref|).  bf16x3 keeps the gate of
tests/test_gpu_bf16x3.py (x3_gate): dropping the lo * lo terms is not an f32-epsilon effect.

emulate(): the epilogue in torch-CPU float32 on an f32 accumulator: ((acc + bias) + resid), clamp_min(0), where(mask > 0, v, 0) —
additions and selects only, nothing a compiler could contract: bit-comparable with the device.

colsum_expected(): the float64 column sums of the stored values, entry by entry, for the entry layouts the kernels write."""
from dataclasses import dataclass, replace

import torch
import torch.nn.functional as F

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
STORE_DTYPE = {"bf16": BF16, "f32": F32, "x3": F32}
X3_ERR_MAX = 1e-4      # tests/test_gpu_bf16x3.py: ERR_MAX (of the output's max |value|)
X3_BF16_FACTOR = 20    # ... and BF16_FACTOR (times closer to float64 than one bf16 pass)
COLSUM_RELERR = 1e-5   # tests/test_gpu_skinny.py: column sums against the stored values


@dataclass(frozen=True)
class Call:
    name: str
    mode: int            # 0 forward, 1 data gradient
    dtype: str           # "bf16", "f32", "x3" (f32 tensors, split-bf16 MFMAs)
    n: int
    hi: int
    wi: int
    ci: int
    ho: int
    wo: int
    co: int
    r: int
    s: int
    stride: int
    pad: int
    sib: bool = False    # fused 1x1 / stride-2 sibling (forward: a second output of co channels; data gradient: a second input of ci)

    @property
    def M(self):
        return self.n * self.ho * self.wo

    @property
    def K(self):
        return self.r * self.s * self.ci + (self.ci if self.sib and self.mode == 1 else 0)

    @property
    def bn(self):  # the column tile vdqn_conv2d picks: the kernels read ceil(co / bn) * bn weight rows
        return 128 if self.co % 128 == 0 else 64

    @property
    def wt_rows(self):
        return (self.co + self.bn - 1) // self.bn * self.bn


def fwd(name, dtype, n, ho, wo, ci, co, k, stride, pad, hi=None, wi=None, sib=False):
    """A forward call by its OUTPUT size (input size: the smallest that gives it, unless given)."""
    hi = (ho - 1) * stride + k - 2 * pad if hi is None else hi
    wi = (wo - 1) * stride + k - 2 * pad if wi is None else wi
    assert (hi + 2 * pad - k) // stride + 1 == ho and (wi + 2 * pad - k) // stride + 1 == wo
    return Call(name, 0, dtype, n, hi, wi, ci, ho, wo, co, k, k, stride, pad, sib)


def dgrad(name, dtype, n, ho, wo, ci, co, k, stride, pad, sib=False):
    """A data-gradient call by its OUTPUT size (= the forward convolution's input size)."""
    hi, wi = (ho + 2 * pad - k) // stride + 1, (wo + 2 * pad - k) // stride + 1
    return Call(name, 1, dtype, n, hi, wi, ci, ho, wo, co, k, k, stride, pad, sib)


def _both(name, dtype, n, h, w, ci, co, k, stride, pad):
    return [fwd(name + "-fwd", dtype, n, h, w, ci, co, k, stride, pad), dgrad(name + "-dgrad", dtype, n, h, w, ci, co, k, stride, pad)]


# The family shapes: the smallest with a ragged last row tile, two row tiles and (where cheap) two column tiles.  Default 5 x 10 x 6
# output pixels (M = 300 = 2 x 128 + 44).  Which kernel takes which call: `route` in tests/test_gpu_conv_epilogue.py.
CALLS = (
    _both("conv64", "bf16", 5, 10, 6, 64, 64, 3, 1, 1)
    + _both("win64", "bf16", 5, 10, 6, 128, 64, 3, 1, 1)            # igemm_win<bf16,64>
    + _both("win3tap128", "bf16", 1, 5, 30, 64, 128, 3, 1, 1)       # igemm_win<bf16,128>: wo > 28 keeps the nine-tap kernels away
    + _both("win9", "bf16", 5, 10, 6, 64, 128, 3, 1, 1)             # igemm_win9: ci % 128 != 0 keeps win9u away
    + _both("win9u", "bf16", 5, 10, 6, 128, 256, 3, 1, 1)           # win9u, 128-row tiles (256-row: VDQN_WIN9_BM256=2)
    + [fwd("win9s-64", "bf16", 5, 6, 6, 64, 128, 3, 2, 1, hi=12, wi=12),
       fwd("win9s-192", "bf16", 5, 6, 6, 192, 128, 3, 2, 1, hi=12, wi=12),
       fwd("win9s-64-sib", "bf16", 5, 6, 6, 64, 128, 3, 2, 1, hi=12, wi=12, sib=True),
       fwd("win9s-192-sib", "bf16", 5, 6, 6, 192, 128, 3, 2, 1, hi=12, wi=12, sib=True),   # three chunks: no fused form, generic kernel
       dgrad("win9d", "bf16", 5, 12, 12, 128, 64, 3, 2, 1),
       dgrad("win9d-sib", "bf16", 5, 12, 12, 128, 64, 3, 2, 1, sib=True)]
    + _both("gen64-1x1", "bf16", 5, 10, 6, 128, 64, 1, 1, 0)        # igemm<bf16,64>, two-stage ring
    + _both("gen64-deep", "bf16", 5, 10, 6, 64, 192, 3, 1, 0)       # igemm<bf16,64>, nine K-steps: the deep ring (forward)
    + _both("gen128", "bf16", 5, 10, 6, 64, 128, 3, 1, 0)           # igemm<bf16,128>
    + [dgrad("gen-s2-3x3", "bf16", 5, 7, 7, 128, 64, 3, 2, 1),      # unequal parity classes (4x4, 4x3, 3x4, 3x3 pixels)
       dgrad("gen-s2-1x1", "bf16", 5, 7, 7, 128, 64, 1, 2, 0)]
    + _both("skinny-linear", "bf16", 37, 1, 1, 256, 64, 1, 1, 0)
    + [fwd("f8-lds", "bf16", 3, 5, 5, 512, 64, 3, 1, 0),             # pixels of whole 1 KB pieces (2 ci % 1024 == 0): f8_lds_kernel
       fwd("f8-global", "bf16", 3, 5, 5, 256, 64, 3, 1, 0)]          # 512-byte pixels: skinny_kernel reading global memory
    + _both("f32-win64", "f32", 5, 10, 6, 64, 64, 3, 1, 1) + _both("x3-win64", "x3", 5, 10, 6, 64, 64, 3, 1, 1)
    + _both("f32-win128", "f32", 5, 10, 6, 64, 128, 3, 1, 1) + _both("x3-win128", "x3", 5, 10, 6, 64, 128, 3, 1, 1)
    + _both("f32-gen-1x1", "f32", 5, 10, 6, 64, 64, 1, 1, 0) + _both("x3-gen-1x1", "x3", 5, 10, 6, 64, 64, 1, 1, 0)
)
CALL_BY_NAME = {c.name: c for c in CALLS}
assert len(CALL_BY_NAME) == len(CALLS) and all(c.M <= 720 and c.K <= 4608 for c in CALLS)


def with_co(c: Call, co: int) -> Call:
    return replace(c, co=co, name=f"{c.name}-co{co}")


def make_operands(c: Call, seed: int = 1):
    """Operands of `c`, CPU f32 tensors holding values of the call's dtype (bf16: rounded; f32 / x3: as drawn).  wt has c.wt_rows rows,
    those from co on zero.  mask: about half the elements <= 0, exact zeros and -0 among them."""
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, c.name)))
    rt = (lambda t: t.to(BF16).float()) if c.dtype == "bf16" else (lambda t: t)

    def u(shape, lo, hi):
        return rt(torch.rand(shape, generator=g) * (hi - lo) + lo)

    o = {"x": u((c.n, c.hi, c.wi, c.ci), -1, 1), "wt": torch.zeros((c.wt_rows, c.r, c.s, c.ci)), "bias": torch.zeros(c.wt_rows)}
    o["wt"][:c.co] = u((c.co, c.r, c.s, c.ci), -0.1, 0.1)
    o["bias"][:c.co] = torch.rand((c.co,), generator=g) * 2 - 1   # f32 for every dtype
    o["resid"] = u((c.n, c.ho, c.wo, c.co), -1, 1)
    m = u((c.n, c.ho, c.wo, c.co), -1, 1)
    m.view(-1)[::7] = 0.0
    m.view(-1)[3::11] = -0.0
    o["mask"] = m
    if c.sib and c.mode == 0:
        o["wt2"] = u((c.co, 1, 1, c.ci), -0.2, 0.2)
        o["bias2"] = torch.rand((c.co,), generator=g) * 2 - 1
    elif c.sib:
        o["x2"] = u((c.n, c.hi, c.wi, c.ci), -1, 1)
        o["wt2"] = u((c.co, 1, 1, c.ci), -0.2, 0.2)
    return o


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def conv(c: Call, x, wt, dtype=F64, r=None, stride=None, pad=None):
    """The bare convolution of the call in `dtype` arithmetic: NHWC [n, ho, wo, co]."""
    r = c.r if r is None else r
    stride, pad = c.stride if stride is None else stride, c.pad if pad is None else pad
    x, wt = x.to(dtype), wt[:c.co].to(dtype)
    if c.mode == 0:
        y = F.conv2d(_nchw(x), _nchw(wt), None, stride, pad)
    else:  # wt [co][r][s][ci] -> the forward convolution's [ci][co][r][s]
        y = F.grad.conv2d_input((c.n, c.co, c.ho, c.wo), wt.permute(3, 0, 1, 2), _nchw(x), stride, pad)
    assert tuple(y.shape) == (c.n, c.co, c.ho, c.wo), (c, tuple(y.shape))
    return y.permute(0, 2, 3, 1).contiguous()


def accumulate(c: Call, o, dtype=F64, absolute=False):
    """The accumulator of the call (the fused data-gradient sibling included) in `dtype`; absolute: of |operands| (the sum S of the
    absolute products)."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    acc = conv(c, f(o["x"]), f(o["wt"]), dtype)
    if c.sib and c.mode == 1:
        acc = acc + conv(c, f(o["x2"]), f(o["wt2"]), dtype, r=1, stride=2, pad=0)
    return acc


def sibling_forward(c: Call, o, dtype=F64, absolute=False):
    """out2 of a forward call with a sibling: conv1x1 / stride 2 (+ bias2 when `bias2`), no ReLU here."""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    c1 = replace(c, r=1, s=1, pad=0)
    return conv(c1, f(o["x"]), f(o["wt2"]), dtype)


def epilogue64(acc, S, K, *, bias=None, resid=None, relu=False, mask=None):
    """float64 epilogue in the library's order on (acc, S) -> (ref, S, B)."""
    v, S = acc.double(), S.double()
    if bias is not None:
        v, S = v + bias.double(), S + bias.double().abs()
    if resid is not None:
        v, S = v + resid.double(), S + resid.double().abs()
    if relu:
        v = v.clamp_min(0)
    if mask is not None:
        v = torch.where(mask > 0, v, torch.zeros_like(v))
    return v, S, K * 2.0 ** -23 * S


def reference(c: Call, o, *, bias=False, resid=False, relu=False, mask=False, pair=None):
    """(ref, S, B) of the call with the flagged operands of `o`.  pair: (acc64, S64) of accumulate() computed before (it does not
    depend on the flags)."""
    acc, S = pair if pair is not None else (accumulate(c, o), accumulate(c, o, absolute=True))
    return epilogue64(acc, S, c.K, bias=o["bias"][:c.co] if bias else None, resid=o["resid"] if resid else None, relu=relu,
                      mask=o["mask"] if mask else None)


def emulate(acc_f32, *, bias=None, resid=None, relu=False, mask=None):
    """The epilogue in f32 on an f32 accumulator (CPU tensors; resid / mask hold values of the storage dtype) -> the f32 copy."""
    assert acc_f32.dtype == F32
    v = acc_f32
    if bias is not None:
        v = v + bias.float()
    if resid is not None:
        v = v + resid.float()
    if relu:
        v = v.clamp_min(0)
    if mask is not None:
        v = torch.where(mask.float() > 0, v, torch.zeros_like(v))
    return v


# ---- the checks: each returns (number of violating elements, largest error / bound) ----
def _ratio(err, bound):
    bad = err > bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0


def check_f32(got, ref, B):
    """An f32 result (the f32 copy; the store of an f32 kernel): |got - ref| <= B, every element."""
    got = got.double()
    bad_nan = int((~torch.isfinite(got)).sum())
    n, ratio = _ratio((got - ref).abs(), B)
    return n + bad_nan, ratio


def check_bf16(got, ref, B):
    """A bf16 store: |got - ref| <= 2^-8 (|ref| + B) + B, every element."""
    got = got.double()
    bad_nan = int((~torch.isfinite(got)).sum())
    n, ratio = _ratio((got - ref).abs(), 2.0 ** -8 * (ref.abs() + B) + B)
    return n + bad_nan, ratio


def x3_gate(got, ref64, ref_bf16):
    """tests/test_gpu_bf16x3.py's gate: (error / max|ref|, the same of one bf16 pass, passed)."""
    scale = max(ref64.abs().max().item(), 1e-300)
    e3 = (got.double() - ref64).abs().max().item() / scale
    e1 = (ref_bf16 - ref64).abs().max().item() / scale
    return e3, e1, bool(e3 <= X3_ERR_MAX and e3 * X3_BF16_FACTOR <= e1)


def store_is_rounded(out, out_f32):
    """E1: the store is the f32 copy rounded to the storage dtype (round to nearest even), compared by value (-0 == +0)."""
    return torch.equal(out.float(), out_f32.to(out.dtype).float())


# ---- column sums ----
def colsum_rows(c: Call, rows: int, order: str):
    """The flat output-pixel indices of every column-sum entry: a list of int64 tensors.
    order "rows": entry e = pixels [e * rows, (e + 1) * rows).  The stride-2 data gradient walks the four output-parity classes
    (ph, pw), class c = 2 ph + pw, each class's pixels (image, row, column) in tiles of `rows`: "class" — the tiles of class 0, then
    1, 2, 3 (ops.conv2d's count); "interleave" — tile t of class k at entry 4 t + k (all classes equally long); "win9d" — the
    plane-window kernel: tile t of class k at entry 4 t + (3 - k)."""
    M = c.M
    if order == "rows":
        return [torch.arange(e, min(e + rows, M)) for e in range(0, M, rows)]
    assert c.mode == 1 and c.stride == 2
    per_class = []
    for k in range(4):
        ph, pw = k >> 1, k & 1
        hc, wc = (c.ho + 1 - ph) // 2, (c.wo + 1 - pw) // 2
        img, oh, ow = torch.meshgrid(torch.arange(c.n), torch.arange(hc), torch.arange(wc), indexing="ij")
        pix = ((img * c.ho + 2 * oh + ph) * c.wo + 2 * ow + pw).reshape(-1)
        per_class.append([pix[e:e + rows] for e in range(0, pix.numel(), rows)])
    if order == "class":
        return [t for k in range(4) for t in per_class[k]]
    nt = len(per_class[0])
    assert all(len(p) == nt for p in per_class), "interleaved orders need equally long classes"
    if order == "interleave":
        return [per_class[k][t] for t in range(nt) for k in range(4)]
    if order == "win9d":
        return [per_class[3 - ph][t] for t in range(nt) for ph in range(4)]
    raise ValueError(order)


def colsum_expected(stored, c: Call, rows: int = 128, order: str = "rows", pair: bool = False):
    """float64 [entries, co]: the sum of the stored values of each entry's pixels.  pair (256-row tiles on the shared epilogue,
    igemm_common.h: 'consumers sum ceil(M / 128) entries'): entry 2 t holds the whole 256-row tile, entry 2 t + 1 zero."""
    flat = stored.double().reshape(c.M, -1)
    exp = torch.stack([flat[idx].sum(0) for idx in colsum_rows(c, rows, order)])
    if pair:
        assert order == "rows" and rows == 128
        for e in range(0, exp.shape[0] - 1, 2):
            exp[e] += exp[e + 1]
            exp[e + 1] = 0
    return exp


def check_colsum(part, expected):
    """Every entry within COLSUM_RELERR (of the entry's largest column sum) of `expected` -> list of offending entries."""
    bad = []
    if part.shape[0] != expected.shape[0]:
        return [("entries", part.shape[0], expected.shape[0])]
    for e in range(expected.shape[0]):
        err = (part[e].double() - expected[e]).abs().max().item()
        scale = expected[e].abs().max().item()
        if not (err < COLSUM_RELERR * scale) and not (scale == 0.0 and err == 0.0):
            bad.append((e, err / max(scale, 1e-300)))
    return bad
