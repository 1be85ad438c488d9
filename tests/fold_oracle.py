"""An independent statement of what csrc/fold.hip writes and reads.  TEST INFRASTRUCTURE ONLY (imported by tests/ alone).

Three things live here, all numpy, none of them needs a GPU:

  * the packed layouts, written as tensor permutations of the reference's OIHW / [out][in] weights (`arrange_wf`, `arrange_wd`) and
    their inverse for the f32 gradient accumulators (`unarrange_dw`); the BatchNorm-eval scale and bias in float64
    (`scale_bias64`), the float64 dL/dgamma (`dgamma64`) and an integer round-to-nearest-even f32 -> bf16 (`bf16_bits`);
  * the layer list of HabitatDQNMultiAction over the torchvision ResNet-18 topology (`layers`) and the master tensors of a layer
    out of a state dict (`master`);
  * the comparisons tests/test_gpu_fold.py makes between what a kernel stored and those statements (`check_fold_layer`,
    `check_poison`, `check_unfold_layer`, `check_dq_pad`), collecting what they find in a `Report` that names layer, region and
    first element.  tests/test_fold_cpu.py runs the same functions on corrupted copies of the oracle's own output.

The error bounds are derived in the docstrings of the functions that apply them."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

BN_EPS = 1e-5
POISON = 0xFF  # the byte the packed buffer is filled with before a fold
SCALE_ULPS = 4.0

# f32 bit patterns on the edges of the f32 -> bf16 rounding
EDGE_BITS = [
    0x3F808000, 0x3F818000,              # ties: to even downwards (..80|8000 -> 3F80), to even upwards (..81|8000 -> 3F82)
    0xBF808000, 0xBF818000,              # the same, negative
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # next to the ties
    0x00000001, 0x00008000, 0x00018000, 0x00007FFF, 0x007FFFFF, 0x807FFFFF, 0x00010000,  # denormals (a tie, below and above one)
    0x00000000, 0x80000000,              # +0, -0
    0x7F7FFFFF, 0xFF7FFFFF,              # the largest finite f32: rounds to infinity
    0x7F7F7FFF, 0x7F7F8000, 0x7F7F8001, 0x7F7E8000,  # around the largest finite bf16 (7F7F): below its upper tie, the tie (-> inf), above, a tie to even
    0x3FFF8000, 0x3FFFFFFF,              # the carry runs from the mantissa into the exponent
]

# kind: "conv" (3x3 / 1x1), "conv1" (the 7x7/2 stem as a space-to-depth operand), "linear_perm" (top.0), "linear"
Spec = namedtuple("Spec", "name kind co ci r s stride pad bn co_pad kf wd_rows kd")


def _spec(name, kind, co, ci, r, s, stride, pad, bn):
    co_pad = (co + 63) // 64 * 64
    if kind == "conv1":
        return Spec(name, kind, co, ci, r, s, stride, pad, bn, co_pad, 4 * 4 * 16, 0, 0)  # no data-gradient operand
    return Spec(name, kind, co, ci, r, s, stride, pad, bn, co_pad, r * s * ci, ci, r * s * co_pad)


def head_rows(head, action_dim=3, num_classes=5):
    return {None: 0, "value": num_classes, "spread": action_dim * num_classes, "policy": action_dim}[head]


def layers(extra_capacity=True, num_frames=1, action_dim=3, num_classes=5, head=None):
    """The layers that own packed operands, in forward order."""
    out = [_spec("resnet.conv1", "conv1", 64, 3, 7, 7, 2, 3, "resnet.bn1")]
    inpl = 64
    for li in range(1, 5):
        planes = 64 << (li - 1)
        for bi in range(2):
            stride = 2 if (li > 1 and bi == 0) else 1
            p = f"resnet.layer{li}.{bi}"
            out.append(_spec(p + ".conv1", "conv", planes, inpl, 3, 3, stride, 1, p + ".bn1"))
            out.append(_spec(p + ".conv2", "conv", planes, planes, 3, 3, 1, 1, p + ".bn2"))
            if stride != 1 or inpl != planes:
                out.append(_spec(p + ".downsample.0", "conv", planes, inpl, 1, 1, stride, 0, p + ".downsample.1"))
            inpl = planes
    nq = action_dim * num_classes + head_rows(head, action_dim, num_classes)
    if extra_capacity:
        out.append(_spec("features.8", "conv", 64, 512, 3, 3, 1, 0, None))
        out.append(_spec("top.0", "linear_perm", 512, 1600 * num_frames, 1, 1, 1, 0, None))
        out.append(_spec("top.2", "linear", 256, 512, 1, 1, 1, 0, None))
        out.append(_spec("top.4", "linear", nq, 256, 1, 1, 1, 0, None))
    else:
        out.append(_spec("top", "linear", nq, 512 * num_frames, 1, 1, 1, 0, None))
    return out


def master(spec, sd, head=None, head_weight=None, head_bias=None):
    """The f32 master tensors of one layer out of a state dict: W (OIHW or [out][in]; the Q layer with the head's rows directly
    behind its own), and gamma / beta / mean / var of its BatchNorm or its own bias."""
    f32 = lambda t: np.ascontiguousarray(np.asarray(t, dtype=np.float32))  # noqa: E731
    m = {"W": f32(sd[spec.name + ".weight"]), "bias": None, "gamma": None}
    if spec.bn is not None:
        m.update(gamma=f32(sd[spec.bn + ".weight"]), beta=f32(sd[spec.bn + ".bias"]), mean=f32(sd[spec.bn + ".running_mean"]),
                 var=f32(sd[spec.bn + ".running_var"]))
    else:
        m["bias"] = f32(sd[spec.name + ".bias"])
    if head is not None and spec.name in ("top.4", "top"):
        m["W"] = np.concatenate([m["W"], f32(head_weight)], 0)
        m["bias"] = np.concatenate([m["bias"], f32(head_bias)], 0)
    assert m["W"].shape[0] == spec.co, (spec.name, m["W"].shape)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------------------------
def _pad_rows(a, rows):
    out = np.zeros((rows,) + a.shape[1:], dtype=a.dtype)
    out[:a.shape[0]] = a
    return out


def arrange_wf(spec, W):
    """The forward operand [co_pad][kf] of (already scaled) weights W; pad rows and pad columns are +0."""
    co = spec.co
    if spec.kind == "conv":  # [co][ci][r][s] -> [co][r][s][ci]
        a = W.transpose(0, 2, 3, 1).reshape(co, spec.kf)
    elif spec.kind == "conv1":
        # The 7x7 window with one zero row on top and one zero column on the left is an 8x8 window = 4x4 blocks of 2x2 pixels:
        # row 2a + bh, column 2j + bw of it is tap (r7, s7) = (2a + bh - 1, 2j + bw - 1).  A block's 12 values in (bh, bw, c) order,
        # then 4 zero channels.
        w8 = np.zeros((co, 3, 8, 8), dtype=W.dtype)
        w8[:, :, 1:, 1:] = W
        blocks = w8.reshape(co, 3, 4, 2, 4, 2).transpose(0, 2, 4, 3, 5, 1).reshape(co, 4, 4, 12)  # [co][a][j][(bh, bw, c)]
        a = np.zeros((co, 4, 4, 16), dtype=W.dtype)
        a[..., :12] = blocks
        a = a.reshape(co, spec.kf)
    elif spec.kind == "linear_perm":  # in-features [F][64 channels][25 pixels] -> [F][25][64]
        a = W.reshape(co, spec.ci // 1600, 64, 25).transpose(0, 1, 3, 2).reshape(co, spec.kf)
    else:
        a = W.reshape(co, spec.kf)
    return _pad_rows(np.ascontiguousarray(a), spec.co_pad)


def arrange_wd(spec, W):
    """The data-gradient operand [wd_rows][kd]: [ci][r][s][co_pad] of a convolution, the padded transpose of Wf of a Linear."""
    assert spec.kind != "conv1", "resnet.conv1 has no data-gradient operand"
    if spec.kind == "conv":
        a = np.zeros((spec.ci, spec.r, spec.s, spec.co_pad), dtype=W.dtype)
        a[..., :spec.co] = W.transpose(1, 2, 3, 0)
        return a.reshape(spec.wd_rows, spec.kd)
    return np.ascontiguousarray(arrange_wf(spec, W).T)  # (the pad rows of Wf are the pad columns here)


def unarrange_dw(spec, dwp):
    """The inverse permutation for the f32 accumulators dW' [co_pad][kf] -> the shape of the master weights."""
    co = spec.co
    d = np.asarray(dwp).reshape(spec.co_pad, spec.kf)[:co]
    if spec.kind == "conv":
        return np.ascontiguousarray(d.reshape(co, spec.r, spec.s, spec.ci).transpose(0, 3, 1, 2))
    if spec.kind == "conv1":
        b = d.reshape(co, 4, 4, 16)[..., :12].reshape(co, 4, 4, 2, 2, 3)  # [co][a][j][bh][bw][c]
        w8 = b.transpose(0, 5, 1, 3, 2, 4).reshape(co, 3, 8, 8)
        return np.ascontiguousarray(w8[:, :, 1:, 1:])
    if spec.kind == "linear_perm":
        return np.ascontiguousarray(d.reshape(co, spec.ci // 1600, 25, 64).transpose(0, 1, 3, 2).reshape(co, spec.ci))
    return np.ascontiguousarray(d.reshape(co, spec.ci))


def _per_channel(spec, v):
    return v.reshape((spec.co,) + (1,) * (3 if spec.kind in ("conv", "conv1") else 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# scale, bias, dgamma in float64; bf16 rounding in integers
# ---------------------------------------------------------------------------------------------------------------------------------
def scale_bias64(spec, m, raw=False):
    """(scale, bias) float64 [co_pad]: gamma / sqrt(var + 1e-5) and beta - mean * scale under a folded BatchNorm, 1 and the layer's
    own bias without one, 1 and 0 under `raw`; rows co..co_pad-1 hold 0 and 0."""
    scale, bias = np.zeros(spec.co_pad), np.zeros(spec.co_pad)
    if spec.bn is not None and not raw:
        s = m["gamma"].astype(np.float64) / np.sqrt(m["var"].astype(np.float64) + BN_EPS)
        scale[:spec.co] = s
        bias[:spec.co] = m["beta"].astype(np.float64) - m["mean"].astype(np.float64) * s
    else:
        scale[:spec.co] = 1.0
        if spec.bn is None:
            bias[:spec.co] = m["bias"].astype(np.float64)
    return scale, bias


def dgamma64(spec, m, dw, dbeta):
    """float64 (dgamma [co], sum|dW'_i W_i| [co], rstd [co]) from the un-permuted f32 accumulators `dw` (shape of W) and the f32
    dbeta:  dgamma = rstd * (<dW'[co, :], W[co, :]> - mean * dbeta)."""
    prod = (dw.astype(np.float64) * m["W"].astype(np.float64)).reshape(spec.co, -1)
    rstd = 1.0 / np.sqrt(m["var"].astype(np.float64) + BN_EPS)
    return rstd * (prod.sum(1) - m["mean"].astype(np.float64) * dbeta.astype(np.float64)), np.abs(prod).sum(1), rstd


def bf16_bits(x):
    """Round-to-nearest-even f32 -> bf16 on the bit patterns (uint16): add 0x7FFF plus the bit that becomes the last kept one, keep
    the high half.  A carry out of the mantissa moves into the exponent, which is what rounding up to the next binade (and, from the
    largest finite values, to infinity) is.  NaN becomes the quiet NaN of its sign."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((u >> 16) | 0x7FC0).astype(np.uint16), r)


def bf16_round(x):
    return (bf16_bits(x).astype(np.uint32) << 16).view(np.float32)


def stored_bits(x, dtype):
    """The bit patterns a kernel stores for the f32 values x: uint16 of round-to-nearest-even bf16, or the uint32 of the f32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return bf16_bits(x) if dtype == "bf16" else x.view(np.uint32)


def _round_exact_f32(fr, near):
    """The f32 nearest the rational `fr` (ties to even), given an f32 `near` at most one step away from it."""
    near = np.float32(near)
    cands = [near, np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))]
    dist = [abs(Fraction(float(c)) - fr) for c in cands]
    best = min(dist)
    win = [c for c, d in zip(cands, dist) if d == best]
    if len(win) > 1:
        win = [c for c in win if (int(np.float32(c).view(np.uint32)) & 1) == 0]
    return win[0]


def fused_f32(beta, mean, sc):
    """fl32(beta - mean * sc) with the product NOT rounded (what a fused multiply-add returns), exactly.  The f32 product is exact
    in float64 (48 bits); the float64 difference is rounded once more, which matters only where it lands next to the midpoint of
    two f32 values — those elements are decided in rational arithmetic."""
    p = mean.astype(np.float64) * sc.astype(np.float64)
    d = beta.astype(np.float64) - p
    out = d.astype(np.float32)
    unsure = np.nextafter(d, -np.inf).astype(np.float32) != np.nextafter(d, np.inf).astype(np.float32)
    for i in np.flatnonzero(unsure):
        fr = Fraction(float(beta[i])) - Fraction(float(mean[i])) * Fraction(float(sc[i]))
        out[i] = _round_exact_f32(fr, out[i])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------------
class Report:
    """Findings of the checks below, one line each: layer, region, how many elements, the first one with both values."""

    def __init__(self):
        self.lines = []

    def add(self, layer, region, text):
        self.lines.append(f"{layer} {region}: {text}")

    def bits(self, layer, region, got, want, what="", poison=None):
        """`got` and `want` are unsigned bit patterns of one shape; a difference is reported with its first index."""
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            self.add(layer, region, f"shape {got.shape}, expected {want.shape}")
            return False
        bad = got != want
        if not bad.any():
            return True
        first = tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape))
        w = got.dtype.itemsize * 2
        extra = ""
        if poison is not None and int(got[first]) == poison:
            extra = " (still the poison value)"
        self.add(layer, region, f"{int(bad.sum())} of {bad.size} elements differ{' ' + what if what else ''}, first at {list(first)}: "
                                f"got 0x{int(got[first]):0{w}x}{extra}, expected 0x{int(want[first]):0{w}x}")
        return False

    def bound(self, layer, region, err, bound, what):
        bad = ~(err <= bound)
        if not bad.any():
            return True
        first = tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), bad.shape))
        self.add(layer, region, f"{int(bad.sum())} of {bad.size} elements outside {what}, first at {list(first)}: error {err[first]:.4e}, "
                                f"bound {bound[first]:.4e}")
        return False

    def __bool__(self):
        return bool(self.lines)

    def text(self):
        return "\n".join(self.lines)

    def assert_clean(self, what=""):
        assert not self.lines, f"{what}: {len(self.lines)} finding(s)\n" + self.text()


def _poison_pattern(itemsize):
    return int.from_bytes(bytes([POISON]) * itemsize, "little")


def check_fold_layer(rep, spec, m, got, dtype, raw=False, with_dgrad=True):
    """One layer of a fold against the oracle.  `got`: {"scale", "bias": f32 [co_pad]; "wf": [co_pad][kf], "wd": [wd_rows][kd] (absent
    for resnet.conv1), both as stored (uint16 bit patterns for bf16, f32 or uint32 for f32)}.  Returns {"scale_ulps": the largest
    scale error in f32 ulps, "bias": "fused" | "product first" | "either" (both roundings agree on every channel) | "exact" (no
    arithmetic: the layer's own bias, or 0)}.

    Scale.  The kernel evaluates gamma / sqrtf(var + 1e-5f) in f32, with u = 2^-24:  a = fl(var + eps) = (var + eps)(1 + d1),
    |d1| <= u;  b = sqrtf(a) is within one ulp of sqrt(a) (HIP's documented bound for sqrtf; a correctly rounded one is within half),
    so b = sqrt(a)(1 + d2), |d2| <= 2u;  the quotient is correctly rounded, (1 + d3), |d3| <= u.  Together
    gamma / sqrt(var + eps) * (1 + d3) / ((1 + d1)^(1/2) (1 + d2)): a relative error of at most u/2 + 2u + u = 3.5u to first order
    (the second-order terms and the 1e-5f constant, 2.5e-13 away from 1e-5 against var + eps >= 1e-5, are below 0.01u).  One ulp of
    the result is more than u times its magnitude, so the error is below 3.5 ulps + that remainder: SCALE_ULPS = 4 ulps of the
    float64 value's f32 neighbour, no relative tolerance on top.  Layers without a folded BatchNorm hold exactly 1.0f, pad rows +0.

    Weights.  fl(w * s) is one multiplication with one rounding, and there is nothing to contract it with: Wf and Wd must equal
    round_T(w * s) bit for bit, where s is the scale the kernel itself stored for that row (so the scale's own error does not enter),
    the product is numpy's f32 product and the arrangement is `arrange_wf` / `arrange_wd`.  Pad elements are +0.

    Bias.  beta - mean * s may be contracted to a fused multiply-add by the compiler.  Both results are computed exactly; every
    channel must equal one of them bit for bit, and all channels of the layer the same one."""
    co, name = spec.co, spec.name
    out = {"scale_ulps": 0.0, "bias": "exact"}
    scale = np.ascontiguousarray(got["scale"], dtype=np.float32)
    bias = np.ascontiguousarray(got["bias"], dtype=np.float32)
    folded = spec.bn is not None and not raw
    s64, b64 = scale_bias64(spec, m, raw)
    ok_scale = True
    if folded:
        ulp = np.spacing(np.abs(s64[:co]).astype(np.float32)).astype(np.float64)
        err = np.abs(scale[:co].astype(np.float64) - s64[:co])
        out["scale_ulps"] = float((err / ulp).max())
        ok_scale = rep.bound(name, "scale", err, SCALE_ULPS * ulp, f"{SCALE_ULPS:g} f32 ulps of gamma / sqrt(var + eps)")
    else:
        ok_scale = rep.bits(name, "scale", scale[:co].view(np.uint32), np.ones(co, np.float32).view(np.uint32), "from 1.0f")
    rep.bits(name, "scale", scale[co:].view(np.uint32), np.zeros(spec.co_pad - co, np.uint32), "from +0 in the pad rows")
    if not np.isfinite(scale).all() or not ok_scale:
        # the weights are checked against the scale read back; with that one off its bound they would only repeat the finding
        scale = np.where(np.isfinite(scale), scale, 0).astype(np.float32)
    # weights
    ws = m["W"] * _per_channel(spec, scale[:co])  # numpy f32 product, one rounding
    assert ws.dtype == np.float32
    pz = _poison_pattern(2 if dtype == "bf16" else 4)
    as_bits = lambda a: np.asarray(a) if np.asarray(a).dtype.kind == "u" else np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)  # noqa: E731
    rep.bits(name, "wf", as_bits(got["wf"]).reshape(spec.co_pad, spec.kf), stored_bits(arrange_wf(spec, ws), dtype), poison=pz)
    if spec.kind != "conv1":
        wd = as_bits(got["wd"]).reshape(spec.wd_rows, spec.kd)
        if with_dgrad:
            rep.bits(name, "wd", wd, stored_bits(arrange_wd(spec, ws), dtype), poison=pz)
        else:
            rep.bits(name, "wd", wd, np.full(wd.shape, pz, wd.dtype), "from the poison value (with_dgrad = 0 must not write Wd)")
    # bias
    if folded:
        fused = fused_f32(m["beta"], m["mean"], scale[:co])
        first = (m["beta"] - (m["mean"] * scale[:co]).astype(np.float32)).astype(np.float32)
        gb, fb, pb = bias[:co].view(np.uint32), fused.view(np.uint32), first.view(np.uint32)
        if (gb == fb).all() and (gb == pb).all():
            out["bias"] = "either"
        elif (gb == fb).all():
            out["bias"] = "fused"
        elif (gb == pb).all():
            out["bias"] = "product first"
        else:
            out["bias"] = "neither"
            neither = (gb != fb) & (gb != pb)
            if neither.any():
                i = int(np.argmax(neither))
                rep.add(name, "bias", f"{int(neither.sum())} of {co} elements are neither rounding of beta - mean * scale, first at [{i}]: got "
                                      f"0x{int(gb[i]):08x}, fused 0x{int(fb[i]):08x}, product first 0x{int(pb[i]):08x}")
            else:
                rep.add(name, "bias", f"the channels mix the two roundings of beta - mean * scale ({int((gb == fb).sum())} fused, "
                                      f"{int((gb == pb).sum())} product first of {co})")
    else:
        want = np.zeros(co, np.float32) if spec.bn is not None else m["bias"]
        rep.bits(name, "bias", bias[:co].view(np.uint32), want.view(np.uint32))
    rep.bits(name, "bias", bias[co:].view(np.uint32), np.zeros(spec.co_pad - co, np.uint32), "from +0 in the pad rows")
    return out


def region_bytes(spec, esz):
    """{region: bytes} of one layer's regions inside the packed buffer."""
    out = {"wf": spec.co_pad * spec.kf * esz, "bias": spec.co_pad * 4, "scale": spec.co_pad * 4}
    if spec.kind != "conv1":
        out["wd"] = spec.wd_rows * spec.kd * esz
    return out


def check_poison(rep, buf, regions, with_dgrad):
    """`buf`: the packed buffer as uint8, filled with POISON before the fold; `regions`: [(layer, region, offset, bytes)].  Every byte
    outside the regions (the alignment gaps), and every byte of a Wd region when with_dgrad = 0, must still be POISON.  (An element
    of a written region that is still the poison pattern, an all-ones NaN, differs from its expected bits in check_fold_layer.)"""
    written = np.zeros(buf.size, dtype=bool)
    for layer, region, off, n in regions:
        if off < 0 or off + n > buf.size or written[off:off + n].any():
            rep.add(layer, region, f"offset {off} + {n} bytes is outside the buffer of {buf.size} bytes or overlaps another region")
            continue
        written[off:off + n] = True
        if region == "wd" and not with_dgrad:
            bad = buf[off:off + n] != POISON
            if bad.any():
                rep.add(layer, region, f"{int(bad.sum())} bytes written although with_dgrad = 0, first at byte {int(np.argmax(bad))} of the region")
    gap = ~written
    touched = gap & (buf != POISON)
    if touched.any():
        at = int(np.argmax(touched))
        before = [(layer, region) for layer, region, off, n in regions if off + n <= at]
        rep.add(before[-1][0] if before else "?", "gap", f"{int(touched.sum())} bytes outside every region were written, first at byte {at} "
                                                         f"(behind {before[-1][1] if before else 'nothing'})")


def check_unfold_layer(rep, spec, m, dwp, g_w, g_gamma=None, dbeta=None, raw=False):
    """One layer of the gradient unfold.  dwp: the f32 accumulators dW' [co_pad][kf]; g_w: the f32 weight gradient the kernel wrote
    (shape of W); g_gamma, dbeta: its dL/dgamma and dL/dbeta [co] under a folded BatchNorm.  Returns the largest err / bound of
    dgamma (0 without a folded BatchNorm).

    dL/dW.  Without a folded BatchNorm the kernel multiplies by 1.0f: the gradient equals the un-permuted dW' bit for bit.  With
    one, every element of output channel c is fl(dW'_i * s_c), one rounding, with ONE f32 s_c for the whole channel; the kernel
    computes s_c = fl(gamma * fl(1 / sqrtf(fl(var + eps)))), where sqrtf and the reciprocal are within an ulp of numpy's (correctly
    rounded) ones, so s_c is numpy's f32 value or one of its two neighbours.  The check asks for one of these three under which ALL
    elements of the channel match bit for bit.

    dL/dgamma = rstd * (dot - mean * dbeta), dot = sum_i dW'_i W_i over the kf elements of the channel's packed row (zeros of the
    space-to-depth operand add nothing).  The products are rounded (or fused into the running sum, which is no worse) and summed in
    some order in f32: |fl(dot) - dot| <= gamma_kf * sum|dW'_i W_i| for any order (Higham, Accuracy and Stability, section 3.1).
    Three more f32 operations follow: the product mean * dbeta, the difference, the product with rstd; each adds a factor (1 + d),
    |d| <= u = 2^-24, to a quantity bounded by sum|dW'_i W_i| + |mean * dbeta|.  So

        |dgamma - dgamma64| <= rstd * 1.01 * (kf + 3) * 2^-24 * (sum|dW'_i W_i| + |mean * dbeta|) + one f32 ulp of |dgamma64|

    with rstd, the sums and dgamma64 in float64, dbeta the engine's own value, 1.01 covering the higher-order terms while
    (kf + 3) * 2^-24 < 0.01 (the largest kf is 4608), the last term standing for the final rounding, and no relative tolerance on top.
    The kernel's own f32 rstd = fl(1 / sqrtf(fl(var + eps))) is within 3.5 u of the float64 one (as the scale of the fold), which is
    3.5 u * |dgamma64| <= 3.5 u * rstd * (sum|..| + |mean * dbeta|) more.  It has its room inside the kf term: that term allows every
    addend kf roundings, and a block of 256 threads that sums kf <= 4608 addends gives none of them more than kf / 256 + 2 of its own
    partial sum and 9 of the reduction tree, 29 at kf = 4608 and 10 at kf = 256."""
    co, name = spec.co, spec.name
    dwp = np.ascontiguousarray(dwp, dtype=np.float32).reshape(spec.co_pad, spec.kf)
    g_w = np.ascontiguousarray(g_w, dtype=np.float32).reshape(m["W"].shape)
    perm = unarrange_dw(spec, dwp)
    if not np.abs(perm).max() > 0:
        rep.add(name, "dw", "the accumulators are all zero: nothing would be checked")
    gb = g_w.view(np.uint32).reshape(co, -1)
    if spec.bn is None or raw:
        rep.bits(name, "grad", g_w.view(np.uint32), perm.view(np.uint32), "from the un-permuted dW'")
        return 0.0
    rstd32 = np.float32(1.0) / np.sqrt(m["var"] + np.float32(BN_EPS))
    s0 = (m["gamma"] * rstd32).astype(np.float32)
    cands = [s0, np.nextafter(s0, np.float32(-np.inf)), np.nextafter(s0, np.float32(np.inf))]
    hits = np.stack([((perm * _per_channel(spec, s)).astype(np.float32).view(np.uint32).reshape(co, -1) == gb) for s in cands])  # [3][co][n]
    whole = hits.all(2)  # [3][co]
    bad = ~whole.any(0)
    if bad.any():
        c = int(np.argmax(bad))
        best = int(np.argmax(hits[:, c].sum(1)))
        e = int(np.argmax(~hits[best, c]))
        idx = [c] + [int(i) for i in np.unravel_index(e, m["W"].shape[1:])]
        want = (perm * _per_channel(spec, cands[best])).astype(np.float32).view(np.uint32).reshape(co, -1)
        rep.add(name, "grad", f"{int(bad.sum())} of {co} channels are not fl(dW' * s) under one s per channel, first at {idx}: got "
                              f"0x{int(gb[c, e]):08x}, expected 0x{int(want[c, e]):08x} with s = {float(cands[best][c])!r} "
                              f"({int((~hits[best, c]).sum())} of {gb.shape[1]} elements of that channel differ)")
    dbeta = np.ascontiguousarray(dbeta, dtype=np.float32)
    dg64, sumabs, rstd = dgamma64(spec, m, perm, dbeta)
    mdb = np.abs(m["mean"].astype(np.float64) * dbeta.astype(np.float64))
    bound = rstd * 1.01 * (spec.kf + 3) * 2.0 ** -24 * (sumabs + mdb) + np.spacing(np.abs(dg64).astype(np.float32)).astype(np.float64)
    err = np.abs(np.ascontiguousarray(g_gamma, dtype=np.float32).astype(np.float64) - dg64)
    rep.bound(name, "dgamma", err, bound, "the f32 summation bound of rstd * (<dW', W> - mean * dbeta)")
    return float((err / bound).max())


def check_dq_pad(rep, got, dq, dtype):
    """The head's gradient operand [rows][64] (bit patterns as stored) against dL/dQ f32 [rows][nq]: round_T(dq) in the first nq
    columns of each row, +0 in every other column."""
    rows, nq = dq.shape
    want = np.zeros((rows, 64), dtype=np.float32)
    want[:, :nq] = dq
    rep.bits("head", "dq", np.asarray(got).reshape(rows, 64), stored_bits(want, dtype))
