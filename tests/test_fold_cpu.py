"""tests/fold_oracle.py on the CPU: its layouts are the operands of the convolutions they claim to be, its bf16 rounding is torch's,
its layer list is the engine's, and the comparator tests/test_gpu_fold.py uses reports every corruption a subtly wrong fold or
unfold kernel could produce, and passes the uncorrupted output.

Layouts.  A packed operand is what an implicit-GEMM kernel multiplies with rows of input patches, so the check IS that product, in
float64: patches [pixels][kf] times Wf^T against F.conv2d(x, W) * s + b, the scatter of gy times Wd against F.grad.conv2d_input,
and gy^T times patches, un-permuted, against F.grad.conv2d_weight.  Both sides are float64 sums of at most 6400 terms of the same
products in different orders: the gate is 1e-12 of the reference's largest magnitude."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fold_oracle as fo
from video_dqn_amd import synth

GATE = 1e-12


@functools.lru_cache(maxsize=None)
def _sd(F_):
    return synth.make_state_dict(7, num_frames=F_)


def _layer(name, F_=1, head=None):
    spec = {s.name: s for s in fo.layers(True, F_, head=head)}[name]
    hw = hb = None
    if head is not None:
        rng = np.random.default_rng(8)
        hw = (0.05 * rng.standard_normal((fo.head_rows(head), 256))).astype(np.float32)
        hb = (0.05 * rng.standard_normal(fo.head_rows(head))).astype(np.float32)
    return spec, fo.master(spec, _sd(F_), head, hw, hb)


def _close(got, want, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    ref = np.abs(np.asarray(want)).max()
    assert ref > 0 and err <= GATE * ref, f"{what}: max error {err:.3e} against a largest magnitude of {ref:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 rounding
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


EDGE_BITS = fo.EDGE_BITS


def test_bf16_rounding_is_torchs_on_the_edges_and_on_random_bits():
    rng = np.random.default_rng(3)
    bits = np.concatenate([np.array(EDGE_BITS, dtype=np.uint32), rng.integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = fo.bf16_bits(x)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(x.view(np.uint32)[i]), hex(got[i]), hex(want[i])) for i in bad[:8]]
    # and the named edges do what their comments say
    e = fo.bf16_bits(_f32(EDGE_BITS[:4] + [0x7F7FFFFF, 0x7F7F8000, 0x80000000, 0x00008000, 0x00018000]))
    assert [hex(v) for v in e] == [hex(v) for v in (0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x7F80, 0x7F80, 0x8000, 0x0000, 0x0002)]


def test_fused_rounding_is_exact_where_float64_rounds_twice():
    """fused_f32 returns the f32 nearest the exact beta - mean * sc: on random operands, on exact ties (decided to even in rational
    arithmetic) and where the float64 difference sits next to a midpoint."""
    from fractions import Fraction
    rng = np.random.default_rng(4)
    beta, mean, sc = (rng.standard_normal(500).astype(np.float32) for _ in range(3))
    # exact ties: (1 + 2^-23) * 1.5 = 1.5 + 2^-23 + 2^-24, half a step above an f32; and its neighbours
    beta[:3], mean[:3], sc[:3] = 0, [-(1 + 2 ** -23), -(1 + 2 ** -22), 1 + 2 ** -23], [1.5, 1.5, -1.5]
    beta[3:5], mean[3:5], sc[3:5] = [2 ** -30, -(2 ** -30)], -(1 + 2 ** -23), 1.5
    got = fo.fused_f32(beta, mean, sc)
    for i in range(beta.size):
        fr = Fraction(float(beta[i])) - Fraction(float(mean[i])) * Fraction(float(sc[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        d, dlo, dhi = (abs(Fraction(float(v)) - fr) for v in (got[i], lo, hi))
        assert d <= dlo and d <= dhi, i
        if d == dlo or d == dhi:
            assert int(got[i].view(np.uint32)) & 1 == 0, i
    assert got[0] == np.float32(1.5 + 2 ** -22) and got[1] == np.float32(1.5 + 3 * 2 ** -23) and got[3] == np.float32(1.5 + 2 ** -22)
    assert got[4] == np.float32(1.5 + 2 ** -23)


# ---------------------------------------------------------------------------------------------------------------------------------
# the layer list and the library's layout entry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra,F_,dtype,head", [(True, 1, "bf16", None), (True, 4, "f32", None), (True, 1, "bf16", "value"),
                                                 (True, 1, "f32", "spread"), (True, 1, "bf16", "policy"), (False, 1, "f32", None),
                                                 (False, 4, "bf16", None), (True, 1, "bf16x3", None)])
def test_packed_offsets_tile_the_buffer_in_the_oracles_regions(extra, F_, dtype, head):
    """vdqn_net_packed_offset names every region of every layer of the oracle's list; in the engine's order the regions follow one
    another at 256-byte alignment with the oracle's sizes and end at vdqn_net_packed_bytes; the two refusals are distinct."""
    from video_dqn_amd.engine import NetEngine
    net = NetEngine(3, 5, F_, extra, dtype, 8, device="cpu", **({f"{head}_head": True} if head else {}))
    esz = 2 if dtype == "bf16" else 4
    off = lambda n: net.lib.vdqn_net_packed_offset(net.handle, n.encode())  # noqa: E731
    regions = []
    for spec in fo.layers(extra, F_, head=head):
        for region, nbytes in fo.region_bytes(spec, esz).items():
            o = off(f"{region}:{spec.name}")
            assert o >= 0 and o % 256 == 0, (region, spec.name, o)
            regions.append((o, nbytes, region, spec.name))
        rows = sum(net.slots[k].shape[0] for k in [spec.name + ".weight"] + ([f"{head}.weight"] if head and spec.name in ("top.4", "top") else []))
        assert rows == spec.co and net.slots[spec.name + ".weight"].shape[1:] == ((spec.ci, spec.r, spec.s) if "conv" in spec.kind else (spec.ci,))
    regions.sort()
    end = 0
    for o, nbytes, region, name in regions:
        assert o == end, f"{region}:{name} starts at {o}, the region before it ends (aligned) at {end}"
        end = (o + nbytes + 255) // 256 * 256
    assert end == net.packed_bytes
    assert off("wd:resnet.conv1") == -2
    for bad in ("wf:resnet.conv9", "wq:resnet.conv1", "resnet.conv1", "wf:", "", "wd:resnet.fc"):
        assert off(bad) == -1, bad


# ---------------------------------------------------------------------------------------------------------------------------------
# layouts: the packed operands are the operands of the convolution
# ---------------------------------------------------------------------------------------------------------------------------------
def _patches(x, r, s, stride, pad):
    """NHWC x -> [n][ho][wo][r][s][c], the rows an implicit-GEMM kernel multiplies with Wf."""
    n, h, w, c = x.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1
    out = np.empty((n, ho, wo, r, s, c))
    for i in range(r):
        for j in range(s):
            out[:, :, :, i, j, :] = xp[:, i:i + stride * ho:stride, j:j + stride * wo:stride, :]
    return out


def _folded64(spec, m):
    s64, b64 = fo.scale_bias64(spec, m)
    return m["W"].astype(np.float64) * fo._per_channel(spec, s64[:spec.co]), s64, b64


@pytest.mark.parametrize("name,hw", [("resnet.layer1.0.conv1", (5, 6)), ("resnet.layer2.0.conv1", (7, 6)),
                                     ("resnet.layer2.0.downsample.0", (7, 6)), ("features.8", (4, 5))])
def test_conv_operands_convolve_like_the_reference(name, hw):
    spec, m = _layer(name)
    rng = np.random.default_rng(11)
    Wfold, s64, b64 = _folded64(spec, m)
    x = rng.standard_normal((2, spec.ci) + hw)
    W_t, x_t = torch.from_numpy(m["W"].astype(np.float64)), torch.from_numpy(x)
    bias_t = None if spec.bn is not None else torch.from_numpy(m["bias"].astype(np.float64))
    ref = F.conv2d(x_t, W_t, bias_t, spec.stride, spec.pad)
    if spec.bn is not None:
        ref = ref * torch.from_numpy(s64[:spec.co]).view(1, -1, 1, 1) + torch.from_numpy(b64[:spec.co]).view(1, -1, 1, 1)
    ref = ref.numpy()
    n, _, ho, wo = ref.shape
    assert ho > 1 and wo > 1
    pt = _patches(x.transpose(0, 2, 3, 1), spec.r, spec.s, spec.stride, spec.pad).reshape(n * ho * wo, spec.kf)
    wf = fo.arrange_wf(spec, Wfold)
    y = (pt @ wf.T + b64).reshape(n, ho, wo, spec.co_pad)
    _close(y[..., :spec.co].transpose(0, 3, 1, 2), ref, name + " forward")
    # data gradient through Wd, against the folded weights' conv2d_input
    gy = np.zeros((n, ho, wo, spec.co_pad))
    gy[..., :spec.co] = rng.standard_normal((n, ho, wo, spec.co))
    gy_t = torch.from_numpy(np.ascontiguousarray(gy[..., :spec.co].transpose(0, 3, 1, 2)))
    wd = fo.arrange_wd(spec, Wfold).reshape(spec.ci, spec.r, spec.s, spec.co_pad)
    dxp = np.zeros((n, hw[0] + 2 * spec.pad, hw[1] + 2 * spec.pad, spec.ci))
    for i in range(spec.r):
        for j in range(spec.s):
            dxp[:, i:i + spec.stride * ho:spec.stride, j:j + spec.stride * wo:spec.stride, :] += gy @ wd[:, i, j, :].T
    dx = dxp[:, spec.pad:spec.pad + hw[0], spec.pad:spec.pad + hw[1], :]
    ref_dx = F.grad.conv2d_input(x_t.shape, torch.from_numpy(Wfold), gy_t, spec.stride, spec.pad).numpy()
    _close(dx.transpose(0, 3, 1, 2), ref_dx, name + " data gradient")
    # weight gradient in the packed layout, un-permuted
    dwp = gy.reshape(-1, spec.co_pad).T @ pt
    ref_dw = F.grad.conv2d_weight(x_t, W_t.shape, gy_t, spec.stride, spec.pad).numpy()
    _close(fo.unarrange_dw(spec, dwp), ref_dw, name + " weight gradient")


def test_conv1_operand_is_the_7x7_stride2_convolution_of_a_space_to_depth_frame():
    spec, m = _layer("resnet.conv1")
    rng = np.random.default_rng(12)
    Wfold, s64, b64 = _folded64(spec, m)
    H, W_ = 11, 10
    x = rng.standard_normal((2, 3, H, W_))
    x_t, W_t = torch.from_numpy(x), torch.from_numpy(m["W"].astype(np.float64))
    ref = (F.conv2d(x_t, W_t, None, 2, 3) * torch.from_numpy(s64[:64]).view(1, -1, 1, 1) + torch.from_numpy(b64[:64]).view(1, -1, 1, 1)).numpy()
    n, _, ho, wo = ref.shape
    # the frame, zero padded by 4 on the top and left, as 2x2 blocks of 12 + 4 channels in (bh, bw, c) order
    hb, wb = ho + 3, wo + 3
    p = np.zeros((n, 3, 2 * hb, 2 * wb))
    p[:, :, 4:4 + H, 4:4 + W_] = x
    s2d = np.zeros((n, hb, wb, 16))
    s2d[..., :12] = p.reshape(n, 3, hb, 2, wb, 2).transpose(0, 2, 4, 3, 5, 1).reshape(n, hb, wb, 12)
    # a 4x1 window over 64 "channels": four consecutive 16-channel blocks of a row
    flat = s2d.reshape(n, hb, wb * 16)
    pt = np.empty((n, ho, wo, 4, 64))
    for a in range(4):
        for o in range(wo):
            pt[:, :, o, a, :] = flat[:, a:a + ho, o * 16:o * 16 + 64]
    pt = pt.reshape(n * ho * wo, spec.kf)
    wf = fo.arrange_wf(spec, Wfold)
    assert wf.shape == (64, 256) and (wf.reshape(64, 4, 4, 16)[..., 12:] == 0).all()
    assert (wf.reshape(64, 4, 4, 16)[:, 0, :, :6] == 0).all() and (wf.reshape(64, 4, 4, 16)[:, :, 0, [0, 1, 2, 6, 7, 8]] == 0).all()  # r7 < 0, s7 < 0
    y = (pt @ wf.T + b64).reshape(n, ho, wo, 64)
    _close(y.transpose(0, 3, 1, 2), ref, "conv1 forward")
    gy = rng.standard_normal((n, ho, wo, 64))
    dwp = gy.reshape(-1, 64).T @ pt
    ref_dw = F.grad.conv2d_weight(x_t, W_t.shape, torch.from_numpy(np.ascontiguousarray(gy.transpose(0, 3, 1, 2))), 2, 3).numpy()
    _close(fo.unarrange_dw(spec, dwp), ref_dw, "conv1 weight gradient")
    with pytest.raises(AssertionError):
        fo.arrange_wd(spec, Wfold)


@pytest.mark.parametrize("name,F_,head", [("top.0", 1, None), ("top.0", 4, None), ("top.4", 1, "value"), ("top.2", 1, None)])
def test_linear_operands_multiply_like_the_reference(name, F_, head):
    spec, m = _layer(name, F_, head)
    rng = np.random.default_rng(13)
    W64, b64 = m["W"].astype(np.float64), m["bias"].astype(np.float64)
    n = 3
    if name == "top.0":  # the reference flattens [F][64 channels][5][5]; the engine's features are [F][25 pixels][64 channels]
        x_ref = rng.standard_normal((n, F_, 64, 25))
        x_eng = x_ref.transpose(0, 1, 3, 2).reshape(n, -1)
        to_ref = lambda d: d.reshape(n, F_, 25, 64).transpose(0, 1, 3, 2).reshape(n, -1)  # noqa: E731
    else:
        x_ref = x_eng = rng.standard_normal((n, spec.ci))
        to_ref = lambda d: d  # noqa: E731
    x_t, W_t = torch.from_numpy(x_ref.reshape(n, -1)).requires_grad_(True), torch.from_numpy(W64).requires_grad_(True)
    ref = F.linear(x_t, W_t, torch.from_numpy(b64))
    wf = fo.arrange_wf(spec, W64)
    bias = np.zeros(spec.co_pad)
    bias[:spec.co] = b64
    y = x_eng @ wf.T + bias
    _close(y[:, :spec.co], ref.detach().numpy(), name + " forward")
    assert (y[:, spec.co:] == 0).all()
    gy = np.zeros((n, spec.co_pad))
    gy[:, :spec.co] = rng.standard_normal((n, spec.co))
    ref.backward(torch.from_numpy(gy[:, :spec.co].copy()))
    wd = fo.arrange_wd(spec, W64)
    assert wd.shape == (spec.ci, spec.co_pad) and (wd[:, spec.co:] == 0).all()
    _close(to_ref(gy @ wd.T), x_t.grad.numpy(), name + " data gradient")
    _close(fo.unarrange_dw(spec, gy.T @ x_eng), W_t.grad.numpy(), name + " weight gradient")
    if head:  # the head's rows sit directly behind the Q rows
        assert spec.co == 15 + 5 and (wf[15:20] == m["W"][15:].astype(np.float64)).all() and (m["W"][:15] == _sd(1)["top.4.weight"].numpy()).all()


def test_scale_and_bias_statements():
    spec, m = _layer("resnet.layer2.0.conv1")
    s, b = fo.scale_bias64(spec, m)
    g, be, mu, var = (m[k].astype(np.float64) for k in ("gamma", "beta", "mean", "var"))
    assert np.array_equal(s, g / np.sqrt(var + 1e-5)) and np.array_equal(b, be - mu * s)
    s, b = fo.scale_bias64(spec, m, raw=True)
    assert (s == 1).all() and (b == 0).all()
    spec, m = _layer("top.4", head="policy")
    s, b = fo.scale_bias64(spec, m)
    assert spec.co == 18 and (s[:18] == 1).all() and (s[18:] == 0).all() and (b[18:] == 0).all() and np.array_equal(b[:18], m["bias"].astype(np.float64))
    sb = {x.name: x for x in fo.layers(False, 4)}
    assert sb["top"].ci == 2048 and "features.8" not in sb


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator: clean output passes, every corruption is reported with layer, region and first element
# ---------------------------------------------------------------------------------------------------------------------------------
def simulate_fold(spec, m, dtype, raw=False, with_dgrad=True):
    """What a correct fold stores for one layer, from the oracle's own statements (numpy f32 arithmetic, the bias fused)."""
    co = spec.co
    scale, bias = np.zeros(spec.co_pad, np.float32), np.zeros(spec.co_pad, np.float32)
    scale[:co] = 1.0
    if spec.bn is not None and not raw:
        scale[:co] = m["gamma"] / np.sqrt(m["var"] + np.float32(fo.BN_EPS))
        bias[:co] = fo.fused_f32(m["beta"], m["mean"], scale[:co])
    elif spec.bn is None:
        bias[:co] = m["bias"]
    ws = m["W"] * fo._per_channel(spec, scale[:co])
    got = {"scale": scale, "bias": bias, "wf": fo.stored_bits(fo.arrange_wf(spec, ws), dtype).copy()}
    if spec.kind != "conv1":
        got["wd"] = fo.stored_bits(fo.arrange_wd(spec, ws), dtype).copy() if with_dgrad else \
            np.full((spec.wd_rows, spec.kd), fo._poison_pattern(2 if dtype == "bf16" else 4), np.uint16 if dtype == "bf16" else np.uint32)
    return got


COMPARATOR_LAYERS = [("resnet.layer2.0.conv1", None), ("resnet.layer2.0.downsample.0", None), ("resnet.conv1", None), ("features.8", None),
                     ("top.0", None), ("top.4", "value")]


def _differing_pair(a, row, step, lo=0):
    """first k >= lo in row `row` of the 2-D array with a[row, k] != a[row, k + step]"""
    k = lo + int(np.argmax(a[row, lo:a.shape[1] - step] != a[row, lo + step:]))
    assert a[row, k] != a[row, k + step]
    return k


def _report(spec, m, got, dtype, **kw):
    rep = fo.Report()
    fo.check_fold_layer(rep, spec, m, got, dtype, **kw)
    return rep


def _expect(rep, layer, region, index=None):
    lines = [ln for ln in rep.lines if ln.startswith(f"{layer} {region}:")]
    assert lines, f"nothing reported for {layer} {region}:\n{rep.text()}"
    if index is not None:
        assert any(f"first at {list(index)}" in ln for ln in lines), (index, lines)


@pytest.mark.parametrize("name,head", COMPARATOR_LAYERS)
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_comparator_passes_clean_folds_and_reports_corrupted_ones(name, head, dtype):
    spec, m = _layer(name, 1, head)
    clean = simulate_fold(spec, m, dtype)
    rep = fo.Report()
    info = fo.check_fold_layer(rep, spec, m, clean, dtype)
    rep.assert_clean(name)
    assert info["bias"] in (("fused", "either") if spec.bn else ("exact",)) and info["scale_ulps"] <= 2.5  # (three correctly rounded operations)
    _report(spec, m, simulate_fold(spec, m, dtype, with_dgrad=False), dtype, with_dgrad=False).assert_clean(name + " without dgrad")
    fresh = lambda: {k: v.copy() for k, v in clean.items()}  # noqa: E731
    row = 3
    taps, per_tap = {"conv": (spec.r * spec.s, spec.ci), "conv1": (4, 64), "linear_perm": (25, 64), "linear": (1, spec.ci)}[spec.kind]

    if dtype == "bf16":  # truncation instead of round-to-nearest-even
        s = clean["scale"][:spec.co]
        g = fresh()
        g["wf"] = (fo.arrange_wf(spec, m["W"] * fo._per_channel(spec, s)).view(np.uint32) >> 16).astype(np.uint16)
        rep = _report(spec, m, g, dtype)
        _expect(rep, name, "wf")
        assert len(rep.lines) == 1

    g = fresh()  # two adjacent channels swapped inside one tap
    k = _differing_pair(g["wf"], row, 1, lo=per_tap + 16 if taps > 1 else 16)
    if k % per_tap == per_tap - 1:  # (stay inside the tap)
        k = _differing_pair(g["wf"], row, 1, lo=k + 1)
    g["wf"][row, [k, k + 1]] = g["wf"][row, [k + 1, k]]
    _expect(_report(spec, m, g, dtype), name, "wf", (row, k))

    if taps > 1:  # two taps swapped
        g = fresh()
        v = g["wf"].reshape(spec.co_pad, taps, per_tap)
        v[row, [1, 2]] = v[row, [2, 1]]
        first = per_tap + int(np.argmax(clean["wf"].reshape(spec.co_pad, taps, per_tap)[row, 1] != clean["wf"].reshape(spec.co_pad, taps, per_tap)[row, 2]))
        _expect(_report(spec, m, g, dtype), name, "wf", (row, first))
        g = fresh()  # the same in the data-gradient operand: two taps of one input channel
        if spec.kind == "conv":
            v = g["wd"].reshape(spec.ci, taps, spec.co_pad)
            v[5, [0, 1]] = v[5, [1, 0]]
            _expect(_report(spec, m, g, dtype), name, "wd")

    g = fresh()  # one row shifted by one
    g["wf"][row] = np.roll(g["wf"][row], 1)
    rep = _report(spec, m, g, dtype)
    _expect(rep, name, "wf")
    assert f"first at [{row}, " in rep.text()

    if spec.bn is not None:  # - mean * scale dropped on one channel; the scale off by five ulps on another
        g = fresh()
        g["bias"][7] = m["beta"][7]
        rep = _report(spec, m, g, dtype)
        _expect(rep, name, "bias", (7,))
        g = fresh()
        for _ in range(5):
            g["scale"][9] = np.nextafter(g["scale"][9], np.float32(np.inf))
        _expect(_report(spec, m, g, dtype), name, "scale", (9,))

    one = 0x3F80 if dtype == "bf16" else 0x3F800000
    if spec.co_pad > spec.co:  # one pad row non-zero: in the operand, in the scale
        g = fresh()
        g["wf"][spec.co_pad - 1, 5] = one
        _expect(_report(spec, m, g, dtype), name, "wf", (spec.co_pad - 1, 5))
        g = fresh()
        g["wd"][4, spec.co] = one
        _expect(_report(spec, m, g, dtype), name, "wd", (4, spec.co))
        g = fresh()
        g["scale"][spec.co] = 1.0
        _expect(_report(spec, m, g, dtype), name, "scale", (0,))
        g = fresh()
        g["bias"][spec.co_pad - 1] = -0.0  # +0 is asked for, bit for bit
        _expect(_report(spec, m, g, dtype), name, "bias", (spec.co_pad - 1 - spec.co,))
    if spec.kind == "conv1":  # a pad channel and a tap above the window non-zero
        for k in (2 * 64 + 1 * 16 + 13, 0 * 64 + 2 * 16 + 4):
            g = fresh()
            g["wf"][row, k] = one
            _expect(_report(spec, m, g, dtype), name, "wf", (row, k))
    else:  # one Wd element left at the poison value; Wd written although it was not asked for
        g = fresh()
        g["wd"][11, 17] = fo._poison_pattern(g["wd"].dtype.itemsize)
        rep = _report(spec, m, g, dtype)
        _expect(rep, name, "wd", (11, 17))
        assert "still the poison value" in rep.text()
        _expect(_report(spec, m, clean, dtype, with_dgrad=False), name, "wd", (0, 0))


def test_comparator_reports_a_raw_fold_that_folded_and_gaps_that_were_written():
    spec, m = _layer("resnet.layer2.0.conv1")
    _report(spec, m, simulate_fold(spec, m, "f32", raw=True), "f32", raw=True).assert_clean("raw")
    rep = _report(spec, m, simulate_fold(spec, m, "f32"), "f32", raw=True)
    _expect(rep, spec.name, "scale", (0,))
    _expect(rep, spec.name, "bias", (0,))
    # the byte-level check: regions of 100 and 40 bytes with a gap between and behind them
    regions = [("a", "wf", 0, 100), ("a", "wd", 256, 40)]
    buf = np.full(512, fo.POISON, np.uint8)
    buf[:100] = 1
    rep = fo.Report()
    fo.check_poison(rep, buf, regions, with_dgrad=False)
    rep.assert_clean("poison")
    buf[300] = 0
    fo.check_poison(rep, buf, regions, with_dgrad=True)
    _expect(rep, "a", "gap")
    assert "first at byte 300" in rep.text()
    rep = fo.Report()
    buf[300], buf[260] = fo.POISON, 7
    fo.check_poison(rep, buf, regions, with_dgrad=False)
    _expect(rep, "a", "wd")
    rep = fo.Report()
    fo.check_poison(rep, buf, regions + [("b", "wf", 290, 10)], with_dgrad=True)
    _expect(rep, "b", "wf")


def simulate_unfold(spec, m, dwp, dbeta, raw=False):
    """What a correct unfold writes: (weight gradient, dgamma or None)."""
    perm = fo.unarrange_dw(spec, dwp)
    if spec.bn is None or raw:
        return perm.copy(), None
    sc = (m["gamma"] * (np.float32(1) / np.sqrt(m["var"] + np.float32(fo.BN_EPS)))).astype(np.float32)
    dg, _, _ = fo.dgamma64(spec, m, perm, dbeta)
    return (perm * fo._per_channel(spec, sc)).astype(np.float32), dg.astype(np.float32)


@pytest.mark.parametrize("name,head", COMPARATOR_LAYERS + [("resnet.layer4.1.conv2", None)])
def test_comparator_passes_clean_unfolds_and_reports_corrupted_ones(name, head):
    spec, m = _layer(name, 1, head)
    rng = np.random.default_rng(21)
    dwp = (1e-3 * rng.standard_normal((spec.co_pad, spec.kf))).astype(np.float32)
    dbeta = rng.standard_normal(spec.co).astype(np.float32)
    g_w, g_gamma = simulate_unfold(spec, m, dwp, dbeta)

    def run(gw, gg=g_gamma, d=dwp):
        rep = fo.Report()
        ratio = fo.check_unfold_layer(rep, spec, m, d, gw, gg, dbeta)
        return rep, ratio
    rep, ratio = run(g_w)
    rep.assert_clean(name)
    assert ratio < 0.1  # (a float64 sum rounded once: far inside the f32 bound)
    idx = (2, 1) + (0,) * (m["W"].ndim - 2)
    bad = g_w.copy()  # one element an ulp off
    bad[idx] = np.nextafter(bad[idx], np.float32(np.inf))
    _expect(run(bad)[0], name, "grad", idx)
    bad = g_w.copy()  # two adjacent elements of one output channel swapped
    flat = bad.reshape(spec.co, -1)
    k = _differing_pair(flat, 5, 1, lo=3)
    flat[5, [k, k + 1]] = flat[5, [k + 1, k]]
    _expect(run(bad)[0], name, "grad", (5,) + tuple(int(i) for i in np.unravel_index(k, m["W"].shape[1:])))
    _expect(run(g_w, d=np.zeros_like(dwp))[0], name, "dw")  # nothing to check is a finding, not a pass
    if spec.bn is not None:
        perm = fo.unarrange_dw(spec, dwp)
        rstd = 1.0 / np.sqrt(m["var"].astype(np.float64) + fo.BN_EPS)
        no_mean = (rstd * (perm.astype(np.float64) * m["W"].astype(np.float64)).reshape(spec.co, -1).sum(1)).astype(np.float32)
        rep, ratio = run(g_w, no_mean)  # dgamma without the mean * dbeta term
        _expect(rep, name, "dgamma", (0,))
        assert ratio > 1 and len(rep.lines) == 1
        # the channel's scale taken from its neighbour (a per-channel s that is not gamma * rstd), and half a channel under another s
        other = (perm * fo._per_channel(spec, np.roll(m["gamma"], 1) / np.sqrt(m["var"] + np.float32(fo.BN_EPS)))).astype(np.float32)
        _expect(run(other)[0], name, "grad")
        half = g_w.copy().reshape(spec.co, -1)
        s_up = np.nextafter((m["gamma"] * (np.float32(1) / np.sqrt(m["var"] + np.float32(fo.BN_EPS)))).astype(np.float32), np.float32(np.inf))
        half[4, ::2] = (perm.reshape(spec.co, -1)[4, ::2] * s_up[4]).astype(np.float32)
        if not np.array_equal(half, g_w.reshape(spec.co, -1)):
            rep = run(half.reshape(g_w.shape))[0]
            _expect(rep, name, "grad")
            assert "first at [4, " in rep.text()


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_comparator_of_the_q_gradient_pad(dtype):
    rng = np.random.default_rng(5)
    dq = rng.standard_normal((5, 15)).astype(np.float32)
    dq[0, :4] = _f32([0x3F808000, 0x3F818000, 0x80000000, 0x00018000])
    want = np.zeros((5, 64), np.float32)
    want[:, :15] = dq
    clean = fo.stored_bits(want, dtype).copy()
    rep = fo.Report()
    fo.check_dq_pad(rep, clean, dq, dtype)
    rep.assert_clean("dq")
    for idx, val in (((2, 15), 1), ((4, 63), 0x8000 if dtype == "bf16" else 0x80000000), ((0, 1), clean[0, 1] - 1)):
        g = clean.copy()
        g[idx] = val
        rep = fo.Report()
        fo.check_dq_pad(rep, g, dq, dtype)
        _expect(rep, "head", "dq", idx)
