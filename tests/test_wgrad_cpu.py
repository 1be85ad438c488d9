"""The weight-gradient oracle (tests/wgrad_oracle.py) checked on the CPU: the integer reference equals torch's own f32 bit for bit and
respects the 2^24 assertion, torch's f32 on real-valued operands lies inside the derived bound B (the ratio is printed: pytest -s),
plan() equals the loaded library's workspace queries (the library loads without a GPU), the library's refusals name their field, and
every injected fault fails the check that exists to catch it."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_oracle as W

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    from video_dqn_amd import _lib
    return _lib.load()


def _args(c):
    from video_dqn_amd import _lib
    a = _lib.WgradArgs()
    a.n_img, a.hi, a.wi, a.ci, a.pix_stride = c.n, c.hi, c.wi, c.ci, c.pix_stride
    a.ho, a.wo, a.co, a.ldg = c.ho, c.wo, c.co, c.ldg
    a.r, a.s, a.stride, a.pad = c.r, c.s, c.stride, c.pad
    a.splitk, a.dtype = c.splitk, {"bf16": _lib.VDQN_BF16, "f32": _lib.VDQN_F32, "x3": _lib.VDQN_F32X3}[c.dtype]
    return a


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.name)
def test_integer_reference_is_exact_in_f32(c):
    o = W.make_operands(c, 1, "int")
    ref, f32 = W.reference(c, o), W.reference(c, o, F32)   # (reference() asserts the 2^24 limit)
    assert W.check_exact(f32["dw"], ref["dw"]) == (0, None)
    assert W.check_exact(f32["dbias"], ref["dbias"]) == (0, None)
    assert torch.equal(ref["dw"], ref["dw"].round()) and float(ref["dw"].abs().max()) > 0
    assert o["x"].abs().max() <= 3 and o["gy"].abs().max() <= 2
    assert float(o["x"][..., c.ci:].abs().sum()) > 0 or c.pix_stride == c.ci or c.is_stem
    assert float(o["gy"][..., c.co:].abs().sum()) > 0 or c.ldg == c.co


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.name)
def test_real_reference_inside_bound(c):
    o = W.make_operands(c, 1, "real")
    ref, f32 = W.reference(c, o), W.reference(c, o, F32)
    bad, ratio = W.check_bound(f32["dw"], ref["dw"], ref["B"])
    bad_b, ratio_b = W.check_bound(f32["dbias"], ref["dbias"], ref["Bb"])
    print(f"\n[ratio] {c.name}: torch f32 against float64, dw {ratio:.3g} x B, dbias {ratio_b:.3g} x B (M = {c.M})")
    assert bad == 0 and bad_b == 0
    assert ratio < 0.1 and ratio_b < 0.1   # the bound is not tight on a plain f32 sum: it leaves the kernels their orders


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.name)
def test_plan_equals_the_library_query(c, lib, monkeypatch):
    for k in ("VDQN_WGRAD_WINDOW", "VDQN_WGRAD_STEM", "VDQN_WGRAD_DS64", "VDQN_WGRAD_BLOCKS", "VDQN_WGRAD_WIN_BLOCKS"):
        monkeypatch.delenv(k, raising=False)   # (the library reads them once per process: tests run without them)
    pl = W.plan(c, {})
    assert lib.vdqn_conv2d_wgrad_workspace_bytes(C.byref(_args(c))) == pl["bytes"]
    from video_dqn_amd import ops
    st = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    assert ops.conv2d_wgrad_workspace_bytes(n=c.n, hi=c.hi, wi=c.wi, ci=c.ci, ho=c.ho, wo=c.wo, co=c.co, r=c.r, s=c.s, stride=c.stride,
                                            pad=c.pad, dtype=st, precision="bf16x3" if c.dtype == "x3" else None, ldg=c.ldg,
                                            pix_stride=c.pix_stride, splitk=c.splitk) == pl["bytes"]


def test_plan_pins_what_the_cases_exist_for():
    p = {c.name: W.plan(c, {}) for c in W.CASES}
    win = "wgrad_win<bf16,64>"
    for name in ("win-2x2", "win-3x3", "win-5x17", "win-10x6", "win-10x6-k3", "win-10x6-k5", "win-8x8", "win-57x56", "win-co100", "win-ldg192"):
        assert p[name]["tag"] == win, name
    assert (p["win-3x3"]["splitk"], p["win-3x3"]["copies"]) == (2, 2)
    assert (p["win-57x56"]["splitk"], p["win-57x56"]["copies"]) == (13, 13) and 57 * 56 == 3192 <= W.CODE_TABLE_BYTES < 58 * 56
    assert p["win-8x8"]["kchunk"] == W.CASE_BY_NAME["win-8x8"].M == 256
    assert p["win-10x6-k3"]["kchunk"] % 60 != 0      # its second split starts inside an image
    assert p["gen-58x56"]["tag"] == "wgrad<bf16,128>" and p["gen-pix128"]["tag"] == "wgrad<bf16,64>" and p["gen-w1"]["tag"] == "wgrad<bf16,64>"
    assert [p[f"s2-odd-{d}"]["tag"] for d in W.ALL3] == ["wgrad<bf16,64>", "wgrad<f32,64>", "wgrad<bf16x3,64>"]
    assert [p[f"s2-14x9-{d}"]["tag"] for d in W.ALL3] == ["wgrad<bf16,128>", "wgrad<f32,128>", "wgrad<bf16x3,128>"]
    assert [p[f"ds-{d}"]["tag"] for d in W.ALL3] == ["wgrad<bf16,64>", "wgrad<f32,128>", "wgrad<bf16x3,128>"]
    assert W.plan(W.CASE_BY_NAME["ds-bf16"], {"VDQN_WGRAD_DS64": "0"})["tag"] == "wgrad<bf16,128>"
    assert [p[f"l4-{d}"]["tag"] for d in ("f32", "x3")] == ["wgrad<f32,128>", "wgrad<bf16x3,128>"]
    assert (p["10x6-k5-f32"]["splitk"], p["10x6-k5-f32"]["copies"]) == (5, 3)    # two splits without pixels
    gen = W.plan(W.CASE_BY_NAME["win-10x6-k3"], {"VDQN_WGRAD_WINDOW": "0"})
    assert (gen["tag"], gen["kchunk"], gen["copies"]) == ("wgrad<bf16,64>", 128, 3)   # splits that start at pixels 128 and 256
    assert [p[n]["rows_per_block"] for n in ("stem-1", "stem-5", "stem-10")] == [1, 2, 3]
    assert all(p[n]["tag"] == "wgrad_stem<bf16>" for n in ("stem-1", "stem-5", "stem-10"))
    assert (10 * 112) % 3 == 1 and 112 % 3 != 0    # stem-10: a one-row last block, blocks that cross images
    assert [p[n]["tag"] for n in ("stem-1-k1", "stem-1-f32", "stem-1-x3")] == ["wgrad<bf16,64>", "wgrad<f32,64>", "wgrad<bf16x3,64>"]
    assert W.plan(W.CASE_BY_NAME["stem-5"], {"VDQN_WGRAD_STEM": "0"})["tag"] == "wgrad<bf16,64>"
    assert [W.stem_pool_grid(n)[:2] for n in range(1, 20)].index((3, 19)) == 18    # n = 19 is the first with three pairs per block
    assert [W.stem_pool_grid(n)[0] for n in W.POOL_N] == [1, 2, 3] and 56 % 3 != 0


@pytest.mark.parametrize("n", list(W.POOL_N) + [2, 9, 18, 64, 256, 600])
def test_stem_pool_grid_equals_the_library_query(n, lib):
    assert lib.vdqn_stem_wgrad_pool_workspace_bytes(n) == W.stem_pool_grid(n)[2]


REFUSED = [
    (dict(ci=96), r"ci=96 and ldg=\d+ must be multiples of 64"),
    (dict(ldg=96), r"ci=\d+ and ldg=96 must be multiples of 64"),
    (dict(co=100, ldg=64), r"ldg=64\) must hold co padded to 64 \(128\)"),
    (dict(stride=3), r"stride 3 unsupported"),
    (dict(n=1, hi=256, wi=256, ho=256, wo=256), r"ho\*wo too large"),
    (dict(n=2 ** 24 // 60 + 1), r"output pixels out of range"),
]


@pytest.mark.parametrize("change, message", REFUSED, ids=[m[:12] for _, m in REFUSED])
def test_workspace_query_refuses_by_name(change, message, lib):
    from dataclasses import replace
    from video_dqn_amd import _lib
    c = replace(W.CASE_BY_NAME["win-10x6"], **change)
    assert W.refusal(c) is not None
    assert lib.vdqn_conv2d_wgrad_workspace_bytes(C.byref(_args(c))) == -1
    msg = lib.vdqn_last_error().decode()
    import re
    assert re.search(message, msg), msg
    from video_dqn_amd import ops
    with pytest.raises(_lib.VdqnError, match=message):
        ops.conv2d_wgrad_workspace_bytes(n=c.n, hi=c.hi, wi=c.wi, ci=c.ci, ho=c.ho, wo=c.wo, co=c.co, r=c.r, s=c.s, stride=c.stride, pad=c.pad,
                                         ldg=c.ldg, pix_stride=c.pix_stride)


# ---- injected faults: each must fail the check that exists to catch it, in both passes ----
def _both_kinds(c):
    for kind in ("int", "real"):
        o = W.make_operands(c, 2, kind)
        yield kind, o, W.reference(c, o)


@pytest.mark.parametrize("name", ["win-5x17", "win-10x6", "win-57x56", "gen-58x56", "s2-odd-bf16", "valid-f32"])
def test_fault_border_column_dropped(name):
    c = W.CASE_BY_NAME[name]
    for kind, o, ref in _both_kinds(c):
        wrong, touched = W.drop_border_column(c, o, kr=1, ks=0 if c.pad == 0 else 1)
        assert W.check_exact(wrong[~touched], ref["dw"][~touched])[0] == 0
        if kind == "int":
            assert W.check_exact(wrong, ref["dw"])[0] > 0.5 * touched.sum()
        else:
            outside = ((wrong - ref["dw"]).abs() > ref["B"])[touched].double().mean().item()
            print(f"\n[fault] {name}: a dropped border column is outside B on {100 * outside:.1f} % of the elements it touches (M = {c.M})")
            assert W.check_bound(wrong, ref["dw"], ref["B"])[0] > 0 and outside > 0.5   # (measured: 90 % and more, 3248 pixels included)


@pytest.mark.parametrize("name", ["win-5x17", "win-10x6", "win-57x56", "win-ldg192"])
def test_fault_ho_wo_exchanged_in_the_window_shift(name):
    c = W.CASE_BY_NAME[name]
    assert c.ho != c.wo
    for kind, o, ref in _both_kinds(c):
        right, wrong = W.window_emulation(c, o), W.window_emulation(c, o, swap_ho_wo=True)
        if kind == "int":
            assert W.check_exact(right, ref["dw"]) == (0, None)    # the linear window addressing with border codes IS the convolution
            assert W.check_exact(wrong, ref["dw"])[0] > 0
            assert W.check_exact(wrong[:, 1], ref["dw"][:, 1])[0] == 0   # the middle kernel row has no row shift
        else:
            assert W.check_bound(right, ref["dw"], ref["B"])[0] == 0
            assert W.check_bound(wrong, ref["dw"], ref["B"])[0] > 0.5 * wrong[:, ::2].numel()


@pytest.mark.parametrize("name, split", [("win-3x3", 1), ("win-57x56", 12), ("10x6-k5-f32", 2), ("s2-14x9-bf16", 0)])
def test_fault_split_dropped(name, split):
    c = W.CASE_BY_NAME[name]
    for kind, o, ref in _both_kinds(c):
        wrong = W.drop_split(c, o, split)
        check = W.check_exact(wrong, ref["dw"]) if kind == "int" else W.check_bound(wrong, ref["dw"], ref["B"])
        assert check[0] > 0.5 * wrong.numel(), (kind, check)


def test_fault_padding_row_written_and_partial_added_twice():
    c = W.CASE_BY_NAME["win-co100"]
    o = W.make_operands(c, 2, "int")
    ref = W.reference(c, o)
    good = o["dw0"].double().clone()
    good[:c.co] += ref["dw"]
    assert W.check_padding_rows(good, c.co) == 0 and W.check_exact(good[:c.co], o["dw0"][:c.co].double() + ref["dw"]) == (0, None)
    assert W.check_padding_rows(W.write_padding_row(good, c), c.co) == 1
    twice = W.add_twice(o["dw0"], ref["dw"], c.co)
    assert W.check_exact(twice[:c.co], good[:c.co])[0] > 0.9 * good[:c.co].numel()
    lost = good.clone()
    lost[:c.co] -= o["dw0"][:c.co].double()     # "=" for "+=": the starting value lost
    assert W.check_exact(lost[:c.co], good[:c.co])[0] > 0.9 * good[:c.co].numel()


@pytest.mark.parametrize("name", ["win-co100", "co130-bf16", "co130-f32", "linear-bf16"])
def test_fault_dbias_over_co_columns(name):
    c = W.CASE_BY_NAME[name]
    for kind, o, ref in _both_kinds(c):
        wrong = W.dbias_over_co(c, o)
        assert W.check_exact(wrong[:c.co], ref["dbias"][:c.co]) == (0, None)
        check = W.check_exact(wrong, ref["dbias"]) if kind == "int" else W.check_bound(wrong, ref["dbias"], ref["Bb"])
        assert check[0] >= 0.8 * (c.co_pad - c.co), (kind, check)


@pytest.fixture(scope="module")
def pool1():
    return {kind: W.make_pool_operands(1, 1, kind) for kind in ("int", "real")}


def test_stem_pool_reference_and_lost_window(pool1):
    for kind, o in pool1.items():
        ref = W.stem_pool_reference(o["g_pool"], o["idx"], o["packed"], kind=kind)
        f32 = W.stem_pool_reference(o["g_pool"], o["idx"], o["packed"], F32, kind=kind)
        wrong = W.stem_pool_reference(o["g_pool"], o["idx"], o["packed"], kind=kind, bwd=W.maxpool_bwd_lost_window)
        if kind == "int":
            assert W.check_exact(f32["dw"], ref["dw"]) == (0, None)
            assert W.check_exact(wrong["dw"], ref["dw"])[0] > 0.9 * ref["dw"].numel()
        else:
            bad, ratio = W.check_bound(f32["dw"], ref["dw"], ref["B"])
            print(f"\n[ratio] pool-1: torch f32 against float64 {ratio:.3g} x B")
            assert bad == 0 and ratio < 0.1
            assert W.check_bound(wrong["dw"], ref["dw"], ref["B"])[0] > 0.5 * ref["dw"].numel()


def test_stem_reference_is_the_7x7_convolution_on_a_packed_frame():
    """The flat-operand definition against torch: on a frame packed by input_grad_oracle.pack_s2d it is conv1's 7 x 7 / stride 2 /
    pad 3 weight gradient, entry by entry (w7_from_operand maps the [64, 4, 4, 16] operand to [64, 3, 7, 7])."""
    import input_grad_oracle as IG
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    frame = torch.randint(-3, 4, (1, 3, 224, 224), generator=g).double()
    gy = torch.randint(-2, 3, (1, 112, 112, 64), generator=g).double()
    c = W.CASE_BY_NAME["stem-1"]
    dw = W.reference(c, {"kind": "int", "x": IG.pack_s2d(frame), "gy": gy})["dw"]
    ref7 = F.grad.conv2d_weight(frame, (64, 3, 7, 7), gy.permute(0, 3, 1, 2), 2, 3)
    assert torch.equal(IG.w7_from_operand(dw.reshape(64, 256)), ref7)
