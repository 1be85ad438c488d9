"""tests/conv_epilogue_oracle.py without a GPU: (a) on every family shape the epilogue emulation on a torch-f32 accumulator lies
inside the oracle's bounds against the float64 reference — so a GPU failure of those bounds is the kernel's, not the reference's;
(b) each planted fault, applied to the emulated result, violates the checks on at least one element — so the checks can see them."""
import pytest
import torch

import conv_epilogue_oracle as E

BF16 = torch.bfloat16
_ratios = {}


def _flag_sets(c):
    third = "relu" if c.mode == 0 else "mask"
    return [dict(), dict(bias=True, resid=True, **{third: True}), dict(resid=True), dict(bias=True, **{third: True})]


def _emulated(c, o, acc32, fl):
    return E.emulate(acc32, bias=o["bias"][:c.co] if fl.get("bias") else None, resid=o["resid"] if fl.get("resid") else None,
                     relu=fl.get("relu", False), mask=o["mask"] if fl.get("mask") else None)


@pytest.mark.parametrize("c", E.CALLS, ids=lambda c: c.name)
def test_reference_alone_is_inside_the_bounds(c):
    o = E.make_operands(c)
    pair = (E.accumulate(c, o), E.accumulate(c, o, absolute=True))
    acc32 = E.accumulate(c, o, torch.float32)
    if c.dtype == "x3":
        ob = dict(o, x=o["x"].to(BF16).float(), wt=o["wt"].to(BF16).float())
        if "x2" in o:
            ob["x2"], ob["wt2"] = o["x2"].to(BF16).float(), o["wt2"].to(BF16).float()
        pair_b = (E.accumulate(c, ob), pair[1])
    for fl in _flag_sets(c):
        ref, S, B = E.reference(c, o, pair=pair, **fl)
        emu = _emulated(c, o, acc32, fl)
        if c.dtype == "x3":
            e3, e1, ok = E.x3_gate(emu, ref, E.reference(c, ob, pair=pair_b, **fl)[0])
            assert ok, (fl, e3, e1)
            continue
        bad, ratio = E.check_f32(emu, ref, B)
        assert bad == 0, (fl, bad, ratio)
        _ratios[c.name] = max(_ratios.get(c.name, 0.0), ratio)   # (summation-order error: a small fraction of K * 2^-23 * S)
        if c.dtype == "bf16":
            bad, ratio = E.check_bf16(emu.to(BF16), ref, B)
            assert bad == 0 and ratio <= 1.0, (fl, bad, ratio)
            assert E.store_is_rounded(emu.to(BF16), emu)
    if c.sib and c.mode == 0:   # the sibling's own output
        ref2, _, B2 = E.epilogue64(E.sibling_forward(c, o), E.sibling_forward(c, o, absolute=True), c.ci, bias=o["bias2"])
        emu2 = E.emulate(E.sibling_forward(c, o, torch.float32), bias=o["bias2"])
        assert E.check_f32(emu2, ref2, B2)[0] == 0 and E.check_bf16(emu2.to(BF16), ref2, B2)[0] == 0


# ---- (b) planted faults ----
FWD = E.CALL_BY_NAME["win9u-fwd"]      # M = 300: rows 256 .. 299 are the ragged tile; 256 columns: two column tiles
DGR = E.CALL_BY_NAME["win9u-dgrad"]
FL_F = dict(bias=True, resid=True, relu=True)
FL_D = dict(resid=True, mask=True)


@pytest.fixture(scope="module")
def fwd_case():
    o = E.make_operands(FWD)
    ref, S, B = E.reference(FWD, o, **FL_F)
    return o, E.accumulate(FWD, o, torch.float32), ref, B


@pytest.fixture(scope="module")
def dgr_case():
    o = E.make_operands(DGR)
    ref, S, B = E.reference(DGR, o, **FL_D)
    return o, E.accumulate(DGR, o, torch.float32), ref, B


def _caught(emu, ref, B):
    """the two reference checks (R) on a faulty f32 copy and its bf16 store"""
    n32, _ = E.check_f32(emu, ref, B)
    n16, _ = E.check_bf16(emu.to(BF16), ref, B)
    return n32, n16


def test_the_unfaulted_emulation_passes(fwd_case, dgr_case):
    for c, (o, acc, ref, B), fl in ((FWD, fwd_case, FL_F), (DGR, dgr_case, FL_D)):
        assert _caught(_emulated(c, o, acc, fl), ref, B) == (0, 0)


def test_fault_one_tap_dropped_on_the_last_image_row(fwd_case):
    o, acc, ref, B = fwd_case
    w1 = torch.zeros_like(o["wt"])
    w1[:, 0, 0] = o["wt"][:, 0, 0]                      # the tap (kr, ks) = (0, 0) alone
    tap = E.conv(FWD, o["x"], w1, torch.float32)
    bad = acc.clone()
    bad[-1, -1] -= tap[-1, -1]                          # last image, last row: 6 pixels x 256 channels
    n32, n16 = _caught(_emulated(FWD, o, bad, FL_F), ref, B)
    assert n32 > 0 and n16 > 0
    # ... and one dropped tap is far outside the bound, not marginally: the median over the hit elements that survive the ReLU
    d = (tap[-1, -1].double().abs() / B[-1, -1])[ref[-1, -1] > 0]
    assert d.median().item() > 8


def test_fault_residual_skipped_on_the_ragged_tile(fwd_case):
    o, acc, ref, B = fwd_case
    res = o["resid"].clone()
    res.view(FWD.M, -1)[FWD.M // 128 * 128:] = 0
    emu = E.emulate(acc, bias=o["bias"][:FWD.co], resid=res, relu=True)
    n32, n16 = _caught(emu, ref, B)
    assert n32 > 0 and n16 > 0
    # only ragged rows are hit
    err = (emu.double() - ref).abs().view(FWD.M, -1)
    assert (err[:FWD.M // 128 * 128] <= B.view(FWD.M, -1)[:FWD.M // 128 * 128]).all()


def test_fault_relu_skipped(fwd_case):
    o, acc, ref, B = fwd_case
    n32, n16 = _caught(_emulated(FWD, o, acc, dict(bias=True, resid=True)), ref, B)
    assert n32 > 0 and n16 > 0


def test_fault_mask_from_the_neighbouring_channel(dgr_case):
    o, acc, ref, B = dgr_case
    emu = E.emulate(acc, resid=o["resid"], mask=o["mask"].roll(1, dims=-1))
    n32, n16 = _caught(emu, ref, B)
    assert n32 > 0 and n16 > 0


def test_fault_bias_shifted_by_one_column(fwd_case):
    o, acc, ref, B = fwd_case
    emu = E.emulate(acc, bias=o["bias"][:FWD.co].roll(1), resid=o["resid"], relu=True)
    n32, n16 = _caught(emu, ref, B)
    assert n32 > 0 and n16 > 0


def test_fault_column_sum_entries_of_a_256_row_tile_swapped(dgr_case):
    o, acc, ref, B = dgr_case
    stored = _emulated(DGR, o, acc, FL_D).to(BF16)
    exp = E.colsum_expected(stored, DGR)                # three entries: rows 0-127, 128-255, 256-299
    assert exp.shape == (3, DGR.co)
    part = exp.float()
    assert E.check_colsum(part, exp) == []
    swapped = part[[1, 0, 2]]
    assert swapped.sum(0).sub(part.sum(0)).abs().max().item() < 1e-4   # what the suite compared before: the total is unchanged
    assert [e for e, _ in E.check_colsum(swapped, exp)] == [0, 1]
    # the shared epilogue's layout on 256-row tiles: the tile's sum in the even entry, zero in the odd one
    pair = E.colsum_expected(stored, DGR, pair=True)
    assert torch.equal(pair[1], torch.zeros(DGR.co, dtype=torch.float64)) and torch.allclose(pair[0], exp[0] + exp[1]) and torch.equal(pair[2], exp[2])
    assert E.check_colsum(part, pair) != []
    assert E.check_colsum(part[:2], exp) != []          # a wrong entry count


def test_fault_store_truncated_instead_of_rounded(fwd_case):
    o, acc, ref, B = fwd_case
    emu = _emulated(FWD, o, acc, FL_F)
    trunc = (emu.view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)   # drop the low 16 bits: round toward zero
    assert not E.store_is_rounded(trunc, emu)           # E1 / E2
    assert E.store_is_rounded(emu.to(BF16), emu)
    assert E.check_bf16(trunc, ref, B)[0] > 0           # and (R): truncation is off by up to a whole ulp, the bound allows half


def test_stride2_column_sum_orders_cover_every_pixel_once():
    for name, orders in (("gen-s2-3x3", ["class"]), ("win9d", ["class", "interleave", "win9d"])):
        c = E.CALL_BY_NAME[name]
        for order in orders:
            idx = torch.cat(E.colsum_rows(c, 128, order))
            assert torch.equal(idx.sort().values, torch.arange(c.M)), (name, order)
    c = E.CALL_BY_NAME["win9d"]                           # 5 x 6 x 6 = 180 rows per class: two tiles each, eight entries
    rows = E.colsum_rows(c, 128, "win9d")
    assert len(rows) == 8 and int(rows[0][0]) == c.wo + 1 and int(rows[3][0]) == 0   # entry 0: class (1, 1); entry 3: class (0, 0)
    assert int(E.colsum_rows(c, 128, "interleave")[1][0]) == 1                       # entry 1: class (0, 1)


def test_emulate_is_the_documented_order():
    acc = torch.tensor([1e8, -3.0, 0.5, -0.0], dtype=torch.float32)
    b = torch.tensor([1.0, 1.0, -1.0, 0.0])
    r = torch.tensor([-1e8, 1.0, 0.25, 0.0])
    m = torch.tensor([1.0, 1.0, -0.0, 1.0])
    out = E.emulate(acc, bias=b, resid=r, relu=True, mask=m)
    assert out.tolist() == [0.0, 0.0, 0.0, 0.0]          # (1e8 + 1) + -1e8 = 0 in f32: bias first, then the residual
    assert E.emulate(acc, bias=b, resid=r).tolist() == [0.0, -1.0, -0.25, 0.0]
