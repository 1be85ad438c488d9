"""Every epilogue operand combination of vdqn_conv2d on every kernel family, element by element (tests/conv_epilogue_oracle.py).

One test per call of conv_epilogue_oracle.CALLS runs the operand matrix
    forward:        bias x resid x relu x f32 copy x column sums
    data gradient:  bias x resid x mask x f32 copy x column sums
wherever dispatch sends each combination, and checks per call
  (R)  every element of `out` and of the f32 copy against the float64 reference inside the oracle's derived bounds (bf16x3: the gate
       of test_gpu_bf16x3.py), no tensor-maximum normalisation, no element left out (the outputs start as NaN);
  (E1) out == out_f32 rounded to the storage type, wherever both exist;
  (E2) the f32 copy == emulate(acc, operands) EXACTLY, acc being the f32 copy of the same call without epilogue operands (where an
       operand re-routes the call — the profiler tag changes — acc comes from the call with the same operands PRESENT but neutral:
       zero bias, zero residual, all-ones mask; routing depends on which pointers are set, never on their values);
  (E3) the call without the f32 copy (the lean epilogue where a family has one) stores exactly the bits of the call with it;
  (C)  column sums entry by entry against the float64 sum of the stored values of the entry's own rows, the entry count, and
       nothing written behind the last entry;
  the profiler tag the dispatch conditions predict (`route`), so that a dispatch change cannot silently empty a row of the matrix.

Which epilogue serves which operand set (vec = 16-byte rows: ldo % 8 == 0; "whole" = co a multiple of the column tile):
  family                 lean forward                              lean data gradient                 otherwise
  conv64                 —                                         —                                  its own (no f32 copy; forward: no column sums), else -> igemm_win<bf16,64>
  igemm_win / win9       —                                         —                                  igemm_epilogue
  win9u (128 / 256 rows) bias, no f32 / mask / colsum, vec, whole  no bias, no f32, vec, whole        igemm_epilogue
  win9s                  no resid / f32 / mask* / colsum*, vec     —                                  igemm_epilogue (* -> generic kernel)
  win9d                  —                                         always (bias / f32 / !vec -> generic kernel)
  generic 128-row, s2    —                                         bf16: no bias, no f32, vec, whole  igemm_epilogue
  generic otherwise      —                                         —                                  igemm_epilogue
  skinny                 its own (a residual -> generic kernel; features.8: mask / colsum -> generic kernel)
VDQN_LEAN_EPILOGUE=0 turns every lean column into igemm_epilogue (and win9d into the generic kernel).

E3 does not apply where the f32 copy itself changes the routing (E3_EXCLUDED); (R) is the check there.  E2 compares f32-copy calls
with each other, which route alike, so it holds everywhere an f32 copy exists.

Record (MI355X, not a threshold; each test prints its own with pytest -s): largest error / bound over a family's whole matrix.
  f32 copy of the bf16 kernels, of B:  conv64 9e-4, igemm_win<64> 8e-4, three-tap 128 1.1e-3, win9 1.1e-3, win9u 7e-4, win9s 1e-3,
      win9d 6e-4, generic 64 (1x1) 3.8e-3, generic 64 (deep ring) 1.2e-3, generic 128 1.1e-3, generic stride-2 dgrad 3.6e-3,
      skinny linear 2e-3, features.8 2e-4 (LDS 1.2e-4)
  bf16 store, of its bound:            0.29 (features.8, LDS) .. 0.98 (generic 64, 1x1): half an ulp is the whole of it
  f32 kernels, of B:                   igemm_win<f32> 3e-3, generic 1x1 2.4e-2;   bf16x3: 4e-6 .. 5e-6 of the output's max (gate 1e-4)
No combination failed on the kernels as they are; nothing here was tuned on them (bounds: conv_epilogue_oracle.py's derivation,
test_gpu_skinny.py's 1e-5 for column sums, test_gpu_bf16x3.py's gate).

The layout group (test_layouts) passes caller-allocated outputs with ldo > co, rows that are no 16-byte multiples (the scalar path
of igemm_epilogue) and co = 72 / 68 (ragged column tiles) and checks that nothing outside [rows, co) is written."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_epilogue_oracle as E  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 768.0   # exact in bf16 and far from every result
E3_EXCLUDED = {    # family -> why the f32 copy changes the kernel
    "conv64-fwd": "conv64 has no f32 copy: the call goes to igemm_win<bf16,64>",
    "conv64-dgrad": "conv64 has no f32 copy: the call goes to igemm_win<bf16,64>",
    "win9d": "the plane-window data gradient has no f32 copy: the call goes to the generic parity-class tiles",
    "win9d-sib": "as win9d",
    "win9s-64-sib": "the fused forward sibling refuses an f32 copy (VDQN_CHECK)",
    "win9s-192-sib": "the fused forward sibling refuses an f32 copy (VDQN_CHECK)",
}
_seen = {}   # call name -> [max error / bound of the f32 copy, of the bf16 store]: printed per test (pytest -s), a record, not a threshold


def _env(name, default):
    v = os.environ.get(name)
    return default if v is None else int(v)


def vec_ok(c, ldo):
    return (ldo * (2 if c.dtype == "bf16" else 4)) % 16 == 0 and ldo % 8 == 0


def route(c, *, bias, resid, mask, f32, colsum, ldo=None):
    """The profiler tag of the kernel vdqn_conv2d's dispatch (csrc/igemm.hip) gives this call, from the same conditions."""
    ldo = c.co if ldo is None else ldo
    bf, kind = c.dtype == "bf16", {"bf16": "bf16", "f32": "f32", "x3": "bf16x3"}[c.dtype]
    mode = 0 if c.mode == 0 else (2 if c.stride == 2 else 1)
    d = ("fwd", "dgrad", "dgrad_s2")[mode]
    vec = vec_ok(c, ldo)
    lean_on = os.environ.get("VDQN_LEAN_EPILOGUE", "1")[:1] != "0"
    if mode != 2 and bf and not c.sib and not resid and ldo % 4 == 0 and c.co % 4 == 0:     # skinny.hip: vdqn_skinny_kind
        linear = c.r == c.s == 1 and c.hi == c.wi == c.ho == c.wo == 1 and c.stride == 1 and c.pad == 0
        if linear and c.M <= 4096 and c.co % 32 == 0:
            return "skinny<bf16,32x32,dgrad>" if mask else "skinny<bf16,32x32,fwd>"
        valid = c.mode == 0 and c.stride == 1 and c.pad == 0 and c.r * c.s > 1 and c.ho == c.hi - c.r + 1 and c.wo == c.wi - c.s + 1
        if valid and not mask and not colsum and c.co == 64 and c.M <= 65536:
            return "skinny<bf16,conv>"
    win = c.r == c.s == 3 and c.stride == 1 and c.pad == 1 and mode != 2 and c.wo >= 2
    if (bf and win and c.ci == 64 and c.co == 64 and c.hi == c.ho and c.wi == c.wo and c.wo <= 56 and not f32 and vec
            and (mode == 1 or not colsum)):
        return f"conv64<bf16,{d}>"
    if win:   # three-tap windows, igemm_win9 (bf16, 128 columns, wo <= 28) and win9u (... and ci % 128 == 0) share one tag
        return f"igemm_win<{kind},{c.bn},{d}>"
    if (mode == 0 and bf and c.r == c.s == 3 and c.stride == 2 and c.pad == 1 and c.bn == 128 and c.hi == 2 * c.ho and c.wi == 2 * c.wo
            and 2 <= c.wo <= 28 and c.ci % 64 == 0 and not colsum and not mask
            and (not c.sib or (c.ci // 64 in (1, 2, 4) and vec and not f32 and not resid))):
        return "igemm_s2win<bf16,128,fwd>"
    if (mode == 2 and bf and c.r == c.s == 3 and c.pad == 1 and c.ho == 2 * c.hi and c.wo == 2 * c.wi and 2 <= c.wi <= 28 and vec
            and not f32 and not bias and lean_on and c.ci % 128 == 0 and c.co % 64 == 0):
        return f"igemm_s2win<bf16,{c.bn},dgrad>"
    if c.bn == 64 and mode != 2 and c.M >= _env("VDQN_BM256_MIN_ROWS", 256 * 1024) and not c.sib:
        return f"igemm<{kind},256x64,{d}>"
    return f"igemm<{kind},{c.bn},{d}>"


def is_win9u(c, tag):
    """igemm_win<bf16,128,*> is three kernels; win9u takes 128-column bf16 calls of images up to 28 wide with ci % 128 == 0
    (VDQN_WIN9_UNROLLED=0: igemm_win9 takes them, which also takes ci % 128 != 0; wider images: the three-tap igemm_win)."""
    return (tag.startswith("igemm_win<bf16,128") and c.wo <= 28 and c.hi == c.ho and c.wi == c.wo and c.ci % 128 == 0
            and _env("VDQN_WIN9_UNROLLED", 1) != 0)


def colsum_layout(c, tag, *, bias, f32, ldo=None):
    """(rows, order, pair) of the column-sum entries the kernel behind `tag` writes for this call."""
    ldo = c.co if ldo is None else ldo
    if tag.startswith("skinny<bf16,32x32"):
        return 32, "rows", False
    if tag.startswith("igemm_s2win") and tag.endswith("dgrad>"):
        return 128, "win9d", False
    if tag.endswith("dgrad_s2>"):
        equal = c.ho % 2 == 0 and c.wo % 2 == 0 and _env("VDQN_DGRAD_S2_INTERLEAVE", 1) != 0
        return 128, "interleave" if equal else "class", False
    if "256x64" in tag:   # igemm_epilogue on a 256-row tile: the tile's sum in its even entry, zero in the odd one
        return 128, "rows", True
    if is_win9u(c, tag) and _env("VDQN_WIN9_BM256", 3) == 2:
        lean_d = (c.mode == 1 and os.environ.get("VDQN_LEAN_EPILOGUE", "1")[:1] != "0" and vec_ok(c, ldo) and not f32 and not bias
                  and c.co % 128 == 0)
        return 128, "rows", not lean_d   # the lean data-gradient epilogue writes both 128-row halves; igemm_epilogue the pair form
    return 128, "rows", False


class Runner:
    """The operands of one call on the device (pitch ldo: resid / mask share out's) and the call itself."""

    def __init__(self, c, ldo=None, seed=1):
        from video_dqn_amd import _lib
        self._lib = _lib
        self.c, self.ldo = c, c.co if ldo is None else ldo
        self.st = E.STORE_DTYPE[c.dtype]
        self.o = o = E.make_operands(c, seed)
        self.pair = (E.accumulate(c, o), E.accumulate(c, o, absolute=True))
        dev = lambda t: t.to(self.st).to(DEV).contiguous()  # noqa: E731
        self.x, self.wt, self.bias = dev(o["x"]), dev(o["wt"]), o["bias"].to(DEV)
        self.resid, self.mask = dev(self._pitched(o["resid"])), dev(self._pitched(o["mask"]))
        self.zero_bias = torch.zeros_like(self.bias)
        self.zero_resid, self.one_mask = torch.zeros_like(self.resid), torch.ones_like(self.mask)
        self.sib = {}
        if c.sib and c.mode == 0:
            self.sib = dict(wt2=dev(o["wt2"]), bias2=o["bias2"].to(DEV), co2=c.co, relu2=False)
        elif c.sib:
            self.sib = dict(wt2=dev(o["wt2"]), in2=dev(o["x2"]))
        if c.dtype == "x3":   # the one-bf16-pass yardstick of the bf16x3 gate
            ob = dict(o, x=o["x"].to(E.BF16).float(), wt=o["wt"].to(E.BF16).float())
            self.ob, self.pair_b = ob, (E.accumulate(c, ob), self.pair[1])

    def _pitched(self, t):
        p = torch.full(tuple(t.shape[:-1]) + (self.ldo,), 0.5)
        p[..., :self.c.co] = t
        return p

    def run(self, *, bias=False, resid=False, relu=False, mask=False, f32=False, colsum=False, neutral=False, fill=float("nan")):
        """-> dict(out, out_f32, part, out2: CPU tensors or None; tag; n_entries: the entries the layout implies)"""
        from video_dqn_amd import ops
        c = self.c
        tag = route(c, bias=bias, resid=resid, mask=mask, f32=f32, colsum=colsum, ldo=self.ldo)
        rows, order, pair = colsum_layout(c, tag, bias=bias, f32=f32, ldo=self.ldo)
        n_entries = len(E.colsum_rows(c, rows, order))
        shape = (c.n, c.ho, c.wo, self.ldo)
        out = torch.full(shape, fill, dtype=self.st, device=DEV)
        out_f32 = torch.full(shape, fill, dtype=torch.float32, device=DEV) if f32 else None
        part = torch.full((n_entries + 1, self.ldo), fill, dtype=torch.float32, device=DEV) if colsum else None
        got = ops.conv2d(self.x, self.wt, ho=c.ho, wo=c.wo, co=c.co, r=c.r, s=c.s, stride=c.stride, pad=c.pad, mode=c.mode, ldo=self.ldo,
                         bias=(self.zero_bias if neutral else self.bias) if bias else None,
                         resid=(self.zero_resid if neutral else self.resid) if resid else None,
                         mask=(self.one_mask if neutral else self.mask) if mask else None, relu=relu and not neutral,
                         precision="bf16x3" if c.dtype == "x3" else None, out=out, out_f32=out_f32, colsum=part, **self.sib)
        torch.cuda.synchronize()
        prof = {k: v["launches"] for k, v in self._lib.profile_collect().items()}
        out2 = got[1].cpu() if (c.sib and c.mode == 0) else None
        return dict(out=out.cpu(), out_f32=None if out_f32 is None else out_f32.cpu(), part=None if part is None else part.cpu(), out2=out2,
                    tag=tag, prof=prof, layout=(rows, order, pair), n_entries=n_entries)


def _check_call(rn, res, fl, fails, what):
    """(R), (E1), (C) and the tag of one call; columns >= co are the caller's."""
    c, co = rn.c, rn.c.co
    if res["prof"] != {res["tag"]: 1}:
        fails.append(f"{what}: ran {res['prof']}, dispatch predicts {res['tag']}")
    ref, S, B = E.reference(c, rn.o, pair=rn.pair, bias=fl["bias"], resid=fl["resid"], relu=fl["relu"], mask=fl["mask"])
    out = res["out"][..., :co]
    seen = _seen.setdefault(c.name, [0.0, 0.0])
    if c.dtype == "x3":
        ref_b = E.reference(c, rn.ob, pair=rn.pair_b, bias=fl["bias"], resid=fl["resid"], relu=fl["relu"], mask=fl["mask"])[0]
        for name, t in (("out", out), ("out_f32", res["out_f32"])):
            if t is not None:
                e3, e1, ok = E.x3_gate(t[..., :co], ref, ref_b)
                seen[0] = max(seen[0], e3)
                if not ok or not torch.isfinite(t[..., :co]).all():
                    fails.append(f"{what}: (R) {name} bf16x3 gate: error {e3:.3g} of max, one bf16 pass {e1:.3g}")
    else:
        if res["out_f32"] is not None:
            bad, ratio = E.check_f32(res["out_f32"][..., :co], ref, B)
            seen[0] = max(seen[0], ratio)
            if bad:
                fails.append(f"{what}: (R) f32 copy: {bad} elements outside B, worst {ratio:.3g} x B")
        bad, ratio = (E.check_bf16 if c.dtype == "bf16" else E.check_f32)(out, ref, B)
        seen[1] = max(seen[1], ratio)
        if bad:
            fails.append(f"{what}: (R) store: {bad} elements outside the bound, worst {ratio:.3g} x bound")
    if res["out_f32"] is not None and not E.store_is_rounded(out, res["out_f32"][..., :co]):
        fails.append(f"{what}: (E1) out != out_f32 rounded to the storage type")
    if res["part"] is not None:
        rows, order, pair = res["layout"]
        exp = E.colsum_expected(out, c, rows, order, pair)
        bad = E.check_colsum(res["part"][:res["n_entries"], :co], exp)
        if bad:
            fails.append(f"{what}: (C) entries (rows {rows}, {order}{', pair' if pair else ''}) off: {bad[:6]}")
    return ref, B


def _untouched(t, co, fill):
    return bool((t[..., co:] == fill).all()) if fill == fill else bool(torch.isnan(t[..., co:]).all())


def _flags(c, combo):
    bias, resid, third, f32, colsum = combo
    return dict(bias=bias, resid=resid, relu=third and c.mode == 0, mask=third and c.mode == 1, f32=f32, colsum=colsum)


def _name(fl):
    return "+".join(k for k, v in fl.items() if v) or "none"


@pytest.fixture(autouse=True)
def _profiler():
    from video_dqn_amd import _lib
    _lib.profile_enable(True)
    yield
    _lib.profile_enable(False)


@pytest.mark.parametrize("c", E.CALLS, ids=lambda c: c.name)
def test_operand_matrix(c):
    from video_dqn_amd import _lib
    rn = Runner(c)
    fails, results = [], {}
    sib_fwd = c.sib and c.mode == 0
    for combo in itertools.product((False, True), repeat=5):
        fl = _flags(c, combo)
        what = f"{c.name}[{_name(fl)}]"
        if sib_fwd and (fl["f32"] or fl["colsum"]):   # the one refusal of the matrix: by name, not a wrong result
            with pytest.raises(_lib.VdqnError, match="fused sibling"):
                rn.run(**fl)
            continue
        res = results[combo] = rn.run(**fl)
        _check_call(rn, res, fl, fails, what)
        if res["part"] is not None and not torch.isnan(res["part"][res["n_entries"]:]).all():
            fails.append(f"{what}: (C) entries behind the last one were written")
        if sib_fwd:   # the sibling's own output: conv1x1 / stride 2 + bias2
            ref2, _, B2 = E.epilogue64(E.sibling_forward(c, rn.o), E.sibling_forward(c, rn.o, absolute=True), c.ci, bias=rn.o["bias2"])
            bad, ratio = E.check_bf16(res["out2"], ref2, B2)
            if bad:
                fails.append(f"{what}: (R) out2: {bad} elements outside the bound, worst {ratio:.3g} x bound")
    # (E2): exact epilogue on the f32-copy calls
    base = results.get((False, False, False, True, False))
    neutral = {}
    for combo, res in results.items():
        if not combo[3]:
            continue
        fl = _flags(c, combo)
        acc = base["out_f32"]
        if res["tag"] != base["tag"]:   # an operand re-routed the call: the same operands present, neutral values
            key = (combo[0], combo[1], fl["mask"], combo[4])
            if key not in neutral:
                neutral[key] = rn.run(**dict(fl, relu=False), neutral=True)
                if neutral[key]["tag"] != res["tag"]:
                    fails.append(f"{c.name}[{_name(fl)}]: neutral call routed to {neutral[key]['tag']}")
            acc = neutral[key]["out_f32"]
        emu = E.emulate(acc, bias=rn.o["bias"][:c.co] if fl["bias"] else None, resid=rn.o["resid"].to(rn.st) if fl["resid"] else None,
                        relu=fl["relu"], mask=rn.o["mask"] if fl["mask"] else None)
        if not torch.equal(res["out_f32"], emu):
            n = int((res["out_f32"] != emu).sum())
            fails.append(f"{c.name}[{_name(fl)}]: (E2) f32 copy != emulate(acc) on {n} elements")
        if not torch.equal(res["out"].float(), emu.to(rn.st).float()):
            fails.append(f"{c.name}[{_name(fl)}]: (E2) out != rounded emulate(acc)")
    # (E3): the variant without the f32 copy stores the same bits
    if c.name not in E3_EXCLUDED:
        for combo, res in results.items():
            if combo[3]:
                continue
            twin = results[combo[:3] + (True,) + combo[4:]]
            fl = _flags(c, combo)
            if twin["tag"] != res["tag"]:
                fails.append(f"{c.name}[{_name(fl)}]: (E3) the f32 copy re-routes {res['tag']} -> {twin['tag']}: list the family in E3_EXCLUDED")
            elif not torch.equal(res["out"].float(), twin["out"].float()):
                n = int((res["out"].float() != twin["out"].float()).sum())
                fails.append(f"{c.name}[{_name(fl)}]: (E3) {n} stored elements differ from the call with the f32 copy")
            ne = res["n_entries"]
            if res["part"] is not None and res["layout"] == twin["layout"] and not torch.equal(res["part"][:ne, :c.co], twin["part"][:ne, :c.co]):
                fails.append(f"{c.name}[{_name(fl)}]: (E3) column sums differ from the call with the f32 copy")
    print(f"\n[ratio] {c.name}: f32 copy {_seen[c.name][0]:.3g}, store {_seen[c.name][1]:.3g} "
          f"({'error / max, bf16x3 gate' if c.dtype == 'x3' else 'largest error / bound'}); kernels: {sorted({r['tag'] for r in results.values()})}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


# ---- layouts ----
LAYOUT_FAMILIES = ["win9u", "win64", "gen64-1x1", "f32-gen-1x1", "skinny-linear"]
LAYOUTS = ["ldo+8", "ldo+4", "co72", "co68"]   # co68: ldo = 68, no 16-byte rows AND ragged columns inside a lane's channels


def _layout_call(c, layout):
    if layout == "ldo+8":
        return c, c.co + 8
    if layout == "ldo+4":
        return c, c.co + 4
    co = 72 if layout == "co72" else 68
    return E.with_co(c, co), co


def _layout_sets(c):
    if c.mode == 0:
        return [dict(bias=True, resid=True, relu=True, f32=True, colsum=True), dict(bias=True, resid=True, relu=True),
                dict(f32=True), dict(relu=True, colsum=True)]
    return [dict(bias=True, resid=True, mask=True, f32=True, colsum=True), dict(resid=True, mask=True, colsum=True),
            dict(f32=True), dict(mask=True)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("family", LAYOUT_FAMILIES)
def test_layouts(family, mode, layout):
    """Caller-allocated outputs filled with a sentinel: (R), (E1), (C) on columns < co, the sentinel on columns >= co of every row
    and entry, and on the entry behind the last."""
    c, ldo = _layout_call(E.CALL_BY_NAME[f"{family}-{mode}"], layout)
    rn = Runner(c, ldo=ldo, seed=2)
    fails = []
    for fs in _layout_sets(c):
        fl = dict(dict(bias=False, resid=False, relu=False, mask=False, f32=False, colsum=False), **fs)
        what = f"{c.name}/ldo{ldo}[{_name(fl)}]"
        res = rn.run(**fl, fill=SENTINEL)
        _check_call(rn, res, fl, fails, what)
        for name in ("out", "out_f32", "part"):
            t = res[name]
            if t is not None and not _untouched(t.float(), c.co, SENTINEL):
                fails.append(f"{what}: {name} columns >= co were written")
        if res["part"] is not None and not (res["part"][res["n_entries"]:] == SENTINEL).all():
            fails.append(f"{what}: (C) entries behind the last one were written")
    print(f"\n[ratio] {c.name}/ldo{ldo}: f32 copy {_seen[c.name][0]:.3g}, store {_seen[c.name][1]:.3g}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


def test_conv2d_refuses_wrong_caller_outputs():
    from video_dqn_amd import ops
    c = E.CALL_BY_NAME["gen64-1x1-fwd"]
    rn = Runner(c)
    kw = dict(ho=c.ho, wo=c.wo, co=c.co, r=1, s=1, stride=1, pad=0)
    with pytest.raises(ValueError, match="out must be"):
        ops.conv2d(rn.x, rn.wt, out=torch.empty((c.n, c.ho, c.wo, c.co + 8), dtype=rn.st, device=DEV), **kw)
    with pytest.raises(ValueError, match="out_f32 must be"):
        ops.conv2d(rn.x, rn.wt, out_f32=torch.empty((c.n, c.ho, c.wo, c.co), dtype=rn.st, device=DEV), **kw)
    with pytest.raises(ValueError, match="colsum must be"):
        ops.conv2d(rn.x, rn.wt, colsum=torch.empty((2, c.co), dtype=torch.float32, device=DEV), **kw)   # M = 300: three entries
    out, out_f32, part = ops.conv2d(rn.x, rn.wt, want_f32=True, out=torch.empty((c.n, c.ho, c.wo, c.co), dtype=rn.st, device=DEV), **kw)
    assert part is None and out_f32 is not None and torch.equal(out, ops.conv2d(rn.x, rn.wt, **kw))


# ---- the same file under the A/B switches that change an epilogue or a tile (child processes, test_conv_256_row_tile_variant's way) ----
def _rerun(env, k):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", k],
                       env=dict(os.environ, **env), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-6000:]


@pytest.mark.parametrize("env", [
    {"VDQN_WIN9_BM256": "2"},        # win9u on 256-row tiles: M = 300 is one full tile and a tile with its first 128-row half only
    {"VDQN_LEAN_EPILOGUE": "0"},     # every lean epilogue off: (E3) compares shared with shared, (R) and (E2) still hold
    pytest.param({"VDQN_BM256_MIN_ROWS": "256"}, marks=pytest.mark.variants),   # the 64-column generic calls on 256 x 64 tiles
    pytest.param({"VDQN_SKINNY_CONV_CFG": "9"}, marks=pytest.mark.variants),    # features.8 on the global-memory kernel at every ci
    pytest.param({"VDQN_WIN9_UNROLLED": "0"}, marks=pytest.mark.variants),      # the win9u calls on igemm_win9
], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_rerun_under_switch(env):
    _rerun(env, "not rerun")
