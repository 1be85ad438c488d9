"""Every weight-gradient kernel element by element, exact on integer operands (tests/wgrad_oracle.py).

One test per case of wgrad_oracle.CASES (vdqn_conv2d_wgrad) and per n of POOL_N (vdqn_stem_wgrad_pool).  Each runs, with the
profiler on and the launches asserted ({tag: 1}, plus colsum for the bias gradient and wgrad_reduce in the ordered mode):
  1. integer pass, atomic mode: dw starts as random integers in rows < co and the sentinel 768 in rows >= co, dbias as random
     integers; afterwards dw[:co] == dw0 + ref and dbias == dbias0 + ref exactly (torch.equal, no tolerance) and the rows >= co
     still hold the sentinel, although gy's padding columns are not zero;
  2. integer pass, ordered mode: a workspace of exactly the reported size plus a 4 KiB guard, every byte 0xFF; the same bits as 1 and
     an unchanged guard: no unwritten copy is read (a NaN would show), nothing is written behind the reported size;
  3. the batch in two calls (images [0, n // 2) and [n // 2, n)) into one dw / dbias: the bits of the single call (dw +=);
  4. real-valued pass on fresh zeros: atomic and ordered results inside B per element (bf16x3: x3_gate), ordered twice bit-identical,
     dbias inside its bound; the largest error / B is printed (pytest -s).

Which kernel serves which case (the tag is asserted; wgrad_oracle.plan restates plan_wgrad of csrc/wgrad.hip):
  wgrad_win<bf16,64>      win-*: 3x3 / stride 1 / pad 1, bf16, pix_stride == ci, wo >= 2, ho * wo <= 3200
  wgrad<bf16,128>         gen-58x56 (3248 table bytes), s2-14x9-bf16
  wgrad<bf16,64>          gen-pix128, gen-w1, s2-odd-bf16, ds-bf16 (VDQN_WGRAD_DS64), ds-odd-bf16, valid-bf16, linear-bf16, co130-bf16,
                          s2-odd-n8-bf16, ds-odd-n8-bf16, valid-n8-bf16, gen-w1-5x1, stem-1-k1 (an explicit splitk keeps the stem
                          kernel away)
  wgrad<f32,64>           s2-odd-f32, valid-f32, linear-f32, co130-f32, 5x17-f32, 10x6-f32, 10x6-k5-f32, stem-1-f32
  wgrad<f32,128>          s2-14x9-f32, ds-f32, l4-f32
  wgrad<bf16x3,64 / 128>  the x3 twins of the f32 cases
  wgrad_stem<bf16>        stem-1, stem-5, stem-10 (1, 2, 3 rows per block)
  wgrad_stem_pool<bf16>   pool-1, pool-10, pool-19 (1, 2, 3 pooled-row pairs per block)
  wgrad_reduce            every ordered-mode call;   colsum   every call with a dbias (24 / 48 column groups: co130-*)
test_rerun_under_switch repeats the file under VDQN_WGRAD_WINDOW=0, VDQN_WGRAD_STEM=0, VDQN_WGRAD_DS64=0 and other automatic splits
(marked `variants`).

Beyond the issue's list, four bf16 cases (s2-odd-n8, ds-odd-n8, valid-n8, gen-w1-5x1) repeat geometries at M > 128: the bf16 64-wide
tiles stage 128 pixels per K-step, so at M <= 128 the slot advances (adv_*, car_ow, car_oh) are computed and never used.

Record (MI355X, not a threshold; each test prints its own with pytest -s): largest error / B of the real-valued pass per family.
  wgrad_win<bf16,64>     3.7e-5 (win-57x56, 13 splits) .. 3.2e-3 (win-ldg192); win-2x2 2.5e-2 (M = 28)
  wgrad<bf16,64>         1.1e-3 (valid-n8) .. 1.7e-2 (co130), gen-w1 2.2e-2 (M = 20); stem-1-k1 1.7e-5
  wgrad<bf16,128>        4.1e-5 (gen-58x56, 13 splits), 5.8e-3 (s2-14x9)
  wgrad<f32,64>          3.7e-3 (10x6-k5) .. 5.4e-2 (co130, M = 32); stem-1-f32 1.2e-5 (49 splits)
  wgrad<f32,128>         1.9e-2 (s2-14x9) .. 2.4e-2 (l4)
  wgrad<bf16x3,*>        3.6e-6 .. 5.2e-6 of the output's max (gate 1e-4)
  wgrad_stem<bf16>       1.7e-5 (stem-1), 2.1e-6 (stem-5), 7.5e-7 (stem-10)
  wgrad_stem_pool<bf16>  2.1e-5 (pool-1), 1.5e-6 (pool-10), 5.2e-7 (pool-19)
  colsum                 at most 1.2e-2 of its bound (linear-x3)
Every integer pass was bit-equal to the reference in atomic, ordered and two-call form on the kernels as they are, under the four
switch variants too; no case failed, nothing here was tuned on the kernels.  The slowest tests: pool-19 1.1 s, stem-10 0.6 s,
pool-10 0.5 s, win-2x2 0.4 s (the first launch), all others under 0.2 s."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import wgrad_oracle as W  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


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


def _dev(t, dtype):
    return t.to(W.STORE_DTYPE[dtype]).to(DEV).contiguous()


def _guarded(nbytes):
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)


def _guard_ok(ws, nbytes):
    return bool((ws[nbytes:] == 0xFF).all())


class Runner:
    def __init__(self, c, kind):
        self.c, self.kind = c, kind
        self.o = W.make_operands(c, 1, kind)
        self.ref = W.reference(c, self.o)
        self.gy, self.x = _dev(self.o["gy"], c.dtype), _dev(self.o["x"], c.dtype)
        self.kw = dict(co=c.co, r=c.r, s=c.s, stride=c.stride, pad=c.pad, ci=c.ci, pix_stride=c.pix_stride, splitk=c.splitk,
                       precision="bf16x3" if c.dtype == "x3" else None)

    def call(self, fails, what, *, dw=None, dbias=None, workspace=None, deterministic=False, images=None, tag=None):
        """One vdqn_conv2d_wgrad -> (dw, dbias) on the CPU; the launches are held against `tag` (None: not asserted)."""
        from video_dqn_amd import ops
        gy, x = (self.gy, self.x) if images is None else (self.gy[images[0]:images[1]], self.x[images[0]:images[1]])
        dw, db = ops.conv2d_wgrad(gy, x, dw=dw, dbias=dbias, workspace=workspace, deterministic=deterministic, want_dbias=True, **self.kw)
        ran = _launches()
        if tag is not None:
            want = {tag: 1, "colsum": 1}
            if deterministic or workspace is not None:
                want["wgrad_reduce"] = 1
            if ran != want:
                fails.append(f"{what}: ran {ran}, the plan predicts {want}")
        return dw.cpu(), db.cpu()

    def start(self):
        return self.o["dw0"].to(DEV), self.o["dbias0"].to(DEV)


def _exact(fails, what, got, expected):
    bad, first = W.check_exact(got, expected)
    if bad:
        fails.append(f"{what}: {bad} of {expected.numel()} elements differ, first at {first}: got {got[first].item() if isinstance(first[0], int) else '?'}"
                     f", expected {expected[first].item() if isinstance(first[0], int) else '?'}")


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.name)
def test_case(c):
    from video_dqn_amd import ops
    pl = W.plan(c)
    fails = []
    st = torch.bfloat16 if c.dtype == "bf16" else torch.float32
    nbytes = ops.conv2d_wgrad_workspace_bytes(n=c.n, hi=c.hi, wi=c.wi, ci=c.ci, ho=c.ho, wo=c.wo, co=c.co, r=c.r, s=c.s, stride=c.stride,
                                              pad=c.pad, dtype=st, precision="bf16x3" if c.dtype == "x3" else None, ldg=c.ldg,
                                              pix_stride=c.pix_stride, splitk=c.splitk)
    assert nbytes == pl["bytes"], (nbytes, pl)

    # ---- integer passes ----
    rn = Runner(c, "int")
    exp_dw = rn.o["dw0"][:c.co].double() + rn.ref["dw"]
    exp_db = rn.o["dbias0"].double() + rn.ref["dbias"]
    # 1. atomic mode
    dw0, db0 = rn.start()
    dw_a, db_a = rn.call(fails, "int/atomic", dw=dw0, dbias=db0, tag=pl["tag"])
    _exact(fails, "int/atomic dw", dw_a[:c.co], exp_dw)
    _exact(fails, "int/atomic dbias", db_a, exp_db)
    if W.check_padding_rows(dw_a, c.co):
        fails.append(f"int/atomic: {W.check_padding_rows(dw_a, c.co)} elements of the rows >= co were written")
    # 2. ordered mode, guarded workspace full of NaN
    dw0, db0 = rn.start()
    ws = _guarded(nbytes)
    dw_o, db_o = rn.call(fails, "int/ordered", dw=dw0, dbias=db0, workspace=ws, tag=pl["tag"])
    _exact(fails, "int/ordered dw", dw_o[:c.co], exp_dw)
    _exact(fails, "int/ordered dbias", db_o, exp_db)
    if not torch.equal(dw_o, dw_a) or not torch.equal(db_o, db_a):
        fails.append("int/ordered: not the bits of the atomic mode")
    if not _guard_ok(ws, nbytes):
        fails.append(f"int/ordered: the guard behind the {nbytes} workspace bytes was written")
    # 3. the batch in two calls into one dw
    if c.n >= 2:
        n1 = c.n // 2
        dw0, db0 = rn.start()
        rn.call(fails, "int/two calls", dw=dw0, dbias=db0, images=(0, n1))
        dw_t, db_t = rn.call(fails, "int/two calls", dw=dw0, dbias=db0, images=(n1, c.n))
        if not torch.equal(dw_t, dw_a) or not torch.equal(db_t, db_a):
            fails.append(f"int/two calls: images [0, {n1}) and [{n1}, {c.n}) into one dw are not the bits of the single call")
        dw0, db0 = rn.start()
        rn.call(fails, "int/two ordered calls", dw=dw0, dbias=db0, images=(0, n1), deterministic=True)
        dw_t, db_t = rn.call(fails, "int/two ordered calls", dw=dw0, dbias=db0, images=(n1, c.n), deterministic=True)
        if not torch.equal(dw_t, dw_a) or not torch.equal(db_t, db_a):
            fails.append("int/two ordered calls: not the bits of the single call")

    # ---- 4. real-valued pass ----
    rr = Runner(c, "real")
    ref = rr.ref
    dw_a, db_a = rr.call(fails, "real/atomic", tag=pl["tag"])
    dw_o, db_o = rr.call(fails, "real/ordered", deterministic=True, tag=pl["tag"])
    dw_p, db_p = rr.call(fails, "real/ordered again", workspace=_guarded(nbytes), tag=pl["tag"])
    if not torch.equal(dw_o, dw_p) or not torch.equal(db_o, db_p):
        fails.append("real/ordered: two runs differ")
    worst = 0.0
    for mode, dw, db in (("atomic", dw_a, db_a), ("ordered", dw_o, db_o)):
        if float(dw[c.co:].abs().max() if c.co < c.co_pad else 0.0) != 0.0:
            fails.append(f"real/{mode}: rows >= co of a zero dw are not zero")
        if c.dtype == "x3":
            ob = dict(rr.o, x=rr.o["x"].to(W.BF16).float(), gy=rr.o["gy"].to(W.BF16).float())
            e3, e1, ok = W.x3_gate(dw[:c.co], ref["dw"], W.reference(c, ob)["dw"])
            worst = max(worst, e3)
            if not ok or not torch.isfinite(dw).all():
                fails.append(f"real/{mode}: bf16x3 gate: error {e3:.3g} of max, one bf16 pass {e1:.3g}")
        else:
            bad, ratio = W.check_bound(dw[:c.co], ref["dw"], ref["B"])
            worst = max(worst, ratio)
            if bad:
                fails.append(f"real/{mode}: {bad} elements of dw outside B, worst {ratio:.3g} x B")
        bad, ratio_b = W.check_bound(db, ref["dbias"], ref["Bb"])
        if bad:
            fails.append(f"real/{mode}: {bad} elements of dbias outside the bound, worst {ratio_b:.3g} x")
    print(f"\n[ratio] {c.name}: {pl['tag']} splitk {pl['splitk']} copies {pl['copies']}: "
          f"{'error / max (bf16x3 gate 1e-4)' if c.dtype == 'x3' else 'largest error / B'} {worst:.3g}, dbias {ratio_b:.3g} x its bound")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


@pytest.mark.parametrize("n", W.POOL_N, ids=lambda n: f"pool-{n}")
def test_stem_pool(n):
    from video_dqn_amd import _lib, ops
    lib = _lib.load()
    ppb, bpi, nbytes = W.stem_pool_grid(n)
    assert lib.vdqn_stem_wgrad_pool_workspace_bytes(n) == nbytes
    tag, fails = "wgrad_stem_pool<bf16>", []

    def call(what, o, ordered=False, images=None, **kw):
        a, b = (0, n) if images is None else images
        dw = ops.stem_wgrad_pool(o["dg"][a:b], o["di"][a:b], o["dp"][a:b], **kw)
        ran = _launches()
        want = {tag: 1, "wgrad_reduce": 1} if ordered else {tag: 1}
        if ran != want:
            fails.append(f"{what}: ran {ran}, expected {want}")
        return dw.cpu()

    def operands(kind):
        o = W.make_pool_operands(n, 1, kind)
        o["dg"], o["di"], o["dp"] = _dev(o["g_pool"], "bf16"), o["idx"].to(DEV), _dev(o["packed"], "bf16")
        return o, W.stem_pool_reference(o["g_pool"], o["idx"], o["packed"], kind=kind)

    o, ref = operands("int")
    exp = o["dw0"].double() + ref["dw"]
    dw_a = call("int/atomic", o, dw=o["dw0"].to(DEV))
    _exact(fails, "int/atomic dw", dw_a, exp)
    ws = _guarded(nbytes)
    dw_o = call("int/ordered", o, ordered=True, dw=o["dw0"].to(DEV), workspace=ws)
    _exact(fails, "int/ordered dw", dw_o, exp)
    if not _guard_ok(ws, nbytes):
        fails.append(f"int/ordered: the guard behind the {nbytes} workspace bytes was written")
    if n >= 2:
        n1, dw0 = n // 2, o["dw0"].to(DEV)
        call("int/two calls", o, images=(0, n1), dw=dw0)
        _exact(fails, "int/two calls dw", call("int/two calls", o, images=(n1, n), dw=dw0), exp)
    del o
    o, ref = operands("real")
    dw_a = call("real/atomic", o)
    dw_o = call("real/ordered", o, ordered=True, deterministic=True)
    dw_p = call("real/ordered again", o, ordered=True, workspace=_guarded(nbytes))
    if not torch.equal(dw_o, dw_p):
        fails.append("real/ordered: two runs differ")
    worst = 0.0
    for mode, dw in (("atomic", dw_a), ("ordered", dw_o)):
        bad, ratio = W.check_bound(dw, ref["dw"], ref["B"])
        worst = max(worst, ratio)
        if bad:
            fails.append(f"real/{mode}: {bad} elements of dw outside B, worst {ratio:.3g} x B")
    print(f"\n[ratio] pool-{n}: {tag}, {ppb} pairs per block, {bpi} blocks per image: largest error / B {worst:.3g}")
    assert not fails, f"{len(fails)} failures:\n" + "\n".join(fails[:40])


def test_dbias_channel_limit_is_refused_by_name():
    """colsum_kernel takes up to 256 16-byte column groups: f32 with co = 1088 (272 groups) and a dbias is an error, not a wrong sum."""
    from video_dqn_amd import _lib, ops
    gy = torch.zeros((2, 1, 1, 1088), dtype=torch.float32, device=DEV)
    x = torch.zeros((2, 1, 1, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.VdqnError, match="dbias path supports up to 1024 channels"):
        ops.conv2d_wgrad(gy, x, co=1088, r=1, s=1, stride=1, pad=0)
    torch.cuda.synchronize()
    dw = ops.conv2d_wgrad(gy, x, co=1088, r=1, s=1, stride=1, pad=0, want_dbias=False)   # without a dbias the call is served
    assert float(dw.abs().max()) == 0.0


def test_wrappers_refuse_wrong_caller_buffers():
    from video_dqn_amd import ops
    c = W.CASE_BY_NAME["win-8x8"]
    rn = Runner(c, "int")
    nbytes = W.plan(c)["bytes"]
    with pytest.raises(ValueError, match="dw must be"):
        ops.conv2d_wgrad(rn.gy, rn.x, dw=torch.zeros((64, 3, 3, 128), device=DEV), **rn.kw)
    with pytest.raises(ValueError, match="dbias must be"):
        ops.conv2d_wgrad(rn.gy, rn.x, dbias=torch.zeros((128,), device=DEV), **rn.kw)
    with pytest.raises(ValueError, match=f"at least {nbytes} bytes"):
        ops.conv2d_wgrad(rn.gy, rn.x, workspace=torch.zeros((nbytes - 1,), dtype=torch.uint8, device=DEV), **rn.kw)
    with pytest.raises(ValueError, match="workspace must be"):
        z = torch.zeros((1, 56, 56, 64), dtype=torch.bfloat16, device=DEV)
        ops.stem_wgrad_pool(z, torch.zeros((1, 56, 56, 64), dtype=torch.uint8, device=DEV),
                            torch.zeros((1, 115, 115, 16), dtype=torch.bfloat16, device=DEV), workspace=torch.zeros((16,), dtype=torch.uint8, device=DEV))
    torch.cuda.synchronize()


# ---- the same file under the switches that move a case to another kernel or another split (child processes) ----
def _rerun(env, k):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-s", "-k", k],
                       env=dict(os.environ, **env), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-6000:]


@pytest.mark.variants
@pytest.mark.parametrize("env", [
    {"VDQN_WGRAD_WINDOW": "0"},      # the window cases on the generic kernel: explicit splits with an empty range
    {"VDQN_WGRAD_STEM": "0"},        # the stem cases on wgrad<bf16,64>
    {"VDQN_WGRAD_DS64": "0"},        # ds-bf16 on 128-wide tiles
    {"VDQN_WGRAD_BLOCKS": "64", "VDQN_WGRAD_WIN_BLOCKS": "64"},   # other automatic splits
], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_rerun_under_switch(env):
    _rerun(env, "test_case or test_stem_pool")
