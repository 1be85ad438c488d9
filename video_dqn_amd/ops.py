"""Operator-level Python wrappers over the C ABI (used by the per-kernel parity tests and available to
callers that want single ops).  Tensors are torch device tensors; layouts are the ABI's (NHWC activations,
[co_pad][r][s][ci] weights)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from .engine import _ptr, _stream, attrib_source_args, norm_pixel, require_gpu  # noqa: F401 (re-exported)

TORCH_DTYPE = {_lib.VDQN_F32: torch.float32, _lib.VDQN_BF16: torch.bfloat16}


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return _lib.VDQN_F32
    if t.dtype == torch.bfloat16:
        return _lib.VDQN_BF16
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def gemm_dtype_code(t: torch.Tensor, precision: Optional[str]) -> int:
    """dtype code of a GEMM call (conv2d, conv2d_wgrad, stem_conv_pool) on tensors like `t`.  precision=None: the tensors' own
    (f32 -> exact f32 MFMAs, bf16 -> bf16 MFMAs); "bf16x3": f32 tensors, the GEMM computed as split bf16 x 3 (VDQN_F32X3)."""
    code = dtype_code(t)
    if precision is None:
        return code
    if precision != "bf16x3":
        raise ValueError(f"unknown precision {precision!r} (None or 'bf16x3')")
    if code != _lib.VDQN_F32:
        raise TypeError(f"precision='bf16x3' splits f32 operands; got {t.dtype}")
    return _lib.VDQN_F32X3


def conv2d(x: torch.Tensor, wt: torch.Tensor, *, ho: int, wo: int, co: int, r: int, s: int, stride: int, pad: int,
           bias: Optional[torch.Tensor] = None, resid: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
           relu: bool = False, mode: int = 0, pix_stride: Optional[int] = None, ci: Optional[int] = None,
           want_f32: bool = False, ldo: Optional[int] = None, want_colsum: bool = False,
           wt2: Optional[torch.Tensor] = None, bias2: Optional[torch.Tensor] = None, co2: int = 0, relu2: bool = False,
           in2: Optional[torch.Tensor] = None, precision: Optional[str] = None,
           out: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None, colsum: Optional[torch.Tensor] = None):
    """x: [n, hi, wi, c] NHWC; wt: [co_pad, r, s, ci].  Returns out [n, ho, wo, ldo] (and the f32 copy).
    out / out_f32 / colsum: caller-allocated outputs ([n, ho, wo, ldo] of x's dtype / of f32; f32 [entries, ldo] with at least the
    entries want_colsum would allocate), written in place of fresh tensors — what the call does not write keeps the caller's bytes.
    out_f32 / colsum imply want_f32 / want_colsum.  With any of the three given the return value is (out, out_f32, colsum), None for
    what the call has not (a forward sibling call still returns (out, out2)).
    precision="bf16x3" (f32 tensors): the GEMM as split bf16 x 3 instead of exact f32 MFMAs (gemm_dtype_code).
    Fused sibling 1x1 / stride 2 (include/vdqn.h): forward — wt2 [co2, 1, 1, ci] (+ bias2, relu2) gives a second output
    (returned after `out`); data gradient — in2 [n, hi, wi, ci2] and wt2 [co, 1, 1, ci2] add the sibling's gradient."""
    lib = _lib.load()
    require_gpu()
    n, hi, wi, cx = x.shape
    ci = cx if ci is None else ci
    pix_stride = cx if pix_stride is None else pix_stride
    ldo = co if ldo is None else ldo
    given = out is not None or out_f32 is not None or colsum is not None
    want_f32 = want_f32 or out_f32 is not None
    want_colsum = want_colsum or colsum is not None
    for name, t, dt in (("out", out, x.dtype), ("out_f32", out_f32, torch.float32)):
        if t is not None and (tuple(t.shape) != (n, ho, wo, ldo) or t.dtype != dt or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"conv2d: {name} must be a contiguous {dt} tensor [{n}, {ho}, {wo}, {ldo}] on {x.device}")
    if out is None:
        out = torch.empty((n, ho, wo, ldo), dtype=x.dtype, device=x.device)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty((n, ho, wo, ldo), dtype=torch.float32, device=x.device)
    a = _lib.ConvArgs()
    a.in_, a.wt, a.bias, a.resid, a.mask = _ptr(x), _ptr(wt), _ptr(bias), _ptr(resid), _ptr(mask)
    a.out, a.out_f32 = _ptr(out), _ptr(out_f32)
    a.n_img, a.hi, a.wi, a.ci, a.pix_stride = n, hi, wi, ci, pix_stride
    a.ho, a.wo, a.co, a.ldo = ho, wo, co, ldo
    a.r, a.s, a.stride, a.pad = r, s, stride, pad
    a.mode, a.relu, a.dtype = mode, int(relu), gemm_dtype_code(x, precision)
    # every field that decides which kernel takes the call is set BEFORE the colsum-row query (the skinny kernels refuse a call with
    # column sums or a sibling: a query on half-filled args would answer for another kernel than the one that runs)
    out2 = None
    if wt2 is not None and mode == 0:
        out2 = torch.empty((n, ho, wo, co2), dtype=x.dtype, device=x.device)
        a.wt2, a.bias2, a.out2, a.co2, a.ldo2, a.relu2 = _ptr(wt2), _ptr(bias2), _ptr(out2), co2, co2, int(relu2)
    elif wt2 is not None:
        a.wt2, a.in2, a.ci2 = _ptr(wt2), _ptr(in2), in2.shape[-1]
    part = None
    if want_colsum:
        a.colsum_part = 16  # non-null placeholder for the query; the real buffer is set below
        rows = lib.vdqn_conv2d_colsum_rows(C.byref(a))  # 128, or the row tile of the kernel that takes this call
        if mode == 1 and stride == 2:  # one run of tiles per output-parity class
            n_tiles = sum((n * hc * wc + rows - 1) // rows for hc in ((ho + 1) // 2, ho // 2) for wc in ((wo + 1) // 2, wo // 2))
        else:
            n_tiles = (n * ho * wo + rows - 1) // rows
        part = colsum
        if part is None:
            part = torch.empty((n_tiles, ldo), dtype=torch.float32, device=x.device)
        elif (part.dim() != 2 or part.shape[0] < n_tiles or part.shape[1] != ldo or part.dtype != torch.float32 or part.device != x.device
              or not part.is_contiguous()):
            raise ValueError(f"conv2d: colsum must be a contiguous float32 tensor [>= {n_tiles}, {ldo}] on {x.device}")
    a.colsum_part = _ptr(part)
    _lib.check(lib.vdqn_conv2d(C.byref(a), _stream()), "vdqn_conv2d")
    if out2 is not None:  # (a forward sibling has neither an f32 copy nor column sums: the library refuses them)
        return out, out2
    if given:
        return out, out_f32, part
    if want_colsum:
        return out, part
    return (out, out_f32) if want_f32 else out


def _wgrad_args(*, n, hi, wi, ci, pix_stride, ho, wo, co, ldg, r, s, stride, pad, splitk, code):
    a = _lib.WgradArgs()
    a.n_img, a.hi, a.wi, a.ci, a.pix_stride = n, hi, wi, ci, pix_stride
    a.ho, a.wo, a.co, a.ldg = ho, wo, co, ldg
    a.r, a.s, a.stride, a.pad = r, s, stride, pad
    a.splitk, a.dtype = splitk, code
    return a


def _wgrad_workspace_query(lib, a) -> int:
    nbytes = lib.vdqn_conv2d_wgrad_workspace_bytes(C.byref(a))
    if nbytes < 0:
        _lib.check(-1, "vdqn_conv2d_wgrad_workspace_bytes")
    return nbytes


def conv2d_wgrad_workspace_bytes(*, n: int, hi: int, wi: int, ci: int, ho: int, wo: int, co: int, r: int, s: int, stride: int, pad: int,
                                 dtype: torch.dtype = torch.bfloat16, precision: Optional[str] = None, ldg: Optional[int] = None,
                                 pix_stride: Optional[int] = None, splitk: int = 0) -> int:
    """Bytes of the workspace the deterministic mode of conv2d_wgrad needs for this geometry (vdqn_conv2d_wgrad_workspace_bytes: one
    partial copy of dw per split that has pixels).  Needs no GPU.  A geometry the library refuses raises VdqnError with its message.
    ldg defaults to co padded to 64, pix_stride to ci."""
    lib = _lib.load()
    code = gemm_dtype_code(torch.empty(0, dtype=dtype), precision)
    a = _wgrad_args(n=n, hi=hi, wi=wi, ci=ci, pix_stride=ci if pix_stride is None else pix_stride, ho=ho, wo=wo, co=co,
                    ldg=(co + 63) // 64 * 64 if ldg is None else ldg, r=r, s=s, stride=stride, pad=pad, splitk=splitk, code=code)
    return _wgrad_workspace_query(lib, a)


def _check_given(what, name, t, shape, dtype, device):
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be a contiguous {dtype} tensor {list(shape)} on {device}")


def _check_workspace(what, ws, nbytes, device):
    if ws.dtype != torch.uint8 or ws.dim() != 1 or not ws.is_contiguous() or ws.device != device or ws.numel() < nbytes:
        raise ValueError(f"{what}: workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {device}")


def conv2d_wgrad(gy: torch.Tensor, x: torch.Tensor, *, co: int, r: int, s: int, stride: int, pad: int,
                 ci: Optional[int] = None, pix_stride: Optional[int] = None, splitk: int = 0, want_dbias: bool = True,
                 deterministic: bool = False, poison_workspace: bool = False, precision: Optional[str] = None,
                 dw: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """gy: [n, ho, wo, ldg]; x: [n, hi, wi, c].  Returns dw f32 [co_pad, r, s, ci] (and dbias [co_pad]).
    precision="bf16x3" (f32 tensors): split bf16 x 3 MFMAs (gemm_dtype_code).
    deterministic: the two-stage ordered reduction (a workspace of vdqn_conv2d_wgrad_workspace_bytes) instead of atomics;
    poison_workspace fills that workspace with NaN first (tests: nothing the call does not write may reach dw).
    dw / dbias: caller-allocated f32 [co_pad, r, s, ci] / [co_pad], ACCUMULATED into (the ABI's dw +=, dbias +=) instead of fresh zero
    tensors; dbias implies want_dbias.  workspace: a uint8 tensor used instead of the one the call allocates (implies deterministic);
    it must hold at least conv2d_wgrad_workspace_bytes, and the library is told exactly that many bytes, whatever lies behind."""
    lib = _lib.load()
    n, ho, wo, ldg = gy.shape
    _, hi, wi, cx = x.shape
    ci = cx if ci is None else ci
    pix_stride = cx if pix_stride is None else pix_stride
    co_pad = (co + 63) // 64 * 64
    want_dbias = want_dbias or dbias is not None
    if dw is not None:
        _check_given("conv2d_wgrad", "dw", dw, (co_pad, r, s, ci), torch.float32, x.device)
    else:
        dw = torch.zeros((co_pad, r, s, ci), dtype=torch.float32, device=x.device)
    if dbias is not None:
        _check_given("conv2d_wgrad", "dbias", dbias, (co_pad,), torch.float32, x.device)
    db = dbias if dbias is not None else (torch.zeros((co_pad,), dtype=torch.float32, device=x.device) if want_dbias else None)
    a = _wgrad_args(n=n, hi=hi, wi=wi, ci=ci, pix_stride=pix_stride, ho=ho, wo=wo, co=co, ldg=ldg, r=r, s=s, stride=stride, pad=pad,
                    splitk=splitk, code=gemm_dtype_code(x, precision))
    a.gy, a.x, a.dw, a.dbias = _ptr(gy), _ptr(x), _ptr(dw), _ptr(db)
    ws = None
    if deterministic or workspace is not None:
        nbytes = _wgrad_workspace_query(lib, a)
        if workspace is not None:
            _check_workspace("conv2d_wgrad", workspace, nbytes, x.device)
            ws = workspace
        else:
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
        if poison_workspace:
            ws.fill_(0xFF)  # every f32 word a NaN
        a.workspace, a.workspace_bytes = _ptr(ws), nbytes
    _lib.check(lib.vdqn_conv2d_wgrad(C.byref(a), _stream()), "vdqn_conv2d_wgrad")
    return (dw, db) if want_dbias else dw


def pack_input(src: torch.Tensor, src_kind: int, n_img: int, dtype: torch.dtype, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out: a caller-allocated [n_img, 115, 115, 16] tensor of `dtype`, written in place of a fresh one (every element is written)."""
    lib = _lib.load()
    if out is not None:
        _check_given("pack_input", "out", out, (n_img, 115, 115, 16), dtype, src.device)
    dst = out if out is not None else torch.empty((n_img, 115, 115, 16), dtype=dtype, device=src.device)
    _lib.check(lib.vdqn_pack_input(_ptr(src), src_kind, _ptr(dst), n_img, dtype_code(dst), _stream()), "vdqn_pack_input")
    return dst


def maxpool_fwd(x: torch.Tensor):
    lib = _lib.load()
    n, hi, wi, c = x.shape
    ho, wo = (hi - 1) // 2 + 1, (wi - 1) // 2 + 1
    out = torch.empty((n, ho, wo, c), dtype=x.dtype, device=x.device)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    _lib.check(lib.vdqn_maxpool_fwd(_ptr(x), _ptr(out), _ptr(idx), n, hi, wi, c, dtype_code(x), _stream()), "vdqn_maxpool_fwd")
    return out, idx


def maxpool_bwd(gy: torch.Tensor, idx: torch.Tensor, x: Optional[torch.Tensor] = None, out_hw=None) -> torch.Tensor:
    """x given: the gradient is also masked by x > 0 (the ReLU in front of the pool); x None: plain unpooling into out_hw."""
    lib = _lib.load()
    if x is not None:
        n, hi, wi, c = x.shape
        gx = torch.empty_like(x)
    else:
        n, _, _, c = gy.shape
        hi, wi = out_hw
        gx = torch.empty((n, hi, wi, c), dtype=gy.dtype, device=gy.device)
    _lib.check(lib.vdqn_maxpool_bwd(_ptr(gy), _ptr(idx), _ptr(x), _ptr(gx), n, hi, wi, c, dtype_code(gy), _stream()), "vdqn_maxpool_bwd")
    return gx


def stem_wgrad_pool(g_pool: torch.Tensor, idx: torch.Tensor, t_in: torch.Tensor, deterministic: bool = False,
                    dw: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """conv1's weight gradient from the pooled gradient: g_pool [n,56,56,64] bf16, idx uint8 (stem_conv_pool / maxpool_fwd),
    t_in [n,115,115,16] (pack_input) -> dw f32 [64,4,1,64] == conv2d_wgrad(maxpool_bwd(g_pool, idx), t_in) on the stem geometry.
    dw: caller-allocated f32 [64,4,1,64], accumulated into.  workspace: a uint8 tensor of at least
    vdqn_stem_wgrad_pool_workspace_bytes(n) used instead of the one the call allocates (implies deterministic); the library is told
    exactly that many bytes."""
    lib = _lib.load()
    n = g_pool.shape[0]
    if dw is not None:
        _check_given("stem_wgrad_pool", "dw", dw, (64, 4, 1, 64), torch.float32, g_pool.device)
    else:
        dw = torch.zeros((64, 4, 1, 64), dtype=torch.float32, device=g_pool.device)
    ws, nbytes = None, 0
    if deterministic or workspace is not None:
        nbytes = lib.vdqn_stem_wgrad_pool_workspace_bytes(n)
        if workspace is not None:
            _check_workspace("stem_wgrad_pool", workspace, nbytes, g_pool.device)
            ws = workspace
        else:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=g_pool.device)
    _lib.check(lib.vdqn_stem_wgrad_pool(_ptr(g_pool), _ptr(idx), _ptr(t_in), _ptr(dw), n, _ptr(ws), nbytes, _stream()), "vdqn_stem_wgrad_pool")
    return dw


def stem_pixel_scale():
    """f32 [3] numpy: d(normalised value) / d(uint8 pixel value) = 1 / (255 std_c), in f32 as the library computes it."""
    import numpy as np
    return np.float32(1.0) / (np.float32(255.0) * np.array([0.229, 0.224, 0.225], dtype=np.float32))


def stem_input_grad(g_pool: torch.Tensor, idx: torch.Tensor, wt: torch.Tensor, pixel_units: bool = False,
                    precision: Optional[str] = None) -> torch.Tensor:
    """The stem's data gradient: g_pool [n,56,56,64] (bf16 or f32), idx uint8 (stem_conv_pool / maxpool_fwd), wt conv1's forward
    operand [64,4,1,64] in g_pool's dtype -> f32 [n,3,224,224] == the input gradient of conv1 applied to maxpool_bwd(g_pool, idx).
    bf16: one fused kernel; f32 (precision None or "bf16x3"): maxpool_bwd into a workspace + an f32 kernel.  pixel_units: times
    stem_pixel_scale() per colour channel (the gradient with respect to the uint8 pixel value)."""
    lib = _lib.load()
    n = g_pool.shape[0]
    code = gemm_dtype_code(g_pool, precision)
    if wt.dtype != g_pool.dtype:
        raise TypeError(f"stem_input_grad: wt is {wt.dtype}, g_pool {g_pool.dtype}")
    out = torch.empty((n, 3, 224, 224), dtype=torch.float32, device=g_pool.device)
    nbytes = lib.vdqn_stem_input_grad_workspace_bytes(n, code)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=g_pool.device) if nbytes > 0 else None
    scale = (C.c_float * 3)(*[float(v) for v in stem_pixel_scale()]) if pixel_units else None
    _lib.check(lib.vdqn_stem_input_grad(_ptr(g_pool), _ptr(idx), _ptr(wt), scale, _ptr(out), n, code, _ptr(ws), max(nbytes, 0), _stream()),
               "vdqn_stem_input_grad")
    return out


def attrib_pack(src: torch.Tensor, n_copies: int, dtype: torch.dtype, *, coef: Optional[torch.Tensor] = None, baseline=None, sigma=None,
                seed: int = 0, s0: int = 0, i0: int = 0) -> torch.Tensor:
    """`n_copies` perturbed copies of the n images of `src` as the stem operand [n_copies * n, 115, 115, 16] of `dtype` (copy s of
    image i at s * n + i), equal to pack_input of the perturbed float frames.  coef (device f32 [n_copies]): path mode, x_s = b +
    coef[s] * (x - b) with the baseline of attrib_source_args; sigma (three floats, normalised units): noise mode, x_s = x + sigma_c * z
    with z the counter-hash noise of (seed, s0 + s, i0 + i, element) (include/vdqn.h)."""
    lib = _lib.load()
    require_gpu()
    if (coef is None) == (sigma is None):
        raise ValueError("attrib_pack: give coef (path mode) or sigma (noise mode), not both")
    shared, keep = attrib_source_args(src, baseline)
    mode = 0 if coef is not None else 1
    if coef is not None and (coef.dtype != torch.float32 or coef.numel() != n_copies or coef.device != src.device or not coef.is_contiguous()):
        raise ValueError(f"attrib_pack: coef must be a contiguous float32 device tensor of {n_copies} elements")
    sg = None if sigma is None else (C.c_float * 3)(*[float(v) for v in sigma])
    dst = torch.empty((max(n_copies, 1) * src.shape[0], 115, 115, 16), dtype=dtype, device=src.device)
    _lib.check(lib.vdqn_attrib_pack(*shared, n_copies, mode, _ptr(coef), sg, int(seed) & (2**64 - 1), s0, i0, _ptr(dst), dtype_code(dst), _stream()),
               "vdqn_attrib_pack")
    del keep
    return dst


def attrib_reduce(g: torch.Tensor, w: torch.Tensor, acc: Optional[torch.Tensor] = None, squared: bool = False) -> torch.Tensor:
    """acc[i] (+)= sum_s w[s] * g[s * n + i] (squared: w[s] * g * g) in ascending s: g f32 [S * n, 3, 224, 224], w device f32 [S]; acc
    None: a new f32 [n, 3, 224, 224] is written, else `acc` is continued in place (chunks then give the bits of one call)."""
    lib = _lib.load()
    S = w.numel()
    if g.dtype != torch.float32 or w.dtype != torch.float32 or S < 1 or g.dim() != 4 or g.shape[0] % S or tuple(g.shape[1:]) != (3, 224, 224):
        raise ValueError(f"attrib_reduce: g must be float32 [S * n, 3, 224, 224] and w float32 [S], not {tuple(g.shape)} and {tuple(w.shape)}")
    n = g.shape[0] // S
    cont = acc is not None
    if cont and (acc.dtype != torch.float32 or tuple(acc.shape) != (n, 3, 224, 224) or not acc.is_contiguous()):
        raise ValueError(f"attrib_reduce: acc must be contiguous float32 [{n}, 3, 224, 224]")
    if not cont:
        acc = torch.empty((n, 3, 224, 224), dtype=torch.float32, device=g.device)
    _lib.check(lib.vdqn_attrib_reduce(_ptr(g.contiguous()), _ptr(w.contiguous()), _ptr(acc), n, S, int(bool(squared)), int(cont), _stream()),
               "vdqn_attrib_reduce")
    return acc


def attrib_finish(acc: torch.Tensor, src: Optional[torch.Tensor] = None, baseline=None, pixel_units: bool = False) -> torch.Tensor:
    """src given: integrated gradients' read-out acc * (x - b) f32 [n, 3, 224, 224], x and b as attrib_pack takes them, with
    pixel_units times stem_pixel_scale().  src None: the saliency read-out max over colour of |acc|, f32 [n, 224, 224]."""
    lib = _lib.load()
    if acc.dtype != torch.float32 or acc.dim() != 4 or tuple(acc.shape[1:]) != (3, 224, 224):
        raise ValueError(f"attrib_finish: acc must be float32 [n, 3, 224, 224], not {acc.dtype} {tuple(acc.shape)}")
    acc = acc.contiguous()
    n = acc.shape[0]
    if src is None:
        out = torch.empty((n, 224, 224), dtype=torch.float32, device=acc.device)
        _lib.check(lib.vdqn_attrib_finish(_ptr(acc), None, 0, None, None, n, 1, 0, _ptr(out), _stream()), "vdqn_attrib_finish")
        return out
    shared, keep = attrib_source_args(src, baseline)
    if src.shape[0] != n:
        raise ValueError(f"attrib_finish: acc has {n} images, src {src.shape[0]}")
    out = torch.empty_like(acc)
    _lib.check(lib.vdqn_attrib_finish(_ptr(acc), *shared, 0, int(bool(pixel_units)), _ptr(out), _stream()), "vdqn_attrib_finish")
    del keep
    return out


LOSS_KINDS = {"l2": 0, "huber": 1}  # vdqn_td_args.loss_kind


def _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect, linear, out_dtype,
             loss_kind, deterministic=False):
    """-> (TdArgs, loss[1], dq[B, ldq] out_dtype, dq_f32): the argument struct of the three TD-loss entries and the outputs it points to."""
    B, ldq = q_before.shape
    dev = q_before.device
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    dq = torch.empty((B, ldq), dtype=out_dtype, device=dev)
    dq32 = torch.empty((B, ldq), dtype=torch.float32, device=dev)
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = _ptr(q_before), _ptr(q_after_online), _ptr(q_after_target)
    a.act, a.rew, a.term, a.valid = _ptr(act), _ptr(rew), _ptr(term), _ptr(valid)
    a.loss, a.dq, a.dq_f32 = _ptr(loss), _ptr(dq), _ptr(dq32)
    a.batch, a.n_cat, a.n_act, a.ldq = B, n_cat, n_act, ldq
    a.gamma = gamma
    a.inv_count = (1.0 / (B * n_cat)) if inv_count is None else inv_count
    a.clip_rect, a.linear, a.use_valid, a.dtype = int(clip_rect), int(linear), int(valid is not None), dtype_code(dq)
    a.loss_kind = LOSS_KINDS[loss_kind]
    a.deterministic = int(deterministic)
    return a, loss, dq, dq32


def td_loss(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, n_cat=5, n_act=3, gamma=0.99,
            inv_count=None, clip_rect=True, linear=False, out_dtype=torch.float32, loss_kind="l2", discount=None):
    """q_*: f32 [B, ldq] (ldq >= n_cat*n_act).  Returns (loss[1], dq[B, ldq] out_dtype, dq_f32).  discount (f32 [B], n-step returns):
    the per-sample discount in place of gamma (td_loss_nstep)."""
    if discount is not None:
        return td_loss_nstep(q_before, q_after_online, q_after_target, act, rew, term, valid, discount=discount, n_cat=n_cat, n_act=n_act,
                             inv_count=inv_count, clip_rect=clip_rect, out_dtype=out_dtype, loss_kind=loss_kind, linear=linear)[:3]
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind)
    _lib.check(lib.vdqn_td_loss(C.byref(a), _stream()), "vdqn_td_loss")
    return loss, dq, dq32


def td_loss_cql(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, cql_alpha, weights=None, with_err=False,
                n_cat=5, n_act=3, gamma=0.99, inv_count=None, clip_rect=True, linear=False, out_dtype=torch.float32, loss_kind="l2",
                deterministic=False, discount=None):
    """td_loss with the conservative Q-learning penalty (vdqn_td_loss_cql): cql_alpha * (logsumexp_a Q(s, .) - Q(s, act)) per sample
    and category, dq dense over the actions.  weights: optional f32 [B].  Returns (loss[1], dq[B, ldq] out_dtype, dq_f32,
    penalty[1], err[B] or None).  discount (f32 [B], n-step returns): the per-sample discount in place of gamma (td_loss_nstep)."""
    if discount is not None:
        return td_loss_nstep(q_before, q_after_online, q_after_target, act, rew, term, valid, discount=discount, weights=weights,
                             with_err=with_err, cql_alpha=cql_alpha, n_cat=n_cat, n_act=n_act, inv_count=inv_count, clip_rect=clip_rect,
                             out_dtype=out_dtype, loss_kind=loss_kind, deterministic=deterministic, linear=linear)
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    penalty = torch.zeros(1, dtype=torch.float32, device=loss.device)
    err = torch.empty(q_before.shape[0], dtype=torch.float32, device=loss.device) if with_err else None
    _lib.check(lib.vdqn_td_loss_cql(C.byref(a), _ptr(weights), _ptr(err), float(cql_alpha), _ptr(penalty), _stream()), "vdqn_td_loss_cql")
    return loss, dq, dq32, penalty, err


def td_loss_nstep(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, discount, weights=None, with_err=False,
                  cql_alpha=0.0, n_cat=5, n_act=3, inv_count=None, clip_rect=True, out_dtype=torch.float32, loss_kind="l2",
                  deterministic=False, linear=False):
    """The TD loss with a per-sample discount (vdqn_td_loss_nstep; n-step returns): discount f32 [B] on the device stands where
    td_loss / td_loss_cql take the scalar gamma.  cql_alpha > 0: the CQL launch; else weights given: the weighted launch (with_err
    needs them); else the plain one.  Returns (loss[1], dq[B, ldq] out_dtype, dq_f32, penalty[1] or None, err[B] or None)."""
    lib = _lib.load()
    if discount is None or discount.dtype != torch.float32 or discount.numel() != q_before.shape[0] or not discount.is_contiguous():
        raise ValueError(f"td_loss_nstep: discount must be a contiguous f32 [{q_before.shape[0]}] device tensor")
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, 0.0, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    penalty = torch.zeros(1, dtype=torch.float32, device=loss.device) if cql_alpha > 0 else None
    err = torch.empty(q_before.shape[0], dtype=torch.float32, device=loss.device) if with_err else None
    _lib.check(lib.vdqn_td_loss_nstep(C.byref(a), _ptr(weights), _ptr(err), float(cql_alpha), _ptr(penalty), _ptr(discount), _stream()),
               "vdqn_td_loss_nstep")
    return loss, dq, dq32, penalty, err


def nstep_walk(idx, next_row, rew, term, *, n, gamma):
    """vdqn_nstep_walk: fold the chain of every sampled row (idx int64 [B]; next_row int32 [N]; rew / term f32 [N, n_cat], all on the
    device) into (rew_n [B, n_cat], term_n [B, n_cat], disc [B], last_row [B] int64, steps [B] int32)."""
    lib = _lib.load()
    B, dev = idx.shape[0], rew.device
    n_cat = rew.shape[1]
    rew_n = torch.empty((B, n_cat), dtype=torch.float32, device=dev)
    term_n = torch.empty((B, n_cat), dtype=torch.float32, device=dev)
    disc = torch.empty(B, dtype=torch.float32, device=dev)
    last_row = torch.empty(B, dtype=torch.int64, device=dev)
    steps = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.vdqn_nstep_walk(_ptr(idx), B, _ptr(next_row), _ptr(rew), _ptr(term), rew.shape[0], n_cat, int(n), float(gamma), _ptr(rew_n),
                                   _ptr(term_n), _ptr(disc), _ptr(last_row), _ptr(steps), _stream()), "vdqn_nstep_walk")
    return rew_n, term_n, disc, last_row, steps


def td_loss_mc(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, mc_return, floor=False, calibrated=False, weights=None,
               with_err=False, cql_alpha=0.0, discount=None, n_cat=5, n_act=3, gamma=0.99, inv_count=None, clip_rect=True,
               out_dtype=torch.float32, loss_kind="l2", deterministic=False, linear=False, mc_flags=None):
    """The TD loss with the Monte-Carlo return of every sampled row (vdqn_td_loss_mc): mc_return f32 [B, n_cat] on the device.  floor:
    y = max(y, G) in front of the rect clip; calibrated (needs cql_alpha > 0): the penalty's logsumexp over max(Q, G).  The mode is
    chosen as td_loss_nstep chooses it; discount (f32 [B]) is optional.  mc_flags overrides the two switches (bit 0 / bit 1).
    Returns (loss[1], dq[B, ldq] out_dtype, dq_f32, penalty[1] or None, err[B] or None, mc_stats[2])."""
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    if mc_return is not None and (mc_return.dtype != torch.float32 or tuple(mc_return.shape) != (q_before.shape[0], n_cat)
                                  or not mc_return.is_contiguous()):
        raise ValueError(f"td_loss_mc: mc_return must be a contiguous f32 [{q_before.shape[0]}, {n_cat}] device tensor")
    flags = ((1 if floor else 0) | (2 if calibrated else 0)) if mc_flags is None else int(mc_flags)
    penalty = torch.zeros(1, dtype=torch.float32, device=loss.device) if cql_alpha > 0 else None
    err = torch.empty(q_before.shape[0], dtype=torch.float32, device=loss.device) if with_err else None
    stats = torch.zeros(2, dtype=torch.float32, device=loss.device)
    _lib.check(lib.vdqn_td_loss_mc(C.byref(a), _ptr(weights), _ptr(err), float(cql_alpha), _ptr(penalty), _ptr(discount), _ptr(mc_return), flags,
                                   _ptr(stats), _stream()), "vdqn_td_loss_mc")
    return loss, dq, dq32, penalty, err, stats


def td_loss_iql(q_before, q_after_online, q_target_before, act, rew, term, valid=None, *, expectile, weights=None, with_err=False,
                discount=None, n_cat=5, n_act=3, gamma=0.99, inv_count=None, clip_rect=True, out_dtype=torch.float32, loss_kind="l2",
                deterministic=False, linear=False, with_stats=True):
    """The implicit Q-learning loss (vdqn_td_loss_iql): rows of ldq >= n_cat * n_act + n_cat columns, Q(c, a) at c * n_act + a and V(c)
    at n_cat * n_act + c.  q_before / q_after_online: the online network at s / s'; q_target_before: the TARGET network at s.  V(s) is
    fitted to Q_target(s, act) by expectile regression, Q(s, act) to rew + gamma (1 - term) V(s').  weights, discount: optional f32 [B].
    Returns (loss[1], dq[B, ldq] out_dtype, dq_f32, stats[2] = {V loss, mean Q_target(s, act) - V(s)} or None, err[B] or None)."""
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_target_before, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    if discount is not None and (discount.dtype != torch.float32 or discount.numel() != q_before.shape[0] or not discount.is_contiguous()):
        raise ValueError(f"td_loss_iql: discount must be a contiguous f32 [{q_before.shape[0]}] device tensor")
    err = torch.empty(q_before.shape[0], dtype=torch.float32, device=loss.device) if with_err else None
    stats = torch.zeros(2, dtype=torch.float32, device=loss.device) if with_stats else None
    _lib.check(lib.vdqn_td_loss_iql(C.byref(a), _ptr(weights), _ptr(err), _ptr(discount), float(expectile), _ptr(stats), _stream()),
               "vdqn_td_loss_iql")
    return loss, dq, dq32, stats, err


def dist_flags(kl_backwards=False, log_sigma=False) -> int:
    """The `flags` word of vdqn_td_loss_dist / vdqn_dist_moments: bit 0 = KL_BACKWARDS, bit 1 = LOG_SIGMA."""
    return (1 if kl_backwards else 0) | (2 if log_sigma else 0)


def td_loss_dist(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, kl_backwards=False, log_sigma=False, sigma_min=0.1,
                 weights=None, with_err=False, discount=None, n_cat=5, n_act=3, gamma=0.99, inv_count=None, clip_rect=True,
                 out_dtype=torch.float32, loss_kind="l2", deterministic=False, linear=False, with_stats=True, with_dq32=True, with_q_copy=False,
                 flags=None):
    """The Gaussian distributional loss (vdqn_td_loss_dist): rows of ldq >= 2 * n_cat * n_act columns, the mean of (c, a) at c * n_act + a
    and its spread parameter n_cat * n_act columns behind.  q_before / q_after_online: the online network at s / s'; q_after_target: the
    target network at s'.  The loss is the KL divergence between N(mean, var)(s, act) and the Double-DQN backup's Gaussian, in the
    direction kl_backwards chooses.  weights, discount: optional f32 [B].  flags: the raw word in place of the two booleans.
    Returns (loss[1], dq[B, ldq] out_dtype, dq_f32 or None, stats[2] = {mean predicted sigma, mean squared standardised error} or None,
    err[B] or None, q_copy[B, n_cat * n_act] or None)."""
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    B = q_before.shape[0]
    if discount is not None and (discount.dtype != torch.float32 or discount.numel() != B or not discount.is_contiguous()):
        raise ValueError(f"td_loss_dist: discount must be a contiguous f32 [{B}] device tensor")
    if not with_dq32:
        dq32, a.dq_f32 = None, None
    q_copy = torch.empty((B, n_cat * n_act), dtype=torch.float32, device=loss.device) if with_q_copy else None
    a.q_copy = _ptr(q_copy)
    err = torch.empty(B, dtype=torch.float32, device=loss.device) if with_err else None
    stats = torch.zeros(2, dtype=torch.float32, device=loss.device) if with_stats else None
    _lib.check(lib.vdqn_td_loss_dist(C.byref(a), _ptr(weights), _ptr(err), _ptr(discount),
                                     dist_flags(kl_backwards, log_sigma) if flags is None else int(flags), float(sigma_min), _ptr(stats),
                                     _stream()), "vdqn_td_loss_dist")
    return loss, dq, dq32, stats, err, q_copy


def dist_moments(q_rows, *, n_cat=5, n_act=3, log_sigma=False, sigma_min=0.1, flags=None):
    """vdqn_dist_moments: f32 [B, n_cat, n_act, 2] = {mean, variance} of every (category, action) from f32 rows [B, ldq] in
    td_loss_dist's layout."""
    lib = _lib.load()
    B, ldq = q_rows.shape
    out = torch.empty((B, n_cat, n_act, 2), dtype=torch.float32, device=q_rows.device)
    _lib.check(lib.vdqn_dist_moments(_ptr(q_rows), _ptr(out), B, n_cat, n_act, ldq, dist_flags(False, log_sigma) if flags is None else int(flags),
                                     float(sigma_min), _stream()), "vdqn_dist_moments")
    return out


def td_loss_bcq(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, threshold=0.3, bc_weight=1.0, logit_reg=0.01,
                weights=None, with_err=False, discount=None, n_cat=5, n_act=3, gamma=0.99, inv_count=None, clip_rect=True,
                out_dtype=torch.float32, loss_kind="l2", deterministic=False, linear=False, with_stats=True, with_dq32=True, with_q_copy=False):
    """The discrete BCQ loss (vdqn_td_loss_bcq): rows of ldq >= n_cat * n_act + n_act columns, Q(c, a) at c * n_act + a and the behaviour
    logit of action a at n_cat * n_act + a.  q_before / q_after_online: the online network at s / s'; q_after_target: the target network
    at s'.  The Double-DQN target's arg-max runs over the actions whose online logit at s' is within log(threshold) of the largest; the
    logits at s are fitted to `act` by cross-entropy.  weights, discount: optional f32 [B].
    Returns (loss[1], dq[B, ldq] out_dtype, dq_f32 or None, stats[3] = {mean cross-entropy, share of targets the constraint changes,
    behaviour accuracy} or None, err[B] or None, q_copy[B, n_cat * n_act] or None)."""
    lib = _lib.load()
    a, loss, dq, dq32 = _td_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, inv_count, clip_rect,
                                 linear, out_dtype, loss_kind, deterministic)
    B = q_before.shape[0]
    if discount is not None and (discount.dtype != torch.float32 or discount.numel() != B or not discount.is_contiguous()):
        raise ValueError(f"td_loss_bcq: discount must be a contiguous f32 [{B}] device tensor")
    if not with_dq32:
        dq32, a.dq_f32 = None, None
    q_copy = torch.empty((B, n_cat * n_act), dtype=torch.float32, device=loss.device) if with_q_copy else None
    a.q_copy = _ptr(q_copy)
    err = torch.empty(B, dtype=torch.float32, device=loss.device) if with_err else None
    stats = torch.zeros(3, dtype=torch.float32, device=loss.device) if with_stats else None
    _lib.check(lib.vdqn_td_loss_bcq(C.byref(a), _ptr(weights), _ptr(err), _ptr(discount), float(threshold), float(bc_weight), float(logit_reg),
                                    _ptr(stats), _stream()), "vdqn_td_loss_bcq")
    return loss, dq, dq32, stats, err, q_copy


def bcq_constrain(q_rows, threshold, *, n_cat=5, n_act=3, with_prob=True):
    """vdqn_bcq_constrain: (q f32 [B, n_cat, n_act] with the disallowed actions at -inf, prob f32 [B, n_act] or None) from f32 rows
    [B, ldq] in td_loss_bcq's layout."""
    lib = _lib.load()
    B, ldq = q_rows.shape
    q = torch.empty((B, n_cat, n_act), dtype=torch.float32, device=q_rows.device)
    prob = torch.empty((B, n_act), dtype=torch.float32, device=q_rows.device) if with_prob else None
    _lib.check(lib.vdqn_bcq_constrain(_ptr(q_rows), _ptr(q), _ptr(prob), B, n_cat, n_act, ldq, float(threshold), _stream()), "vdqn_bcq_constrain")
    return q, prob


def mc_returns(next_row, rew, term, *, gamma, rounds, out=None, workspace=None):
    """vdqn_mc_returns: the Monte-Carlo return table G f32 [N, n_cat] over the first 2^rounds rows of every row's chain (next_row int32
    [N]; rew / term f32 [N, n_cat], all on the device, none written).  workspace: a device byte tensor of at least
    vdqn_mc_returns_workspace_bytes(N, n_cat) bytes (allocated when None)."""
    lib = _lib.load()
    N, n_cat = rew.shape
    G = torch.empty((N, n_cat), dtype=torch.float32, device=rew.device) if out is None else out
    if workspace is None:
        workspace = torch.empty(max(int(lib.vdqn_mc_returns_workspace_bytes(N, n_cat)), 4), dtype=torch.uint8, device=rew.device)
    _lib.check(lib.vdqn_mc_returns(_ptr(next_row), _ptr(rew), _ptr(term), N, n_cat, float(gamma), int(rounds), _ptr(G), _ptr(workspace),
                                   workspace.numel() * workspace.element_size(), _stream()), "vdqn_mc_returns")
    return G


def td_eval(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, acc=None, n_cat=5, n_act=3, gamma=0.99,
            clip_rect=True, linear=False, loss_kind="l2"):
    """Held-out validation metrics of the TD loss (vdqn_td_eval): eight f64 sums per category — count, loss, |TD error|, Q(s, a_data),
    max_a Q(s, a), the target y, the conservative penalty, agreement of the greedy action with the data — ADDED into acc (f64
    [n_cat, 8] on the device; None: a fresh table of zeros).  q_*: f32 [B, ldq] (ldq >= n_cat * n_act).  Returns acc."""
    lib = _lib.load()
    B, ldq = q_before.shape
    if acc is None:
        acc = torch.zeros((n_cat, 8), dtype=torch.float64, device=q_before.device)
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = _ptr(q_before), _ptr(q_after_online), _ptr(q_after_target)
    a.act, a.rew, a.term, a.valid = _ptr(act), _ptr(rew), _ptr(term), _ptr(valid)
    a.batch, a.n_cat, a.n_act, a.ldq = B, n_cat, n_act, ldq
    a.gamma = gamma
    a.clip_rect, a.linear, a.use_valid = int(clip_rect), int(linear), int(valid is not None)
    a.loss_kind = LOSS_KINDS[loss_kind]
    _lib.check(lib.vdqn_td_eval(C.byref(a), _ptr(acc), _stream()), "vdqn_td_eval")
    return acc


def _eval_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, clip_rect, linear, loss_kind):
    a = _lib.TdArgs()
    a.q_before, a.q_after_online, a.q_after_target = _ptr(q_before), _ptr(q_after_online), _ptr(q_after_target)
    a.act, a.rew, a.term, a.valid = _ptr(act), _ptr(rew), _ptr(term), _ptr(valid)
    a.batch, a.n_cat, a.n_act, a.ldq = q_before.shape[0], n_cat, n_act, q_before.shape[1]
    a.gamma = gamma
    a.clip_rect, a.linear, a.use_valid = int(clip_rect), int(linear), int(valid is not None)
    a.loss_kind = LOSS_KINDS[loss_kind]
    return a


def _head_acc(acc, n_cat, device):
    return torch.zeros((n_cat + 1, 8), dtype=torch.float64, device=device) if acc is None else acc


def td_eval_iql(q_before, q_after_online, q_target_before, act, rew, term, valid=None, *, expectile, acc=None, n_cat=5, n_act=3, gamma=0.99,
                clip_rect=True, linear=False, loss_kind="l2"):
    """Held-out metrics of the implicit Q-learning head (vdqn_td_eval_iql), rows in td_loss_iql's layout; q_target_before: the TARGET
    network at s.  Eight f64 sums per category — count, the expectile loss, Q_target(s, act) - V(s), the Q loss and |error| against rew +
    gamma (1 - term) V(s'), V(s), that target, [advantage > 0] — ADDED into acc (f64 [n_cat + 1, 8] on the device, the last row
    untouched; None: a fresh table of zeros).  Returns acc."""
    acc = _head_acc(acc, n_cat, q_before.device)
    a = _eval_args(q_before, q_after_online, q_target_before, act, rew, term, valid, n_cat, n_act, gamma, clip_rect, linear, loss_kind)
    _lib.check(_lib.load().vdqn_td_eval_iql(C.byref(a), float(expectile), _ptr(acc), _stream()), "vdqn_td_eval_iql")
    return acc


def td_eval_dist(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, kl_backwards=False, log_sigma=False, sigma_min=0.1,
                 flags=None, acc=None, n_cat=5, n_act=3, gamma=0.99, clip_rect=True, linear=False, loss_kind="l2"):
    """Held-out metrics of the distributional head (vdqn_td_eval_dist), rows in td_loss_dist's layout.  Eight f64 sums per category —
    count, the KL, the predicted sigma, the squared standardised error, the Gaussian NLL of the backup's mean (constant dropped), the
    one-sigma coverage, the backup's sigma, the predicted sigma of the greedy action — ADDED into acc (f64 [n_cat + 1, 8] on the
    device, the last row untouched; None: a fresh table of zeros).  Returns acc."""
    acc = _head_acc(acc, n_cat, q_before.device)
    a = _eval_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, clip_rect, linear, loss_kind)
    _lib.check(_lib.load().vdqn_td_eval_dist(C.byref(a), dist_flags(kl_backwards, log_sigma) if flags is None else int(flags), float(sigma_min),
                                             _ptr(acc), _stream()), "vdqn_td_eval_dist")
    return acc


def td_eval_bcq(q_before, q_after_online, q_after_target, act, rew, term, valid=None, *, threshold=0.3, acc=None, n_cat=5, n_act=3,
                gamma=0.99, clip_rect=True, linear=False, loss_kind="l2"):
    """Held-out metrics of the BCQ policy head (vdqn_td_eval_bcq), rows in td_loss_bcq's layout.  Eight f64 sums per category — count,
    the loss and |error| against the constrained target, that target, [the constraint changes the target's action], [the constrained
    policy at s picks act], [the constraint changes the greedy action at s], the constrained policy's Q — and in the last row per
    sample: count, cross-entropy, [arg-max of the logits == act], mean squared logit, allowed actions at s, softmax(logits)[act],
    allowed actions at s', 0 — ADDED into acc (f64 [n_cat + 1, 8] on the device; None: a fresh table of zeros).  Returns acc."""
    acc = _head_acc(acc, n_cat, q_before.device)
    a = _eval_args(q_before, q_after_online, q_after_target, act, rew, term, valid, n_cat, n_act, gamma, clip_rect, linear, loss_kind)
    _lib.check(_lib.load().vdqn_td_eval_bcq(C.byref(a), float(threshold), _ptr(acc), _stream()), "vdqn_td_eval_bcq")
    return acc


def gt_loss(q_before, act, gt, *, n_cat=5, n_act=3, inv_count=None, value_learning=False):
    lib = _lib.load()
    B, ldq = q_before.shape
    dev = q_before.device
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    dq32 = torch.empty((B, ldq), dtype=torch.float32, device=dev)
    inv = (1.0 / (B * n_cat)) if inv_count is None else inv_count
    _lib.check(lib.vdqn_gt_loss(_ptr(q_before), _ptr(act), _ptr(gt), _ptr(loss), None, _ptr(dq32), B, n_cat, n_act, ldq,
                                inv, int(value_learning), _lib.VDQN_F32, _stream()), "vdqn_gt_loss")
    return loss, dq32


def _adam(entry, p, g, m, v, step, lr, beta1, beta2, eps, *more):
    """One of the three Adam entries (csrc/optim.hip) over the flat tensors p, g, m, v; `more` = what the entry takes behind eps."""
    _lib.check(getattr(_lib.load(), entry)(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), step, lr, beta1, beta2, eps, *more, _stream()), entry)


def adam(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    _adam("vdqn_adam", p, g, m, v, step, lr, beta1, beta2, eps)


def clip_workspace(device, n_ranges: int = 1) -> torch.Tensor:
    """The norm workspace for up to n_ranges (1..8) ranges: slot s = int64 count + 512 f64 partials (csrc/optim.hip)."""
    nbytes = _lib.load().vdqn_clip_workspace_bytes(n_ranges)
    if nbytes < 0:
        raise _lib.VdqnError(f"clip_workspace: n_ranges {n_ranges} (1..8)")
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def grad_sumsq(g: torch.Tensor, workspace: torch.Tensor, slot: int = 0) -> None:
    """f64 sum of squares of the contiguous f32 range g (any 4-byte aligned start) as per-block partials into `slot` of the workspace."""
    _lib.check(_lib.load().vdqn_grad_sumsq(_ptr(g), g.numel(), _ptr(workspace), slot, _stream()), "vdqn_grad_sumsq")


def clip_finalize(workspace: torch.Tensor, n_ranges: int, max_norm: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> f32 [2] on the device: {global L2 norm over slots 0 .. n_ranges-1, min(1, max_norm / (norm + 1e-6))}
    (torch.nn.utils.clip_grad_norm_); nothing is read back."""
    if out is None:
        out = torch.zeros(2, dtype=torch.float32, device=workspace.device)
    _lib.check(_lib.load().vdqn_clip_finalize(_ptr(workspace), n_ranges, max_norm, _ptr(out), _stream()), "vdqn_clip_finalize")
    return out


def adam_scaled(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, coef: Optional[torch.Tensor] = None):
    """torch.optim.AdamW on g * coef[0] (coef: f32 device tensor, e.g. clip_finalize(..)[1:]; None = 1)."""
    _adam("vdqn_adam_scaled", p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, _ptr(coef))


def polyak_update(target: torch.Tensor, online: torch.Tensor, tau: float) -> None:
    """Soft target update in place: target <- target + tau * (online - target) over two contiguous f32 device tensors of one size
    (vdqn_polyak: torch.lerp's two-branch rule, every product rounded on its own; tau in (0, 1], tau = 1 copies)."""
    if target.numel() != online.numel():
        raise _lib.VdqnError(f"polyak_update: target has {target.numel()} elements, online {online.numel()}")
    _lib.check(_lib.load().vdqn_polyak(_ptr(target), _ptr(online), target.numel(), float(tau), _stream()), "vdqn_polyak")


def adam_polyak(p, g, m, v, target, tau, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, coef: Optional[torch.Tensor] = None):
    """adam_scaled and polyak_update(target, p, tau) in one launch: the new p is lerped into `target` from registers."""
    if target.numel() != p.numel():
        raise _lib.VdqnError(f"adam_polyak: target has {target.numel()} elements, p {p.numel()}")
    _adam("vdqn_adam_polyak", p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, _ptr(coef), _ptr(target), float(tau))


def bn_train_fwd(y: torch.Tensor, gamma, beta, running_mean=None, running_var=None, *, resid=None, relu=False,
                 num_frames=1, imgs_per_half=None, momentum=0.1, eps=1e-5, deterministic=False):
    """Train-mode BatchNorm2d over NHWC y [n, h, w, c] (statistic groups: see include/vdqn.h).
    Returns (z, work) — `work` f32 [groups, 6, c] is what bn_train_bwd needs.
    deterministic: ordered two-stage statistic sums (a NaN-filled workspace of vdqn_bn_train_workspace_bytes) instead of atomics."""
    lib = _lib.load()
    n, h, w, c = y.shape
    iph = n if imgs_per_half is None else imgs_per_half
    groups = n // iph * num_frames
    z = torch.empty_like(y)
    work = torch.zeros((groups, 6, c), dtype=torch.float32, device=y.device)
    ws, nbytes = _bn_workspace(lib, y, n, h * w, c, num_frames, iph, deterministic)
    _lib.check(lib.vdqn_bn_train_fwd(_ptr(y), _ptr(resid), _ptr(z), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var),
                                     _ptr(work), n, h * w, c, num_frames, iph, int(relu), momentum, eps, dtype_code(y), _ptr(ws), nbytes,
                                     _stream()), "vdqn_bn_train_fwd")
    return z, work


def _bn_workspace(lib, y, n, hw, c, num_frames, iph, deterministic):
    if not deterministic:
        return None, 0
    nbytes = lib.vdqn_bn_train_workspace_bytes(n, hw, c, num_frames, iph)
    if nbytes < 0:
        _lib.check(-1, "vdqn_bn_train_workspace_bytes")
    return torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=y.device), nbytes


def bn_train_bwd(g: torch.Tensor, y: torch.Tensor, work: torch.Tensor, *, num_frames=1, imgs_per_half=None, deterministic=False):
    """Returns (dy, dgamma, dbeta) for the BatchNorm whose forward filled `work`."""
    lib = _lib.load()
    n, h, w, c = y.shape
    iph = n if imgs_per_half is None else imgs_per_half
    dy = torch.empty_like(y)
    dgamma = torch.empty(c, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(c, dtype=torch.float32, device=y.device)
    ws, nbytes = _bn_workspace(lib, y, n, h * w, c, num_frames, iph, deterministic)
    _lib.check(lib.vdqn_bn_train_bwd(_ptr(g), _ptr(y), _ptr(dy), _ptr(work), _ptr(dgamma), _ptr(dbeta), n, h * w, c, num_frames, iph,
                                     dtype_code(y), _ptr(ws), nbytes, _stream()), "vdqn_bn_train_bwd")
    return dy, dgamma, dbeta


def avgpool_fwd(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    n, h, w, c = x.shape
    out = torch.empty((n, c), dtype=x.dtype, device=x.device)
    _lib.check(lib.vdqn_avgpool_fwd(_ptr(x), _ptr(out), n, h * w, c, dtype_code(x), _stream()), "vdqn_avgpool_fwd")
    return out


def avgpool_bwd(g: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """g [n, c]; x [n, h, w, c] (post-ReLU input of the pool): gx = (x > 0) * g / (h*w)."""
    lib = _lib.load()
    n, h, w, c = x.shape
    gx = torch.empty_like(x)
    _lib.check(lib.vdqn_avgpool_bwd(_ptr(g), _ptr(x), _ptr(gx), n, h * w, c, dtype_code(x), _stream()), "vdqn_avgpool_bwd")
    return gx


def stem_conv_pool(t_in: torch.Tensor, wt: torch.Tensor, bias: torch.Tensor, want_idx: bool = True, n_idx: int = None,
                   precision: Optional[str] = None, pool: Optional[torch.Tensor] = None, idx: Optional[torch.Tensor] = None):
    """t_in [n,115,115,16] (pack_input), wt [64,4,1,64], bias f32 [64] -> (pool [n,56,56,64], idx uint8).
    precision="bf16x3" (f32 tensors): split bf16 x 3 MFMAs (gemm_dtype_code).

    want_idx=False: frames that never see a backward pass — idx is None and the arg-max bytes are not computed.
    n_idx: arg-max bytes for the first n_idx images only (vdqn_stem_conv_pool_n); the other rows of idx stay as allocated.
    pool / idx: caller-allocated outputs ([n,56,56,64] of t_in's dtype / of uint8) written in place of fresh tensors; what the call
    does not write (the rows of idx from n_idx on) keeps the caller's bytes."""
    lib = _lib.load()
    n = t_in.shape[0]
    dt = gemm_dtype_code(t_in, precision)
    if pool is not None:
        _check_given("stem_conv_pool", "pool", pool, (n, 56, 56, 64), t_in.dtype, t_in.device)
    else:
        pool = torch.empty((n, 56, 56, 64), dtype=t_in.dtype, device=t_in.device)
    if idx is not None:
        if not want_idx:
            raise ValueError("stem_conv_pool: idx given with want_idx=False")
        _check_given("stem_conv_pool", "idx", idx, (n, 56, 56, 64), torch.uint8, t_in.device)
    if n_idx is not None:
        if idx is None:
            idx = torch.zeros((n, 56, 56, 64), dtype=torch.uint8, device=t_in.device)
        _lib.check(lib.vdqn_stem_conv_pool_n(_ptr(t_in), _ptr(wt), _ptr(bias), _ptr(pool), _ptr(idx), n, int(n_idx), dt, _stream()),
                   "vdqn_stem_conv_pool_n")
        return pool, idx
    if idx is None and want_idx:
        idx = torch.empty((n, 56, 56, 64), dtype=torch.uint8, device=t_in.device)
    _lib.check(lib.vdqn_stem_conv_pool(_ptr(t_in), _ptr(wt), _ptr(bias), _ptr(pool), _ptr(idx) if want_idx else None, n, dt, _stream()),
               "vdqn_stem_conv_pool")
    return pool, idx
