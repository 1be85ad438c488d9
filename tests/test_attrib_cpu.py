"""The attribution oracle (tests/attrib_oracle.py) against its own definitions, and the new C entries' exports and argument checks
(no GPU: every call fails before it reaches the device)."""
import ctypes as C

import numpy as np
import pytest

import attrib_oracle as AO

NEW = ("vdqn_net_backward_data", "vdqn_attrib_pack", "vdqn_attrib_reduce", "vdqn_attrib_finish", "vdqn_net_forward_attrib")


# ---- the noise -------------------------------------------------------------------------------------------------------------------
def test_noise_constant_and_hash():
    assert float(AO.KZ).hex() == "0x1.bb67ae0000000p-16"  # what csrc/attrib.hip writes as a hex literal
    assert AO.STREAM.to_bytes(8, "big") == b"ATTRIB01"
    # splitmix64's published first outputs for the state 0 (the state advances by the golden-ratio constant)
    assert int(AO.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(AO.splitmix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4
    assert int(AO.hash_fields_sum(np.uint64(0xFFFF_0001_0002_0003))) == 0xFFFF + 6
    assert AO.z_from_hash(np.uint64(0)) == np.float32(-131070.0) * AO.KZ and AO.z_from_hash(np.uint64(AO.M64)) == np.float32(131070.0) * AO.KZ
    assert float(AO.z_from_hash(np.uint64(AO.M64))) == AO.Z_MAX


def test_noise_moments_and_support():
    """10^6 draws: |mean| < 0.01, variance within 1 % of 1, support inside +-3.4642.  All three follow from the integer definition:
    four uniform 16-bit fields have mean 131070 and variance (2^32 - 1) / 3, and kZ is that variance's inverse root to 2^-24; the
    sample mean of 10^6 unit-variance draws has a standard deviation of 1e-3, the sample variance of 1.3e-3."""
    z = AO.noise_z(3, 1, 2, np.arange(10 ** 6)).astype(np.float64)
    assert abs(z.mean()) < 0.01
    assert abs(z.var() - 1.0) < 0.01
    assert np.abs(z).max() <= AO.Z_MAX < 3.4642
    assert np.abs(z).max() > 3.0  # the tails are there
    # its own stream, and every index matters
    base = AO.noise_z(3, 1, 2, np.arange(64))
    for other in (AO.noise_z(4, 1, 2, np.arange(64)), AO.noise_z(3, 0, 2, np.arange(64)), AO.noise_z(3, 1, 3, np.arange(64)),
                  AO.noise_z(3, 1, 2, np.arange(64) + 1)):
        assert not np.array_equal(base, other)
    # chunking: copy s0 + s of a later call is copy s0 + s of one long call
    x = np.zeros((1, 3, 224, 224), dtype=np.float32)
    long = AO.noise_frames(x, [1, 1, 1], 9, 3)
    assert np.array_equal(AO.noise_frames(x, [1, 1, 1], 9, 1, s0=2), long[2:3])
    assert long.dtype == np.float32 and np.array_equal(long[0, 1].reshape(-1)[:5], AO.noise_z(9, 0, 0, 224 * 224 + np.arange(5)))


# ---- the path --------------------------------------------------------------------------------------------------------------------
def test_path_end_points():
    rng = np.random.default_rng(1)
    # values on a 2^-10 grid in [-4, 4): x - b and b + (x - b) are exact in float32
    x = (rng.integers(-4096, 4096, size=(2, 3, 224, 224)) / 1024.0).astype(np.float32)
    b = (rng.integers(-4096, 4096, size=(2, 3, 224, 224)) / 1024.0).astype(np.float32)
    assert np.array_equal(AO.path_frames(x, b, [1.0]), x)
    assert np.array_equal(AO.path_frames(x, b, [0.0]), b)
    const = AO.norm_pixel([0, 0, 0])
    got = AO.path_frames(x, const, [0.0, 0.5])
    assert got.shape == (4, 3, 224, 224) and np.array_equal(got[:2], np.broadcast_to(const.reshape(1, 3, 1, 1), x.shape))
    assert np.array_equal(got[2:], const.reshape(1, 3, 1, 1) + np.float32(0.5) * (x - const.reshape(1, 3, 1, 1)))
    u8 = rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)
    xn = AO.normalise(u8)
    assert xn.shape == (1, 3, 224, 224) and xn[0, 2, 5, 7] == (np.float32(u8[0, 5, 7, 2]) / np.float32(255) - AO.MEAN[2]) / AO.STD[2]
    assert np.array_equal(AO.normalise(np.zeros((1, 224, 224, 3), dtype=np.uint8))[0, :, 0, 0], const)


# ---- reduce and finish -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squared", [False, True])
def test_reduce_stays_within_the_summation_bound(squared):
    """S roundings per element (S products, S - 1 sums that round): |float32 result - float64 sum| <= (S + 2) 2^-24 sum_s |w_s g_s|
    to first order (Higham, Accuracy and Stability, 4.2), g_s squared where asked, which costs one more product."""
    rng = np.random.default_rng(2)
    S, n = 7, 2
    g = rng.standard_normal((S * n, 3, 224, 224)).astype(np.float32)
    w = (rng.random(S) / 3 + 0.01).astype(np.float32)
    got = AO.reduce(g, w, squared=squared)
    terms = np.stack([w[s].astype(np.float64) * g[s * n:(s + 1) * n].astype(np.float64) ** (2 if squared else 1) for s in range(S)])
    bound = (S + 2) * 2.0 ** -24 * 1.001 * np.abs(terms).sum(0)  # (squared: one more product)
    assert got.dtype == np.float32 and np.all(np.abs(got.astype(np.float64) - terms.sum(0)) <= bound)
    # chunks continued give the bits of one call
    part = AO.reduce(g[:3 * n], w[:3], squared=squared)
    assert np.array_equal(AO.reduce(g[3 * n:], w[3:], acc=part, squared=squared), got)


def test_finish():
    rng = np.random.default_rng(3)
    acc = rng.standard_normal((2, 3, 224, 224)).astype(np.float32)
    x = rng.standard_normal((2, 3, 224, 224)).astype(np.float32)
    const = AO.norm_pixel([10, 20, 30])
    got = AO.finish_ig(acc, x, const)
    assert got[1, 2, 3, 4] == acc[1, 2, 3, 4] * (x[1, 2, 3, 4] - const[2])
    sc = np.array([2.0, 3.0, 5.0], dtype=np.float32)
    assert AO.finish_ig(acc, x, const, sc)[0, 1, 8, 9] == (acc[0, 1, 8, 9] * (x[0, 1, 8, 9] - const[1])) * sc[1]
    m = AO.finish_max(acc)
    assert m.shape == (2, 224, 224) and m[1, 5, 6] == max(abs(acc[1, c, 5, 6]) for c in range(3))


# ---- the library -----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols_at_abi_16():
    from video_dqn_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    assert lib.vdqn_abi_version() == 16 == _lib.ABI_VERSION
    assert lib.vdqn_abi_struct_size(7) == -1  # no new argument struct: every new argument is a plain one


P = 4096  # a 16-byte aligned address that is never dereferenced: every call below fails its argument check


def _f3(*v):
    return (C.c_float * 3)(*v)


def test_pack_reduce_finish_refuse_bad_arguments():
    from video_dqn_amd import _lib
    lib = _lib.load()

    def pack(src=P, kind=0, base=None, const=None, n=1, S=2, mode=0, coef=P, sigma=None, seed=0, s0=0, i0=0, dst=P, dtype=_lib.VDQN_BF16):
        return lib.vdqn_attrib_pack(src, kind, base, const, n, S, mode, coef, sigma, seed, s0, i0, dst, dtype, None)
    bad = [dict(src=None), dict(dst=None), dict(kind=2), dict(kind=-1), dict(n=0), dict(S=0), dict(S=65536), dict(mode=2), dict(coef=None),
           dict(coef=P + 2), dict(src=P + 4), dict(base=P + 8), dict(dst=P + 8), dict(dtype=7), dict(dtype=_lib.VDQN_F32X3), dict(n=2000, S=100),
           dict(const=_f3(0, float("nan"), 0)), dict(mode=1), dict(mode=1, sigma=_f3(0.1, -0.1, 0.1)), dict(mode=1, sigma=_f3(0.1, float("inf"), 0.1)),
           dict(mode=1, sigma=_f3(1, 1, 1), s0=-1), dict(mode=1, sigma=_f3(1, 1, 1), i0=-1), dict(mode=1, sigma=_f3(1, 1, 1), s0=2 ** 31 - 1)]
    for kw in bad:
        assert pack(**kw) != 0, kw
        assert b"vdqn_attrib_pack" in lib.vdqn_last_error(), kw
    assert pack(n=2000, S=100) != 0 and b"split the copies" in lib.vdqn_last_error()
    assert pack(mode=1) != 0 and b"sigma" in lib.vdqn_last_error()

    def red(g=P, w=P, acc=P, n=1, S=2, sq=0, cont=0):
        return lib.vdqn_attrib_reduce(g, w, acc, n, S, sq, cont, None)
    for kw in (dict(g=None), dict(w=None), dict(acc=None), dict(n=0), dict(S=0), dict(g=P + 4), dict(acc=P + 8), dict(w=P + 1), dict(sq=2), dict(cont=-1)):
        assert red(**kw) != 0, kw
        assert b"vdqn_attrib_reduce" in lib.vdqn_last_error(), kw

    def fin(acc=P, src=P, kind=1, base=None, const=None, n=1, mode=0, scale=0, out=P):
        return lib.vdqn_attrib_finish(acc, src, kind, base, const, n, mode, scale, out, None)
    for kw in (dict(acc=None), dict(out=None), dict(mode=2), dict(n=0), dict(acc=P + 4), dict(out=P + 8), dict(src=None), dict(kind=3), dict(scale=2),
               dict(base=P + 2), dict(const=_f3(float("inf"), 0, 0)), dict(mode=1, n=0), dict(mode=1, out=None)):
        assert fin(**kw) != 0, kw
        assert b"vdqn_attrib_finish" in lib.vdqn_last_error(), kw


def test_engine_entries_refuse_bad_arguments_and_basic_by_name():
    from video_dqn_amd import _lib
    from video_dqn_amd.engine import NetEngine
    ext = NetEngine(3, 5, 2, extra_capacity=True, dtype="bf16", max_batch=4, device="cpu")
    basic = NetEngine(3, 5, 2, extra_capacity=False, dtype="bf16", max_batch=4, device="cpu")
    lib = ext.lib
    a = _lib.StepArgs()
    a.batch = a.acts_samples = 2
    a.packed_online = a.acts_online = a.bwd = P  # grads, params, bnstats stay NULL: not asked for

    def bwd(net=ext.handle, args=a, dq=P, out=P, scale=0):
        return lib.vdqn_net_backward_data(net, C.byref(args), dq, out, scale, None)
    assert bwd(net=basic.handle) != 0 and b"basic" in lib.vdqn_last_error() and b"vdqn_net_backward_data" in lib.vdqn_last_error()
    for field in ("packed_online", "acts_online", "bwd"):
        b = _lib.StepArgs()
        C.memmove(C.byref(b), C.byref(a), C.sizeof(a))
        setattr(b, field, None)
        assert bwd(args=b) != 0 and b"null buffer" in lib.vdqn_last_error(), field
    for kw, word in ((dict(net=None), b"null"), (dict(dq=None), b"null"), (dict(out=None), b"null"), (dict(out=P + 4), b"aligned"), (dict(scale=2), b"scale_kind")):
        assert bwd(**kw) != 0 and word in lib.vdqn_last_error(), kw
    for batch, samples in ((0, 0), (5, 5), (2, 0), (2, 4)):
        b = _lib.StepArgs()
        C.memmove(C.byref(b), C.byref(a), C.sizeof(a))
        b.batch, b.acts_samples = batch, samples
        assert bwd(args=b) != 0 and b"acts_samples" in lib.vdqn_last_error(), (batch, samples)

    def fwd(net=ext.handle, packed=P, src=P, kind=0, n=4, S=2, mode=0, coef=P, sigma=None, ns=4, acts=P, q=P):
        return lib.vdqn_net_forward_attrib(net, packed, src, kind, None, None, n, S, mode, coef, sigma, 0, 0, 0, ns, acts, q, None)
    assert fwd(net=basic.handle) != 0 and b"basic" in lib.vdqn_last_error()
    for kw, word in ((dict(net=None), b"null"), (dict(packed=None), b"null"), (dict(acts=None), b"null"), (dict(q=None), b"null"),
                     (dict(ns=0), b"n_samples"), (dict(ns=5), b"max_batch"), (dict(n=4, S=1), b"copies"), (dict(n=0, S=0), b"copies"),
                     (dict(n=1, S=8), b"whole number"), (dict(src=None), b"src is NULL"), (dict(coef=None), b"coef"), (dict(kind=5), b"src_kind"),
                     (dict(mode=1), b"sigma")):
        assert fwd(**kw) != 0, kw
        assert word in lib.vdqn_last_error(), (kw, lib.vdqn_last_error())
