"""The attribution kernels (video_dqn_amd/csrc/attrib.hip) restated in numpy float32, one rounding per product and per sum, as
include/vdqn.h states them: the perturbed frames of both modes, the counter hash and its noise, the weighted sum over the copies
and the two read-outs.  Everything works on NCHW float32 frames [n, 3, 224, 224]; `normalise` turns uint8 NHWC frames into them
with vdqn_pack_input's expression."""
import numpy as np

F32 = np.float32
MEAN = np.array([0.485, 0.456, 0.406], dtype=F32)
STD = np.array([0.229, 0.224, 0.225], dtype=F32)
STREAM = 0x4154545249423031  # "ATTRIB01"
KZ = F32(1.0 / np.sqrt((2 ** 32 - 1) / 3.0))  # the f32 nearest to 1 / sqrt((2^32 - 1) / 3)
Z_MAX = float(F32(131070.0) * KZ)  # the largest |z|
M64 = (1 << 64) - 1


def normalise(u8):
    """uint8 [n, 224, 224, 3] -> f32 [n, 3, 224, 224]: ((float)u / 255 - mean_c) / std_c, each operation rounded to float32."""
    x = u8.astype(F32) / F32(255.0)
    x = (x - MEAN) / STD
    return np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def norm_pixel(values):
    v = np.asarray(values, dtype=F32).reshape(3)
    return (v / F32(255.0) - MEAN) / STD


def baseline_frames(b, shape):
    """The baseline as frames: three normalised constants broadcast over `shape` [n, 3, 224, 224], or frames as they are."""
    b = np.asarray(b, dtype=F32)
    return np.broadcast_to(b.reshape(1, 3, 1, 1), shape) if b.size == 3 else b


def path_frames(x, b, coef):
    """[S * n, 3, 224, 224]: copy s of image i at s * n + i is b + coef[s] * (x - b)."""
    x = np.asarray(x, dtype=F32)
    b = baseline_frames(b, x.shape)
    d = x - b
    return np.concatenate([(b + F32(c) * d).astype(F32) for c in np.asarray(coef, dtype=F32)], 0)


def splitmix64(x):
    """uint64 array -> uint64 array (wrapping arithmetic)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def hash_fields_sum(h):
    """The sum of the four 16-bit fields of each hash, int64."""
    h = np.asarray(h, dtype=np.uint64)
    m = np.uint64(0xFFFF)
    return ((h & m) + ((h >> np.uint64(16)) & m) + ((h >> np.uint64(32)) & m) + (h >> np.uint64(48))).astype(np.int64)


def z_from_hash(h):
    """f32: (float)(h0 + h1 + h2 + h3 - 131070) * kZ; the integer is below 2^24, its conversion exact."""
    return (hash_fields_sum(h) - 131070).astype(F32) * KZ


def noise_z(seed, copy, image, elements):
    """z of the elements (NCHW indices inside an image, any integer array) of `image` in copy `copy`."""
    key = splitmix64(np.uint64((int(seed) ^ STREAM) & M64))
    key_ci = splitmix64(key ^ np.uint64(((int(copy) & 0xFFFFFFFF) << 32) | (int(image) & 0xFFFFFFFF)))
    return z_from_hash(splitmix64(key_ci ^ np.asarray(elements, dtype=np.uint64)))


def noise_frames(x, sigma, seed, n_copies, s0=0, i0=0):
    """[S * n, 3, 224, 224]: copy s of image i is x + sigma[c] * z(seed, s0 + s, i0 + i, element)."""
    x = np.asarray(x, dtype=F32)
    n = x.shape[0]
    sg = np.asarray(sigma, dtype=F32).reshape(3, 1, 1)
    elems = np.arange(3 * 224 * 224, dtype=np.uint64)
    out = np.empty((n_copies * n, 3, 224, 224), dtype=F32)
    for s in range(n_copies):
        for i in range(n):
            z = noise_z(seed, s0 + s, i0 + i, elems).reshape(3, 224, 224)
            out[s * n + i] = x[i] + (sg * z).astype(F32)
    return out


def reduce(g, w, acc=None, squared=False):
    """acc (+)= sum_s w[s] * g[s * n + i] in ascending s, the running sum rounded after every addend; squared: (w[s] * g) * g."""
    g = np.asarray(g, dtype=F32)
    w = np.asarray(w, dtype=F32)
    n = g.shape[0] // len(w)
    run = np.zeros((n,) + g.shape[1:], dtype=F32) if acc is None else np.array(acc, dtype=F32)
    for s in range(len(w)):
        t = w[s] * g[s * n:(s + 1) * n]
        if squared:
            t = t * g[s * n:(s + 1) * n]
        run = (run + t).astype(F32)
    return run


def finish_ig(acc, x, b, scale=None):
    """acc * (x - b), then times scale[c] (f32 [3]) if given."""
    x = np.asarray(x, dtype=F32)
    r = np.asarray(acc, dtype=F32) * (x - baseline_frames(b, x.shape))
    if scale is not None:
        r = r * np.asarray(scale, dtype=F32).reshape(1, 3, 1, 1)
    return r.astype(F32)


def finish_max(acc):
    """[n, 224, 224]: max over colour of |acc|."""
    return np.abs(np.asarray(acc, dtype=F32)).max(1)
