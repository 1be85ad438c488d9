"""numpy restatement of the random-rotation augmentation (video_dqn_amd/csrc/augment.hip): the integer sine and cosine, the per-sample
draw of the angle, its composition with a zoom row into an affine row, and the affine bilinear resample with its composition with
the shift / mirror remap (tests/aug_oracle.py) and the colour transform (tests/aug_color_oracle.py), written from the arithmetic
alone.  The GPU tests compare the kernels against it bit for bit.

All integers; ">>" is arithmetic and "//" floors (numpy's and Python's do).  The unit of angle is 1 / 64 degree.  An affine row is int32
{axx, axy, bx, 0, ayx, ayy, by, 0} in Q16.  Output pixel (Y, X) of a frame Z, per channel:
    u = bx + X * axx + Y * axy;  x0 = u >> 16;  wx = (u >> 8) & 255;     v = by + X * ayx + Y * ayy;  y0 = v >> 16;  wy = (v >> 8) & 255
    xa = clamp(x0, 0, 223), xb = clamp(x0 + 1, 0, 223), ya, yb likewise
    top = Z[ya][xa] * (256 - wx) + Z[ya][xb] * wx;   bot = the same on row yb;   out = (top * (256 - wy) + bot * wy + 32768) >> 16
The kernel clamps axx, ayy to [0, 65536], axy, ayx to +-65536 and bx, by to +-448 * 65536 before use; so does `clamp_rows`."""
import numpy as np

import aug_color_oracle
import aug_oracle
import aug_zoom_oracle
from aug_oracle import M64, splitmix64

ROTATE_STREAM = 0x415547524F544131  # "AUGROTA1"
ONE = 65536
MAX_JR = 1920  # 30 degrees
# a diagonal term is at least 0 and a cross term at least -65536: at bx = 448 * 65536, u >= (448 - 223) * 65536 and x0 >= 225 at every
# output pixel, so both taps clamp to 223; at bx = -448 * 65536, u <= (-448 + 446) * 65536 and x0 + 1 <= -1: both taps clamp to 0
MAX_ORIGIN = 448 * 65536
Q30 = 1 << 30
IDENTITY = (ONE, 0, 0, 0, 0, ONE, 0, 0)


def jr(j: float) -> int:
    """The angle range in 1 / 64 degree."""
    return int(j * 64 + 0.5)


def sincos(k: int):
    """(S, C), Q16, of the angle k / 64 degrees, |k| <= 1920: Taylor polynomials in Q30, Horner form."""
    t = k * 292818  # Q30 radians: 292818 = round(pi / 11520 * 2^30)
    t2 = (t * t) >> 30
    a = Q30 - t2 // 42
    a = Q30 - ((t2 * a) >> 30) // 20
    a = Q30 - ((t2 * a) >> 30) // 6
    s = (t * a) >> 30
    b = Q30 - t2 // 56
    b = Q30 - ((t2 * b) >> 30) // 30
    b = Q30 - ((t2 * b) >> 30) // 12
    b = Q30 - ((t2 * b) >> 30) // 2
    return (s + 8192) >> 14, (b + 8192) >> 14


def angle(seed: int, step: int, global_batch: int, jr: int, j: int) -> int:
    key = splitmix64((seed & M64) ^ ROTATE_STREAM)
    h = splitmix64(key ^ (((step & M64) * global_batch + j) & M64))
    return (((h & 0xFFFF) * (2 * jr + 1)) >> 16) - jr


def compose(k: int, zoom_row=aug_zoom_oracle.IDENTITY) -> tuple:
    """The affine row of a rotation by k about the picture's centre (index 111.5) in front of the zoom map {ax, ay, bxz, byz}."""
    ax, ay, bxz, byz = (int(v) for v in zoom_row)
    S, C = sincos(k)
    axx, axy = (ax * C + 32768) >> 16, -((ax * S + 32768) >> 16)
    ayx, ayy = (ay * S + 32768) >> 16, (ay * C + 32768) >> 16
    return (axx, axy, bxz + ((223 * (ax - axx - axy)) >> 1), 0, ayx, ayy, byz + ((223 * (ay - ayx - ayy)) >> 1), 0)


def draw(seed: int, step: int, global_batch: int, jr: int, zoom=None, first: int = 0, n: int = None) -> np.ndarray:
    """int32 [n][8] of samples first .. first + n of the global batch at update `step`; `zoom` int [n][4], the slice's zoom rows, or None."""
    n = global_batch - first if n is None else n
    out = np.zeros((n, 8), np.int64)
    for i in range(n):
        out[i] = compose(angle(seed, step, global_batch, jr, first + i), aug_zoom_oracle.IDENTITY if zoom is None else zoom[i])
    assert np.abs(out).max() < 2**31
    return out.astype(np.int32)


def clamp_rows(rows: np.ndarray) -> np.ndarray:
    """int64 [n][8]: the rows as the kernel uses them (words 3 and 7 are ignored: 0 here)."""
    r = np.asarray(rows).reshape(-1, 8).astype(np.int64)
    out = np.zeros_like(r)
    out[:, [0, 5]] = np.clip(r[:, [0, 5]], 0, ONE)
    out[:, [1, 4]] = np.clip(r[:, [1, 4]], -ONE, ONE)
    out[:, [2, 6]] = np.clip(r[:, [2, 6]], -MAX_ORIGIN, MAX_ORIGIN)
    return out


def coords(row):
    """(u, v), int64 [224][224] indexed [Y][X]: the Q16 source coordinates of every output pixel under a (clamped) row."""
    axx, axy, bx, _, ayx, ayy, by, _ = (int(v) for v in clamp_rows(row)[0])
    Y, X = np.mgrid[0:224, 0:224].astype(np.int64)
    u, v = bx + X * axx + Y * axy, by + X * ayx + Y * ayy
    assert max(np.abs(u).max(), np.abs(v).max()) < 2**31  # the kernel's int32 arithmetic does not wrap
    return u, v


def resample(frame: np.ndarray, row) -> np.ndarray:
    """frame uint8 [224][224][3], row of 8 words (clamped here) -> uint8 [224][224][3]."""
    u, v = coords(row)
    x0, y0 = u >> 16, v >> 16
    wx, wy = ((u >> 8) & 255)[..., None], ((v >> 8) & 255)[..., None]
    xa, xb, ya, yb = np.clip(x0, 0, 223), np.clip(x0 + 1, 0, 223), np.clip(y0, 0, 223), np.clip(y0 + 1, 0, 223)
    z = np.asarray(frame).astype(np.int64)
    top = z[ya, xa] * (256 - wx) + z[ya, xb] * wx
    bot = z[yb, xa] * (256 - wx) + z[yb, xb] * wx
    out = (top * (256 - wy) + bot * wy + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def affine(frames: np.ndarray, rows: np.ndarray, frames_per_sample: int = 1) -> np.ndarray:
    """frames uint8 [n][224][224][3]; frame i takes rows[(i // frames_per_sample) % len(rows)]."""
    frames = np.asarray(frames)
    rows = np.asarray(rows).reshape(-1, 8)
    out = np.empty_like(frames)
    for i in range(frames.shape[0]):
        out[i] = resample(frames[i], rows[(i // frames_per_sample) % len(rows)])
    return out


def augment(frames: np.ndarray, params: np.ndarray, rows: np.ndarray, color: np.ndarray = None, frames_per_sample: int = 1) -> np.ndarray:
    """The composition the pack applies: color(affine(shift_mirror(frames))); `color` None = no colour transform."""
    out = affine(aug_oracle.augment_frames(frames, params, frames_per_sample), rows, frames_per_sample)
    return out if color is None else aug_color_oracle.color(out, color, frames_per_sample)
