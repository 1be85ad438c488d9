"""numpy restatement of the random-zoom augmentation (video_dqn_amd/csrc/augment.hip): the per-sample draw of the window, the integer
bilinear resample and its composition with the shift / mirror remap (tests/aug_oracle.py) and the colour transform
(tests/aug_color_oracle.py), written from the arithmetic alone.  The GPU tests compare the kernels against it bit for bit.

All integers; ">>" is arithmetic (numpy's and Python's are).  A row is int32 {ax, ay, bx, by}: ax, ay the Q16 source step per output
pixel (65536 = 1.0), bx, by the Q16 source coordinate of output pixel 0.  Output pixel (Y, X) of a frame Z, per channel:
    u = bx + X * ax;  x0 = u >> 16;  wx = (u >> 8) & 255;     v = by + Y * ay;  y0 = v >> 16;  wy = (v >> 8) & 255
    xa = clamp(x0, 0, 223), xb = clamp(x0 + 1, 0, 223), ya, yb likewise
    top = Z[ya][xa] * (256 - wx) + Z[ya][xb] * wx;   bot = the same on row yb;   out = (top * (256 - wy) + bot * wy + 32768) >> 16
The kernel clamps ax, ay to [0, 65536] and bx, by to +-224 * 65536 before use; so does `clamp_rows`."""
import numpy as np

import aug_color_oracle
import aug_oracle
from aug_oracle import M64, splitmix64

ZOOM_STREAM = 0x4155475A4F4F4D31  # "AUGZOOM1"
ONE = 65536
MAX_JZ = 32768
MAX_ORIGIN = 224 * 65536
IDENTITY = (ONE, ONE, 0, 0)


def jz(j: float) -> int:
    """Q16 width of the side range [1 - J, 1]."""
    return int(j * 65536 + 0.5)


def origin(a: int, hk: int) -> int:
    r = (224 * ONE - 224 * a) >> 8
    o = ((hk * (r + 1)) >> 16) << 8
    return o + (a >> 1) - 32768


def draw(seed: int, step: int, global_batch: int, jz: int, aspect: bool, first: int = 0, n: int = None) -> np.ndarray:
    """int32 [n][4] {ax, ay, bx, by} of samples first .. first + n of the global batch at update `step`; jz in 0 .. 32768."""
    n = global_batch - first if n is None else n
    key = splitmix64((seed & M64) ^ ZOOM_STREAM)
    out = np.zeros((n, 4), np.int32)
    for i in range(n):
        h = splitmix64(key ^ (((step & M64) * global_batch + first + i) & M64))
        hk = [(h >> (16 * k)) & 0xFFFF for k in range(4)]
        ax = ONE - ((hk[0] * (jz + 1)) >> 16)
        ay = ONE - ((hk[1] * (jz + 1)) >> 16) if aspect else ax
        out[i] = (ax, ay, origin(ax, hk[2]), origin(ay, hk[3]))
    return out


def clamp_rows(rows: np.ndarray) -> np.ndarray:
    """int64 [n][4]: the rows as the kernel uses them."""
    rows = np.asarray(rows).reshape(-1, 4).astype(np.int64)
    return np.concatenate([np.clip(rows[:, :2], 0, ONE), np.clip(rows[:, 2:], -MAX_ORIGIN, MAX_ORIGIN)], 1)


def taps(a: int, b: int):
    """One axis of a clamped row -> (index of the first tap, index of the second, weight of the second), each int64 [224]."""
    u = b + np.arange(224, dtype=np.int64) * a
    i0 = u >> 16
    return np.clip(i0, 0, 223), np.clip(i0 + 1, 0, 223), (u >> 8) & 255


def resample(frame: np.ndarray, row) -> np.ndarray:
    """frame uint8 [224][224][3], row {ax, ay, bx, by} (clamped here) -> uint8 [224][224][3]."""
    ax, ay, bx, by = (int(v) for v in clamp_rows(row)[0])
    xa, xb, wx = taps(ax, bx)
    ya, yb, wy = taps(ay, by)
    z = np.asarray(frame).astype(np.int64)
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = z[ya][:, xa] * (256 - wx) + z[ya][:, xb] * wx
    bot = z[yb][:, xa] * (256 - wx) + z[yb][:, xb] * wx
    out = (top * (256 - wy) + bot * wy + 32768) >> 16
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def zoom(frames: np.ndarray, rows: np.ndarray, frames_per_sample: int = 1) -> np.ndarray:
    """frames uint8 [n][224][224][3]; frame i takes rows[(i // frames_per_sample) % len(rows)]."""
    frames = np.asarray(frames)
    rows = np.asarray(rows).reshape(-1, 4)
    out = np.empty_like(frames)
    for i in range(frames.shape[0]):
        out[i] = resample(frames[i], rows[(i // frames_per_sample) % len(rows)])
    return out


def augment(frames: np.ndarray, params: np.ndarray, rows: np.ndarray, color: np.ndarray = None, frames_per_sample: int = 1) -> np.ndarray:
    """The composition the pack applies: color(zoom(shift_mirror(frames))); `color` None = no colour transform."""
    out = zoom(aug_oracle.augment_frames(frames, params, frames_per_sample), rows, frames_per_sample)
    return out if color is None else aug_color_oracle.color(out, color, frames_per_sample)


def source_rows(row, sy: int, Y0: int) -> np.ndarray:
    """The distinct source rows the four output rows Y0 .. Y0 + 3 read under a (clamped) zoom row and a vertical shift sy (clamped to
    +-224 as the kernel does), sorted."""
    _, ay, _, by = (int(v) for v in clamp_rows(row)[0])
    sy = min(max(int(sy), -224), 224)
    v = by + np.arange(Y0, Y0 + 4, dtype=np.int64) * ay
    y0 = v >> 16
    t = np.concatenate([np.clip(y0, 0, 223), np.clip(y0 + 1, 0, 223)])
    return np.unique(np.clip(t + sy, 0, 223))
