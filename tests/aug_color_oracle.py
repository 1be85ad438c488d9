"""numpy restatement of the colour-jitter augmentation (video_dqn_amd/csrc/augment.hip): the per-sample draw of the Q8 factors and the
uint8 -> uint8 transform, written from the arithmetic alone.  The GPU tests compare the kernels against it bit for bit.

All integers; "// 256" is floor division.  Factors are Q8: 256 = 1.0.  One source pixel (R, G, B), in this fixed order:
    saturation:  g = (77 R + 150 G + 29 B + 128) // 256;  v = clamp(g + ((v - g) * f_s + 128) // 256, 0, 255)  for v in R, G, B
    brightness:  v = min(255, (v * f_b + 128) // 256)
    contrast:    v = clamp(128 + ((v - 128) * f_c + 128) // 256, 0, 255)
The kernel clamps every factor to [0, 512] before use; so does `color`."""
import numpy as np

from aug_oracle import M64, splitmix64

COLOR_STREAM = 0x415547434F4C5231  # "AUGCOLR1"
MAX_FACTOR = 512


def jq(j: float) -> int:
    """Q8 half-width of a factor range [1 - J, 1 + J]."""
    return int(j * 256 + 0.5)


def draw(seed: int, step: int, global_batch: int, jb: int, jc: int, js: int, first: int = 0, n: int = None) -> np.ndarray:
    """int32 [n][4] {f_b, f_c, f_s, 0} of samples first .. first + n of the global batch at update `step`; jb, jc, js in 0 .. 256."""
    n = global_batch - first if n is None else n
    key = splitmix64((seed & M64) ^ COLOR_STREAM)
    out = np.zeros((n, 4), np.int32)
    for i in range(n):
        h = splitmix64(key ^ (((step & M64) * global_batch + first + i) & M64))
        for k, j in enumerate((jb, jc, js)):
            out[i, k] = 256 - j + ((((h >> (16 * k)) & 0xFFFF) * (2 * j + 1)) >> 16)
    return out


def saturation(px: np.ndarray, fs: int) -> np.ndarray:
    """px integer [..., 3] with values 0 .. 255 -> int64 [..., 3]."""
    px = np.asarray(px).astype(np.int64)
    g = (77 * px[..., 0] + 150 * px[..., 1] + 29 * px[..., 2] + 128) // 256
    g = g[..., None]
    return np.clip(g + ((px - g) * int(fs) + 128) // 256, 0, 255)


def brightness(v: np.ndarray, fb: int) -> np.ndarray:
    return np.minimum(255, (np.asarray(v).astype(np.int64) * int(fb) + 128) // 256)


def contrast(v: np.ndarray, fc: int) -> np.ndarray:
    return np.clip(128 + ((np.asarray(v).astype(np.int64) - 128) * int(fc) + 128) // 256, 0, 255)


def bc(fb: int, fc: int) -> np.ndarray:
    """The byte -> byte map that follows saturation: int64 [256]."""
    return contrast(brightness(np.arange(256), fb), fc)


def color(frames: np.ndarray, factors: np.ndarray, frames_per_sample: int = 1) -> np.ndarray:
    """frames uint8 [n][224][224][3]; frame i takes factors[(i // frames_per_sample) % len(factors)], each clamped to [0, 512]."""
    frames = np.asarray(frames)
    factors = np.clip(np.asarray(factors).reshape(-1, 4).astype(np.int64), 0, MAX_FACTOR)
    out = np.empty_like(frames)
    for i in range(frames.shape[0]):
        fb, fc, fs = (int(v) for v in factors[(i // frames_per_sample) % len(factors)][:3])
        out[i] = contrast(brightness(saturation(frames[i], fs), fb), fc).astype(np.uint8)
    return out
