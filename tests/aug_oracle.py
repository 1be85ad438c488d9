"""numpy restatement of the shift / mirror augmentation (video_dqn_amd/csrc/augment.hip): the per-sample draw, the frame transform
and the action exchange, written from the arithmetic alone.  The GPU tests compare the kernels against it bit for bit."""
import numpy as np

M64 = (1 << 64) - 1
AUG_STREAM = 0x4155474D454E5431  # "AUGMENT1"


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed: int, step: int, global_batch: int, pad: int, flip: bool, first: int = 0, n: int = None) -> np.ndarray:
    """int32 [n][4] {sx, sy, flip, 0} of samples first .. first + n of the global batch at update `step`."""
    n = global_batch - first if n is None else n
    key = splitmix64((seed & M64) ^ AUG_STREAM)
    out = np.zeros((n, 4), np.int32)
    for i in range(n):
        h = splitmix64(key ^ (((step & M64) * global_batch + first + i) & M64))
        out[i, 0] = (((h & 0xFFFF) * (2 * pad + 1)) >> 16) - pad
        out[i, 1] = ((((h >> 16) & 0xFFFF) * (2 * pad + 1)) >> 16) - pad
        out[i, 2] = (h >> 32) & 1 if flip else 0
    return out


def augment_frames(frames: np.ndarray, params: np.ndarray, frames_per_sample: int = 1) -> np.ndarray:
    """frames uint8 [n][224][224][3]; frame i takes params[(i // frames_per_sample) % len(params)]."""
    frames = np.asarray(frames)
    params = np.asarray(params).reshape(-1, 4).astype(np.int64)
    out = np.empty_like(frames)
    ar = np.arange(224, dtype=np.int64)
    for i in range(frames.shape[0]):
        sx, sy, flip = (int(v) for v in params[(i // frames_per_sample) % len(params)][:3])
        xs = np.clip(ar + sx, 0, 223)
        ys = np.clip(ar + sy, 0, 223)
        if flip != 0:
            xs = 223 - xs
        out[i] = frames[i][ys][:, xs]
    return out


def swap_actions(act: np.ndarray, params: np.ndarray, a0: int = 1, a1: int = 2) -> np.ndarray:
    act = np.asarray(act).copy()
    flipped = np.asarray(params).reshape(-1, 4)[:, 2] != 0
    is0, is1 = (act == a0) & flipped, (act == a1) & flipped
    act[is0], act[is1] = a1, a0
    return act
