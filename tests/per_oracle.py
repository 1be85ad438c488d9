"""numpy restatement of the prioritized-replay kernels (video_dqn_amd/csrc/replay.hip): the same f64 sums in the same order,
so the draws match the device's index for index."""
import numpy as np

SEG, SEGS_PER_CHUNK = 32, 64
CHUNK = SEG * SEGS_PER_CHUNK
EPS = 1e-6
M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def uniforms(seed: int, step: int, G: int) -> np.ndarray:
    key = splitmix64(seed & M64)
    return np.array([(splitmix64(key ^ ((step * G + j) & M64)) >> 11) * 2.0 ** -53 for j in range(G)], dtype=np.float64)


def _left_to_right(x2d: np.ndarray) -> np.ndarray:
    acc = np.zeros(x2d.shape[0], dtype=np.float64)
    for k in range(x2d.shape[1]):
        acc = acc + x2d[:, k]
    return acc


def sums(p: np.ndarray):
    """-> (seg, chunk, P): segment sums, chunk sums and the chunk prefix (S = P[-1])."""
    p = np.asarray(p, dtype=np.float32).astype(np.float64)
    n = p.shape[0]
    nchunk = -(-n // CHUNK)
    pad = np.zeros(nchunk * CHUNK, dtype=np.float64)
    pad[:n] = p
    seg = _left_to_right(pad.reshape(-1, SEG))
    chunk = _left_to_right(seg.reshape(-1, SEGS_PER_CHUNK))
    P = np.cumsum(chunk)  # add.accumulate: strictly left to right
    return seg, chunk, P


def _first_exceeding(vals: np.ndarray, t: float):
    run, before = 0.0, 0.0
    for k, v in enumerate(vals):
        nr = run + v
        if nr > t:
            return k, run
        run = nr
    return -1, before


def sample(p, G: int, seed: int, step: int, beta: float):
    """-> (idx int64 [G], weight float32 [G]) as vdqn_per_sample computes them."""
    p32 = np.asarray(p, dtype=np.float32)
    n = p32.shape[0]
    seg, chunk, P = sums(p32)
    S = P[-1]
    nseg = -(-n // SEG)
    nz = np.nonzero(chunk > 0)[0]
    last_chunk = int(nz[-1]) if nz.size else -1
    r = uniforms(seed, step, G)
    idx = np.zeros(G, dtype=np.int64)
    for j in range(G):
        u = ((np.float64(j) + r[j]) * S) / np.float64(G)
        c = int(np.searchsorted(P, u, side="right"))  # smallest c with P[c] > u
        if c < len(P):
            t = u - P[c - 1] if c > 0 else u
        else:
            c, t = last_chunk, np.inf
        if c < 0:
            continue
        s0, s_end = c * SEGS_PER_CHUNK, min((c + 1) * SEGS_PER_CHUNK, nseg)
        sv = seg[s0:s_end]
        k, before = _first_exceeding(sv, t)
        if k >= 0:
            s, t2 = s0 + k, t - before
        else:
            s, t2 = s0 + int(np.nonzero(sv > 0)[0][-1]), np.inf
        e0, e_end = s * SEG, min(s * SEG + SEG, n)
        ev = p32[e0:e_end].astype(np.float64)
        k2, _ = _first_exceeding(ev, t2)
        if k2 >= 0:
            idx[j] = e0 + k2
        else:
            pos = np.nonzero(ev > 0)[0]
            idx[j] = e0 + (int(pos[-1]) if pos.size else 0)
    w = np.power(np.float64(n) * p32[idx].astype(np.float64) / S, -beta)
    return idx, (w / w.max()).astype(np.float32)


def update(p, idx, err, alpha: float) -> np.ndarray:
    """vdqn_per_update: p[idx[j]] = (err[j] + EPS)^alpha, the largest j winning a repeated index."""
    out = np.array(p, dtype=np.float32, copy=True)
    for j in range(len(idx)):  # ascending j: a later store overwrites an earlier one
        out[idx[j]] = np.float32(np.power(np.float64(err[j]) + EPS, alpha))
    return out


def beta_at(beta0: float, step: int, num_steps: int) -> float:
    return beta0 + (1.0 - beta0) * min(1.0, step / max(1, num_steps))
