"""Oracles of the n-step chain walk (vdqn_nstep_walk, video_dqn_amd/csrc/nstep.hip).

`walk_f32` restates the kernel's float32 arithmetic in numpy, operation for operation (every product and sum rounds on its own):
its five outputs are the kernel's bit for bit.  `nested_f64` evaluates the target the walk stands for,

    y = r(i0) + g (1 - t(i0)) [ r(i1) + g (1 - t(i1)) [ ... g (1 - t(i_{m-1})) Q(s^(m)) ] ]

from the inside out in float64 along the chain alone; it shares neither the accumulation order nor the early stop with the
kernel.  `target_from_walk` is what the loss launch makes of the walk's outputs: rew_n + disc * (1 - term_n) * Q(last row)."""
import numpy as np

F = np.float32


def walk_f32(idx, next_row, rew, term, n, gamma):
    """-> (rew_n [B, n_cat] f32, term_n [B, n_cat] f32, disc [B] f32, last_row [B] i64, steps [B] i32).  All samples at once: one
    pass of the loop body per chain row, samples whose walk has ended masked out; every array is float32, so each product and sum
    rounds once, as in the kernel."""
    idx = np.asarray(idx, dtype=np.int64)
    next_row = np.asarray(next_row, dtype=np.int64)
    rew, term = np.asarray(rew, dtype=F), np.asarray(term, dtype=F)
    N, n_cat = rew.shape
    B = idx.shape[0]
    gamma = F(gamma)
    row = np.clip(idx, 0, N - 1)
    w, g = np.ones((B, n_cat), F), np.zeros((B, n_cat), F)
    pw, m, last = np.ones(B, F), np.zeros(B, np.int32), row.copy()
    active = np.ones(B, bool)
    for step in range(n):
        a = active
        g[a] = g[a] + (pw[a, None] * w[a]) * rew[row[a]]
        w[a] = w[a] * (F(1) - term[row[a]])
        pw[a] = pw[a] * gamma
        m[a] += 1
        last[a] = row[a]
        if step + 1 == n:
            break
        nxt = next_row[row]
        active = a & (nxt >= 0) & (nxt < N) & np.any(w != 0, axis=1)
        row = np.where(active, nxt, row)
    assert g.dtype == F and w.dtype == F and pw.dtype == F
    return g, (F(1) - w).astype(F), pw, last, m


def chain(i0, next_row, n, N):
    """The rows the chain of row i0 provides: at most n, ending where the successor is outside [0, N)."""
    rows = [int(min(max(int(i0), 0), N - 1))]
    while len(rows) < n:
        nxt = int(next_row[rows[-1]])
        if nxt < 0 or nxt >= N:
            break
        rows.append(nxt)
    return rows


def nested_f64(idx, next_row, rew, term, n, gamma, q_boot):
    """float64 y [B, n_cat] of the nested formula; q_boot [N, n_cat] is Q_target(s', argmax_a Q_online(s', .)) of every row's own
    `after` frames (the chain's last row supplies s^(m))."""
    rew, term, q_boot = (np.asarray(x, dtype=np.float64) for x in (rew, term, q_boot))
    N = rew.shape[0]
    out = np.zeros((len(idx), rew.shape[1]))
    for b, i0 in enumerate(idx):
        rows = chain(i0, next_row, n, N)
        y = q_boot[rows[-1]]
        for r in reversed(rows):
            y = rew[r] + float(gamma) * (1.0 - term[r]) * y
        out[b] = y
    return out


def target_from_walk(walk, q_boot):
    """float32 y [B, n_cat] as td_error_of forms it (without the rect clip) from a walk's outputs: (qa * (1 - term_n)) * disc + rew_n,
    each operation rounded on its own (exact for the dyadic inputs the CPU test uses, so contraction could not change it)."""
    rew_n, term_n, disc, last_row, _ = walk
    qa = (np.asarray(q_boot, dtype=F)[last_row] * (F(1) - term_n)).astype(F)
    return (rew_n + (disc[:, None] * qa).astype(F)).astype(F)


def tables(N, n_cat, seed, fractional=False):
    """A successor table with every case the walk has to get right (as far as N allows) and reward / terminal tables.
    -> (next_row int32 [N], rew f32 [N, n_cat], term f32 [N, n_cat])."""
    rng = np.random.default_rng(seed)
    next_row = rng.integers(0, N, N).astype(np.int64)
    if N >= 7:
        next_row[0] = 0               # a self-loop
        next_row[1], next_row[2] = 2, 1  # a 2-cycle
        next_row[3] = -1              # no successor
        next_row[4] = -7              # outside the table: "none"
        next_row[5] = N               # likewise, one past the end
        next_row[6] = 2**31 - 1       # likewise, the largest int32
    if N >= 300:
        next_row[10:40] = np.arange(11, 41)  # a chain of 31 rows: longer than any n
        next_row[40] = -1
        next_row[50:52] = [51, -1]           # a chain of 2 rows: shorter than n = 3
    if fractional:
        rew = rng.random((N, n_cat)).astype(F)
        term = (rng.random((N, n_cat)) * 0.9).astype(F)
    else:
        rew = (rng.random((N, n_cat)) < 0.3).astype(F)
        term = (rng.random((N, n_cat)) < 0.15).astype(F)
    return next_row.astype(np.int32), rew, term


def indices(N, B, seed):
    """B sample indices: random rows with repeats, the special rows of `tables`, and values below 0 and >= N (clamped)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, N, B).astype(np.int64)
    special = [0, 1, 3, 4, 5, 6, 10, 50, -1, -2**40, N, N + 5, 2**40, 0, 0]
    for k, v in enumerate(special[:B]):
        idx[B - 1 - k] = v
    return idx
