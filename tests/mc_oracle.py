"""Oracles of the Monte-Carlo return table (vdqn_mc_returns, video_dqn_amd/csrc/mcreturn.hip) and of its two uses inside the TD-loss
launch (vdqn_td_loss_mc, csrc/pointwise.hip).

`returns_f32` restates the table's pointer-doubling rounds in numpy float32, operation for operation (every product and sum rounds
on its own): the kernel's bits.  `returns_f64_walk` is the definition itself,

    G(i) = sum_{k < 2^R} g^k prod_{j<k}(1 - t(i_j)) r(i_k),

walked row by row in float64 — it shares neither the doubling nor the order of the sums with the kernel — and S, the same sum over
|r|, which scales the rounding bound.  `objective` is the float64 loss with the floor and the calibrated penalty, differentiated by
autograd; it takes its inputs and its unpacking from tests/cql_oracle.py and states the target itself (the floor sits between
cql_oracle's target and its clip)."""
import numpy as np
import torch

import cql_oracle

F = np.float32


def sanitise(next_row, N):
    nr = np.asarray(next_row).astype(np.int64)
    return np.where((nr < 0) | (nr >= N), -1, nr)


def returns_f32(next_row, rew, term, gamma, rounds):
    """-> G f32 [N, n_cat]: the kernel's rounds.  State (j, A, B); all float arrays are float32, so each product and each sum rounds
    once; every round builds new arrays from the old ones (no update in place)."""
    rew, term = np.asarray(rew, dtype=F), np.asarray(term, dtype=F)
    N = rew.shape[0]
    j = sanitise(next_row, N)
    B = rew.copy()
    A = (F(gamma) * (F(1) - term)).astype(F)
    for _ in range(int(rounds)):
        has = j >= 0
        jj = np.where(has, j, 0)
        prod = (A * B[jj]).astype(F)
        B_new = np.where(has[:, None], (B + prod).astype(F), B)
        A_new = np.where(has[:, None], (A * A[jj]).astype(F), F(0))
        j_new = np.where(has, j[jj], -1)
        j, A, B = j_new, A_new.astype(F), B_new.astype(F)
    assert B.dtype == F and A.dtype == F
    return B


def returns_f64_walk(next_row, rew, term, gamma, rounds):
    """-> (G, S) float64 [N, n_cat]: the recurrence walked for 2^rounds rows of every chain, and the same with |r|.  gamma is the
    float32 the kernel is handed (the bound counts the roundings of operations, not of the caller's constant)."""
    rew, term = np.asarray(rew, dtype=np.float64), np.asarray(term, dtype=np.float64)
    N = rew.shape[0]
    nr = sanitise(next_row, N)
    g = float(F(gamma))
    cur = np.arange(N)
    alive = np.ones(N, bool)
    w = np.ones_like(rew)  # g^k prod_{j<k} (1 - t(i_j))
    G, S = np.zeros_like(rew), np.zeros_like(rew)
    for _ in range(2 ** int(rounds)):
        r = rew[cur] * alive[:, None]
        G += w * r
        S += np.abs(w) * np.abs(r)
        w = w * (g * (1.0 - term[cur]))
        nxt = nr[cur]
        alive = alive & (nxt >= 0)
        if not alive.any():
            break
        cur = np.where(alive, nxt, cur)
    return G, S


def bound(rounds, S):
    """|f32 - f64| <= (3 R + 3) 2^-24 S per element: three roundings per round (A * B[j], the sum, and A * A[j] feeding the next
    round's product) on a quantity bounded by S, plus the three of the initial state (1 - t, g * (1 - t), and r itself exact)."""
    return (3 * int(rounds) + 3) * 2.0 ** -24 * S


def tables(N, n_cat, seed, fractional=False):
    """Chains i -> i + 3 (a backup row spans three frames) with random breaks; from N > 11 on a self-loop, a 2-cycle and the successors
    -7, N and 2^31 - 1 (all "none").  Binary rewards with term = rew (the reference's labels), or fractional rewards and terminals.
    -> (next_row int32 [N], rew f32 [N, n_cat], term f32 [N, n_cat])."""
    rng = np.random.default_rng(seed)
    next_row = np.arange(N, dtype=np.int64) + 3
    next_row[next_row >= N] = -1
    next_row[rng.random(N) < 0.02] = -1
    if N > 11:
        next_row[0] = 0                    # a self-loop
        next_row[1], next_row[2] = 2, 1    # a 2-cycle
        next_row[3] = -7                   # outside the table: "none"
        next_row[4] = N                    # one past the end
        next_row[5] = 2**31 - 1            # the largest int32
    if fractional:
        rew = rng.random((N, n_cat)).astype(F)
        term = (rng.random((N, n_cat)) * 0.9).astype(F)
    else:
        rew = (rng.random((N, n_cat)) < 0.05).astype(F)
        term = rew.copy()
    return next_row.astype(np.int32), rew, term


# ---- the loss ------------------------------------------------------------------------------------------------------------------------
FLOOR, CALIBRATED = 1, 2


def objective(inputs, alpha, G, flags, *, weight=None, use_valid=True, loss_kind=0, clip_rect=1, gamma=0.9, discount=None, n_cat=5,
              n_act=3, inv_count=None):
    """float64, autograd.  inputs as cql_oracle.td_inputs; G [B, n_cat]; discount [B] or None (the scalar gamma); alpha 0 = no penalty.
    -> dict(loss, penalty, dq [B, n_cat * n_act], err [B], stats [2], y_pre [B, n_cat] (the target before floor and clip), raised
    [B, n_cat] bool)."""
    q, qo3, qt3, act, rew, term, vm, w = cql_oracle._f64(inputs, n_cat, n_act, weight, use_valid)
    B = q.shape[0]
    G = G.detach().cpu().double()
    inv = float(F(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    disc = torch.full((B, 1), float(gamma), dtype=torch.float64) if discount is None else discount.detach().cpu().double().view(B, 1)
    best = qo3.argmax(2, keepdim=True)
    qa = qt3.gather(2, best).squeeze(2) * (1 - term)
    y_pre = rew + disc * qa
    raised = G > y_pre
    y = torch.maximum(y_pre, G) if flags & FLOOR else y_pre
    if clip_rect:
        y = y.clamp(0, 1)  # the clip keeps the last word
    q = q.clone().requires_grad_(True)
    q_s = q.gather(2, act.view(B, 1, 1).expand(B, n_cat, 1)).squeeze(2)
    if loss_kind == 1:
        l = torch.nn.functional.smooth_l1_loss(q_s, y, reduction="none", beta=1.0)
    else:
        l = 0.5 * (q_s - y) ** 2
    if flags & CALIBRATED:
        Gc = G.unsqueeze(2).expand_as(q)
        qc = torch.where(q >= Gc, q, Gc)  # at a tie the Q value takes the gradient (torch.maximum would halve it)
    else:
        qc = q
    pen = torch.logsumexp(qc, 2) - q_s
    s = w.view(B, 1) * vm
    loss = inv * (s * (l + alpha * pen)).sum() if alpha > 0 else inv * (s * l).sum()
    dq, = torch.autograd.grad(loss, q)
    d = (q_s - y).detach()
    stats = torch.stack([inv * (vm * raised.double()).sum(), inv * (vm * (q_s.detach() - G)).sum()])
    return dict(loss=loss.detach(), penalty=(inv * (s * pen).sum()).detach(), dq=dq.reshape(B, n_cat * n_act), err=(d.abs() * vm).sum(1) / n_cat,
                stats=stats, y_pre=y_pre, raised=raised, d=d)


def loss_inputs(B, seed, *, ldq=64, n_cat=5, n_act=3, gamma=0.9, discount=None):
    """cql_oracle.td_inputs plus a return table G [B, n_cat] drawn around the targets: G = y_pre +- U(0.05, 0.5), the sign alternating, so
    the floor raises about half of the targets and no |y_pre - G| is small — except the ties built in from exactly representable
    values: term = 1, G = r (y_pre == r == G exactly in float32 and float64), and Q(s, a) == G on some (b, c, a) for the calibrated
    gradient.  -> (inputs, G, tie_y [B, n_cat] bool, tie_q [B, n_cat, n_act] bool)."""
    inputs = cql_oracle.td_inputs(B, seed, ldq=ldq, n_cat=n_cat, n_act=n_act)
    qb, qo, qt, act, rew, term, valid = inputs
    g = torch.Generator().manual_seed(seed + 1000)
    tie_y = torch.rand(B, n_cat, generator=g) < 0.1
    tie_y[0, 0] = True
    term[tie_y] = 1.0
    rew[tie_y] = (torch.randint(0, 5, (B, n_cat), generator=g).float() * 0.25)[tie_y]  # 0, 0.25, .., 1: exact
    n = n_cat * n_act
    disc = torch.full((B, 1), float(gamma), dtype=torch.float64) if discount is None else discount.double().view(B, 1)
    best = qo[:, :n].reshape(B, n_cat, n_act).double().argmax(2, keepdim=True)
    y_pre = rew.double() + disc * qt[:, :n].reshape(B, n_cat, n_act).double().gather(2, best).squeeze(2) * (1 - term.double())
    sign = ((torch.arange(B).view(B, 1) + torch.arange(n_cat).view(1, n_cat)) % 2) * 2 - 1  # alternating: half of the targets either way
    delta = (torch.rand(B, n_cat, generator=g, dtype=torch.float64) * 0.45 + 0.05) * sign
    G = (y_pre + delta).float()
    G[tie_y] = rew[tie_y]
    tie_q = torch.rand(B, n_cat, n_act, generator=g) < 0.1
    tie_q[0, n_cat - 1, 0] = True
    q3 = qb[:, :n].reshape(B, n_cat, n_act).clone()
    q3[tie_q] = G.unsqueeze(2).expand(B, n_cat, n_act)[tie_q]
    qb[:, :n] = q3.reshape(B, n)
    return inputs, G.contiguous(), tie_y, tie_q
