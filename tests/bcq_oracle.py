"""Oracle of the discrete BCQ loss (vdqn_td_loss_bcq, csrc/bcq.hip), in float64.

A row of ldq columns holds Q(c, a) at column c * A + a and the behaviour logit i(a) at column C * A + a.  With a* = act[b],
s_bc = w_b * vm_bc (w_b = 1 without weights, vm_bc = valid or 1), i the logits of Q_online(s) and i' those of Q_online(s'):

    allowed(a) = (i'_a - max i') > log(threshold)      (threshold 0: every action)
    a'  = first arg-max of Q_online(s')[c, a] over the allowed a          a0 = the free first arg-max
    y   = r + gamma_b ((1 - term) Q_target(s')[c, a'])      rect clip on y; gamma_b = gamma or sample_gamma[b]
    d   = Q_online(s)[c, a*] - y                            l(d): half squared error or Huber with beta 1
    ce_b = logsumexp(i) - i_{a*}      reg_b = mean_a i_a^2      L_B = bc_weight (ce_b + logit_reg reg_b)
    loss = inv * sum_bc s_bc l(d_bc) + C inv * sum_b w_b L_B
    err[b] = sum_c |d_bc| vm_bc / C
    ce = C inv sum_b ce_b      constrained_share = inv sum_bc vm_bc [a' != a0]      accuracy = C inv sum_b [argmax i == a*]

`objective` writes that with torch ops and lets autograd differentiate it with respect to the whole Q(s) row; `closed_form` is the
gradient by hand.  The allowed set is a comparison of a float32 difference with a float32 constant in the kernel and of float64
ones here; `inputs` therefore keeps every non-arg-max logit of s' at least MARGIN away from the boundary of every threshold in
THRESHOLDS, and every two online Q(s') values of one (sample, category) at least MARGIN apart, so both take the same branch;
`margin` measures the two, and tests/test_bcq_cpu.py asserts them for every case in CASES, the seeds and shapes the GPU tests use.
The logits of s' are drawn wider than the Q values (LOGIT_SCALE) so that threshold 0.3 changes a good share of the targets."""
import math

import numpy as np
import torch

MARGIN = 1e-3
THRESHOLDS = (0.0, 0.3, 0.9)
LOGIT_SCALE = 2.0

# (B, ldq, n_cat, n_act) of every operator input the GPU tests generate: iql_oracle.OPERATOR_SHAPES with ldq adapted to C * A + A
OPERATOR_SHAPES = [(96, 64, 5, 3), (1, 64, 5, 3), (3, 64, 5, 3), (96, 18, 5, 3), (7, 6, 2, 2)]
OPERATOR_SEEDS = [11, 12, 13, 14]
TWIN_CASE = (70, 64, 5, 3, 29)
DET_CASE = (96, 64, 5, 3, 41)
HALVES_CASE = (8, 64, 5, 3, 17)
OPS_CASE = (5, 64, 5, 3, 2)
CASES = [s + (seed,) for s in OPERATOR_SHAPES for seed in OPERATOR_SEEDS] + [TWIN_CASE, DET_CASE, HALVES_CASE, OPS_CASE]


def log_threshold(threshold):
    """log of the float32 the kernel is handed, in float64; -inf for 0."""
    t = float(np.float32(threshold))
    return math.log(t) if t > 0 else -math.inf


def inputs(B, seed, ldq=64, n_cat=5, n_act=3, scale=0.7):
    """-> [q_before, q_after_online, q_after_target (f32 [B, ldq]), act i64 [B], rew, term, valid (f32 [B, n_cat])]: the draws of
    tests/cql_oracle.py::td_inputs with the logit columns of s' widened by LOGIT_SCALE; then every non-arg-max logit of s' closer
    than 4 * MARGIN to the boundary of a threshold is moved 8 * MARGIN below it, and every online Q(s') value closer than 4 * MARGIN
    to another of its (sample, category) is moved up by 16 * MARGIN until none is."""
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, ldq, generator=g) * scale for _ in range(3)]
    act = torch.randint(0, n_act, (B,), generator=g)
    rew = (torch.rand(B, n_cat, generator=g) < 0.3).float()
    term = (torch.rand(B, n_cat, generator=g) < 0.2).float()
    valid = (torch.rand(B, n_cat, generator=g) < 0.8).float()
    n = n_cat * n_act
    lg = q[1][:, n:n + n_act] * LOGIT_SCALE
    m = lg.max(1, keepdim=True).values
    for t in THRESHOLDS:
        if t > 0:
            lt = log_threshold(t)
            near = ((lg - m) - lt).abs() < 4 * MARGIN
            lg = torch.where(near, m + lt - 8 * MARGIN, lg)
    q[1][:, n:n + n_act] = lg
    qo = q[1][:, :n].clone().view(B, n_cat, n_act)
    for _ in range(8):
        moved = False
        for a1 in range(n_act):
            for a2 in range(a1 + 1, n_act):
                near = (qo[:, :, a1] - qo[:, :, a2]).abs() < 4 * MARGIN
                if near.any():
                    qo[:, :, a2] = torch.where(near, qo[:, :, a2] + 16 * MARGIN, qo[:, :, a2])
                    moved = True
        if not moved:
            break
    q[1][:, :n] = qo.reshape(B, n)
    return q + [act, rew, term, valid]


def _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma):
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in inp]
    B = qb.shape[0]
    vm = valid if use_valid else torch.ones_like(rew)
    w = torch.ones(B, dtype=torch.float64) if weight is None else weight.detach().cpu().double()
    g = torch.full((B, 1), float(np.float32(gamma)), dtype=torch.float64) if discount is None else discount.detach().cpu().double().view(B, 1)
    return qb, qo, qt, act, rew, term, vm, w, g


def allowed_set(qo, threshold, n_cat, n_act):
    """bool [B, n_act]: the actions the logits of the rows `qo` allow."""
    n = n_cat * n_act
    lg = qo[:, n:n + n_act]
    return (lg - lg.max(1, keepdim=True).values) > log_threshold(threshold)


def choices(qo, threshold, n_cat, n_act):
    """(a' [B, n_cat], a0 [B, n_cat]): the constrained and the free first arg-max of the online Q(s')."""
    B, n = qo.shape[0], n_cat * n_act
    q3 = qo[:, :n].reshape(B, n_cat, n_act)
    ok = allowed_set(qo, threshold, n_cat, n_act).view(B, 1, n_act)
    masked = torch.where(ok, q3, torch.full_like(q3, -math.inf))
    return masked.argmax(2), q3.argmax(2)


def _target(qo, qt, rew, term, g, threshold, n_cat, n_act, clip_rect):
    B, n = qo.shape[0], n_cat * n_act
    best, free = choices(qo, threshold, n_cat, n_act)
    qa = qt[:, :n].reshape(B, n_cat, n_act).gather(2, best.unsqueeze(2)).squeeze(2)
    y = rew + g * ((1 - term) * qa)
    return (y.clamp(0, 1) if clip_rect else y), best, free


def margin(inp, threshold, n_cat=5, n_act=3):
    """(the smallest |i'_a - m' - log(threshold)| over the non-arg-max actions of every sample, the smallest gap between the two best
    allowed online Q(s') values over every (sample, category)); inf where there is nothing to measure."""
    qo = inp[1].detach().cpu().double()
    B, n = qo.shape[0], n_cat * n_act
    lg = qo[:, n:n + n_act]
    rel = lg - lg.max(1, keepdim=True).values
    lt = log_threshold(threshold)
    not_max = torch.ones_like(rel, dtype=torch.bool)
    not_max[torch.arange(B), lg.argmax(1)] = False
    m_logit = (rel - lt).abs()[not_max].min().item() if (not_max.any() and lt > -math.inf) else math.inf
    ok = allowed_set(qo, threshold, n_cat, n_act).view(B, 1, n_act)
    q3 = qo[:, :n].reshape(B, n_cat, n_act)
    masked = torch.where(ok, q3, torch.full_like(q3, -math.inf))
    top = masked.sort(2, descending=True).values
    gap = top[:, :, 0] - top[:, :, 1]
    return m_logit, gap.min().item()


def changed_share(inp, threshold, n_cat=5, n_act=3):
    """The share of (sample, category) targets whose action the constraint changes, no mask."""
    best, free = choices(inp[1].detach().cpu().double(), threshold, n_cat, n_act)
    return (best != free).double().mean().item()


def objective(inp, threshold, *, weight=None, use_valid=True, loss_kind=0, clip_rect=1, gamma=0.9, discount=None, n_cat=5, n_act=3,
              inv_count=None, bc_weight=1.0, logit_reg=0.01):
    """float64, autograd.  -> dict(loss, td_loss, dq [B, n_cat * n_act + n_act], err [B], ce, constrained_share, accuracy, d, y, best)."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    bcw, reg = float(np.float32(bc_weight)), float(np.float32(logit_reg))
    row = qb[:, :n + n_act].clone().requires_grad_(True)
    y, best, free = _target(qo, qt, rew, term, g, threshold, n_cat, n_act, clip_rect)
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    q_s = row.gather(1, cols)
    l_q = torch.nn.functional.smooth_l1_loss(q_s, y, reduction="none", beta=1.0) if loss_kind == 1 else 0.5 * (q_s - y) ** 2
    lg = row[:, n:]
    ce = torch.logsumexp(lg, 1) - lg.gather(1, act.view(B, 1)).squeeze(1)
    l_b = bcw * (ce + reg * (lg ** 2).mean(1))
    td = inv * (w.view(B, 1) * vm * l_q).sum()
    loss = td + n_cat * inv * (w * l_b).sum()
    dq, = torch.autograd.grad(loss, row)
    d = (q_s - y).detach()
    return dict(loss=loss.detach(), td_loss=td.detach(), dq=dq, err=(d.abs() * vm).sum(1) / n_cat, ce=n_cat * inv * ce.detach().sum(),
                constrained_share=inv * (vm * (best != free).double()).sum(), accuracy=n_cat * inv * (lg.detach().argmax(1) == act).double().sum(),
                d=d, y=y, best=best)


def closed_form(inp, threshold, *, weight=None, use_valid=True, loss_kind=0, clip_rect=1, gamma=0.9, discount=None, n_cat=5, n_act=3,
                inv_count=None, bc_weight=1.0, logit_reg=0.01):
    """float64 by hand: dq[b][c * A + a*] = dl(d) s inv, dq[b][C * A + a] = bc_weight (softmax(i)_a - [a == a*] + logit_reg 2 i_a / A)
    w_b C inv, every other column 0.  -> dq [B, n + n_act]."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))
    bcw, reg = float(np.float32(bc_weight)), float(np.float32(logit_reg))
    y, _, _ = _target(qo, qt, rew, term, g, threshold, n_cat, n_act, clip_rect)
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    d = qb.gather(1, cols) - y
    dl = d.clamp(-1, 1) if loss_kind == 1 else d
    dq = torch.zeros(B, n + n_act, dtype=torch.float64)
    dq.scatter_(1, cols, dl * w.view(B, 1) * vm * inv)
    lg = qb[:, n:n + n_act]
    hit = torch.nn.functional.one_hot(act, n_act).double()
    dq[:, n:] = bcw * (torch.softmax(lg, 1) - hit + reg * 2 * lg / n_act) * w.view(B, 1) * (n_cat * inv)
    return dq
