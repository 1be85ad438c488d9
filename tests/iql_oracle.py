"""Oracle of the implicit Q-learning loss (vdqn_td_loss_iql, csrc/iql.hip), in float64.

A row of ldq columns holds Q(c, a) at column c * A + a and V(c) at column C * A + c.  With a* = act[b], tau the expectile,
s_bc = w_b * vm_bc (w_b = 1 without weights, vm_bc = valid or 1):

    v   = Q_online(s )[b][V(c)]            v'  = Q_online(s')[b][V(c)]   (no gradient through v')
    qt  = Q_target(s )[b][Q(c, a*)]        (the TARGET network at s, not at s')
    u   = qt - v        omega = (u > 0) ? tau : 1 - tau        L_V = omega u^2        dL_V/dv = -2 omega u
    y   = r + gamma_b ((1 - term) v')      rect clip on y; gamma_b = gamma or sample_gamma[b]
    d   = Q_online(s)[b][Q(c, a*)] - y     L_Q = l(d): half squared error or Huber with beta 1
    loss     = inv * sum s_bc (L_Q + L_V)      stats[0] = inv * sum s_bc L_V      stats[1] = inv * sum vm_bc u
    err[b]   = sum_c |d_bc| vm_bc / C

`objective` writes that with torch ops and lets autograd differentiate it with respect to the whole Q(s) row; `closed_form` is the
gradient by hand.  The expectile weight has a kink at u = 0, where a float32 kernel and a float64 oracle may land on different
sides: `inputs` therefore guarantees min |u| >= 1e-3 over EVERY term (valid or not) by moving the few V(s) entries that come
closer; `min_abs_u` measures it, and tests/test_iql_cpu.py asserts it for every case in CASES, the seeds and shapes the GPU tests
use."""
import numpy as np
import torch

MIN_ABS_U = 1e-3

# (B, ldq, n_cat, n_act, seed) of every operator input the GPU tests generate
OPERATOR_SHAPES = [(96, 64, 5, 3), (1, 64, 5, 3), (3, 64, 5, 3), (96, 20, 5, 3), (7, 6, 2, 2)]
OPERATOR_SEEDS = [11, 12, 13, 14]
TWIN_CASE = (70, 64, 5, 3, 29)
DET_CASE = (96, 64, 5, 3, 41)
HALVES_CASE = (8, 64, 5, 3, 17)
OPS_CASE = (5, 64, 5, 3, 2)
CASES = [s + (seed,) for s in OPERATOR_SHAPES for seed in OPERATOR_SEEDS] + [TWIN_CASE, DET_CASE, HALVES_CASE, OPS_CASE]


def inputs(B, seed, ldq=64, n_cat=5, n_act=3, scale=0.7):
    """-> [q_before, q_after_online, q_target_before (f32 [B, ldq]), act i64 [B], rew, term, valid (f32 [B, n_cat])]: the draws of
    tests/cql_oracle.py::td_inputs, then every V(s) whose u = Q_target(s, a*) - V(s) is closer to 0 than 4 * MIN_ABS_U is moved to
    qt - 8 * MIN_ABS_U (u = +8e-3 up to one float32 rounding)."""
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, ldq, generator=g) * scale for _ in range(3)]
    act = torch.randint(0, n_act, (B,), generator=g)
    rew = (torch.rand(B, n_cat, generator=g) < 0.3).float()
    term = (torch.rand(B, n_cat, generator=g) < 0.2).float()
    valid = (torch.rand(B, n_cat, generator=g) < 0.8).float()
    n = n_cat * n_act
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    qt = q[2].gather(1, cols)
    v = q[0][:, n:n + n_cat]
    near = (qt - v).abs() < 4 * MIN_ABS_U
    q[0][:, n:n + n_cat] = torch.where(near, qt - 8 * MIN_ABS_U, v)
    return q + [act, rew, term, valid]


def _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma):
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in inp]
    B = qb.shape[0]
    vm = valid if use_valid else torch.ones_like(rew)
    w = torch.ones(B, dtype=torch.float64) if weight is None else weight.detach().cpu().double()
    g = torch.full((B, 1), float(np.float32(gamma)), dtype=torch.float64) if discount is None else discount.detach().cpu().double().view(B, 1)
    return qb, qo, qt, act, rew, term, vm, w, g


def _parts(row, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect):
    """(Q(s, a*), V(s), u, y) [B, n_cat] from the Q(s) row `row` [B, >= n_cat * n_act + n_cat]."""
    B, n = row.shape[0], n_cat * n_act
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    q_s = row.gather(1, cols)
    v = row[:, n:n + n_cat]
    u = qt.gather(1, cols) - v
    y = rew + g * ((1 - term) * qo[:, n:n + n_cat])
    return q_s, v, u, (y.clamp(0, 1) if clip_rect else y)


def min_abs_u(inp, n_cat=5, n_act=3):
    """The smallest |Q_target(s, a*) - V(s)| over every (sample, category) term of `inp`, none excluded."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, None, False, None, 0.9)
    return _parts(qb, qo, qt, act, rew, term, g, n_cat, n_act, True)[2].abs().min().item()


def objective(inp, tau, *, weight=None, use_valid=True, loss_kind=0, clip_rect=1, gamma=0.9, discount=None, n_cat=5, n_act=3,
              inv_count=None):
    """float64, autograd.  -> dict(loss, v_loss, advantage, dq [B, n_cat * n_act + n_cat], err [B], d, u [B, n_cat])."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    tau = float(np.float32(tau))
    row = qb[:, :n + n_cat].clone().requires_grad_(True)
    q_s, v, u, y = _parts(row, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect)
    if loss_kind == 1:
        l_q = torch.nn.functional.smooth_l1_loss(q_s, y, reduction="none", beta=1.0)
    else:
        l_q = 0.5 * (q_s - y) ** 2
    l_v = torch.where(u > 0, torch.full_like(u, tau), torch.full_like(u, 1 - tau)) * u ** 2
    s = w.view(B, 1) * vm
    loss = inv * (s * (l_q + l_v)).sum()
    dq, = torch.autograd.grad(loss, row)
    d = (q_s - y).detach()
    return dict(loss=loss.detach(), v_loss=inv * (s * l_v).sum().detach(), advantage=inv * (vm * u).sum().detach(), dq=dq,
                err=(d.abs() * vm).sum(1) / n_cat, d=d, u=u.detach())


def closed_form(inp, tau, *, weight=None, use_valid=True, loss_kind=0, clip_rect=1, gamma=0.9, discount=None, n_cat=5, n_act=3,
                inv_count=None):
    """float64 by hand: dq[b][Q(c, a*)] = dl(d) s inv, dq[b][V(c)] = -2 omega u s inv, every other column 0.  -> dq [B, n + n_cat]."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))
    tau = float(np.float32(tau))
    q_s, v, u, y = _parts(qb, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect)
    d = q_s - y
    dl = d.clamp(-1, 1) if loss_kind == 1 else d
    s = w.view(B, 1) * vm
    dq = torch.zeros(B, n + n_cat, dtype=torch.float64)
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    dq.scatter_(1, cols, dl * s * inv)
    om = torch.where(u > 0, torch.full_like(u, tau), torch.full_like(u, 1 - tau))
    dq[:, n:] = -2 * om * u * s * inv
    return dq
