"""Oracle of the Gaussian distributional loss (vdqn_td_loss_dist, csrc/dist.hip).

A row of ldq columns holds the mean of (c, a) at column M(c, a) = c * A + a and its spread parameter rho at column
S(c, a) = C * A + c * A + a.  With a* = act[b], smin2 = sigma_min^2, s_bc = w_b * vm_bc (w_b = 1 without weights, vm_bc = valid or 1),
gamma_b = gamma or sample_gamma[b]:

    var(rho) = e(rho) + smin2;  LOG_SIGMA: e = exp(2 clamp(rho, -8, 4));  otherwise e = softplus(rho)^2 (rho > 20: softplus = rho)
    a'  = first arg-max of Q_online(s')[b][M(c, .)]
    mt  = Q_target(s')[b][M(c, a')]          vt = var(Q_target(s')[b][S(c, a')])
    m   = r + gamma_b ((1 - term) mt), rect clip        g = gamma_b (1 - term)        v = max(g^2 vt, smin2)
    mu  = Q_online(s)[b][M(c, a*)]           s2 = var(Q_online(s)[b][S(c, a*)])         d = mu - m
    KL_BACKWARDS False: L = KL(N(m, v) || N(mu, s2))        True: L = KL(N(mu, s2) || N(m, v))
    loss = inv * sum s_bc L      stats[0] = inv * sum vm_bc sqrt(s2)      stats[1] = inv * sum vm_bc d^2 / s2
    err[b] = sum_c |d_bc| vm_bc / C

`objective` states that in float64 with torch.distributions.Normal and kl_divergence and lets autograd differentiate it with respect
to the whole Q(s) row; `closed_form` is the gradient by hand in float64; `restate_f32` is the closed form in numpy float32 in the
kernel's expression order — its distance from `objective` is the rounding the arithmetic itself carries, and the GPU tests gate the
kernel's dq at four times that distance, case by case.

The arg-max has a kink where two means of Q_online(s') tie, and the LOG_SIGMA clamp one at rho = -8 and rho = 4 (softplus switches
form at rho = 20), where a float32 kernel and a float64 oracle may land on different sides.  `inputs` keeps every arg-max gap at
ARGMAX_GAP or more by raising the few maxima that come closer; the spread draws (randn * 0.7) stay far inside the clamp, and a test
that wants entries outside places them there on purpose.  `argmax_gap` and `clamp_margin` measure both, and tests/test_distributional_cpu.py
asserts them for every case in CASES, the seeds and shapes the GPU tests use."""
import numpy as np
import torch

ARGMAX_GAP = 1e-3
CLAMP_MARGIN = 1e-2
CLAMP_LO, CLAMP_HI, SOFTPLUS_LINEAR = -8.0, 4.0, 20.0

# (B, ldq, n_cat, n_act) of every operator input the GPU tests generate, then the seeds
OPERATOR_SHAPES = [(96, 64, 5, 3), (1, 64, 5, 3), (3, 64, 5, 3), (96, 32, 5, 3), (7, 8, 2, 2), (3, 64, 5, 1)]
OPERATOR_SEEDS = [11, 12]
TWIN_CASE = (70, 64, 5, 3, 29)
TAILS_CASE = (6, 64, 5, 3, 23)
DET_CASE = (96, 64, 5, 3, 41)
HALVES_CASE = (8, 64, 5, 3, 17)
OPS_CASE = (5, 64, 5, 3, 2)
MOMENTS_CASE = (9, 64, 5, 3, 5)
CASES = [s + (seed,) for s in OPERATOR_SHAPES for seed in OPERATOR_SEEDS] + [TWIN_CASE, TAILS_CASE, DET_CASE, HALVES_CASE, OPS_CASE, MOMENTS_CASE]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]  # (kl_backwards, log_sigma)


def inputs(B, seed, ldq=64, n_cat=5, n_act=3, scale=0.7):
    """-> [q_before, q_after_online, q_after_target (f32 [B, ldq]), act i64 [B], rew, term, valid (f32 [B, n_cat])]: the draws of
    tests/cql_oracle.py::td_inputs, then every maximum of Q_online(s')[b][M(c, .)] that leads the runner-up by less than
    4 * ARGMAX_GAP is raised to the runner-up + 8 * ARGMAX_GAP."""
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, ldq, generator=g) * scale for _ in range(3)]
    act = torch.randint(0, n_act, (B,), generator=g)
    rew = (torch.rand(B, n_cat, generator=g) < 0.3).float()
    term = (torch.rand(B, n_cat, generator=g) < 0.2).float()
    valid = (torch.rand(B, n_cat, generator=g) < 0.8).float()
    if n_act > 1:
        n = n_cat * n_act
        means = q[1][:, :n].reshape(B, n_cat, n_act).clone()
        top = means.topk(2, dim=2)
        near = (top.values[..., 0] - top.values[..., 1]) < 4 * ARGMAX_GAP
        raised = torch.where(near, top.values[..., 1] + 8 * ARGMAX_GAP, top.values[..., 0])
        means.scatter_(2, top.indices[..., :1], raised.unsqueeze(2))
        q[1][:, :n] = means.reshape(B, n)
    return q + [act, rew, term, valid]


def smin2_of(sigma_min):
    """sigma_min * sigma_min as the entry forms it: one float32 product."""
    return float(np.float32(sigma_min) * np.float32(sigma_min))


def _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma):
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in inp]
    B = qb.shape[0]
    vm = valid if use_valid else torch.ones_like(rew)
    w = torch.ones(B, dtype=torch.float64) if weight is None else weight.detach().cpu().double()
    g = torch.full((B, 1), float(np.float32(gamma)), dtype=torch.float64) if discount is None else discount.detach().cpu().double().view(B, 1)
    return qb, qo, qt, act, rew, term, vm, w, g


def var_of(rho, log_sigma, smin2):
    """var(rho) with torch ops (any dtype; autograd gives de/drho, exactly 0 outside the LOG_SIGMA clamp)."""
    if log_sigma:
        return torch.exp(2 * rho.clamp(CLAMP_LO, CLAMP_HI)) + smin2
    return torch.nn.functional.softplus(rho, beta=1.0, threshold=SOFTPLUS_LINEAR) ** 2 + smin2


def _choice(qo, n_cat, n_act):
    B = qo.shape[0]
    return qo[:, :n_cat * n_act].reshape(B, n_cat, n_act).argmax(dim=2)  # (first maximum; `inputs` leaves no tie)


def _parts(row, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect, log_sigma, smin2):
    """(mu, s2, m, v) [B, n_cat] from the Q(s) row `row` [B, >= 2 * n_cat * n_act]."""
    B, n = row.shape[0], n_cat * n_act
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    mu = row.gather(1, cols)
    s2 = var_of(row.gather(1, n + cols), log_sigma, smin2)
    tcols = torch.arange(n_cat).view(1, n_cat) * n_act + _choice(qo, n_cat, n_act)
    mt = qt.gather(1, tcols)
    vt = var_of(qt.gather(1, n + tcols), log_sigma, smin2)
    m = rew + g * ((1 - term) * mt)
    if clip_rect:
        m = m.clamp(0, 1)
    gg = g * (1 - term)
    v = torch.clamp(gg * gg * vt, min=smin2)
    return mu, s2, m.detach(), v.detach()


def argmax_gap(inp, n_cat=5, n_act=3):
    """The smallest lead of the maximum over the runner-up among the means of Q_online(s'), over every (sample, category); inf for one action."""
    if n_act < 2:
        return float("inf")
    qo = inp[1].detach().cpu().double()
    top = qo[:, :n_cat * n_act].reshape(qo.shape[0], n_cat, n_act).topk(2, dim=2).values
    return (top[..., 0] - top[..., 1]).min().item()


def clamp_margin(inp, n_cat=5, n_act=3):
    """The smallest distance of any spread entry of Q_online(s) and Q_target(s') from -8, 4 and 20."""
    n = n_cat * n_act
    rho = torch.cat([inp[0][:, n:2 * n], inp[2][:, n:2 * n]]).detach().cpu().double()
    return min((rho - k).abs().min().item() for k in (CLAMP_LO, CLAMP_HI, SOFTPLUS_LINEAR))


def objective(inp, *, kl_backwards=False, log_sigma=False, sigma_min=0.1, weight=None, use_valid=True, clip_rect=1, gamma=0.9, discount=None,
              n_cat=5, n_act=3, inv_count=None):
    """float64, torch.distributions and autograd.  -> dict(loss, sigma, z2, dq [B, 2 * n_cat * n_act], err [B], d, L, v, s2 [B, n_cat])."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    smin2 = smin2_of(sigma_min)
    row = qb[:, :2 * n].clone().requires_grad_(True)
    mu, s2, m, v = _parts(row, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect, log_sigma, smin2)
    backup = torch.distributions.Normal(m, v.sqrt())
    pred = torch.distributions.Normal(mu, s2.sqrt())
    L = torch.distributions.kl_divergence(pred, backup) if kl_backwards else torch.distributions.kl_divergence(backup, pred)
    s = w.view(B, 1) * vm
    loss = inv * (s * L).sum()
    dq, = torch.autograd.grad(loss, row)
    d = (mu - m).detach()
    s2 = s2.detach()
    return dict(loss=loss.detach(), sigma=inv * (vm * s2.sqrt()).sum(), z2=inv * (vm * d * d / s2).sum(), dq=dq,
                err=(d.abs() * vm).sum(1) / n_cat, d=d, L=L.detach(), v=v, s2=s2)


def closed_form(inp, *, kl_backwards=False, log_sigma=False, sigma_min=0.1, weight=None, use_valid=True, clip_rect=1, gamma=0.9, discount=None,
                n_cat=5, n_act=3, inv_count=None):
    """float64 by hand: dq[b][M(c, a*)] = dL/dmu s inv, dq[b][S(c, a*)] = dL/ds2 de/drho s inv, every other column 0.
    -> (dq [B, 2 n], L [B, n_cat])."""
    qb, qo, qt, act, rew, term, vm, w, g = _f64(inp, n_cat, n_act, weight, use_valid, discount, gamma)
    B, n = qb.shape[0], n_cat * n_act
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))
    smin2 = smin2_of(sigma_min)
    mu, s2, m, v = _parts(qb, qo, qt, act, rew, term, g, n_cat, n_act, clip_rect, log_sigma, smin2)
    cols = torch.arange(n_cat).view(1, n_cat) * n_act + act.view(B, 1)
    rho = qb.gather(1, n + cols)
    if log_sigma:
        e = torch.exp(2 * rho.clamp(CLAMP_LO, CLAMP_HI))
        de = torch.where((rho > CLAMP_LO) & (rho < CLAMP_HI), 2 * e, torch.zeros_like(e))
    else:
        sp = torch.where(rho > SOFTPLUS_LINEAR, rho, torch.log1p(torch.exp(rho)))
        de = 2 * sp * torch.sigmoid(rho)
    d = mu - m
    if kl_backwards:
        L = 0.5 * (torch.log(v / s2) + (s2 + d * d) / v - 1)
        dmu, ds2 = d / v, 0.5 * (1 / v - 1 / s2)
    else:
        L = 0.5 * (torch.log(s2 / v) + (v + d * d) / s2 - 1)
        dmu, ds2 = d / s2, 0.5 * (1 / s2 - (v + d * d) / s2 ** 2)
    s = w.view(B, 1) * vm
    dq = torch.zeros(B, 2 * n, dtype=torch.float64)
    dq.scatter_(1, cols, dmu * s * inv)
    dq.scatter_(1, n + cols, ds2 * de * s * inv)
    return dq, L


def _var_f32(rho, log_sigma, smin2):
    """(var, de/drho) in numpy float32, the order of dist_var in csrc/dist.hip."""
    f = np.float32
    with np.errstate(over="ignore"):
        if log_sigma:
            rc = np.minimum(np.maximum(rho, f(CLAMP_LO)), f(CLAMP_HI))
            e = np.exp(f(2) * rc)
            de = np.where((rho > f(CLAMP_LO)) & (rho < f(CLAMP_HI)), f(2) * e, f(0))
        else:
            sp = np.where(rho > f(SOFTPLUS_LINEAR), rho, np.log1p(np.exp(rho)))
            e = sp * sp
            de = (f(2) * sp) * (f(1) / (f(1) + np.exp(-rho)))
    return (e + smin2).astype(f), de.astype(f)


def restate_f32(inp, *, kl_backwards=False, log_sigma=False, sigma_min=0.1, weight=None, use_valid=True, clip_rect=1, gamma=0.9, discount=None,
                n_cat=5, n_act=3, inv_count=None):
    """The closed form in numpy float32, every product, quotient and sum in the kernel's order and rounded on its own.
    -> dict(loss, sigma, z2 (float64 sums of the float32 terms, times the float32 inv), dq f32 [B, 2 n], err f32 [B], d, L, v, s2)."""
    f = np.float32
    qb, qo, qt = [t.detach().cpu().numpy().astype(f) for t in inp[:3]]
    act = inp[3].detach().cpu().numpy()
    rew, term, valid = [t.detach().cpu().numpy().astype(f) for t in inp[4:7]]
    B, n = qb.shape[0], n_cat * n_act
    vm = valid if use_valid else np.ones_like(rew)
    inv = f(1.0 / (n_cat * B) if inv_count is None else inv_count)
    smin2 = f(sigma_min) * f(sigma_min)
    g = np.full((B, 1), f(gamma), dtype=f) if discount is None else discount.detach().cpu().numpy().astype(f).reshape(B, 1)
    rows = np.arange(B).reshape(B, 1)
    cols = np.arange(n_cat).reshape(1, n_cat) * n_act + act.reshape(B, 1)
    best = qo[:, :n].reshape(B, n_cat, n_act).argmax(axis=2)  # first maximum
    tcols = np.arange(n_cat).reshape(1, n_cat) * n_act + best
    one = f(1)
    qa = qt[rows, tcols] * (one - term)
    m = rew + g * qa
    if clip_rect:
        m = np.minimum(np.maximum(m, f(0)), one)
    vt, _ = _var_f32(qt[rows, n + tcols], log_sigma, smin2)
    gg = g * (one - term)
    v = np.maximum((gg * gg) * vt, smin2)
    mu = qb[rows, cols]
    s2, de = _var_f32(qb[rows, n + cols], log_sigma, smin2)
    d = mu - m
    half = f(0.5)
    if kl_backwards:
        L = half * (np.log(v / s2) + (s2 + d * d) / v - one)
        dmu = d / v
        ds2 = half * ((s2 - v) / (v * s2))
    else:
        L = half * (np.log(s2 / v) + (v + d * d) / s2 - one)
        dmu = d / s2
        ds2 = half * ((s2 - (v + d * d)) / (s2 * s2))
    L = np.maximum(L, f(0))
    drho = ds2 * de
    lw, dmu_w, drho_w = L, dmu, drho
    if weight is not None:
        w = weight.detach().cpu().numpy().astype(f).reshape(B, 1)
        lw, dmu_w, drho_w = L * w, dmu * w, drho * w
    dq = np.zeros((B, 2 * n), dtype=f)
    dq[rows, cols] = dmu_w * vm * inv
    dq[rows, n + cols] = drho_w * vm * inv
    err = np.zeros(B, dtype=f)
    for c in range(n_cat):
        err = err + np.abs(d[:, c]) * vm[:, c]
    err = err / f(n_cat)
    assert all(x.dtype == f for x in (m, v, s2, d, L, dq, err, drho))
    return dict(loss=float((lw * vm).astype(np.float64).sum() * inv), sigma=float((vm * np.sqrt(s2)).astype(np.float64).sum() * inv),
                z2=float((vm * ((d * d) / s2)).astype(np.float64).sum() * inv), dq=dq, err=err, d=d, L=L, v=v, s2=s2)


def deviation(inp, **kw):
    """(worst |restate_f32 dq - objective dq| in units of the largest objective dq element, relative loss deviation) of one case."""
    o, r = objective(inp, **kw), restate_f32(inp, **kw)
    scale = o["dq"].abs().max().item()
    dq_dev = (torch.from_numpy(r["dq"]).double() - o["dq"]).abs().max().item() / scale
    return dq_dev, abs(r["loss"] - o["loss"].item()) / abs(o["loss"].item())
