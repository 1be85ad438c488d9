"""Oracle of the TD loss with the conservative Q-learning penalty (vdqn_td_loss_cql, csrc/pointwise.hip):

    loss    = inv_count * sum_bc s_bc * ( l(d_bc) + alpha * (logsumexp_a q_bc. - q_bc,a*) )        s_bc = w_b * valid_bc
    penalty = inv_count * sum_bc s_bc *                  (logsumexp_a q_bc. - q_bc,a*)

`objective` writes that in float64 with torch.logsumexp and lets autograd differentiate it: it shares no closed form with the
kernel.  `closed_form` is the gradient by hand in float64 (softmax minus one-hot), and `restate_f32` repeats the kernel's own
float32 arithmetic, operation for operation, in numpy: what a float32 implementation can be expected to reach against float64.
Inputs are those of tests/test_gpu_replay.py::_td_inputs: q_before, q_after_online, q_after_target f32 [B, ldq], act i64 [B],
rew / term / valid f32 [B, n_cat]."""
import numpy as np
import torch


def td_inputs(B, seed, ldq=64, n_cat=5, n_act=3, scale=0.7):
    """tests/test_gpu_replay.py::_td_inputs on the CPU (the same generator and order of draws), with a Q scale."""
    g = torch.Generator().manual_seed(seed)
    q = [torch.randn(B, ldq, generator=g) * scale for _ in range(3)]
    act = torch.randint(0, n_act, (B,), generator=g)
    rew = (torch.rand(B, n_cat, generator=g) < 0.3).float()
    term = (torch.rand(B, n_cat, generator=g) < 0.2).float()
    valid = (torch.rand(B, n_cat, generator=g) < 0.8).float()
    return q + [act, rew, term, valid]


def _f64(inputs, n_cat, n_act, weight, use_valid):
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu() for t in inputs]
    B, n = qb.shape[0], n_cat * n_act
    q, qo3, qt3 = (t[:, :n].reshape(B, n_cat, n_act) for t in (qb, qo, qt))
    vm = valid if use_valid else torch.ones_like(rew)
    w = torch.ones(B, dtype=torch.float64) if weight is None else weight.detach().cpu().double()
    return q, qo3, qt3, act, rew, term, vm, w


def _target(qo3, qt3, rew, term, linear, clip_rect, gamma):
    best = qo3.argmax(2, keepdim=True)  # (float32 values held in float64: the same order, the first maximum)
    qa = qt3.gather(2, best).squeeze(2) * (1 - term)
    y = rew + (qa - 0.1) if linear else rew + gamma * qa
    return y.clamp(0, 1) if clip_rect else y


def objective(inputs, alpha, *, weight=None, use_valid=True, loss_kind=0, linear=0, clip_rect=1, gamma=0.9, n_cat=5, n_act=3,
              inv_count=None):
    """float64, autograd.  -> dict(loss, penalty, dq [B, n_cat * n_act], err [B], d [B, n_cat], s [B, n_cat])."""
    q, qo3, qt3, act, rew, term, vm, w = _f64(inputs, n_cat, n_act, weight, use_valid)
    B = q.shape[0]
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    q = q.clone().requires_grad_(True)
    q_s = q.gather(2, act.view(B, 1, 1).expand(B, n_cat, 1)).squeeze(2)
    y = _target(qo3, qt3, rew, term, linear, clip_rect, gamma)
    if loss_kind == 1:
        l = torch.nn.functional.smooth_l1_loss(q_s, y, reduction="none", beta=1.0)
    else:
        l = 0.5 * (q_s - y) ** 2
    pen = torch.logsumexp(q, 2) - q_s
    s = w.view(B, 1) * vm
    loss = inv * (s * (l + alpha * pen)).sum()
    penalty = inv * (s * pen).sum()
    dq, = torch.autograd.grad(loss, q)
    d = (q_s - y).detach()
    return dict(loss=loss.detach(), penalty=penalty.detach(), dq=dq.reshape(B, n_cat * n_act), err=(d.abs() * vm).sum(1) / n_cat,
                d=d, s=s)


def closed_form(inputs, alpha, *, weight=None, use_valid=True, loss_kind=0, linear=0, clip_rect=1, gamma=0.9, n_cat=5, n_act=3,
                inv_count=None):
    """float64 by hand: dq = inv * s * ([a == a*] * dl(d) + alpha * (softmax(q) - [a == a*])).  -> dict(dq, pen_grad) where
    pen_grad = inv * s * alpha * (softmax - onehot) alone (what the penalty adds to the TD loss's dq)."""
    q, qo3, qt3, act, rew, term, vm, w = _f64(inputs, n_cat, n_act, weight, use_valid)
    B = q.shape[0]
    inv = float(np.float32(1.0 / (n_cat * B) if inv_count is None else inv_count))  # the float32 the kernel is handed
    onehot = torch.zeros_like(q).scatter_(2, act.view(B, 1, 1).expand(B, n_cat, 1), 1.0)
    d = (q * onehot).sum(2) - _target(qo3, qt3, rew, term, linear, clip_rect, gamma)
    dl = d.clamp(-1, 1) if loss_kind == 1 else d
    m = q.max(2, keepdim=True).values
    e = torch.exp(q - m)
    p = e / e.sum(2, keepdim=True)
    s = (w.view(B, 1) * vm).unsqueeze(2)
    pen_grad = inv * s * alpha * (p - onehot)
    return dict(dq=(inv * s * onehot * dl.unsqueeze(2) + pen_grad).reshape(B, -1), pen_grad=pen_grad.reshape(B, -1))


def restate_f32(inputs, alpha, *, weight=None, use_valid=True, loss_kind=0, linear=0, clip_rect=1, gamma=0.9, n_cat=5, n_act=3,
                inv_count=None):
    """The kernel's float32 arithmetic in numpy, in its order of operations (sums over the actions from a = 0 up; the loss and the
    penalty are summed in float64 here: their float32 summation order is the block reduction's, which this does not restate).
    -> dict(loss, penalty, dq [B, n_cat * n_act] float32, err [B] float32)."""
    f = np.float32
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().numpy() for t in inputs]
    B, n = qb.shape[0], n_cat * n_act
    q, qo3, qt3 = (np.ascontiguousarray(t[:, :n], dtype=f).reshape(B, n_cat, n_act) for t in (qb, qo, qt))
    rew, term = rew.astype(f), term.astype(f)
    vm = valid.astype(f) if use_valid else np.ones((B, n_cat), f)
    w = np.ones(B, f) if weight is None else weight.detach().cpu().numpy().astype(f)
    inv = f(1.0 / (n_cat * B)) if inv_count is None else f(inv_count)
    alpha, gamma = f(alpha), f(gamma)
    rows = np.arange(B)
    best = qo3.argmax(2)
    qa = np.take_along_axis(qt3, best[..., None], 2)[..., 0] * (f(1) - term)
    y = rew + (qa - f(0.1)) if linear else rew + gamma * qa
    if clip_rect:
        y = np.minimum(np.maximum(y, f(0)), f(1))
    q_s = q[rows, :, act]
    d = q_s - y
    if loss_kind == 1:
        ad = np.abs(d)
        l, dl = np.where(ad < 1, f(0.5) * d * d, ad - f(0.5)).astype(f), np.minimum(np.maximum(d, f(-1)), f(1))
    else:
        l, dl = f(0.5) * d * d, d
    m = q.max(2)
    total = np.zeros((B, n_cat), f)
    for a in range(n_act):
        total = total + np.exp(q[:, :, a] - m)
    p = np.exp(q - m[..., None]) / total[..., None]
    pen = np.log(total) + (m - q_s)
    s = w[:, None] * vm
    onehot = np.zeros((B, n_cat, n_act), bool)
    onehot[rows, :, act] = True
    g = np.where(onehot, dl[..., None] + alpha * (p - f(1)), alpha * p).astype(f)
    dq = (g * s[..., None] * inv).astype(f)
    loss_terms, pen_terms = s * (l + alpha * pen), s * pen
    assert p.dtype == f and pen.dtype == f and loss_terms.dtype == f and dq.dtype == f
    return dict(loss=float(loss_terms.astype(np.float64).sum() * np.float64(inv)), penalty=float(pen_terms.astype(np.float64).sum() * np.float64(inv)),
                dq=dq.reshape(B, n), err=((np.abs(d) * vm).sum(1) / f(n_cat)).astype(f))
