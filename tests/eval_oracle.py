"""Oracle of the validation metrics launch (vdqn_td_eval, csrc/eval.hip): per category c, eight sums over the samples b of

    0: vm   1: vm l(d)   2: vm |d|   3: vm Q(s,c,a_data)   4: vm max_a Q(s,c,a)   5: vm y   6: vm pen   7: vm [argmax_a Q(s,c,.) == a_data]

with y the Double-DQN target, d = Q(s,c,a_data) - y, l the half squared error or Huber, pen = logsumexp_a Q(s,c,.) - Q(s,c,a_data)
(identically 0 with one action) and vm = valid or 1.  `sums_f64` writes them in float64 with torch.logsumexp / argmax on the float32
inputs; `restate_f32` repeats the kernel's float32 term arithmetic in numpy and sums the terms in float64.  Both return
(table [n_cat, 8] float64, abs_table [n_cat, 8] float64 = the sums of the terms' absolute values: what a relative gate is taken
against, because the signed sums of slots 3-5 cancel).  Inputs are those of cql_oracle.td_inputs."""
import numpy as np
import torch

import cql_oracle


def sums_f64(inputs, *, use_valid=True, loss_kind=0, linear=0, clip_rect=1, gamma=0.9, n_cat=5, n_act=3):
    q, qo3, qt3, act, rew, term, vm, _ = cql_oracle._f64(inputs, n_cat, n_act, None, use_valid)
    B = q.shape[0]
    q_s = q.gather(2, act.view(B, 1, 1).expand(B, n_cat, 1)).squeeze(2)
    y = cql_oracle._target(qo3, qt3, rew, term, linear, clip_rect, gamma)
    d = q_s - y
    if loss_kind == 1:
        l = torch.nn.functional.smooth_l1_loss(q_s, y, reduction="none", beta=1.0)
    else:
        l = 0.5 * d ** 2
    pen = torch.logsumexp(q, 2) - q_s if n_act > 1 else torch.zeros_like(q_s)
    agree = (q.argmax(2) == act.view(B, 1)).double()  # (float32 values held in float64: the first maximum)
    terms = torch.stack([torch.ones_like(vm), l, d.abs(), q_s, q.max(2).values, y, pen, agree], 2) * vm.unsqueeze(2)  # [B, n_cat, 8]
    return terms.sum(0).numpy(), terms.abs().sum(0).numpy()


def restate_f32(inputs, *, use_valid=True, loss_kind=0, linear=0, clip_rect=1, gamma=0.9, n_cat=5, n_act=3):
    f = np.float32
    qb, qo, qt, act, rew, term, valid = [t.detach().cpu().numpy() for t in inputs]
    B, n = qb.shape[0], n_cat * n_act
    q, qo3, qt3 = (np.ascontiguousarray(t[:, :n], dtype=f).reshape(B, n_cat, n_act) for t in (qb, qo, qt))
    rew, term = rew.astype(f), term.astype(f)
    vm = valid.astype(f) if use_valid else np.ones((B, n_cat), f)
    gamma = f(gamma)
    rows = np.arange(B)
    best = qo3.argmax(2)
    qa = np.take_along_axis(qt3, best[..., None], 2)[..., 0] * (f(1) - term)
    y = rew + (qa - f(0.1)) if linear else rew + gamma * qa
    if clip_rect:
        y = np.minimum(np.maximum(y, f(0)), f(1))
    q_s = q[rows, :, act]
    d = q_s - y
    ad = np.abs(d)
    l = np.where(ad < 1, f(0.5) * d * d, ad - f(0.5)).astype(f) if loss_kind == 1 else f(0.5) * d * d
    m = q.max(2)
    if n_act > 1:
        total = np.zeros((B, n_cat), f)
        for a in range(n_act):
            total = total + np.exp(q[:, :, a] - m)
        pen = np.log(total) + (m - q_s)
    else:
        pen = np.zeros((B, n_cat), f)
    agree = (q.argmax(2) == act[:, None]).astype(f)
    terms = np.stack([np.ones((B, n_cat), f) * vm, l * vm, ad * vm, q_s * vm, m * vm, y * vm, pen * vm, agree * vm], 2)
    assert terms.dtype == f
    t64 = terms.astype(np.float64)
    return t64.sum(0), np.abs(t64).sum(0)


def worst_per_slot(got, want, abs_table):
    """max over the categories of |got - want| / sum |terms| per slot (0 where a slot has no terms)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (np.abs(got - want) / np.maximum(abs_table, 1e-300)).max(0)
