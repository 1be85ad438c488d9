"""float64 numpy restatement of the optimiser controls (video_dqn_amd/csrc/optim.hip, video_dqn_amd/optim.py): the clip coefficient
of torch.nn.utils.clip_grad_norm_, one torch.optim.AdamW step on the scaled gradient, the learning-rate schedule, and the fixed
summation order of the device norm (so a test can reproduce the kernels' f64 sum bit for bit from their workspace)."""
import math

import numpy as np

CLIP_MAX_PARTS = 512      # csrc/optim.hip: kClipMaxParts
CLIP_SLOT_DOUBLES = 513   # int64 count + the partials


def clip_coef(grad, max_norm):
    """-> (norm, coef) in float64: coef = min(1, max_norm / (norm + 1e-6))."""
    g = np.asarray(grad, np.float64).reshape(-1)
    norm = math.sqrt(math.fsum(g * g))
    return norm, min(1.0, max_norm / (norm + 1e-6))


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, coef=1.0):
    """One AdamW step in float64 on gs = g * coef; returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    gs = g * coef
    p = p * (1.0 - lr * wd)
    m = b1 * m + (1.0 - b1) * gs
    v = b2 * v + (1.0 - b2) * gs * gs
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v


def lr_at(t, base, warmup=0, schedule="constant", final_fraction=0.0, num_steps=0):
    mult = min(1.0, t / warmup) if warmup > 0 else 1.0
    if schedule != "constant":
        progress = min(1.0, max(0.0, (t - warmup) / (num_steps - warmup)))
        if schedule == "linear":
            mult *= 1.0 + (final_fraction - 1.0) * progress
        elif schedule == "cosine":
            mult *= final_fraction + (1.0 - final_fraction) * 0.5 * (1.0 + math.cos(math.pi * progress))
        else:
            raise ValueError(schedule)
    return base * mult


def workspace_sum(ws, n_slots):
    """The finalise kernel's sum from a read-back workspace (float64 [slots * 513]): the partials of slot 0, then slot 1, ..., added
    left to right."""
    ws = np.asarray(ws, np.float64)
    total = np.float64(0.0)
    for s in range(n_slots):
        slot = ws[s * CLIP_SLOT_DOUBLES:(s + 1) * CLIP_SLOT_DOUBLES]
        count = int(slot[:1].view(np.int64)[0])
        assert 1 <= count <= CLIP_MAX_PARTS, count
        for x in slot[1:1 + count]:
            total = total + x
    return float(total)
