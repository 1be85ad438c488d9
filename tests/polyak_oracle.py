"""Oracle of the soft (Polyak) target update theta- <- theta- + tau (theta - theta-): the float64 statement, and the numpy float32
restatement of the kernel's arithmetic (include/vdqn.h, vdqn_polyak) — torch.lerp's two-branch rule with every product rounded
on its own, which the kernels must reproduce bit for bit."""
import numpy as np


def lerp(t, p, tau):
    """float64: t + tau * (p - t)."""
    t, p = np.asarray(t, np.float64), np.asarray(p, np.float64)
    return t + float(tau) * (p - t)


def lerp_f32(t, p, tau):
    """The kernel's three roundings: d = p - t; tau < 0.5: t + tau_f * d; otherwise p - d * omt_f, omt_f = (float)(1.0 - tau)."""
    t, p = np.asarray(t, np.float32), np.asarray(p, np.float32)
    d = p - t
    if tau < 0.5:
        return t + np.float32(tau) * d
    return p - d * np.float32(1.0 - float(tau))

