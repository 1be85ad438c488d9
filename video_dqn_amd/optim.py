"""Optimiser controls of the Q trainer: the learning-rate schedule (pure host arithmetic, evaluated once per update from the
trainer's 1-based ``sample_number``, so a resumed run uses the uninterrupted run's rates) and the validation of the config keys
GRAD_CLIP_NORM / WEIGHT_DECAY / LR_WARMUP_STEPS / LR_SCHEDULE / LR_FINAL_FRACTION.  The device side — the gradient norm, the clip
coefficient and the AdamW update — is csrc/optim.hip, driven by ``TDStepper``."""
from __future__ import annotations

import math

SCHEDULES = ("constant", "linear", "cosine")


def lr_at(t, base, warmup=0, schedule="constant", final_fraction=0.0, num_steps=0) -> float:
    """Learning rate of update ``t`` (1-based): ``base * min(1, t / warmup) * s(progress)`` with
    ``progress = clamp((t - warmup) / (num_steps - warmup), 0, 1)`` and ``s`` going from 1 to ``final_fraction``:
    'constant' 1, 'linear' ``1 - (1 - f) * progress``, 'cosine' ``f + (1 - f) * (1 + cos(pi * progress)) / 2``."""
    if schedule not in SCHEDULES:
        raise ValueError(f"LR_SCHEDULE must be one of {list(SCHEDULES)}")
    t, w, f = float(t), float(warmup), float(final_fraction)
    mult = min(1.0, t / w) if w > 0 else 1.0
    if schedule != "constant":
        span = float(num_steps) - w
        progress = min(1.0, max(0.0, (t - w) / span)) if span > 0 else (1.0 if t > w else 0.0)
        if schedule == "linear":
            mult *= 1.0 - (1.0 - f) * progress
        else:
            mult *= f + (1.0 - f) * 0.5 * (1.0 + math.cos(math.pi * progress))
    return float(base) * mult


def schedule_active(warmup, schedule) -> bool:
    return int(warmup) > 0 or schedule != "constant"


def check_config(grad_clip_norm, weight_decay, warmup, schedule, final_fraction, num_steps) -> None:
    """Raise ValueError naming the config key (before any device work)."""
    for key, v in (("GRAD_CLIP_NORM", grad_clip_norm), ("WEIGHT_DECAY", weight_decay), ("LR_FINAL_FRACTION", final_fraction)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{key} must be a finite number >= 0, not {v!r}")
    if isinstance(warmup, bool) or not isinstance(warmup, int) or warmup < 0:
        raise ValueError(f"LR_WARMUP_STEPS must be an integer >= 0, not {warmup!r}")
    if schedule not in SCHEDULES:
        raise ValueError(f"LR_SCHEDULE must be one of {list(SCHEDULES)}, not {schedule!r}")
    if final_fraction > 1:
        raise ValueError(f"LR_FINAL_FRACTION must be <= 1 (the schedule decays from LEARNING_RATE), not {final_fraction!r}")
    if schedule != "constant" and warmup >= num_steps:
        raise ValueError(f"LR_WARMUP_STEPS ({warmup}) must be < NUM_STEPS ({num_steps}) with LR_SCHEDULE '{schedule}': "
                         "the decay runs from the end of the warm-up to NUM_STEPS")
