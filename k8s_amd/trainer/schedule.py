"""The trainer's learning-rate schedule: one pure function of the step."""
from __future__ import annotations

import math

SCHEDULES = ("constant", "poly", "cosine")


def lr_at(step: int, lr: float, warmup_steps: int = 0, steps: int = 0, schedule: str = "constant",
          lr_end: float = 0.0, power: float = 2.0) -> float:
    """Learning rate of 0-based ``step`` of a ``steps``-step run.

    Linear warmup over the first ``warmup_steps`` steps (step ``warmup_steps - 1`` runs at ``lr``), then

    * ``constant``: ``lr``;
    * ``poly``:     ``lr_end + (lr - lr_end) (1 - t)^power``;
    * ``cosine``:   ``lr_end + (lr - lr_end) (1 + cos(pi t)) / 2``,

    with ``t = (step + 1 - warmup_steps) / (steps - warmup_steps)`` clamped to [0, 1]: the decay runs over the
    steps after the warmup and the last step runs at ``lr_end``."""
    if schedule not in SCHEDULES:
        raise ValueError("unknown lr schedule %r" % (schedule,))
    warm = lr * min(1.0, (step + 1) / warmup_steps) if warmup_steps else lr
    if schedule == "constant" or step < warmup_steps:
        return warm
    span = steps - warmup_steps
    t = min(1.0, max(0.0, (step + 1 - warmup_steps) / span)) if span > 0 else 1.0
    if schedule == "poly":
        f = (1.0 - t) ** power
    else:
        f = 0.5 * (1.0 + math.cos(math.pi * t))
    return lr_end + (lr - lr_end) * f
