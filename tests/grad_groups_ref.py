"""The per-group clip rule of ``ssi/grad_groups.py`` restated in numpy float64, one group at a time, as plain control flow.

For optimizer step ``t`` = 1, 2, ... and a group with threshold ``m`` (``inf``: never), ``n`` the norm of the group's gradient as AdamW would see it:

* ``n`` not finite: coefficient NaN (the kernel leaves the group alone), ``gamma`` stays, ``skipped += 1``;
* ``gamma`` unset, or fixed mode, or ``t <= warmup_steps``: ``c = min(1, m / (n + 1e-6))``; in adaptive mode with ``n > 0``: ``gamma = min(gamma, c n)``,
  an unset ``gamma`` takes ``c n``;
* otherwise: ``c = min(1, min(m, rel gamma) / (n + 1e-6))``, ``gamma = beta gamma + (1 - beta) c n``.

``DEFECTS`` names planted deviations; ``run(..., defect=name)`` is the mirror with that one planted, for the tests that show each is caught."""
import math

import numpy as np

DEFECTS = ("rel_in_warmup", "gamma_from_unclipped_norm", "skip_resets_gamma", "zero_norm_sets_gamma", "max_norm_ignored_after_warmup",
           "warmup_off_by_one")


def step(state, n, t, *, max_norm=math.inf, adaptive=None, defect=None):
    """One group, one step.  ``state``: ``{"gamma": float | None, "skipped": int}``, updated in place.  Returns the coefficient."""
    n = float(n)
    if not math.isfinite(n):
        state["skipped"] += 1
        if defect == "skip_resets_gamma":
            state["gamma"] = None
        return math.nan
    gamma = state["gamma"]
    warm = adaptive is None or t <= adaptive["warmup_steps"] + (1 if defect == "warmup_off_by_one" else 0)
    if gamma is None or warm:
        limit = max_norm
        if defect == "rel_in_warmup" and adaptive is not None and gamma is not None:
            limit = min(max_norm, adaptive["rel"] * gamma)
        c = min(1.0, limit / (n + 1e-6))
        if adaptive is not None and (n > 0 or defect == "zero_norm_sets_gamma"):
            seen = n if defect == "gamma_from_unclipped_norm" else c * n
            state["gamma"] = seen if gamma is None else min(gamma, seen)
        return c
    limit = adaptive["rel"] * gamma if defect == "max_norm_ignored_after_warmup" else min(max_norm, adaptive["rel"] * gamma)
    c = min(1.0, limit / (n + 1e-6))
    seen = n if defect == "gamma_from_unclipped_norm" else c * n
    state["gamma"] = adaptive["beta"] * gamma + (1.0 - adaptive["beta"]) * seen
    return c


def run(norms, *, max_norm=math.inf, adaptive=None, defect=None):
    """A sequence of norms of ONE group -> per step ``(c, gamma or nan, skipped)`` as a float64 array ``[steps, 3]``."""
    state = {"gamma": None, "skipped": 0}
    out = []
    for t, n in enumerate(norms, start=1):
        c = step(state, n, t, max_norm=max_norm, adaptive=adaptive, defect=defect)
        out.append((c, math.nan if state["gamma"] is None else state["gamma"], state["skipped"]))
    return np.asarray(out, dtype=np.float64)
