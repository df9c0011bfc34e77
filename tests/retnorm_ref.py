"""TEST INFRASTRUCTURE: numpy / float64 restatement of the percentile return normalisation's running range
(``ActorCritic.return_normalization = percentile``; DESIGN.md, "Return normalisation").

State: ``lo``, ``hi``, ``count`` (updates made), ``skipped`` (updates refused), all float64, all zero when empty.
A step divides the returns of the actor objective by ``scale(state, floor)`` of the state as it stands BEFORE the step,
then ``update`` folds the step's own lambda-returns in.
"""
from __future__ import annotations

import math

import numpy as np


def empty_state() -> dict:
    return dict(lo=0.0, hi=0.0, count=0.0, skipped=0.0)


def ranks(M: int, q_lo: float = 0.05, q_hi: float = 0.95):
    """k_q = floor(q (M - 1)) in Python floats."""
    return int(math.floor(q_lo * (M - 1))), int(math.floor(q_hi * (M - 1)))


def scale(state: dict, floor: float = 1.0) -> np.float32:
    """S = max(floor, hi - lo), rounded to fp32; `floor` while the state is empty."""
    return np.float32(max(float(floor), float(state["hi"]) - float(state["lo"])))


def update(state: dict, returns, k_lo: int, k_hi: int, decay: float) -> dict:
    """The state after one step whose M fp32 lambda-returns are `returns` (any shape).  p_lo, p_hi = elements k_lo, k_hi of
    their ascending sort; the first update takes them as they are, later ones mix in float64, each product and the sum
    rounded once.  Any NaN or infinity: nothing changes but `skipped`."""
    x = np.asarray(returns, dtype=np.float32).reshape(-1)
    assert 0 <= k_lo <= k_hi < x.size
    out = {k: float(v) for k, v in state.items()}
    if not np.isfinite(x).all():
        out["skipped"] += 1.0
        return out
    srt = np.sort(x)
    p_lo, p_hi = np.float64(srt[k_lo]), np.float64(srt[k_hi])
    if out["count"] == 0.0:
        out["lo"], out["hi"] = float(p_lo), float(p_hi)
    else:
        d = np.float64(decay)
        out["lo"] = float(d * np.float64(out["lo"]) + (np.float64(1.0) - d) * p_lo)
        out["hi"] = float(d * np.float64(out["hi"]) + (np.float64(1.0) - d) * p_hi)
    out["count"] += 1.0
    return out
