"""TEST INFRASTRUCTURE, and the specification of the two-hot critic head (``ActorCritic.critic_head = twohot``; DESIGN.md,
"Two-hot critic"; include/bigdreamer_hip.h, bd_twohot_*): numpy restatement in float64 and, with ``dtype=np.float32``,
the same formulas evaluated in float32.

Bins, uniform in symlog space:   z_i = -Z + i delta,  delta = 2 Z / (K - 1),  i = 0 .. K - 1   -- formed as
(2 i - (K - 1)) Z / (K - 1), the same numbers with z_i = -z_{K-1-i} exactly.
symlog(y) = sign(y) log1p(|y|),   symexp(z) = sign(z) expm1(|z|).

decode:           p = softmax(l) (maximum subtracted),  m = sum_i p_i z_i,  v = symexp(m).  The sum is taken over the
                  mirrored pairs p_i z_i + p_{K-1-i} z_{K-1-i}, so uniform logits decode to exactly 0.
decode_backward:  dl_i = dv exp(|m|) p_i (z_i - m).
encode:           t = clamp(symlog(y), -Z, Z),  u = (t + Z) / delta,  k = min(floor(u), K - 2),  w = u - k,
                  q_k = 1 - w,  q_{k+1} = w.  (k, w) is continuous across a bin edge (w -> 1 at k is w = 0 at k + 1), so
                  float32 and float64 may take different k next to an edge and still agree in q: compare q, never k.
nll:              loss_r = w_r (logsumexp(l) - (1 - w) l_k - w l_{k+1}),  dl_i = grad_scale w_r (p_i - q_i).
                  A NaN target gives a NaN loss.

Error budgets (the constants at the end): the float32 restatement against the float64 one over the fillings and targets
below (every K of KS, every row count of ROWS and one row per target; ld does not enter), the largest error found on the CPU, times 4 because a kernel's
reduction order differs from numpy's.  Value and loss errors are relative to max(1, |v|), gradient errors to the row's
largest |dl| (the nll gradient: on well-conditioned rows, and a second measure on all, see the constants).
``python -m tests.twohot_ref`` prints the measured values.
"""
from __future__ import annotations

import numpy as np

KS = (2, 3, 63, 64, 65, 255, 256, 257, 1024)
ROWS = (1, 3, 63, 64, 65, 257)
Z_DEFAULT = 20.0
FLT_MAX = float(np.finfo(np.float32).max)
DENORMAL = float(np.float32(1e-42))
FILLINGS = ("normal", "equal", "spike", "low", "ramp_hi", "ramp_lo")


def bins(K: int, Z: float, dtype=np.float64) -> np.ndarray:
    h = dtype(Z) / dtype(K - 1)
    return (2 * np.arange(K) - (K - 1)).astype(dtype) * h


def symlog(y):
    return np.sign(y) * np.log1p(np.abs(y))


def symexp(z):
    return np.sign(z) * np.expm1(np.abs(z))


def softmax(l):
    e = np.exp(l - l.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def decode(logits, Z: float, dtype=np.float64):
    """(v, m) of rows of K logits."""
    l = np.asarray(logits).astype(dtype)
    t = softmax(l) * bins(l.shape[-1], Z, dtype)
    m = dtype(0.5) * (t + t[..., ::-1]).sum(-1)
    return symexp(m), m


def decode_backward(logits, dv, Z: float, dtype=np.float64):
    l = np.asarray(logits).astype(dtype)
    p, z = softmax(l), bins(l.shape[-1], Z, dtype)
    m = decode(l, Z, dtype)[1][..., None]
    return np.asarray(dv).astype(dtype)[..., None] * np.exp(np.abs(m)) * p * (z - m)


def encode(y, K: int, Z: float, dtype=np.float64):
    """q [rows x K], the two-hot encoding of symlog(y)."""
    y = np.asarray(y).astype(dtype).reshape(-1)
    Zd = dtype(Z)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.clip(symlog(y), -Zd, Zd)
        u = (t + Zd) / (dtype(2) * (Zd / dtype(K - 1)))
        k = np.where(np.isnan(u), 0, np.minimum(np.floor(u), K - 2)).astype(np.int64)
        w = u - k.astype(dtype)
    q = np.zeros((y.size, K), dtype)
    r = np.arange(y.size)
    q[r, k] = dtype(1) - w
    q[r, k + 1] = w
    return q


def nll(logits, y, Z: float, weight=None, grad_scale: float = 1.0, dtype=np.float64):
    """(loss [rows], dlogits [rows x K])."""
    l = np.asarray(logits).astype(dtype)
    K = l.shape[-1]
    q = encode(y, K, Z, dtype)
    wr = np.ones(l.shape[0], dtype) if weight is None else np.asarray(weight).astype(dtype)
    mx = l.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        # logsumexp(l) - q . l with the row maximum taken out of both terms (sum q = 1): no cancellation at large |l|
        dot = np.where(q != 0, q * (l - mx), dtype(0)).sum(-1)          # (a NaN w stays NaN)
        loss = wr * (np.log(np.exp(l - mx).sum(-1)) - dot)
        dl = dtype(grad_scale) * wr[:, None] * (softmax(l) - q)
    return loss, dl


# ------------------------------------------------------------------------------------------ fillings and targets
def filling(name: str, rows: int, K: int, Z: float = Z_DEFAULT, seed: int = 0) -> np.ndarray:
    """Logits [rows x K] fp32: unit normal | all equal | one logit at +80, the rest 0 | all at -1e4 | ramps that put the
    softmax mean within delta of +Z / -Z."""
    rng = np.random.Generator(np.random.PCG64(seed + 31 * K + rows))
    if name == "normal":
        return rng.standard_normal((rows, K), dtype=np.float32)
    if name == "equal":
        return np.full((rows, K), 0.37, np.float32)
    if name == "spike":
        l = np.zeros((rows, K), np.float32)
        l[np.arange(rows), rng.integers(0, K, rows)] = 80.0
        return l
    if name == "low":
        return np.full((rows, K), -1e4, np.float32)
    if name in ("ramp_hi", "ramp_lo"):
        # l_i = 3 (i - (K - 1)): p_{K-1} > 0.95, so the mean lies within 0.06 delta of +Z (mirrored: of -Z)
        ramp = (3.0 * (np.arange(K) - (K - 1))).astype(np.float32)
        l = np.tile(ramp if name == "ramp_hi" else ramp[::-1], (rows, 1))
        return l + 0.01 * rng.standard_normal((rows, 1), dtype=np.float32)
    raise KeyError(name)


def targets(K: int, Z: float = Z_DEFAULT) -> np.ndarray:
    """fp32 targets: 0 and +-denormal, every bin centre symexp(z_i) and every midpoint, nextafter on both sides of the
    edges, +-1e9 (clamped) and +-FLT_MAX."""
    z = bins(K, Z)
    with np.errstate(over="ignore"):
        centres = symexp(z).astype(np.float32)
        mids = symexp(0.5 * (z[1:] + z[:-1])).astype(np.float32)
    edges = np.concatenate([np.nextafter(centres, np.float32(-np.inf)), np.nextafter(centres, np.float32(np.inf))])
    special = np.array([0.0, -0.0, DENORMAL, -DENORMAL, 1e9, -1e9, FLT_MAX, -FLT_MAX], np.float32)
    out = np.concatenate([special, centres, mids, edges]).astype(np.float32)
    return out[np.isfinite(out)]


def value_err(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if want.size else 0.0


def grad_err(got, want, floor=None) -> float:
    """Largest error of a gradient relative to its row's largest |dl| (rows whose gradient is all zero: absolute).
    floor [rows]: only rows whose largest |dl| reaches it are measured (NLL_GRAD_COND below)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max(-1, keepdims=True)
    err = np.abs(got - want) / np.where(scale > 0, scale, 1.0)
    if floor is not None:
        err = err[scale[:, 0] >= np.asarray(floor, np.float64)]
    return float(err.max()) if err.size else 0.0


def grad_err_to(got, want, scale) -> float:
    """Largest error of a gradient relative to a given per-row scale (rows whose scale is 0: absolute)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.asarray(scale, np.float64).reshape(-1, 1)
    return float(np.max(np.abs(got - want) / np.where(scale > 0, scale, 1.0)))


NLL_GRAD_COND = 1e-3


def measure(Z: float = Z_DEFAULT) -> dict:
    """The float32 restatement against float64 over every filling, every K of KS, every row count of ROWS (targets
    cycling) and one row per target."""
    worst = dict(value=0.0, mean=0.0, decode_grad=0.0, loss=0.0, nll_grad=0.0, nll_grad_to_weight=0.0)
    f32, gs = np.float32, 0.25
    for K in KS:
        tg = targets(K, Z)
        for name in FILLINGS:
            for rows, y in [(r, np.resize(tg, r)) for r in ROWS] + [(tg.size, tg)]:
                l = filling(name, rows, K, Z)
                rng = np.random.Generator(np.random.PCG64(K))
                dv = rng.standard_normal(rows, dtype=f32)
                wr = rng.uniform(0.0, 1.0, rows).astype(f32)
                v64, m64 = decode(l, Z)
                v32, m32 = decode(l, Z, f32)
                worst["value"] = max(worst["value"], value_err(v32, v64))
                worst["mean"] = max(worst["mean"], value_err(m32, m64))
                worst["decode_grad"] = max(worst["decode_grad"], grad_err(decode_backward(l, dv, Z, f32), decode_backward(l, dv, Z)))
                lo64, g64 = nll(l, y, Z, wr, gs)
                lo32, g32 = nll(l, y, Z, wr, gs, f32)
                worst["loss"] = max(worst["loss"], value_err(lo32, lo64))
                worst["nll_grad"] = max(worst["nll_grad"], grad_err(g32, g64, NLL_GRAD_COND * gs * wr))
                worst["nll_grad_to_weight"] = max(worst["nll_grad_to_weight"], grad_err_to(g32, g64, gs * wr))
    return worst


# measured on the CPU (python -m tests.twohot_ref), times 4
VALUE_BUDGET = 4 * 2.841e-06            # measured 2.841e-06: |m| <= 20 carries ~2^-24 * 20 into exp
MEAN_BUDGET = 4 * 1.783e-06             # measured 1.783e-06
DECODE_GRAD_BUDGET = 4 * 1.050e-04      # measured 1.050e-04: z_i - m cancels on the ramps (m within 0.06 delta of +-Z)
LOSS_BUDGET = 4 * 1.038e-03             # measured 1.038e-03: fp32 resolves w to ulp(2 Z) / delta (1e-4 at K = 1024), times the ramps' slope 3
# The nll gradient relative to the row's largest |dl| is measured on the rows where that is at least NLL_GRAD_COND (1e-3)
# times grad_scale * w_r, i.e. where p and q differ by 1e-3 somewhere.  Where they nearly coincide -- the spike on the
# target's own bin -- the row's largest |dl| is itself the rounding error of w (1e-8 in float64, 1e-6 in float32; with the
# target 0 on the centre bin it is (K - 1) e^-80), and an error relative to it measures nothing: the float32 restatement
# reads 224 on one pairing of rows and targets and 4978 on another.  Every row is held by the second measure, relative to
# grad_scale * w_r, the scale of a row's gradient (its L1 norm is at most twice that).
NLL_GRAD_BUDGET = 4 * 3.070e-04         # measured 3.070e-04
NLL_GRAD_TO_WEIGHT_BUDGET = 4 * 6.239e-05     # measured 6.239e-05: the resolution of w, as above


if __name__ == "__main__":
    for key, val in measure().items():
        print(f"{key:12s} {val:.3e}")
