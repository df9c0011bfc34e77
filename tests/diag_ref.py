"""Float64 numpy restatements of the training-diagnostics kernels (csrc/diag.hip), written from the text of
include/bigdreamer_hip.h, and the error magnitudes their fp32-evaluated terms are held to.  Plain helpers, not a conftest:
test_diag_ref_cpu.py checks them against torch.distributions, test_diag_kernels_gpu.py checks the kernels against them.

Inputs are fp32 arrays; every function evaluates its formula in float64 ON those fp32 values.

Tolerances (u = 2^-24), in the manner of tests/reduce_ref.py: a reduced result obeys |got - ref| <= C_TOL * S with S the float64
sum of a magnitude of every per-element term, since each term is evaluated in fp32 (a few u of its pieces) and the
accumulation is fp64 (its own error, count * 2^-52 * S, is far below).
- bd_moments and bd_segment_sumsq evaluate nothing in fp32 (a difference p - q IS the fp32 difference by definition, the
  squares are formed in fp64): count, min, max and the non-finite count are exact, the sums agree with the float64 sum of
  the same values to n * 2^-52 * sum|term| (the fp64 additions, any order).
- Gaussian entropy term 0.5 ln(2 pi e) + ln s: magnitude 0.5 ln(2 pi e) + |ln s|.  KL term: 0.5 (vr + t^2 + 1 + |ln vr|), the
  pieces of the kernel's 0.5 (vr + t^2 - 1 - ln vr) in absolute value (reduce_ref.kl_terms_abs).
- Categorical factor: lq = x - lse carries an absolute error of a few u (|x| + |lse| + 4) =: u A (reduce_ref.cat_probs_ref,
  cat_kl_ref), q = exp(lq) the same as a relative error.  So a KL class term q (lq - lp) has magnitude q (Aq + Ap), an
  entropy class term q lq has q (1 + |lq|) Aq, and a factor's largest probability has q_max Aq.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
C_TOL = 1e-6                   # tests/dense_ref.py
EPS64 = 2.0 ** -52
GAUSS_ENT_CONST = 0.5 * np.log(2 * np.pi * np.e)
WORDS, LATENT_WORDS, LATENT_CAT_WORDS = 6, 15, 5


# ---- bd_moments ----------------------------------------------------------------------------------------------------------

def moments_ref(p: np.ndarray, q: np.ndarray = None):
    """(sextuple, S_sum, S_sumsq): count of finite values, sum, sum of squares, min, max, count of non-finite values of p (or
    of the fp32 difference p - q), and the float64 sums of |v| and v^2 that scale the two sums' tolerance."""
    v = np.asarray(p, dtype=np.float32).ravel()
    if q is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            v = (v - np.asarray(q, dtype=np.float32).ravel()).astype(np.float32)
    fin = np.isfinite(v)
    f = v[fin].astype(np.float64)
    out = np.array([f.size, f.sum(), (f * f).sum(), f.min() if f.size else np.inf, f.max() if f.size else -np.inf,
                    v.size - f.size], dtype=np.float64)
    return out, float(np.abs(f).sum()), float((f * f).sum())


def sum_bound(n: int, S: float) -> float:
    """fp64 accumulation of n terms in any order."""
    return n * EPS64 * S


# ---- bd_segment_sumsq ------------------------------------------------------------------------------------------------------

def segment_sumsq_ref(x: np.ndarray, offsets) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return np.array([(x[a:b] ** 2).sum() for a, b in zip(offsets[:-1], offsets[1:])], dtype=np.float64)


# ---- bd_latent_stats -------------------------------------------------------------------------------------------------------

def gauss_entropy(s):
    return GAUSS_ENT_CONST + np.log(s)


def gauss_kl(qm, qs, pm, ps):
    """ln(ps / qs) + (qs^2 + (qm - pm)^2) / (2 ps^2) - 1/2, elementwise."""
    return np.log(ps / qs) + (qs * qs + (qm - pm) ** 2) / (2 * ps * ps) - 0.5


def latent_stats_ref(qm, qs, pm, ps):
    """(out[15], colsum[S], S_out[3], S_col[S]) for [rows x S] fp32 inputs; S_* are the tolerance magnitudes of the three
    fp32-evaluated sums and of the column sums."""
    qm, qs, pm, ps = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (qm, qs, pm, ps))
    kl = gauss_kl(qm, qs, pm, ps)
    out = np.empty(LATENT_WORDS)
    out[0], out[1], out[2] = gauss_entropy(qs).sum(), gauss_entropy(ps).sum(), kl.sum()
    out[3:9] = moments_ref(qs.astype(np.float32))[0]
    out[9:15] = moments_ref(ps.astype(np.float32))[0]
    vr = (qs / ps) ** 2
    kl_abs = 0.5 * (vr + ((qm - pm) / ps) ** 2 + 1 + np.abs(np.log(vr)))
    mags = np.array([(GAUSS_ENT_CONST + np.abs(np.log(qs))).sum(), (GAUSS_ENT_CONST + np.abs(np.log(ps))).sum(), kl_abs.sum()])
    return out, kl.sum(0), mags, kl_abs.sum(0)


# ---- bd_latent_stats_categorical -------------------------------------------------------------------------------------------

def log_softmax(x):
    m = x.max(-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(-1, keepdims=True))
    return x - lse, lse


def cat_entropy(l):
    """-sum_c q ln q with 0 ln 0 = 0, from normalised log-probabilities."""
    q = np.exp(l)
    return -np.where(q == 0, 0.0, q * l).sum(-1)


def cat_kl(lq, lp):
    q = np.exp(lq)
    return np.where(q == 0, 0.0, q * (lq - lp)).sum(-1)


def latent_stats_cat_ref(ql, pl):
    """(out[5], colsum[D], used[D, C], S_out[5], S_col[D]) for [rows x D x C] fp32 logits."""
    xq, xp = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (ql, pl))
    lq, lseq = log_softmax(xq)
    lp, lsep = log_softmax(xp)
    q, p = np.exp(lq), np.exp(lp)
    kl = cat_kl(lq, lp)                                                  # (rows, D)
    out = np.array([cat_entropy(lq).sum(), cat_entropy(lp).sum(), kl.sum(), q.max(-1).sum(), p.max(-1).sum()])
    D, C = xq.shape[1:]
    used = np.zeros((D, C), dtype=np.uint32)
    arg = np.asarray(ql, dtype=np.float32).argmax(-1)                    # first maximum wins; x -> x - lse keeps the order
    used[np.broadcast_to(np.arange(D), arg.shape).ravel(), arg.ravel()] = 1
    Aq, Ap = np.abs(xq) + np.abs(lseq) + 4, np.abs(xp) + np.abs(lsep) + 4
    kl_abs = (q * (Aq + Ap)).sum(-1)
    mags = np.array([(q * (1 + np.abs(lq)) * Aq).sum(), (p * (1 + np.abs(lp)) * Ap).sum(), kl_abs.sum(),
                     (q * Aq).max(-1).sum(), (p * Ap).max(-1).sum()])
    return out, kl.sum(0), used, mags, kl_abs.sum(0)


# ---- diagnostics.py's derivations ------------------------------------------------------------------------------------------

def stats_ref(v: np.ndarray) -> dict:
    """mean, population std, min, max, rms of the finite values of v in float64 (two-pass variance)."""
    v = np.asarray(v, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        return dict(mean=np.nan, std=np.nan, min=np.inf, max=-np.inf, rms=np.nan, var=np.nan)
    return dict(mean=v.mean(), std=v.std(), min=v.min(), max=v.max(), rms=np.sqrt((v * v).mean()), var=v.var())


def explained_variance_ref(returns, values) -> float:
    r, v = (np.asarray(a, dtype=np.float64).ravel() for a in (returns, values))
    if not r.var() > 0:
        return np.nan
    return 1.0 - (r - v).var() / r.var()
