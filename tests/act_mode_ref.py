"""Float64 reference of the evaluation policy's selection rule (tanh_normal_mode_index in csrc/act.hip, behind
bd_tanh_normal_mode and the fused acting step's action_mode = BD_POLICY_MODE): SampleDist.mode (src/models.py:708-723) -- of
n draws y_j = tanh(mean + sd e_j) per row, the one with the largest tanh-Normal log-density summed over the A action
dimensions, the first maximum winning.

The per-draw terms are those of tests/entropy_ref.py (``sample64``: Term(ref, S, allow) of lp per (draw, row, dim),
evaluated at an fp32 value of y as that file explains).  The kernel adds a draw's A terms in fp32 in column order, a
chain of A additions: the sum bound of reduce_ref.py, red_c(A) sum|lp|, joins the sum of the per-term bounds
(``estimate64`` forms the entropy the same way).  So per (draw j, row)

    ref(j) = sum_c lp(j, c),     bound(j) = red_c(A) sum_c |lp(j, c)| + sum_c (C_TOL S(j, c) + allow(j, c)).

An argmax cannot be compared with a tolerance; what fp32 code can be held to is this: the true fp32 winner's float64 value
is at most bound away from what the kernel saw, so index j is *admissible* when

    ref(j) + bound(j) >= max_k (ref(k) - bound(k)).

A kernel that returns an inadmissible index has mis-evaluated a log-density by more than its bound, or mis-reduced.  Rows
with one admissible index pin the index; rows with several (near ties, by construction rare in the test inputs) accept any
of them -- except where the tie is exact in the INPUTS (two identical draws): there the first index is required, which the
GPU test plants.  The expected action of index j is tanh(mean + sd e_j) in float64.

The bounds hold for draws in the regular (|u| <= U_REG) or saturated (|u| >= U_SAT) regime only; the cases below are
constructed that way and the CPU test asserts it, with the cap on rows with more than one admissible index
(MULTI_CAP) as a condition on the inputs."""
from __future__ import annotations

import torch

from tests import entropy_ref as ER
from tests.dense_ref import C_TOL
from tests.reduce_ref import red_c

D64 = torch.float64
MULTI_CAP = 0.10            # share of rows with more than one admissible index, per case


def draw_terms(mean, sd, eps):
    """mean, sd [N, A], eps [n, N, A] (fp32 values) -> (ref [n, N], bound [n, N]) of the summed log-density, float64."""
    A = eps.shape[-1]
    t = ER.sample64(mean.unsqueeze(0), sd.unsqueeze(0), eps)["lp"]
    ref = t.ref.sum(-1)
    bound = red_c(A) * t.ref.abs().sum(-1) + (C_TOL * t.S + t.allow).sum(-1)
    return ref, bound


def admissible(mean, sd, eps):
    """[n, N] bool: the indices a correct fp32 evaluation may return."""
    ref, bound = draw_terms(mean, sd, eps)
    return ref + bound >= (ref - bound).max(0, keepdim=True).values


def winner(mean, sd, eps):
    """The float64 argmax per row, first maximum winning: [N] int64."""
    ref, _ = draw_terms(mean, sd, eps)
    n = ref.shape[0]
    is_max = ref == ref.max(0, keepdim=True).values
    return torch.where(is_max, torch.arange(n).view(n, 1).expand_as(ref), n).min(0).values


def action_of(mean, sd, eps, index):
    """tanh(mean + sd e_j) in float64 for j = index [N]: [N, A]."""
    n, N, A = eps.shape
    e = torch.gather(eps.double(), 0, index.long().view(1, N, 1).expand(1, N, A)).squeeze(0)
    return torch.tanh(mean.double() + sd.double() * e)


def regular_or_saturated(mean, sd, eps):
    """[N] bool: every draw of the row lies in the regular or the saturated regime (the float64 u)."""
    u = mean.double().unsqueeze(0) + sd.double().unsqueeze(0) * eps.double()
    return (ER.regime_of(u) != ER.BETWEEN).all(-1).all(0)


def multi_share(mean, sd, eps) -> float:
    """Share of rows with more than one admissible index."""
    return float((admissible(mean, sd, eps).sum(0) > 1).double().mean())


def check(index, action, mean, sd, eps, tol, tag=""):
    """The kernel's (index [N], action [N, A]) against the reference: every index admissible, the action within `tol` of the
    float64 action of THAT index.  Returns the number of rows with more than one admissible index."""
    adm = admissible(mean, sd, eps)
    index = index.long().cpu()
    n, N = adm.shape
    assert bool(((index >= 0) & (index < n)).all()), f"{tag}index out of range: {index.tolist()}"
    ok = torch.gather(adm, 0, index.view(1, N)).squeeze(0)
    if not bool(ok.all()):
        r = int((~ok).nonzero()[0])
        ref, bound = draw_terms(mean, sd, eps)
        w = int(winner(mean, sd, eps)[r])
        raise AssertionError(f"{tag}row {r}: index {int(index[r])} is not admissible: ref {float(ref[index[r], r])!r} + bound "
                             f"{float(bound[index[r], r]):.3e} < float64 winner {w}: {float(ref[w, r])!r} - {float(bound[w, r]):.3e}")
    want = action_of(mean, sd, eps, index)
    err = (action.double().cpu() - want).abs()
    assert bool((err <= tol + tol * want.abs()).all()), f"{tag}action: max err {float(err.max()):.3e} against index' float64 action"
    return int((adm.sum(0) > 1).sum())


# ---- the GPU cases of bd_tanh_normal_mode (tests/test_act_mode_kernels_gpu.py; the CPU test asserts their conditions) ------
# N rows: 1, 17 (more than one workgroup of 8 waves), 70; A: 2, 3, 17; n: 1, 64 and 65 (the pass boundary of the 64-lane
# walk), 100 (the workload's value: a partial second pass).  A >= 2 everywhere: with A = 1 and a small std the top draws
# pack too tightly for the cap on near ties.
SIZES = [(N, A, n) for N in (1, 17, 70) for A in (2, 3, 17) for n in (1, 64, 65, 100)]
SAT_MEAN, SAT_SD = 20.0, 1.5


def kinds_of(A: int):
    """The input kinds run at width A: "mixed" needs two regular dimensions beside the saturated one."""
    return ("regular", "mixed") if A >= 3 else ("regular",)


def case_seed(N: int, A: int, n: int, kind: str) -> int:
    return 1000 + 97 * SIZES.index((N, A, n)) + ("regular", "mixed").index(kind)


def make_case(N: int, A: int, n: int, kind: str):
    """(mean, sd, eps) fp32, every draw regular or saturated.
    regular: |mean| <= 1, sd in [0.2, 0.8], |e| <= 2.49 (entropy_ref.make_regular): |u| < 3.
    mixed: the same, but dimension row % A of every row has mean = +-20 and sd = 1.5: |u| >= 20 - 1.5 * 2.49 = 16.3, the
    saturated regime for every draw.  One saturated dimension per row, and sd no smaller: its term is the same for every
    draw (y = +-1 exactly), but its bound is not zero -- the quadratic (atanh(c) - 20)^2 / (2 sd^2) = 28 is an operand
    like any other -- and widens every draw's bound by 1e-4; at sd = 0.2 it would be 1600 and every draw admissible."""
    seed = case_seed(N, A, n, kind)
    mean, sd, eps = ER.make_regular(1, N, A, n, seed)
    mean, sd, eps = mean[0].clone(), sd[0].clone(), eps[0].clone()
    if kind == "mixed":
        row, col = torch.arange(N).view(N, 1), torch.arange(A).view(1, A)
        sat = col == row % A
        sign = torch.where(row % 2 == 0, 1.0, -1.0).expand(N, A)
        mean = torch.where(sat, SAT_MEAN * sign, mean)
        sd = torch.where(sat, torch.full_like(sd, SAT_SD), sd)
    return mean.contiguous(), sd.contiguous(), eps.contiguous()


# planted exact ties per n: (j1, j2), j1 < j2 -- two lanes of one pass; one lane in two passes (0 and 64; 5 and 69); neighbours
TIES = {64: [(10, 42)], 65: [(0, 64)], 100: [(5, 69), (37, 38)]}


def peak_draw(mean, sd):
    """Per (row, dim) the e in [-2.49, 2.49] that maximises that dimension's log-density term -e^2 / 2 + 2 (x + softplus(-2 x)),
    x = mean + sd e (regular regime: the clamp is far away), on a grid of 1e-3, as fp32: [N, A].  A sum of A such terms is
    largest where each is."""
    grid = torch.linspace(-2.49, 2.49, 4981, dtype=D64).view(-1, 1, 1)
    x = mean.double().unsqueeze(0) + sd.double().unsqueeze(0) * grid
    f = -0.5 * grid * grid + 2.0 * (x + torch.nn.functional.softplus(-2.0 * x))
    return grid.view(-1)[f.argmax(0)].float()


def plant_tie(mean, sd, eps, j1: int, j2: int):
    """Draws j1 < j2 made identical in every row, and the winners: both get each regular dimension's peak (peak_draw; in
    a saturated dimension, |mean| = 20, every draw gives the same term and the planted value 0 keeps |u| = 20).  That
    they are the only admissible indices of every row is asserted on the float64 side (the CPU test)."""
    e = torch.where(mean.abs() >= 20.0, torch.zeros_like(mean), peak_draw(mean, sd))
    eps = eps.clone()
    eps[j1] = e
    eps[j2] = e
    return eps


# ---- the fused acting step with an evaluation policy (tests/test_act_mode_gpu.py) -------------------------------------------
# name -> (dims, data seed): the four (latent, actor) configurations at the tiny dims of tests/test_act_step_gpu.py /
# tests/act_cat_ref.py (no width a multiple of 16), and 32 x 32 latents for the register form of the latent argmax.
def fused_cases():
    from tests import act_cat_ref as CR
    return {"gauss_tanh": (CR._dims(), 0), "cat3x5_tanh": CR.CASES["cat3x5_tanh"], "cat32_tanh": CR.CASES["cat32_tanh"],
            "cat3x5_disc2": CR.CASES["cat3x5_disc2"], "gauss_disc2": CR.CASES["gauss_disc2"]}


FUSED_B = (1, 17)           # one row; one more than the 16-row tile
FUSED_PARAM_SEED = 11


def policy_ref(P, d, data, B, form, state_mean):
    """The float64 decision of call 0 on the first B rows under action_mode = "mean" (tanh(mean); Categorical actor: the
    class of argmax p, q = 1) and the given state_mean (posterior noise 0, or q = 1): (belief', state', action', info,
    actor mean, actor std) -- mean / std None for the Categorical actor -- from tests/act_cat_ref.py's restatement."""
    import numpy as np
    from tests import act_cat_ref as CR
    from tests import act_ref
    post = data["post"][0, :B]
    if state_mean:
        post = np.ones_like(post) if d.categorical else np.zeros_like(post)
    act = np.ones((B, d.A), np.float32) if d.discrete_actions else np.zeros((B, d.A), np.float32)
    kw = {"obs": data["obs"][0, :B]} if form == "obs" else {"embedding": data["emb"][0, :B]}
    h2, s2, a2, info = CR.act_step_cat(P, d, data["belief"][:B], data["state"][:B], data["action"][:B], post, act, **kw)
    mean = std = None
    if d.discrete_actions:
        a2 = np.eye(d.A)[info["actor_idx"]]
    else:
        ao = act_ref.dense(P["actor"], np.concatenate([h2, s2], 1))
        mean = act_ref.ACT_MEAN_SCALE * np.tanh(ao[:, :d.A] / act_ref.ACT_MEAN_SCALE)
        std = act_ref._softplus(ao[:, d.A:] + np.log(np.expm1(act_ref.ACT_INIT_STD))) + act_ref.ACT_MIN_STD
    return h2, s2, a2, info, mean, std


def eps_for_stats(mean, sd, n, seed):
    """n draws per row for GIVEN statistics [N, A] (the kernel's own act_stats_out: a fresh actor's std is about 5, and
    standard normal draws would leave the regular regime without reaching the saturated one): e = (target - mean) / sd
    with the target u uniform in [-2.9, 2.9].  eps [n, N, A] fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    N, A = mean.shape
    target = -2.9 + 5.8 * torch.rand(n, N, A, generator=g, dtype=D64)
    return ((target - mean.double().cpu().unsqueeze(0)) / sd.double().cpu().unsqueeze(0)).float()
