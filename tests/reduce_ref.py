"""Float64 references and tolerances for the loss, KL, latent-head, lambda-return, clip+Adam and polyak kernels
(csrc/reduce.hip) and bd_colsum (csrc/conv.hip).  Plain helpers, not a conftest: the CPU sharpness tests
(test_reduce_ref_cpu.py) import them on CPU tensors, the GPU tests (test_reduce_kernels_gpu.py) on copies of the
kernels' inputs.  Comparison, sentinel and buffer placement come from tests/dense_ref.py.

References.  The oracle's own functions evaluated in float64 with autograd (lambda_return, normal_nll_mean, kl_loss,
kl_loss_categorical, kl_categorical; (rows, ...) operands are viewed as (T=1, B=rows, ...)), and torch itself in float64
where torch has the operation (binary_cross_entropy_with_logits, softplus(threshold=20), softmax, torch.optim.Adam with
torch.nn.utils.clip_grad_norm_).  The oracle builds its free-nats tensor with torch.full, so the references run under a
float64 default dtype: free_nats then enters the float64 comparison unrounded.

Tolerances (u = 2^-24, the fp32 unit roundoff).
- Reductions (the scalar in scalars[slot]): |got - ref| <= c * sum|term_i| + allow, sum|term_i| the float64 sum of the
  absolute pieces of every per-element term (a KL term 0.5 (vr + t^2 - 1 - log vr) contributes
  0.5 (vr + t^2 + 1 + |log vr|): the pieces cancel, their rounding errors do not).  Each term is fp32, the block and
  final sums fp64, the result one fp32 rounding: the error is a few u per term.  c = C_TOL = 1e-6, raised to
  (chain + 8) u where a term is itself an fp32 sequential sum of `chain` pieces (the KL sum form: S or D + 9 additions).
- Elementwise outputs: |got - ref| <= c * S + allow with S a float64 magnitude of the same formula in absolute values,
  c = C_TOL.  `allow` is nonzero only where the default build uses the hardware __expf / __logf / rcp forms
  (bd_device.h softplusf / sigmoidf, about 2e-7 absolute): SOFTPLUS_ALLOW on std and on state (times |eps|),
  SOFTPLUS_ALLOW * |g| on the std pre-activation gradient.  A long fp32 recurrence (lambda-return) gets c * (steps) * S:
  the error of step t is carried by the factor discount * lambda <= 1 into every later step.  bd_colsum sums in fp32:
  c = (chain + 8) u with chain the longest sequential addition chain of its two-pass dispatch (colsum_chain).
- Adam.  The kernel receives fp32 hyper-parameters, so the reference runs torch.optim.Adam on those fp32 values
  (1 - fl(beta2) is exact in both).  With all fp32 ops rounding by u:
      gc = g coef          coef = clamp(max_norm / (sqrt(sumsq) + 1e-6), max=1) carries ~4u:  |dgc| <= 6u |gc|
      gw = gc + wd p                                                         |dgw| <= 8u Sgw,  Sgw = |gc| + |wd p|
      m' = m + (1 - b1)(gw - m)                                              |dm'| <= 12u Am,  Am = b1 |m| + (1-b1) Sgw
      v' = b2 v + (1 - b2) gw^2                                              |dv'| <= 20u Av,  Av = b2 v + (1-b2) Sgw^2
      D  = sqrt(v') / sqrt(bc2) + eps       |dD| <= |dv'| / (2 sqrt(v') sqrt(bc2)) + 3u D
      p' = p - ss m' / D  (ss = lr / bc1)   |dp'| <= u |p'| + ss (|dm'| / D + |m'| |dD| / D^2) + 3u ss |m'| / D
  which gives  |dp'| <= c (|p'| + |p| + ss Am / D + ss |m'| Av / (sqrt(v' bc2) D^2)),  c = C_TOL ~ 16.8u covering the
  constants above; g', m' and v' are checked against c * |gc|, c * Am, c * Av.
- Branch decisions (free nats, argmax) are made in fp32: the cases either keep a margin far wider than fp32 error or
  make an exact tie in both arithmetics.  The Categorical sample is compared with argmax(probs_got / q) evaluated in
  fp32 on the CPU (first maximum wins); probs are compared separately with the float64 softmax.
"""
from __future__ import annotations

import contextlib
import math

import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O
from tests.dense_ref import C_TOL, SENTINEL, Placed, check_close, placed_input  # noqa: F401  (re-exported)

U = 2.0 ** -24
SOFTPLUS_ALLOW = 2e-7      # |__logf(1 + __expf(x)) - softplus(x)| and the rcp sigmoid, absolute (bd_device.h)
TINY = 1e-37               # fp32 underflow: probabilities below the normal range keep no relative accuracy
D64 = torch.float64


@contextlib.contextmanager
def f64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(D64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def f32(x: float) -> float:
    """The value an fp32 ABI argument carries."""
    return float(torch.tensor(x, dtype=torch.float32))


def red_c(chain: int = 0) -> float:
    return max(C_TOL, (chain + 8) * U)


def check_scalar(name: str, got: float, ref: float, S: float, c: float = C_TOL, allow: float = 0.0) -> float:
    """|got - ref| <= c * S + allow for one reduced scalar (NaN fails); returns |got - ref| / S."""
    err = abs(got - ref)
    if not err <= c * S + allow:
        raise AssertionError(f"{name}: scalar out of tolerance: got {got!r}, ref {ref!r}, sum|term| {S!r}, c {c}")
    return err / S if S > 0 else 0.0


def mg64(x, fn: float):
    """torch.maximum's backward factor for x against free_nats (float64 tensor)."""
    return torch.where(x < fn, torch.zeros_like(x), torch.where(x == fn, torch.full_like(x, 0.5), torch.ones_like(x)))


# ---- reductions --------------------------------------------------------------------------------------------------------

def sum_ref(x: torch.Tensor, square: bool = False):
    x = x.double()
    t = x * x if square else x
    return float(t.sum()), float(t.abs().sum())


def normal_nll_ref(pred, target, grad_scale: float):
    """scalar = sum(0.5 d^2 + log sqrt(2 pi)), dpred = grad_scale * d: (scalar, S, dpred64, Sd)."""
    p = pred.double().detach().requires_grad_(True)
    t = target.double()
    rows = p.shape[0]
    with f64_default():
        loss = O.normal_nll_mean(p, t) * rows       # the kernel's scalar: the sum over rows of the oracle's per-row loss
    loss.backward()
    d = p.detach() - t
    S = float((0.5 * d * d + O.HALF_LOG_2PI).sum())
    dref = p.grad * float(grad_scale)
    return float(loss.detach()), S, dref, dref.abs()


def bernoulli_ref(x, t, grad_scale: float):
    xx = x.double().detach().requires_grad_(True)
    tt = t.double()
    loss = F.binary_cross_entropy_with_logits(xx, tt, reduction="sum")
    loss.backward()
    xd = xx.detach()
    S = float((xd.clamp(min=0) + (xd * tt).abs() + torch.log1p(torch.exp(-xd.abs()))).sum())
    gs = float(grad_scale)
    dref = xx.grad * gs
    Sd = (torch.sigmoid(xd) + tt.abs()) * abs(gs)
    return float(loss.detach()), S, dref, Sd


# ---- Gaussian KL ---------------------------------------------------------------------------------------------------------

def kl_terms_abs(qm, qs, pm, ps):
    qm, qs, pm, ps = (a.double() for a in (qm, qs, pm, ps))
    vr = (qs / ps) ** 2
    t2 = ((qm - pm) / ps) ** 2
    return 0.5 * (vr + t2 + 1 + vr.log().abs())


def kl_ref(qm, qs, pm, ps, free_nats: float, kl_balance: float, weight: float):
    """The kernel pair's outputs in float64: (scalar, S_scalar, mean-or-None, [dqm, dqs, dpm, dps], [S for each]).
    balanced: scalar = sum of the KL terms; sum form (kl_balance = -1): scalar = sum_rows max(sum_S KL, free_nats).
    Gradients: d(weight * kl_loss) by autograd through the oracle."""
    rows, S = qm.shape
    ins = [a.double().detach().reshape(1, rows, S).requires_grad_(True) for a in (qm, qs, pm, ps)]
    with f64_default():
        kl = O.kl_normal(*[a.detach() for a in ins])[0]
        loss = weight * O.kl_loss((ins[0], ins[1]), (ins[2], ins[3]), kl_balance, free_nats)
    loss.sum().backward()
    grads = [a.grad.reshape(rows, S) for a in ins]
    tabs = kl_terms_abs(qm, qs, pm, ps)
    a, b, c, d = (x.double() for x in (qm, qs, pm, ps))
    diff = (a - c).abs()
    if kl_balance == -1:
        rs = kl.sum(-1)
        scalar = float(torch.maximum(rs, torch.full_like(rs, free_nats)).sum())
        Ssc = float(tabs.sum()) + rows * abs(free_nats)
        f = mg64(rs, free_nats)[:, None] * abs(weight) / rows
        fq = fp = f
        mean = None
    else:
        scalar = float(kl.sum())
        Ssc = float(tabs.sum())
        mean = float(kl.mean())
        f = float(mg64(torch.tensor(mean), free_nats)) * abs(weight) / (rows * S)
        fq, fp = abs(1 - kl_balance) * f, abs(kl_balance) * f
    mags = [fq * diff / d ** 2, fq * (b / d ** 2 + 1 / b), fp * diff / d ** 2, fp * (1 / d + (b * b + diff * diff) / d ** 3)]
    return scalar, Ssc, mean, grads, mags


# ---- Gaussian head -------------------------------------------------------------------------------------------------------

def gauss_head_ref(out, eps, min_std: float):
    """(mean, std, state) of GaussianBeliefModel's tail in float64 and (S, allow) for each."""
    M, S2 = out.shape
    S = S2 // 2
    o = out.double()
    m, raw = o[:, :S], o[:, S:]
    sp = F.softplus(raw, beta=1, threshold=20)
    std = sp + min_std
    e = eps.double()
    state = m + std * e
    return ((m, m.abs(), 0.0), (std, sp + abs(min_std), SOFTPLUS_ALLOW),
            (state, m.abs() + (std * e).abs(), SOFTPLUS_ALLOW * e.abs()))


def gauss_head_bwd_ref(out, eps, dstate, dmean, dstd):
    """dout = [dmean + dstate | (dstd + dstate * eps) * sigmoid(raw)] by autograd; (ref, S, allow)."""
    M, S2 = out.shape
    S = S2 // 2
    o = out.double().detach().requires_grad_(True)
    m, raw = o[:, :S], o[:, S:]
    std = F.softplus(raw, beta=1, threshold=20) + 0.1
    z = torch.zeros(M, S, dtype=D64)
    e = eps.double() if eps is not None else z
    loss = (std * (dstd.double() if dstd is not None else z)).sum() + (m * (dmean.double() if dmean is not None else z)).sum()
    if dstate is not None:
        loss = loss + ((m + std * e) * dstate.double()).sum()
    loss.backward()
    ds = dstate.double().abs() if dstate is not None else z
    gs_abs = ds * e.abs() + (dstd.double().abs() if dstd is not None else z)
    sig = torch.sigmoid(raw.detach())
    Sg = torch.cat([ds + (dmean.double().abs() if dmean is not None else z), gs_abs * sig], 1)
    allow = torch.cat([z, SOFTPLUS_ALLOW * gs_abs], 1)
    return o.grad, Sg, allow


# ---- lambda-return -------------------------------------------------------------------------------------------------------

def lambda_ref(reward, value, disc: float, lam: float, dret=None, dconst: float = 0.0):
    """returns, d reward, d value through the oracle's lambda_return (bootstrap = value[Hm-1]) in float64, and the
    magnitudes: the same recursions in absolute values times the number of steps they chain."""
    Hm, N = reward.shape
    r = reward.double().detach().requires_grad_(True)
    v = value.double().detach().requires_grad_(True)
    ret = O.lambda_return(r, v, v[Hm - 1], disc, lam)
    g = dret.double() if dret is not None else torch.full((Hm, N), float(dconst), dtype=D64)
    ret.backward(g)
    ra, va = reward.double().abs(), value.double().abs()
    dl, w = abs(disc * lam), abs(disc * (1 - lam))
    Sret = torch.empty(Hm, N, dtype=D64)
    last = va[Hm - 1]
    for t in reversed(range(Hm)):
        nxt = va[Hm - 1] if t == Hm - 1 else va[t + 1]
        last = ra[t] + w * nxt + dl * last
        Sret[t] = last * (Hm - t)
    ga = g.abs()
    SG = torch.empty(Hm, N, dtype=D64)
    G = torch.zeros(N, dtype=D64)
    for t in range(Hm):
        G = ga[t] + dl * G
        SG[t] = G * (t + 1)
    Sv = torch.zeros(Hm, N, dtype=D64)
    Sv[1:] = SG[:-1] * w
    Sv[Hm - 1] += SG[Hm - 1] * (w + dl)
    return ret.detach(), Sret, r.grad, SG, v.grad, Sv


# ---- clip + Adam -------------------------------------------------------------------------------------------------------

class AdamRef:
    """torch.optim.Adam + clip_grad_norm_ on float64 copies of one flat parameter.  step() takes the state the kernel
    holds (p, m, v and the gradient it read) and returns the reference after one step with the magnitudes above."""

    def __init__(self, n: int, lr, betas, eps, wd, max_norm, start_step: int = 0):
        self.hp = dict(lr=f32(lr), betas=(f32(betas[0]), f32(betas[1])), eps=f32(eps), weight_decay=f32(wd))
        self.max_norm = f32(max_norm)
        self.p = torch.zeros(n, dtype=D64, requires_grad=True)
        self.opt = torch.optim.Adam([self.p], **self.hp)
        self.step_no = start_step

    def step(self, p, g, m, v):
        b1, b2 = self.hp["betas"]
        wd, lr, eps = self.hp["weight_decay"], self.hp["lr"], self.hp["eps"]
        with torch.no_grad():
            self.p.copy_(p.double())
        self.p.grad = g.double().clone()
        st = self.opt.state[self.p]
        st["step"] = torch.tensor(float(self.step_no), dtype=torch.float32)
        st["exp_avg"] = m.double().clone()
        st["exp_avg_sq"] = v.double().clone()
        torch.nn.utils.clip_grad_norm_([self.p], self.max_norm)
        gc = self.p.grad.clone()
        self.opt.step()
        self.step_no += 1
        k = self.step_no
        bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
        ss = lr / bc1
        p0, m0, v0 = p.double(), m.double(), v.double()
        Sgw = gc.abs() + (wd * p0).abs()
        Am = b1 * m0.abs() + (1 - b1) * Sgw
        Av = b2 * v0.abs() + (1 - b2) * Sgw * Sgw
        m1, v1, p1 = st["exp_avg"], st["exp_avg_sq"], self.p.detach()
        D = v1.sqrt() / math.sqrt(bc2) + eps
        rt = (v1 * bc2).sqrt()
        vterm = torch.where(rt > 0, m1.abs() * Av / (rt * D * D + (rt == 0).double()), torch.zeros_like(rt))
        Sp = p1.abs() + p0.abs() + ss * (Am / D + vterm)
        return dict(p=(p1.clone(), Sp), g=(gc, gc.abs()), m=(m1.clone(), Am), v=(v1.clone(), Av))


def polyak_ref(t, s, w: float):
    t64, s64 = t.double(), s.double()
    return s64 * w + t64 * (1 - w), (s64 * w).abs() + (t64 * (1 - w)).abs()


# ---- Categorical latents -----------------------------------------------------------------------------------------------

def cat_probs_ref(logits):
    """float64 softmax of (rows, D, C) logits and (S, allow): the fp32 kernel loses |x| + |lse| ulps in the exponent."""
    x = logits.double()
    lse = x.logsumexp(-1, keepdim=True)
    p = torch.softmax(x, -1)
    return p, p * (8 + 2 * x.abs() + 3 * lse.abs()), TINY


def expected_state(probs_got, q):
    """one_hot(argmax(probs / q)) in fp32 on the CPU: the first maximum wins."""
    r = probs_got.float().cpu() / q.float().cpu()
    return F.one_hot(r.argmax(-1), r.shape[-1]).to(torch.float32)


def cat_head_bwd_ref(dstate, probs):
    """dlogits = p (g - sum_c p g) in float64 from the kernel's probs; (ref, S)."""
    p, g = probs.double(), dstate.double()
    dot = (p * g).sum(-1, keepdim=True)
    return p * (g - dot), p * (g.abs() + (p * g).abs().sum(-1, keepdim=True))


def cat_kl_ref(ql, pl, free_nats: float, kl_balance: float, weight: float):
    """(scalar, S_scalar, mean-or-None, dql, Sq, dpl, Sp) through the oracle's kl_loss_categorical in float64.
    Logits are (rows, D, C).  Magnitudes: a class term q (lq - lp) carries the ulps of x and of both lse's."""
    rows, D, C = ql.shape
    a = ql.double().detach().reshape(1, rows, D, C).requires_grad_(True)
    b = pl.double().detach().reshape(1, rows, D, C).requires_grad_(True)
    with f64_default():
        kl = O.kl_categorical(a.detach(), b.detach())[0]             # (rows, D)
        loss = weight * O.kl_loss_categorical(a, b, kl_balance, free_nats)
    loss.sum().backward()
    xq, xp = ql.double(), pl.double()
    lseq, lsep = xq.logsumexp(-1, keepdim=True), xp.logsumexp(-1, keepdim=True)
    qv, pv = torch.softmax(xq, -1), torch.softmax(xp, -1)
    mag = xq.abs() + xp.abs() + lseq.abs() + lsep.abs() + 4
    tabs = (qv * mag).sum(-1)                                        # (rows, D)
    if kl_balance == -1:
        rs = kl.sum(-1)
        scalar = float(torch.maximum(rs, torch.full_like(rs, free_nats)).sum())
        Ssc = float(tabs.sum()) + rows * abs(free_nats)
        f = (mg64(rs, free_nats) * abs(weight) / rows)[:, None, None]
        fq = fp = f
        mean = None
    else:
        scalar, Ssc, mean = float(kl.sum()), float(tabs.sum()), float(kl.mean())
        f = float(mg64(torch.tensor(mean), free_nats)) * abs(weight) / (rows * D)
        fq, fp = abs(1 - kl_balance) * f, abs(kl_balance) * f
    Sq = fq * qv * (mag + tabs[..., None])
    Sp = fp * (pv + qv) * (1 + mag)
    return scalar, Ssc, mean, a.grad.reshape(rows, D, C), Sq, b.grad.reshape(rows, D, C), Sp


# ---- bd_colsum -----------------------------------------------------------------------------------------------------------

K_COLSUM_BLOCKS = 1024


def colsum_chain(M: int, N: int) -> int:
    """Longest fp32 addition chain of bd_colsum (conv.hip colsum_partial_kernel + colsum_final_kernel)."""
    Np = 1
    while Np < N:
        Np <<= 1
    rstep = 256 // Np
    nb = (M + 63) // 64 if M < K_COLSUM_BLOCKS * 64 else K_COLSUM_BLOCKS
    per = -(-M // nb)
    return -(-per // rstep) + rstep + -(-nb // 256) + 8


def colsum_ref(x, chunk: int = 1 << 20):
    ref = torch.zeros(x.shape[1], dtype=D64, device=x.device)
    S = torch.zeros_like(ref)
    for r0 in range(0, x.shape[0], chunk):
        c = x[r0:r0 + chunk].double()
        ref += c.sum(0)
        S += c.abs().sum(0)
    return ref, S
