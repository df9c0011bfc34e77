"""Float64 references, one step and one layer at a time, for the Categorical RSSM scan kernels: the observe scan in its
one-workgroup and cluster forms (csrc/scan_cat.hip, observe_cat_cluster.hip) and the imagination scan with the tanh-Normal
actor or the Categorical one (csrc/scan_cat.hip; the latter restated in tests/scan_ref.py), heads and one-hot state
helpers from csrc/bd_categorical.h.  The method, the `(value, S, A)`
triples, `check_layers` / `fill_layers` and every allowance are those of tests/scan_ref.py (read its docstring first);
this file adds what the one-hot state changes.

State.  The state of a step is D class indices (`sidx`, uint8) and `feat[:, Be:]` their one-hot image: both are compared
EXACTLY (`feat` against one_hot(sidx), `sv_s` against the masked one-hot of the step before, zero rows staying zero).  A
layer that reads the state (embed, actor layer 0) is the float64 contraction over the action / belief columns plus the sum
of the D selected weight columns, selected BY THE KERNEL'S OWN sidx of the step before (`init_state` / `start_feat` at
t = 0), times the nonterminal factor; S holds the same terms in absolute value.

The sample.  The kernel's class k of a factor is compared with the float64 ratios r_c = softmax(l)_c / q_c of the kernel's
own fp32 logits l and the caller's fp32 draws q: it must satisfy r_k >= (1 - m) * max_c r_c.  m bounds the relative error
of the two computed ratios the decision compared (u = 2^-24, d_c = l_c - max l <= 0; `*` = the float64 winner):
- C == 32, default build (cat_sample_reg<32>): r^_c = fl(__expf(fl(l_c - max)) * rcp(q_c)).  The subtraction is rounded
  once (absolute error u |d_c| in the exponent, i.e. relative u |d_c| in the result), __expf(x) has relative error
  (|x| + 2) u (scan_ref.py: v_exp_f32 is 1 ulp = 2u, the multiplication by log2 e perturbs the exponent by u |x| log2 e),
  v_rcp_f32 is 1 ulp = 2u, the product rounds once: e_c <= (2 |d_c| + 5) u.  The kernel chose k because r^_k >= r^_* (k is
  the first maximum, so this holds whichever comes first), hence r_k (1 + e_k) >= r_* (1 - e_*) and
      m_hw = e_k + e_* = (2 |d_k| + 2 |d_*| + 10) u.
- every other C, and every C in the -DBD_EXACT_MATH build (cat_sample_any, the exact branch of cat_sample_reg): three libm
  exponentials and two divisions per class, r^_c = fl(fl(expf(fl(fl(l_c - lse) - m2)) / s2) / q_c).  The first two
  exponentials only enter lse, m2 = fl(max - lse) and s2, numbers SHARED by the C classes of the factor: whatever their
  error, they multiply every ratio by the same positive factor and drop out of the comparison.  Per class: fl(l_c - lse)
  has absolute error u |l_c - lse| <= u (|d_c| + ln C) (lse - max = ln sum exp(d) <= ln C), the second subtraction
  u |d_c| (to first order), so the exponent is off by (2 |d_c| + ln C) u, which is the relative error of the result; libm
  expf is 1 ulp = 2u; both divisions are correctly rounded, u each: e_c <= (2 |d_c| + ln C + 4) u and
      m_libm = (2 |d_k| + 2 |d_*| + 2 ln C + 8) u.
Both assume ratios in the normal range (|d| < 80 and q >= 1e-30: asserted).  m is a function of the two distances only,
nothing is fitted to a run.  Every (row, factor) is checked.  A factor whose float64 runner-up lies within m of the best is
AMBIGUOUS: either class passes there by the same inequality; `sample_check` returns their count and the CPU tests assert
on the float64 reference alone that their share stays at or below 0.1 % for every case and seed of the tables.

Backward.  g[t] = nonterm[t+1] * (d_embed_pre[t+1] W_es) + dfeat[t][:, Be:], teacher-forced from the kernel's own
d_embed_pre[t+1] (g[T-1] = dfeat alone); d logits = p (g - sum_c p g) + dpost_logits with p from the kernel's logits.
Magnitudes: p carries reduce_ref.cat_probs_ref's S_p = p (8 + 2 |l| + 3 |lse|) (in units of C_TOL, as there), g carries
S_g = |d_embed_pre| |W_es| * nonterm + |dfeat| + |g| from its contraction, the dot product S_dot = sum_c (S_p |g| + p S_g)
+ sum_c |p g|, and the product S_p |g - dot| + p (S_g + S_dot + |g - dot|) + |p (g - dot)|
(reduce_ref.cat_head_bwd_ref's p (|g| + sum |p g|), plus what g and p inherit).  d_q1_pre, d_gi, d_gh, d_embed_pre follow
with the belief-carry recursion of scan_ref.observe_bwd_layers.  In the imagination backward the world model is frozen:
both carries recurse in float64 as triples, the state gradient passes through the straight-through Jacobian of the
kernel's prior_logits at every step (its allowance A pushed through p (A_g + sum_c p A_g)), and the rest is
scan_ref.imagine_bwd_layers with that head.
"""
from __future__ import annotations

import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import scan_ref as R
from tests.dense_ref import elu64
from tests.scan_ref import (ALL, D64, HW, U, cdiv, discrete_actor_layers, discrete_actor_tail, exp1, first_max,  # noqa: F401
                            jacobian, lin, ratios64)

_CD = namedtuple("CDims", "T B Be D C A Hd")     # imagination: T = Hm, B = N


class CDims(_CD):
    __slots__ = ()

    @property
    def S(self):
        return self.D * self.C


# ---- parameters, inputs -------------------------------------------------------------------------------------------------

def make_weights(d: CDims, seed: int, device="cpu", imagine: bool = False, bias_high: bool = False, actor=None):
    """scan_ref.make_weights with the head narrowed to S logits.  bias_high: b_2 raised on the upper half of the classes,
    so that class indices >= C / 2 are the ones sampled (C = 256: indices that do not fit a signed byte)."""
    W = R.make_weights(d, seed, device, imagine, actor)
    W["W_2"], W["b_2"] = W["W_2"][:d.S].contiguous(), W["b_2"][:d.S].contiguous()
    if bias_high:
        W["b_2"].view(d.D, d.C)[:, d.C // 2:] += 6.0
    return W


INIT_KINDS = ("zeros", "onehot", "mixed")


def one_hot_rows(idx, C):
    """[rows x D] class indices -> [rows x D*C] float64 one-hot."""
    return F.one_hot(idx.long(), C).to(D64).reshape(idx.shape[0], -1)


def make_state(B, D, C, kind, g):
    """A [B x S] state whose factors are zero or one-hot: 'zeros', 'onehot', or 'mixed' (even rows zero, odd rows one-hot)."""
    s = one_hot_rows(torch.randint(0, C, (B, D), generator=g), C).float()
    if kind == "zeros":
        s.zero_()
    elif kind == "mixed":
        s[0::2] = 0.0
    return s


def make_observe_inputs(d: CDims, seed: int, device="cpu", nonterm="zeros", init="mixed"):
    I = R.make_observe_inputs(d, seed, "cpu", nonterm=nonterm)
    g = torch.Generator().manual_seed(seed + 5000)
    del I["eps_post"]
    I["init_state"] = make_state(d.B, d.D, d.C, init, g)
    I["q_post"] = exp1(g, d.T, d.B, d.S)
    return {k: (v.to(device) if v is not None else None) for k, v in I.items()}


def make_observe_grads(d: CDims, seed: int, device="cpu", dpl=True):
    g = torch.Generator().manual_seed(seed + 2000)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    return dict(dfeat=r(d.T, d.B, d.Be + d.S), dpost_logits=r(d.T, d.B, d.S) if dpl else None)


def make_imagine_inputs(d: CDims, seed: int, device="cpu", start="mixed", discrete=False, saturated=False):
    """discrete: eps_action holds the Exp(1) draws of the Categorical actor's sampler; saturated: scan_ref.set_sat_gate."""
    g = torch.Generator().manual_seed(seed + 3000)
    r = lambda *s: torch.randn(*s, generator=g)
    h = torch.tanh(r(d.B, d.Be))
    I = dict(eps_action=exp1(g, d.T, d.B, d.A) if discrete else r(d.T, d.B, d.A), q_prior=exp1(g, d.T, d.B, d.S))
    I["start_feat"] = torch.cat([h, make_state(d.B, d.D, d.C, start, g)], 1)
    if saturated:
        R.set_sat_gate(I["start_feat"])
    return {k: v.to(device) for k, v in I.items()}


make_imagine_grads = R.make_imagine_grads


def make_discrete_case(d, seed, variant="regular", device="cpu"):
    return R.make_discrete_case(d, seed, variant, device, make_weights, make_imagine_inputs)


# ---- the sample ---------------------------------------------------------------------------------------------------------

def sample_path(C: int, exact: bool = False) -> str:
    return "hw" if (C == 32 and not exact) else "libm"


def sample_margin(dk, dstar, C: int, path: str):
    """m of the module docstring from |l_k - max l| and |l_* - max l|."""
    if path == "hw":
        return (2 * dk.abs() + 2 * dstar.abs() + 10) * U
    return (2 * dk.abs() + 2 * dstar.abs() + 2 * math.log(max(C, 1)) + 8) * U


def sample_check(logits, q, sidx, D, C, path, tag="", margin_C=None):
    """Every (row, factor): the kernel's class within the margin of the float64 winner.  Returns (ambiguous factors,
    factors, factors whose class is >= 128).  margin_C: the class count of the margin's ln C where it is not C."""
    mC = margin_C or C
    r, d = ratios64(logits, q, D, C)
    k = sidx.long().reshape(-1, D, 1)
    assert int(k.min()) >= 0 and int(k.max()) < C, f"{tag}class index outside [0, {C})"
    top = r.topk(min(2, C), -1)
    star = top.indices[..., :1]
    rk, rs = r.gather(-1, k), top.values[..., :1]
    dk, dst = d.gather(-1, k), d.gather(-1, star)
    bad = ~(rk >= (1 - sample_margin(dk, dst, mC, path)) * rs)
    if bool(bad.any()):
        row, f, _ = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{tag}sample[row={row}, factor={f}]: {int(bad.sum())} of {bad.numel()} outside the margin; class "
                             f"{int(k[row, f])} with ratio {float(rk[row, f]):.9e}, float64 winner {int(star[row, f])} with "
                             f"{float(rs[row, f]):.9e}")
    amb = 0
    if C > 1:
        second = top.indices[..., 1:2]
        amb = int((top.values[..., 1:2] >= (1 - sample_margin(d.gather(-1, second), dst, mC, path)) * rs).sum())
    return amb, bad.numel(), int((k >= 128).sum())


def actor_sample_check(norm, q, action, A, rows=None, dup=None, tag="", path="libm"):
    """The Categorical actor's draws of one step: the class read from `action` [N x A] against the margin on the kernel's
    norm [N x A] (one factor of A classes, the libm path in both builds: bd_discrete.h has no hardware-exponential branch;
    `path` lets the CPU tests count the ambiguous draws under the narrower hardware margin as well).
    rows: the rows to check (the `saturated` variant passes its regular rows: the others are outside ratios64's domain and
    are asserted exactly by the layers).  dup = (lo, hi): class hi is a planted copy of class lo, so their ratios tie by
    construction and every row the pair wins would count as ambiguous; hi must never be the class (asserted), its column
    is left out of the count, and the margin keeps ln A (lse runs over all A classes).  Returns sample_check's triple."""
    k = action.argmax(-1, keepdim=True)
    if rows is not None:
        norm, q, k = norm[rows], q[rows], k[rows]
    if dup is not None:
        lo, hi = dup
        assert not bool((k == hi).any()), f"{tag}class {hi} sampled although class {lo} ties with it"
        keep = [c for c in range(A) if c != hi]
        norm, q, k = norm[:, keep], q[:, keep], k - (k > hi).long()
    if norm.shape[0] == 0:
        return 0, 0, 0
    return sample_check(norm, q, k, 1, norm.shape[1], path, tag, margin_C=A)


def actor_checks(d, norm, eps, action, sat=None, dup=None, tag="", path="libm"):
    """actor_sample_check over every step of a case ([T x N x A] tensors) and, with a planted pair, the duplicate check.
    Returns (ambiguous draws, draws checked, times the planted pair won or None)."""
    rows = None if sat is None else ~sat
    amb = n = 0
    for t in range(d.T):
        a, m, _ = actor_sample_check(norm[t], eps[t], action[t], d.A, rows, dup, f"{tag}action t={t} ", path)
        amb, n = amb + a, n + m
    return amb, n, (R.actor_duplicate_check(d, norm, action) if dup is not None else None)


DUP_LO, DUP_HI = 3, 11


def dup_factors(d):
    return (0, d.D - 1)


def plant_duplicate(d, W, q):
    """The duplicate-class case: in two factors class DUP_HI gets the W_2 row, the bias (raised, so that the pair wins
    often) and the draws of class DUP_LO.  Their ratios tie exactly; the first maximum, DUP_LO, must be the one sampled."""
    for f in dup_factors(d):
        lo, hi = f * d.C + DUP_LO, f * d.C + DUP_HI
        W["b_2"][lo] += 3.0
        W["W_2"][hi], W["b_2"][hi] = W["W_2"][lo], W["b_2"][lo]
        q[..., hi] = q[..., lo]


def duplicate_check(d, logits, sidx):
    """Bit-equal logits of the planted pair, and never the higher index sampled.  Returns how often the pair won."""
    won = 0
    for f in dup_factors(d):
        lo, hi = f * d.C + DUP_LO, f * d.C + DUP_HI
        assert torch.equal(logits[..., lo], logits[..., hi]), f"factor {f}: the logits of two identical classes differ in bits"
        assert not bool((sidx[..., f] == DUP_HI).any()), f"factor {f}: class {DUP_HI} sampled although class {DUP_LO} ties with it"
        won += int((sidx[..., f] == DUP_LO).sum())
    return won


# ---- observe forward ----------------------------------------------------------------------------------------------------

OBS_FWD_TENSORS = dict(feat=lambda d: d.Be + d.S, post_logits=lambda d: d.S, sv_s=lambda d: d.S, sv_x=lambda d: d.Be,
                       sv_gates=lambda d: 4 * d.Be, sv_q=lambda d: d.Hd)
OBS_BWD_TENSORS = dict(d_embed_pre=lambda d: d.Be, d_gi=lambda d: 3 * d.Be, d_gh=lambda d: 3 * d.Be, d_q1_pre=lambda d: d.Hd,
                       d_q2_out=lambda d: d.S)


def observe_fwd_layers(d: CDims, W, I, K, AL=HW, chain=False):
    """W, I float64; K: float64 tensors [T, B, width] named as in bd_observe_cat_fwd_args plus K["sidx"] [T, B, D] (long).
    K may lack sv_s (NULL).  chain: K["sidx"][t] is set from K["post_logits"][t] (fill_layers: the chained reference)."""
    for t in range(d.T):
        h_prev = K["feat"][t - 1][:, :d.Be] if t else I["init_belief"]
        s_prev = one_hot_rows(K["sidx"][t - 1], d.C) if t else I["init_state"]
        s = s_prev * I["nonterm"][t][:, None] if I.get("nonterm") is not None else s_prev
        if K.get("sv_s") is not None:
            yield "sv_s", t, ALL, s, 0.0 * s, 0.0
        pre, S = lin(torch.cat([s, I["actions"][t]], 1), W["W_e"], W["b_e"])
        yield "sv_x", t, ALL, elu64(pre), S, AL.act
        yield from R.gru_layers(W, K["sv_x"][t], h_prev, K, t, AL, d.Be)
        pre, S = lin(K["feat"][t][:, :d.Be], W["W_1"], W["b_1"], I["pre_emb"][t])
        yield "sv_q", t, ALL, elu64(pre), S, AL.act
        out, So = lin(K["sv_q"][t], W["W_2"], W["b_2"])
        yield "post_logits", t, ALL, out, So, 0.0
        if chain:
            K["sidx"][t] = first_max(K["post_logits"][t], I["q_post"][t], d.D, d.C)
        hot = one_hot_rows(K["sidx"][t], d.C)
        yield "feat", t, slice(d.Be, d.Be + d.S), hot, 0.0 * hot, 0.0


# ---- observe backward ---------------------------------------------------------------------------------------------------

def observe_bwd_layers(d: CDims, W, I, K, G, AL=HW):
    """I: forward inputs plus the forward's tensors the backward reads (feat, post_logits, sv_x, sv_gates, sv_q);
    G: dfeat / dpost_logits (None allowed); K: the five d_* tensors."""
    Be, S_ = d.Be, d.S
    Wes = W["W_e"][:, :S_]
    z0 = torch.zeros(d.B, S_, dtype=D64, device=Wes.device)
    dhc = Sdhc = torch.zeros(d.B, Be, dtype=D64, device=Wes.device)
    for t in reversed(range(d.T)):
        if t + 1 < d.T:
            de1 = K["d_embed_pre"][t + 1]
            ds, Sds = de1 @ Wes, de1.abs() @ Wes.abs()
            if I.get("nonterm") is not None:
                nt = I["nonterm"][t + 1][:, None]
                ds, Sds = ds * nt, Sds * nt.abs()
        else:
            ds, Sds = z0, z0
        dfs = G["dfeat"][t][:, Be:]
        g = ds + dfs
        v, Sv, Av = jacobian(I["post_logits"][t], g, Sds + dfs.abs() + g.abs(), 0.0, d.D, d.C)
        dpl = G["dpost_logits"][t] if G.get("dpost_logits") is not None else z0
        yield "d_q2_out", t, ALL, v + dpl, Sv + dpl.abs() + (v + dpl).abs(), Av
        yield ("d_q1_pre", t, ALL) + R.dgrad(K["d_q2_out"][t], W["W_2"], I["sv_q"][t], AL)
        dq = K["d_q1_pre"][t]
        dfh = G["dfeat"][t][:, :Be]
        dh = dq @ W["W_1"] + dhc + dfh
        Sdh = dq.abs() @ W["W_1"].abs() + Sdhc + dfh.abs() + dh.abs()
        hprev = I["feat"][t - 1][:, :Be] if t else I["init_belief"]
        gg = R.gate_grads(dh, Sdh, 0.0, I["sv_gates"][t], hprev, Be)
        for name, third in (("d_gi", "ni"), ("d_gh", "nh")):
            for i, k in enumerate(("r", "z", third)):
                yield name, t, slice(i * Be, (i + 1) * Be), gg[k][0], gg[k][1], 0.0
        yield ("d_embed_pre", t, ALL) + R.dgrad(K["d_gi"][t], W["W_ih"], I["sv_x"][t], AL)
        dgh, z = K["d_gh"][t], I["sv_gates"][t][:, Be:2 * Be]
        dhc = dh * z + dgh @ W["W_hh"]
        Sdhc = Sdh * z + (dh * z).abs() + dgh.abs() @ W["W_hh"].abs() + dhc.abs()


# ---- imagination --------------------------------------------------------------------------------------------------------

def img_fwd_tensors(d: CDims, discrete=False):
    if discrete:
        t = dict(feat=d.Be + d.S, prior_logits=d.S, action=d.A, sv_act_stats=d.A, entropy=1, sv_x=d.Be, sv_gates=4 * d.Be, sv_p=d.Hd)
        t.update({f"sv_actor{l}": d.Hd for l in range(4)})
        return t
    t = dict(feat=d.Be + d.S, prior_logits=d.S, action=d.A, sv_act_stats=4 * d.A, sv_x=d.Be, sv_gates=4 * d.Be, sv_p=d.Hd,
             sv_act_us=2 * d.A)
    t.update({f"sv_actor{l}": d.Hd for l in range(4)})
    return t


def imagine_fwd_layers(d: CDims, W, I, K, AL=HW, chain=False, discrete=False, sat=None):
    """bd_imagine_cat_forward with sv_act_stats given; tanh-Normal actor, or the Categorical one (discrete).  The start
    state is the dense I["start_feat"][:, Be:] (what start_sidx == NULL reads; with start_sidx the caller passes its
    one-hot image there)."""
    Be = d.Be
    for t in range(d.T):
        h_prev = K["feat"][t - 1][:, :Be] if t else I["start_feat"][:, :Be]
        s_prev = one_hot_rows(K["sidx"][t - 1], d.C) if t else I["start_feat"][:, Be:]
        if discrete:
            yield from discrete_actor_layers(d, W, torch.cat([h_prev, s_prev], 1), I, K, t, AL, chain, sat)
        else:
            yield from R.actor_layers(d, W, torch.cat([h_prev, s_prev], 1), I, K, t, AL)
        pre, S = lin(torch.cat([s_prev, K["action"][t]], 1), W["W_e"], W["b_e"])
        yield "sv_x", t, ALL, elu64(pre), S, AL.act
        yield from R.gru_layers(W, K["sv_x"][t], h_prev, K, t, AL, Be)
        pre, S = lin(K["feat"][t][:, :Be], W["W_1"], W["b_1"])
        yield "sv_p", t, ALL, elu64(pre), S, AL.act
        out, So = lin(K["sv_p"][t], W["W_2"], W["b_2"])
        yield "prior_logits", t, ALL, out, So, 0.0
        if chain:
            K["sidx"][t] = first_max(K["prior_logits"][t], I["q_prior"][t], d.D, d.C)
        hot = one_hot_rows(K["sidx"][t], d.C)
        yield "feat", t, slice(Be, Be + d.S), hot, 0.0 * hot, 0.0


def imagine_bwd_layers(d: CDims, W, I, K, G, dentropy, AL=HW, actor_pre=True, discrete=False, sat=None):
    """scan_ref.imagine_bwd_layers with the Categorical prior head: I additionally holds prior_logits.  discrete: the
    Categorical actor (sv_act_stats = norm [.. x A], d_actor_out [.. x A]; d_actor_pre0..3 as the caller's bd_mlp_backward
    writes them from d_actor_out).  sat: the saturated rows (scan_ref.discrete_actor_layers)."""
    def head(t, dm, Sdm, Adm):
        return R._mm(*jacobian(I["prior_logits"][t], dm, Sdm, Adm, d.D, d.C), W["W_2"])
    tail = discrete_actor_tail(d, I, K, G, dentropy, sat) if discrete else None
    yield from R.imagine_bwd_layers(d, W, I, K, G, dentropy, 0.0, AL, actor_pre, head=head, actor_tail=tail)


def empty_set(widths, d: CDims, device="cpu"):
    K = R.empty_set(widths, d, device)
    K["sidx"] = torch.zeros(d.T, d.B, d.D, dtype=torch.long, device=device)
    return K


# ---- host dispatch, restated (bd_categorical.h CatGeo / CatFull, scan_cat.hip, observe_cat_cluster.hip) -------------------

K_CAT_OWN_BLOCKS, K_CUS = 8, 256
K_WAVES, K_FRAG, K_MAX_LDS, K_MAX_CLUSTER, K_LOCAL_BLOCKS = R.K_WAVES, R.K_FRAG, R.K_MAX_LDS, R.K_MAX_CLUSTER, R.K_LOCAL_BLOCKS
K_SPLIT_SCRATCH, K_HEAD_MAX_N = R.K_SPLIT_SCRATCH, R.K_HEAD_MAX_N
Geo = namedtuple("Geo", "S CW NCH nF ld image ok")


def cat_geo(D: int, C: int) -> Geo:
    S = D * C
    CW, NCH, nF = (cdiv(S, 16) * 16, 1, D) if S <= 256 else (256, cdiv(S, 256), 256 // max(C, 1))
    ok = 1 <= C <= 256 and D >= 1 and (S <= 256 or (256 % C == 0 and S % 16 == 0))
    return Geo(S, CW, NCH, nF, CW + 8, 16 * (CW + 8), ok)


def full_image(D: int, C: int) -> int:
    return 16 * (cdiv(D * C, 16) * 16 + 8)


def hd_ok(Hd: int) -> bool:
    return Hd <= 16 * 2 * K_WAVES and Hd <= 256


def pick_cat_cluster(B, Be, D, C, max_wgs) -> int:
    Nb, tiles = cdiv(Be, 16), cdiv(B, 16)
    max_wgs = min(max_wgs, 256)
    Cm = K_MAX_CLUSTER
    while Cm >= 4:
        ncols = (D // Cm) * C
        if (D % Cm == 0 and ncols % 16 == 0 and ncols // 16 <= K_CAT_OWN_BLOCKS and ncols // 16 <= K_WAVES and
                Nb <= K_LOCAL_BLOCKS * Cm and tiles * Cm <= max_wgs):
            return Cm
        Cm >>= 1
    return 0


def cluster_ok(B, Be, D, C, Hd, Cm) -> bool:
    """The BD_CATC_GEO conditions of the cluster launchers."""
    if not (D > 0 and C > 0 and cat_geo(D, C).ok and hd_ok(Hd)):
        return False
    if not (2 <= Cm <= K_MAX_CLUSTER and D % Cm == 0):
        return False
    ncols = (D // Cm) * C
    return (ncols % 16 == 0 and ncols // 16 <= K_CAT_OWN_BLOCKS and ncols // 16 <= K_WAVES and
            cdiv(Be, 16) <= K_LOCAL_BLOCKS * Cm and cdiv(B, 16) * Cm <= 256)


def cluster_sizes(B, Be, D, C, Hd):
    """Every cluster size the launchers accept for the shape, the default (bd_observe_cat_cluster_size, 256 workgroups)
    first, then D / 8 and D / 16 factor groups where also valid (the explicit sizes of the GPU test)."""
    ok = lambda Cm: (cluster_ok(B, Be, D, C, Hd, Cm) and
                     max(lds_bytes(e, Be, D, C, 1, Hd, Cm) for e in ("cluster_fwd", "cluster_bwd")) <= K_MAX_LDS)
    first = pick_cat_cluster(B, Be, D, C, 256)
    out = [first] if first and ok(first) else []
    return out + [Cm for Cm in (16, 8, 4) if Cm not in out and ok(Cm)]


def cluster_ws_floats(B, Be, Hd, D, Cm) -> int:
    tiles = cdiv(B, 16)
    nh, nhd = cdiv(Be, 16) * K_FRAG, cdiv(Hd, 16) * K_FRAG
    return tiles * K_MAX_CLUSTER + 16 + tiles * max(2 * nh + 2 * 16 * D, 2 * (2 * nh) + 2 * Cm * nhd)


def cat_scratch(nbl: int, fwd: bool) -> int:
    return max(K_WAVES * K_LOCAL_BLOCKS * (4 if fwd else 2) * 64 * 4, K_WAVES * nbl * 64 * 4, K_SPLIT_SCRATCH)


def lds_bytes(entry: str, Be, D, C, A, Hd, Cm: int = 0) -> int:
    """Dynamic LDS every entry point asks for (before cat_grid / launch_lds round it up).  The CPU test holds it to the
    library at every table shape through bd_scan_lds_bytes, and through the figure in the "needs N B of LDS" error of shapes
    above 160 KiB.  `cat_grid` below has no such tie: the library exports no query for its launch grid (which also follows
    BD_CAT_TILE_LOOP), so the "grid is 129" assertions check this restatement of the host code, not the launch."""
    h, a, hd, g = cdiv(Be, 16), cdiv(A, 16), cdiv(Hd, 16), cat_geo(D, C)
    if entry == "observe_fwd":
        n = (3 * h + hd + a) * K_FRAG + 16 * Be + full_image(D, C) + 2 * 16 * D + 16
    elif entry == "observe_bwd":
        n = (6 * h + hd + g.CW // 16) * K_FRAG + 2 * g.image + 16
    elif entry == "cluster_fwd":
        n = ((3 * h + hd + a) * K_FRAG + 16 * Be + full_image(D // Cm, C) + 2 * 16 * D + 16 +
             cat_scratch((D // Cm) * C // 16, True))
    elif entry == "cluster_bwd":
        n = ((6 * h + hd + (D // Cm) * C // 16) * K_FRAG + 2 * cat_geo(D // Cm, C).image + 16 +
             cat_scratch((D // Cm) * C // 16, False))
    elif entry == "imagine_fwd":
        uni = max(K_SPLIT_SCRATCH, K_WAVES * 16 * A * 3, full_image(D, C))
        n = (3 * h + 2 * hd + a) * K_FRAG + 16 * max(Be, Hd) + 3 * 16 * A + 2 * 16 * D + uni
    elif entry == "imagine_bwd":
        uni = max(2 * g.image + (g.CW // 16) * K_FRAG, K_SPLIT_SCRATCH, 2 * hd * K_FRAG)
        n = (6 * h + hd + 2 * a) * K_FRAG + uni
    else:
        raise ValueError(entry)
    return 4 * n


def cat_grid(N: int) -> int:
    """Workgroups of an imagination launch: one per tile up to 256 tiles, whole rounds above."""
    tiles = cdiv(N, 16)
    return tiles if tiles <= K_CUS else cdiv(tiles, cdiv(tiles, K_CUS))


def paths(D: int, C: int, Be: int, Hd: int):
    """What the shape takes: (backward chunks, 'partial' / 'full' last chunk, sampler and Jacobian path, staging and
    one-hot form, gather form of the embed layer, gather remainder D % 8)."""
    g = cat_geo(D, C)
    last = g.S - (g.NCH - 1) * g.CW
    vec = C % 4 == 0 and g.S % 4 == 0 and last % 4 == 0          # cat_stage / write_onehot: 16-byte accesses
    return dict(chunks=g.NCH, last="partial" if (g.NCH > 1 and last < g.CW) else "full", math="quad32" if C == 32 else "generic",
                staging="vec" if vec else "scalar", gather="vec" if Be % 4 == 0 else "scalar", rem=D % 8)


def accepts(D, C, Hd) -> bool:
    return D > 0 and C > 0 and cat_geo(D, C).ok and hd_ok(Hd)


# ---- the GPU shape tables (the CPU tests assert every column through the mirror) -------------------------------------------
# name -> (T, B, Be, D, C, A, Hd), default cluster size, backward chunks, last chunk, math path, staging, gather, D % 8
_BASE = dict(Be=40, D=4, C=16, A=3, Hd=32)      # 4 x 16 latents: the base of the row / time edge variants


def _edge(T, B):
    return CDims(T, B, **_BASE)


OBSERVE_SHAPES = {
    "c32_d32": (CDims(3, 18, 64, 32, 32, 3, 48), 16, 4, "full", "quad32", "vec", "vec", 0),
    "c32_d12": (CDims(2, 17, 40, 12, 32, 3, 32), 4, 2, "partial", "quad32", "vec", "vec", 4),
    "c32_d3": (CDims(2, 5, 40, 3, 32, 2, 20), 0, 1, "full", "quad32", "vec", "vec", 3),
    "c16_d20": (CDims(3, 19, 42, 20, 16, 3, 30), 4, 2, "partial", "generic", "vec", "scalar", 4),
    "c64_d16": (CDims(2, 16, 48, 16, 64, 3, 32), 16, 4, "full", "generic", "vec", "vec", 0),
    "c256_d2": (CDims(2, 16, 32, 2, 256, 1, 16), 0, 2, "full", "generic", "vec", "vec", 2),
    "c2_d136": (CDims(2, 9, 32, 136, 2, 2, 16), 0, 2, "partial", "generic", "scalar", "vec", 0),
    "c5_d3": (CDims(5, 3, 24, 3, 5, 2, 20), 0, 1, "full", "generic", "scalar", "vec", 3),
    "c9_d7": (CDims(2, 20, 40, 7, 9, 3, 32), 0, 1, "full", "generic", "scalar", "vec", 7),
    "c1_d16": (CDims(2, 4, 24, 16, 1, 2, 16), 0, 1, "full", "generic", "scalar", "vec", 0),
    # S = 272: the last chunk holds ONE factor (16 columns); accepted, since 272 is a multiple of 16
    "c16_d17": (CDims(2, 17, 40, 17, 16, 3, 32), 0, 2, "partial", "generic", "vec", "vec", 1),
    "b1": (_edge(2, 1), 4, 1, "full", "generic", "vec", "vec", 4),
    "b16": (_edge(2, 16), 4, 1, "full", "generic", "vec", "vec", 4),
    "b33": (_edge(2, 33), 4, 1, "full", "generic", "vec", "vec", 4),
    "t1": (_edge(1, 17), 4, 1, "full", "generic", "vec", "vec", 4),
    "t7": (_edge(7, 17), 4, 1, "full", "generic", "vec", "vec", 4),
    "hd256": (CDims(2, 16, 48, 8, 32, 3, 256), 8, 1, "full", "quad32", "vec", "vec", 0),
    "full_width": (CDims(2, 40, 200, 32, 32, 6, 200), 16, 4, "full", "quad32", "vec", "vec", 0),
}
# (nonterm, init_state, dpost_logits), cycled over the shape table; the CPU test asserts that every value occurs with a
# cluster shape and with a generic-path shape
VARIANTS = (("zeros", "mixed", True), ("none", "onehot", False), ("ones", "zeros", True), ("zeros", "onehot", False),
            ("none", "mixed", True))


def observe_variant(name):
    return VARIANTS[list(OBSERVE_SHAPES).index(name) % len(VARIANTS)]


# (Hm, N, Be, D, C, A, Hd)
IMAGINE_SHAPES = {
    "n1_h1": CDims(1, 1, **_BASE),
    "n17_h14": CDims(14, 17, 40, 4, 16, 6, 32),
    "c32_d32_a17": CDims(2, 17, 64, 32, 32, 17, 48),
    "c32_d12": CDims(2, 17, 40, 12, 32, 3, 32),
    "c16_d20": CDims(3, 19, 42, 20, 16, 3, 30),
    "c5_d3": CDims(5, 3, 24, 3, 5, 2, 20),
    "c256_d2": CDims(2, 16, 32, 2, 256, 1, 16),
    "tile_loop": CDims(2, 4112, 32, 4, 8, 2, 32),
    "discrete": CDims(3, 19, 40, 4, 16, 5, 32),      # discrete_actions = 1: the Categorical actor on A = 5 classes
    # the smallest shape at which the entropy partial sums [8 waves][16][A][3] decide the size of the forward scan's shared LDS
    # region: 10752 floats against 10240 of split-K scratch and 1152 of logit image
    "a28": CDims(2, 17, 24, 4, 16, 28, 32),
}
# the Categorical actor (scan_ref.DISCRETE_SHAPES, read its comment): the A edges, one row with one class, and the tile
# loop of cat_grid (257 tiles on 129 workgroups, as "tile_loop") with a second column block of actor logits
DISCRETE_SHAPES = {
    **{f"a{A}": CDims(3, 19, 40, 4, 16, A, 32) for A in (2, 16, 17, 33, 64)},
    "n1_a1": CDims(1, 1, 40, 4, 16, 1, 32),
    "tile_loop_a17": CDims(2, 4112, 32, 4, 8, 17, 32),
}
# dynamic LDS above 64 KiB: entry point -> shape names on the far side (every other shape of the table is below)
OBSERVE_BIG_LDS = {"observe_fwd": {"c32_d32", "c64_d16", "full_width"},
                   "observe_bwd": {"c32_d32", "c32_d12", "c16_d20", "c64_d16", "c16_d17", "hd256", "full_width"}}
# (tile_loop asks for the CU's whole LDS whatever its formula says: cat_grid keeps two of its workgroups off one CU)
IMAGINE_BIG_LDS = {"imagine_fwd": {"c32_d32_a17"}, "imagine_bwd": {"c32_d32_a17", "c32_d12", "c16_d20"}}
SEEDS = R.SEEDS           # the GPU tests' seeds: the CPU test asserts the ambiguous share of each on the float64 reference
