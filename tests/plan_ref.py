"""Float64 references, one step at a time, for the CEM planner kernels of csrc/planner.hip: the rollout
plan_rollout_kernel<LC> (bd_plan_rollout, bd_plan_rollout_cat) and the refit cem_refit_kernel (bd_cem_refit).  Plain helpers
like scan_ref.py / scan_cat_ref.py (read their docstrings first): the CPU tests run them on CPU tensors, the GPU tests on
device tensors.  C_TOL, the activation allowances, `lin`, `check_layers` / `fill_layers`, the sampler margin and the
host-side constants are THEIRS; nothing is restated here.

Method.  The rollout is launched with `feat` (and `sidx`) given, so every step's [h'; s'] is an output, and nothing compares
a whole sequence: each quantity of step t is recomputed in float64 FROM THE KERNEL'S OWN OUTPUTS OF THE STEP BEFORE
(`feat[t-1]`, `sidx[t-1]`; `init_*` expanded per environment at t = 0; row = b * cand + c belongs to environment b) and held
to |got - ref| <= C_TOL * S + A.  `returns` is checked against the kernel's own `feat` of the same launch: one launch with
`feat` and `returns` both given writes the bits of the two single-output launches (asserted by the GPU tests), so the
`feat` it shows is the recurrence its returns were summed over.

Composition.  The planner saves no intermediate (x, the gates, the prior hidden layer, the reward model's activations), so
gru_layers / head_layers of scan_ref.py, which read the kernel's saved gates and std, do not apply; their rules are
composed instead, as scan_ref._mm and imagine_bwd_layers do for the backward carries.  A quantity is a triple
(value, S, A): |kernel - value| <= C_TOL * S + A to first order.  An exact input (a kernel output, a caller's tensor) is
(v, 0, 0).
- contraction y = x W^T + b of a triple x:  S_y = S_x |W|^T + |x| |W|^T + |b|  (what x inherited, plus this layer's own
  sum of absolute products),  A_y = A_x |W|^T.
- ELU: f' = 1 (pre > 0) or e^pre <= 1:  S f', A f' + ACT_ALLOW.
- sigmoid v: v (1 - v) S + v, v (1 - v) A + SIGMOID_ALLOW;  tanh n: (1 - n^2) S + |n|, (1 - n^2) A + TANH_ALLOW.
- candidate pre-activation gi_n + r gh_n: S_gi + S_r |gh_n| + r S_gh + |r gh_n| + |pre| (the product and the sum round),
  A_gi + A_r |gh_n|.
- h' = (1 - z) n + z h:  S_z (|n| + |h|) + (1 - z) S_n + |(1 - z) n| + |z h| + |n| + |h'|  (1 - z rounds absolutely, hence
  |n|),  A_z (|n| + |h|) + (1 - z) A_n.
- std = softplus(raw) + min_std: sigmoid(raw) S_raw + std, sigmoid(raw) A_raw + SOFTPLUS_ALLOW;
  s' = mean + std eps: S_mean + S_std |eps| + |std eps| + |s'|, A_mean + A_std |eps|.
- actions = act_mean + act_std eps: S = |mean| + |std eps|, A = 0: one rounding (fused) or two (not) of terms each below S.
- returns: the five-layer chain of the reward model from the kernel's feat[t] by the first two rules (dense_ref.py has the
  single-layer rule only), then the sum over t in step order: S = sum_t S_t + sum_t |partial sum after step t|,
  A = sum_t A_t.
The decisions (ELU at 0, softplus at 20) are continuous to far below the bound (scan_ref.py, "Decisions"): no element is
left out.

Categorical latents.  The state is D class indices; `feat[t][:, Be:]` must equal one_hot(sidx[t]) EXACTLY.  The state that
enters step t + 1 is one_hot(sidx[t]) (weight 1 whatever the start weights were); at t = 0 it is the caller's `init_state`,
all-zero or a scaled one-hot per factor, which as a dense vector IS index times stored weight (the state_to_indices rule),
so the float64 embed layer reads it densely.  The logits are not an output: they are recomputed from the kernel's h'[t]
through the prior hidden layer (triple rules above), which gives every class an absolute bound b_c = C_TOL S_c + A_c on
the kernel's fp32 logit.  The ratio r_c = softmax(l)_c / q_c moves by the relative amount b_c with its logit (the
normaliser is shared by the classes of a factor and drops out of the comparison), so the kernel's class k must satisfy
    r_k >= (1 - m - b_k - b_*) max_c r_c,     m = scan_cat_ref.sample_margin(|d_k|, |d_*|)   (* = the float64 winner),
with the first maximum winning on exact ties (planted duplicates: bit-equal logits and draws, b = 0 between them).  A
factor with ANY second class inside its own such margin is AMBIGUOUS: the kernel may pick any class inside; every other
draw is thereby compared exactly.  An ambiguous draw never reaches a later comparison, since step t + 1 is fed the
kernel's own sidx[t].  Cap, a condition and not a measurement: at most 1e-3 of a case's draws may be ambiguous; the
relative margin of one draw is uniform on (0, 1) (planner_cat_oracle.MIN_GAP), so the expected share is about m + 2 b,
around 1e-5.  The CPU test asserts the share on the float64 reference for every case and seed of the tables below.

Refit.  Selection is exact: the kernel's return is r = 0.f + x_0 + x_1 + ... in step order, adds only, which numpy float32
reproduces bit for bit (the sum starts from +0, so r is never -0); the selection is the first `top` of the order "NaN
first, then descending return, then ascending index" (-0 = +0).  No tolerance on which candidates are chosen: the kernel
shows its selection only through the statistics, and a wrong candidate moves them by O(spread / top).
Statistics over the n = top selected values x_j, u = 2^-24, L = ceil(n / 64), the kernel's two-pass form:
- m^ = fl(fl(sum) * fl(1 / n)): each lane sums <= L values in sequence, six shuffle levels follow, then the product:
  |m^ - m| <= dm = (L + 8) u mean|x|.
- v^ = fl(sum_j fl(fl(x_j - m^)^2)) * fl(1 / n).  sum_j (x_j - m^)^2 / n = v + (m^ - m)^2 EXACTLY (sum_j (x_j - m) = 0): the
  variance inherits the shift term dm^2 and nothing of the offset's magnitude (a one-pass E[x^2] - m^2 would inherit
  u mean(x^2)).  The difference rounds once, relatively (u); square, lane sum, tree, product and the square root's own
  rounding (2u on std = 4u on v): |v^ - v| <= dv = (L + 15) u (v + dm^2) + dm^2.
- std^ = sqrt(v^): |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= sqrt(|a - b|), so the bound is
  min(dv / (2 std), sqrt(dv)); std = 0 (all selected equal) is held to sqrt(dv).
- top = 1: the sum is 0 + x, inv = 1, m^ = x, every difference 0: std^ = 0 EXACTLY (asserted).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.dense_ref import C_TOL, elu64
from tests.scan_ref import ALL, D64, HW, U, cdiv, f32, lin

AMBIGUOUS_CAP = 1e-3

_PD = namedtuple("PDims", "H B cand Be S A Hd")
_PCD = namedtuple("PCDims", "H B cand Be D C A Hd")


class PDims(_PD):
    __slots__ = ()
    cat = False

    @property
    def rows(self):
        return self.B * self.cand


class PCDims(_PCD):
    __slots__ = ()
    cat = True

    @property
    def rows(self):
        return self.B * self.cand

    @property
    def S(self):
        return self.D * self.C


# ---- parameters, inputs -------------------------------------------------------------------------------------------------

def synth_dims(d):
    """The engine's Dims of a planner case (batch, chunk, embedding and observation sizes as small as they go)."""
    from big_dreamer_amd import synth
    kw = dict(cat_D=d.D, cat_C=d.C) if d.cat else {}
    return synth.Dims(B=2, L=3, H=3, Be=d.Be, S=d.S, Hd=d.Hd, E=8, A=d.A, O=3, **kw)


def make_params(d, seed: int, bias_high: bool = False, logit_gain: float = 1.0):
    """synth.make_params at the case's dims.  bias_high: the prior logits' bias raised on the upper half of the classes
    (C = 256: sampled indices that do not fit a signed byte), the last class three more (index 255 occurs).  Categorical latents: the logit layer is scaled by
    `logit_gain` so that the classes are not near-uniform."""
    from big_dreamer_amd import synth
    P = synth.make_params(synth_dims(d), seed)
    tm = P["transition_model"]
    if d.cat:
        tm["belief_prior.model.2.weight"] *= np.float32(logit_gain)
        if bias_high:
            tm["belief_prior.model.2.bias"].reshape(d.D, d.C)[:, d.C // 2:] += np.float32(6.0)
            tm["belief_prior.model.2.bias"].reshape(d.D, d.C)[:, d.C - 1] += np.float32(3.0)      # and the last class often
    return P


def weights_of(P, device="cpu"):
    """The planner's weights out of a synth / state_dict parameter set, named as scan_ref.make_weights names them, plus the
    reward model's five layers W_r / b_r.  fp32 tensors."""
    t = lambda x: torch.as_tensor(np.asarray(x)).to(device)
    tm, rm = P["transition_model"], P["reward_model"]
    return dict(W_e=t(tm["fc_embed_state_action.0.weight"]), b_e=t(tm["fc_embed_state_action.0.bias"]),
                W_ih=t(tm["rnn.weight_ih"]), W_hh=t(tm["rnn.weight_hh"]), b_ih=t(tm["rnn.bias_ih"]), b_hh=t(tm["rnn.bias_hh"]),
                W_1=t(tm["belief_prior.model.0.weight"]), b_1=t(tm["belief_prior.model.0.bias"]),
                W_2=t(tm["belief_prior.model.2.weight"]), b_2=t(tm["belief_prior.model.2.bias"]),
                W_r=[t(rm[f"model.{2 * l}.weight"]) for l in range(5)], b_r=[t(rm[f"model.{2 * l}.bias"]) for l in range(5)])


START_KINDS = ("zeros", "onehot", "half", "mix")


def start_state(D, C, kind, g):
    """One environment's [S] start state: per factor all-zero, exact one-hot, one-hot scaled by 0.5, or ('mix') the three
    in turn over the factors."""
    hot = RC.one_hot_rows(torch.randint(0, C, (1, D), generator=g), C).float().view(D, C)
    scale = {"zeros": [0.0], "onehot": [1.0], "half": [0.5], "mix": [1.0, 0.0, 0.5]}[kind]
    for f in range(D):
        hot[f] *= scale[f % len(scale)]
    return hot.reshape(-1)


def make_inputs(d, seed: int, device="cpu", kinds=None):
    """Random non-trivial action belief, distinct start belief / state per environment, explicit draws.  Categorical
    latents: environment b starts from kind kinds[b % len(kinds)] (default: START_KINDS rotated by the seed)."""
    g = torch.Generator().manual_seed(seed + 6000)
    r = lambda *s: torch.randn(*s, generator=g)
    I = dict(init_belief=torch.tanh(r(d.B, d.Be)), act_mean=0.3 * r(d.H, d.B, d.A),
             act_std=0.2 + torch.rand(d.H, d.B, d.A, generator=g), eps_action=r(d.H, d.rows, d.A))
    if d.cat:
        kinds = kinds or tuple(START_KINDS[(seed + i) % 4] for i in range(4))
        I["init_state"] = torch.stack([start_state(d.D, d.C, kinds[b % len(kinds)], g) for b in range(d.B)])
        I["eps_state"] = RC.exp1(g, d.H, d.rows, d.S)
    else:
        I["init_state"] = r(d.B, d.S)
        I["eps_state"] = r(d.H, d.rows, d.S)
    return {k: v.to(device) for k, v in I.items()}


def plant_duplicate(d, P, q):
    """scan_cat_ref.plant_duplicate on a parameter set: class DUP_HI of two factors gets the logit row, the (raised) bias and
    the draws of class DUP_LO."""
    tm = P["transition_model"]
    W = dict(W_2=torch.from_numpy(tm["belief_prior.model.2.weight"]), b_2=torch.from_numpy(tm["belief_prior.model.2.bias"]))
    RC.plant_duplicate(d, W, q)


def empty_set(d, device="cpu"):
    K = dict(actions=torch.zeros(d.H, d.rows, d.A, dtype=D64, device=device),
             feat=torch.zeros(d.H, d.rows, d.Be + d.S, dtype=D64, device=device),
             returns=torch.zeros(1, d.rows, 1, dtype=D64, device=device))
    if d.cat:
        K["sidx"] = torch.zeros(d.H, d.rows, d.D, dtype=torch.long, device=device)
    return K


# ---- triples ------------------------------------------------------------------------------------------------------------

def _exact(v):
    z = torch.zeros_like(v)
    return v, z, z


def _lin3(x, W, b=None):
    """Contraction of a triple."""
    v, S, A = x
    Wa = W.abs().t()
    y, Sown = lin(v, W, b)
    return y, S @ Wa + Sown, A @ Wa


def _elu3(p, AL):
    pre, S, A = p
    f = torch.where(pre > 0, torch.ones_like(pre), torch.exp(pre))
    return elu64(pre), S * f, A * f + AL.act


def _sigmoid3(p, AL):
    pre, S, A = p
    v = torch.sigmoid(pre)
    return v, v * (1 - v) * S + v, v * (1 - v) * A + AL.sigmoid


def belief_step(d, W, s_prev, a, h_prev, AL=HW):
    """h' of one step as a triple from exact s_prev (dense), a, h_prev: embed + ELU -> GRU cell."""
    Be = d.Be
    x = _elu3(_lin3(_exact(torch.cat([s_prev, a], 1)), W["W_e"], W["b_e"]), AL)
    gi = _lin3(x, W["W_ih"], W["b_ih"])
    gh = _lin3(_exact(h_prev), W["W_hh"], W["b_hh"])
    sl = lambda tr, i: tuple(c[:, i * Be:(i + 1) * Be] for c in tr)
    add = lambda p, q: tuple(u + v for u, v in zip(p, q))
    r, z = _sigmoid3(add(sl(gi, 0), sl(gh, 0)), AL), _sigmoid3(add(sl(gi, 1), sl(gh, 1)), AL)
    gin, ghn = sl(gi, 2), sl(gh, 2)
    pre = gin[0] + r[0] * ghn[0]
    Sp = gin[1] + r[1] * ghn[0].abs() + r[0] * ghn[1] + (r[0] * ghn[0]).abs() + pre.abs()
    Ap = gin[2] + r[2] * ghn[0].abs()
    n = torch.tanh(pre)
    Sn, An = (1 - n * n) * Sp + n.abs(), (1 - n * n) * Ap + AL.tanh
    hn = (1 - z[0]) * n + z[0] * h_prev
    mag = n.abs() + h_prev.abs()
    Sh = z[1] * mag + (1 - z[0]) * Sn + ((1 - z[0]) * n).abs() + (z[0] * h_prev).abs() + n.abs() + hn.abs()
    return hn, Sh, z[2] * mag + (1 - z[0]) * An


def prior_out(W, h, AL=HW):
    """The prior head's output layer (mean | raw, or the logits) as a triple from the exact h'."""
    return _lin3(_elu3(_lin3(_exact(h), W["W_1"], W["b_1"]), AL), W["W_2"], W["b_2"])


def gauss_state(d, W, h, eps, ms, AL=HW):
    out = prior_out(W, h, AL)
    S_ = d.S
    mean, Sm, Am = (c[:, :S_] for c in out)
    raw, Sr, Ar = (c[:, S_:] for c in out)
    std = F.softplus(raw, beta=1, threshold=20) + ms
    sg = torch.sigmoid(raw)
    Sstd, Astd = sg * Sr + std, sg * Ar + AL.softplus
    s = mean + std * eps
    return s, Sm + Sstd * eps.abs() + (std * eps).abs() + s.abs(), Am + Astd * eps.abs()


def reward_chain(W, feat, AL=HW):
    """The reward model on exact [h'; s'] rows as a triple [rows x 1]."""
    y = _exact(feat)
    for l in range(4):
        y = _elu3(_lin3(y, W["W_r"][l], W["b_r"][l]), AL)
    return _lin3(y, W["W_r"][4], W["b_r"][4])


def _expand(x, cand):
    return x.repeat_interleave(cand, 0)


def rollout_layers(d, W, I, K, min_std=0.0, AL=HW, chain=False, min_std_f32=True):
    """W, I float64 (scan_ref.to64); K: float64 actions [H, rows, A], feat [H, rows, Be + S], returns [1, rows, 1] and -- Categorical
    latents -- sidx [H, rows, D] (long).  chain: K["sidx"][t] is set from the recomputed logits (fill_layers: the chained
    reference).  min_std is taken as the kernel receives it, a C float (min_std_f32 = False: as the float64 oracle adds it).
    Yields what check_layers / fill_layers take."""
    ms, Be = (f32(min_std) if min_std_f32 else min_std), d.Be
    for t in range(d.H):
        mean, std, eps = _expand(I["act_mean"][t], d.cand), _expand(I["act_std"][t], d.cand), I["eps_action"][t]
        yield "actions", t, ALL, mean + std * eps, mean.abs() + (std * eps).abs(), 0.0
        if t:
            h_prev = K["feat"][t - 1][:, :Be]
            s_prev = RC.one_hot_rows(K["sidx"][t - 1], d.C) if d.cat else K["feat"][t - 1][:, Be:]
        else:
            h_prev, s_prev = _expand(I["init_belief"], d.cand), _expand(I["init_state"], d.cand)
        h, Sh, Ah = belief_step(d, W, s_prev, K["actions"][t], h_prev, AL)
        yield "feat", t, slice(0, Be), h, Sh, Ah
        hk = K["feat"][t][:, :Be]
        if d.cat:
            if chain:
                K["sidx"][t] = RC.first_max(prior_out(W, hk, AL)[0], I["eps_state"][t], d.D, d.C)
            hot = RC.one_hot_rows(K["sidx"][t], d.C)
            yield "feat", t, slice(Be, Be + d.S), hot, 0.0 * hot, 0.0
        else:
            s, Ss, As = gauss_state(d, W, hk, I["eps_state"][t], ms, AL)
            yield "feat", t, slice(Be, Be + d.S), s, Ss, As
    total = S = A = part = 0.0
    for t in range(d.H):
        v, Sv, Av = reward_chain(W, K["feat"][t], AL)
        total, S, A = total + v, S + Sv, A + Av
        part = part + total.abs()
    yield "returns", 0, ALL, total, S + part, A


def split_feat(layers, K, Be):
    """The layers of rollout_layers with `feat` renamed 'h' (belief columns) and 's' (state columns), K given the two views:
    check_layers then reports h' and s' apart."""
    K["h"], K["s"] = K["feat"][..., :Be], K["feat"][..., Be:]
    for name, t, sl, ref, S, allow in layers:
        if name == "feat":
            name, sl = ("h", ALL) if sl.start == 0 else ("s", ALL)
        yield name, t, sl, ref, S, allow


def sample_checks(d, W, I, K, AL=HW, exact=False, tag=""):
    """Every draw of a Categorical rollout against the rule of the module docstring.  Returns (ambiguous draws, draws,
    draws whose class is >= 128)."""
    path = RC.sample_path(d.C, exact)
    amb = n = high = 0
    for t in range(d.H):
        l, Sl, Al = prior_out(W, K["feat"][t][:, :d.Be], AL)
        b = (C_TOL * Sl + Al).reshape(-1, d.D, d.C)
        r, dist = RC.ratios64(l, I["eps_state"][t], d.D, d.C)
        k = K["sidx"][t].long().reshape(-1, d.D, 1)
        assert int(k.min()) >= 0 and int(k.max()) < d.C, f"{tag}t={t}: class index outside [0, {d.C})"
        star = r.argmax(-1, keepdim=True)
        rs, ds, bs = r.gather(-1, star), dist.gather(-1, star), b.gather(-1, star)
        inside = r >= (1 - RC.sample_margin(dist, ds, d.C, path) - b - bs) * rs          # per class, against the winner
        l3, q3 = l.reshape(-1, d.D, d.C), I["eps_state"][t].reshape(-1, d.D, d.C)
        same = (l3 == l3.gather(-1, star)) & (q3 == q3.gather(-1, star))      # the winner and its bit-equal duplicates: an
        ambiguous = (inside & ~same).sum(-1) > 0                              # exact tie, and `star` is the first of them
        ok = torch.where(ambiguous.unsqueeze(-1), inside.gather(-1, k), k == star)
        if not bool(ok.all()):
            row, f, _ = (int(i) for i in (~ok).nonzero()[0])
            raise AssertionError(f"{tag}sample[t={t}, row={row}, factor={f}]: {int((~ok).sum())} of {ok.numel()} wrong; class "
                                 f"{int(k[row, f])} with ratio {float(r[row, f, int(k[row, f])]):.9e}, float64 winner "
                                 f"{int(star[row, f])} with {float(rs[row, f]):.9e}, ambiguous {bool(ambiguous[row, f])}")
        amb, n, high = amb + int(ambiguous.sum()), n + ambiguous.numel(), high + int((k >= 128).sum())
    return amb, n, high


# ---- refit --------------------------------------------------------------------------------------------------------------

def refit_returns(returns, B, cand):
    """[ret_steps x B*cand] -> [B x cand] as the kernel sums it: from +0, in step order, in the array's own precision."""
    ret = np.asarray(returns)
    r = np.zeros(B * cand, ret.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(ret.shape[0]):
            r = r + ret[t]
    return r.reshape(B, cand)


def refit_select(r, top):
    """[B x cand] returns -> [B x top] indices: NaN first, then descending return (-0 = +0), then ascending index."""
    B, cand = r.shape
    out = np.empty((B, top), np.int64)
    for b in range(B):
        nan = np.isnan(r[b])
        key = np.where(nan, 0.0, -r[b].astype(np.float64)) + 0.0
        out[b] = np.lexsort((np.arange(cand), key, ~nan))[:top]
    return out


def refit_ref(returns, actions, H, B, cand, top, A):
    """returns [ret_steps x B*cand] (numpy; float32 = the kernel's sum bit for bit), actions [H x B*cand x A] (torch).
    Returns (mean, std, bound of mean, bound of std), float64 [H x B x A], and the selection [B x top]."""
    sel = refit_select(refit_returns(returns, B, cand), top)
    idx = torch.as_tensor(sel + cand * np.arange(B)[:, None], device=actions.device)
    x = actions.double()[:, idx.reshape(-1)].reshape(H, B, top, A)
    m = x.mean(2)
    v = ((x - m.unsqueeze(2)) ** 2).mean(2)
    L = cdiv(top, 64)
    dm = (L + 8) * U * x.abs().mean(2)
    dv = (L + 15) * U * (v + dm * dm) + dm * dm
    std = v.sqrt()
    bs = torch.minimum(dv / (2 * std).clamp_min(1e-300), dv.sqrt())
    return m, std, dm, bs, sel


def check_refit(tag, mean, std, ref, top, report=None):
    m, s, bm, bs, _ = ref
    for name, got, want, bound in (("mean", mean.double(), m, bm), ("std", std.double(), s, bs)):
        err = (got - want).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            i = tuple(int(j) for j in bad.nonzero()[0])
            raise AssertionError(f"{tag} refit {name}{list(i)}: {int(bad.sum())} of {bad.numel()} out of tolerance; got "
                                 f"{float(got[i])!r}, ref {float(want[i])!r}, err {float(err[i]):.3e}, bound {float(bound[i]):.3e}")
        if report is not None:
            pos = bound > 0
            assert bool((err[~pos] == 0).all()), f"{tag} refit {name}: nonzero error where the bound is zero"
            if bool(pos.any()):
                report["refit_" + name] = max(report.get("refit_" + name, 0.0), float((err[pos] / bound[pos]).max()))
    if top == 1:
        assert bool((std == 0).all()), f"{tag}: top = 1 must give std = 0 exactly"


RETURN_PATTERNS = ("normal", "all_equal", "ties", "zeros", "nans_few", "nans_many", "infs", "inf_minus_inf")
ACTION_PATTERNS = ("normal", "offset", "identical")


def refit_inputs(H, B, cand, top, A, ret_steps, seed, returns="normal", actions="normal"):
    """numpy float32 returns [ret_steps x B*cand] and actions [H x B*cand x A] of one refit case."""
    rng = np.random.Generator(np.random.PCG64(seed + 8000))
    n = B * cand
    ret = rng.standard_normal((ret_steps, n), dtype=np.float32)
    if returns == "all_equal":
        ret[:] = np.float32(0.25)
    elif returns == "ties":                   # five values: blocks of ties, one of which straddles the cut
        ret = rng.integers(-2, 3, size=(ret_steps, n)).astype(np.float32)
    elif returns == "zeros":                  # +0 and -0 mixed, a few nonzero values below them
        ret = np.where(rng.random((ret_steps, n)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        ret[:, ::7] = np.float32(-1.0)
    elif returns in ("nans_few", "nans_many"):
        k = max(1, top // 3) if returns == "nans_few" else min(cand, top + 5)
        for b in range(B):
            ret[rng.integers(0, ret_steps, size=k), b * cand + rng.choice(cand, size=k, replace=False)] = np.nan
    elif returns == "infs":
        ret[0, 1::5], ret[0, 2::11] = np.inf, -np.inf
    elif returns == "inf_minus_inf":          # + inf and - inf in different steps of one candidate: its sum is NaN
        ret[0, 3::9], ret[-1, 3::9] = np.inf, -np.inf
        if ret_steps == 1:
            ret[0, 3::9] = np.nan
        ret[0, 4::13] = np.inf
    act = rng.standard_normal((H, n, A), dtype=np.float32)
    if actions == "offset":
        act = (np.float32(100.0) + np.float32(1e-3) * act).astype(np.float32)
    elif actions == "identical":
        act[:] = act[:, :1]
    return ret, act


# (H, B, cand, top, A): each with ret_steps 1 and H
REFIT_SHAPES = ((1, 1, 1, 1, 1), (3, 2, 2, 1, 2), (4, 2, 64, 64, 2), (5, 3, 257, 19, 17), (2, 1, 1024, 100, 3),
                (2, 1, 1025, 100, 3), (1, 1, 4096, 1024, 1), (2, 2, 4095, 1000, 1), (15, 1, 1000, 100, 1))
REFIT_MID = (5, 3, 257, 19, 17)          # the shape of the return / action patterns


def refit_cases():
    """(name, shape, ret_steps, returns pattern, actions pattern, seed)."""
    out = []
    for i, sh in enumerate(REFIT_SHAPES):
        for rs in sorted({1, sh[0]}):
            out.append((f"shape{i}_rs{rs}", sh, rs, "normal", "normal", 100 + i))
    for j, pat in enumerate(RETURN_PATTERNS[1:]):
        for rs in ((1, REFIT_MID[0]) if pat in ("zeros", "ties") else (1,) if pat == "all_equal" else (REFIT_MID[0],)):
            out.append((f"{pat}_rs{rs}", REFIT_MID, rs, pat, "normal", 200 + j))
    for j, pat in enumerate(ACTION_PATTERNS[1:]):
        out.append((f"act_{pat}", REFIT_MID, 1, "normal", pat, 300 + j))
        out.append((f"act_{pat}_top100", (2, 1, 1000, 100, 3), 2, "ties", pat, 310 + j))
    return out


# ---- host formulas, restated (PlanDims of csrc/planner.hip) ---------------------------------------------------------------

def lds_bytes(Be, S, A, Hd, D=0, C=0) -> int:
    """PlanDims::lds_floats * 4; D > 0: Categorical latents."""
    h, s, a, hd, f = cdiv(Be, 16), cdiv(S, 16), cdiv(A, 16), cdiv(Hd, 16), cdiv(Be + S, 16)
    if D > 0:
        n_state, n_uni = 16 * max(Be, Hd) + 2 * 16 * D, max(R.K_SPLIT_SCRATCH, RC.full_image(D, C))
    else:
        n_state, n_uni = (s + f) * R.K_FRAG, R.K_SPLIT_SCRATCH
    return 4 * ((3 * h + 2 * hd + a) * R.K_FRAG + n_state + 16 + n_uni)


def accepts(d) -> bool:
    if d.cat:
        return RC.cat_geo(d.D, d.C).ok and lds_bytes(d.Be, d.S, d.A, d.Hd, d.D, d.C) <= R.K_MAX_LDS
    return d.S <= R.K_HEAD_MAX_N and lds_bytes(d.Be, d.S, d.A, d.Hd) <= R.K_MAX_LDS


def dual_head_form(S: int) -> str:
    """tile_dual_head_elem: split-K up to kSplitPairs column blocks, column blocks above; the element tail loop runs when
    16 S exceeds the thread count."""
    return ("splitk" if cdiv(S, 16) <= 2 else "blocks") + ("+tail" if 16 * S > R.K_THREADS else "")


# ---- the GPU case tables (the CPU tests run the emulation and the ambiguous share on every entry) ----------------------------
# Gaussian latents: one axis swept at a time from the ragged base Be 24, S 6, Hd 20, A 2
def _g(H=2, B=2, cand=21, Be=24, S=6, A=2, Hd=20):
    return PDims(H, B, cand, Be, S, A, Hd)


GAUSS_CASES = {f"rows_{B}x{c}_h{H}": _g(H=H, B=B, cand=c)
               for B, c in ((1, 1), (1, 15), (1, 16), (1, 17), (3, 7), (2, 21), (3, 50)) for H in (1, 4)}
GAUSS_CASES.update({f"s{S}": _g(S=S) for S in (1, 16, 17, 32, 33, 48, 64)})
GAUSS_CASES.update({f"a{A}": _g(A=A) for A in (1, 16, 17, 33)})
GAUSS_CASES.update({f"be{Be}": _g(Be=Be) for Be in (16, 40, 193, 200, 208, 209)})
GAUSS_CASES["be200_hd200"] = _g(Be=200, Hd=200)
GAUSS_CASES.update({f"hd{Hd}": _g(Hd=Hd) for Hd in (8, 36, 72)})
GAUSS_CASES["ragged_be24_s30"] = _g(Be=24, S=30)
GAUSS_CASES["ragged_be40_s64"] = _g(Be=40, S=64)
# the widest belief PlanDims admits at the base widths: (3 * 28 + 4 + 1 + 1 + 29) * 256 + 16 + 10240 floats = 162 880 B;
# one more belief column makes 29 belief blocks and 165 952 B
GAUSS_WIDEST, GAUSS_TOO_WIDE = _g(Be=448), _g(Be=449)
GAUSS_CASES["widest"] = GAUSS_WIDEST
GAUSS_SEED = 31


def _c(D, C, H=3, B=2, cand=21, Be=40, A=3, Hd=32):
    return PCDims(H, B, cand, Be, D, C, A, Hd)


CAT_DC = ((3, 5), (1, 2), (4, 6), (4, 16), (16, 16), (32, 16), (4, 64), (2, 128), (1, 256), (32, 32))
CAT_CASES = {f"d{D}_c{C}": _c(D, C) for D, C in CAT_DC}
CAT_CASES["starts"] = _c(4, 16, B=4, cand=5)              # the four start kinds, several environments per tile
CAT_CASES["rows_3x7"] = _c(3, 5, B=3, cand=7)
CAT_CASES["hd_gt_be"] = _c(4, 6, Hd=48)
CAT_CASES["dup"] = _c(4, 16)                              # planted duplicate classes
CAT_SEEDS = (41, 42)
CAT_LOGIT_GAIN = 3.0


def cat_case(name, seed, device="cpu"):
    """(d, P, I) of a Categorical case: parameters (numpy, as the engine takes them) and fp32 inputs."""
    d = CAT_CASES[name]
    P = make_params(d, seed, bias_high=(d.C == 256), logit_gain=CAT_LOGIT_GAIN)
    I = make_inputs(d, seed, kinds=START_KINDS if name == "starts" else None)
    if name == "dup":
        plant_duplicate(d, P, I["eps_state"])
    return d, P, {k: v.to(device) for k, v in I.items()}


def gauss_case(name, device="cpu"):
    d = GAUSS_CASES[name]
    return d, make_params(d, GAUSS_SEED), make_inputs(d, GAUSS_SEED, device)
