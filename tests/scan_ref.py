"""Float64 references, one step and one layer at a time, for the Gaussian RSSM scan kernels: the observe scan in its three
forms (csrc/observe.hip, observe_cluster.hip, observe_ksplit.hip) and the imagination scan with the tanh-Normal actor
or the Categorical one (csrc/imagine.hip; the Categorical actor's restatement, csrc/bd_discrete.h, lives here for both
latent kinds: `discrete_actor_layers`, `discrete_actor_tail`, its variants `peaked` / `saturated` / duplicate classes in
`make_discrete_case`).  Plain helpers like dense_ref.py / reduce_ref.py: the CPU tests run them on CPU tensors, the GPU
tests on device tensors.

Method.  A recurrence amplifies rounding error, so nothing here compares a whole sequence.  Every layer of every step is
recomputed in float64 FROM THE KERNEL'S OWN TENSORS OF THE LAYER BEFORE (its saved activations, its outputs of the step
before, `init_*` at t = 0) and compared componentwise,

    |got - ref| <= C_TOL * S + allow,

with S the float64 contraction of the absolute operands (dense_ref.py) and `allow` the absolute allowance of the
activation that closes the layer.  A value f(pre) of a smooth activation inherits C_TOL * |f'(pre)| * S_pre from its
pre-activation and gets |f(pre)| added to S for its own rounding.  Each generator below yields
(tensor name, step, column slice, reference, S, allow); `check_layers` compares, `fill_layers` writes the reference
into the tensor set instead, which chains the per-step reference over the whole sequence (the CPU tests compare that
chain with the oracle and with autograd).

Backward carries.
- Observe, state carry: d loss / d state_t arrives as nonterm[t+1] * (d_embed_pre[t+1] W_e[:, :S]) and d_embed_pre is an
  output, so the carry into step t is recomputed from the kernel's own d_embed_pre[t+1] (teacher-forced): no growth.
- Observe, belief carry: dh[t] = d_q1_pre[t] W_q1h + dfeat_h[t] + dh[t+1] * z[t+1] + d_gh[t+1] W_hh.  dh is not an output.
  The W_hh term is taken from the kernel's d_gh[t+1]; dh[t+1] * z[t+1] is the reference's own float64 recursion.  Let
  e[t] = |dh_kernel[t] - dh_ref[t]|.  The kernel forms dh[t] from the same d_q1_pre[t], dfeat and d_gh[t+1] as the
  reference and from ITS dh[t+1], so e[t] <= z[t+1] * e[t+1] + (rounding of this step's sums and products)
  <= z[t+1] * e[t+1] + C_TOL * s[t], s[t] = |d_q1_pre| |W_q1h| + |dfeat_h| + |dh[t+1] z[t+1]| + |d_gh[t+1]| |W_hh| + |dh[t]|.
  Hence e[t] <= C_TOL * Sdh[t] with Sdh[t] = s[t] + z[t+1] * Sdh[t+1]: the magnitude runs through the same recurrence
  in absolute values, every carry factor z < 1.  With comparable s this is the `c * steps * S` of the lambda-return
  bound in reduce_ref.py, written per element.  The gate gradients are dh times factors built from saved numbers, so
  they inherit Sdh times the absolute factor; a factor of the form (1 - v) or (1 - v * v) is evaluated in fp32 with an
  ABSOLUTE error of about one unit roundoff, so the unfactored magnitude is added to S as well.
- Imagination: the world model is frozen, the only outputs are d_actor_out / d_actor_pre, so neither carry can be
  teacher-forced.  The reference recurses both in float64 and every carried quantity is a triple (value, S, A): S as
  above, pushed through |W| at every contraction, A the accumulated absolute allowances pushed the same way.  The bound
  therefore widens with the number of steps carried (it is exact-to-rounding at t = Hm - 1, where nothing is carried).
  d_actor_pre is off the recurrence and is checked layer by layer from the kernel's own d_actor_out.

Activation allowances (default build, bd_device.h:97-101; u = 2^-24).  The CDNA ISA states 1 ulp for v_exp_f32, v_rcp_f32
and v_log_f32, i.e. a relative error of at most 2u.  __expf(x) = v_exp_f32(x * log2 e): rounding the product perturbs
the exponent by u * |x| log2 e, i.e. the result by the relative amount u * |x|.  So E = __expf(x) has relative error
(|x| + 2) u.
- sigmoidf(x) = rcp(1 + E), E = exp(-x), s = 1 / (1 + E).  ds/dE = -s^2, so the error of E moves s by
  s (1 - s) (|x| + 2) u <= (0.224 + 0.5) u (max of |x| s (1 - s) is 0.224 at |x| = 1.54); rounding 1 + E moves it by
  at most s u <= u; rcp adds 2 u s <= 2u.  Total <= 3.73 u.  SIGMOID_ALLOW = 4u.
- tanh_act(x) = 1 - 2 rcp(E + 1), E = exp(2x), t = tanh x.  dt/dE = 2 / (E + 1)^2 and 2E / (E + 1)^2 = (1 - t^2) / 2, so
  the error of E moves t by (1 - t^2) / 2 * (2|x| + 2) u <= (0.45 + 1) u (max of |x| (1 - t^2) is 0.448); rounding E + 1:
  (1 - t^2) / 2 * u <= 0.5u; rcp: 2u * 2 / (E + 1) = 2u (1 - t) <= 4u; the product by 2 is exact; the final subtraction
  rounds by at most u.  Total <= 6.95 u.  TANH_ALLOW = 8u.
ACT_ALLOW (ELU, dense_ref.py) and SOFTPLUS_ALLOW (softplus and the 1 - exp(-x) sigmoid recovery, reduce_ref.py) are
reused.  A backward term that multiplies such a value gets allow * |g|.
-DBD_EXACT_MATH build (bd_device.h:89-95; ROCm's device libm states 1 ulp for expf, 2 ulp for expm1f, log1pf, tanhf;
fp32 division is correctly rounded): ELU and tanh <= 4u |y| <= 4u; sigmoid 1 / (1 + expf(-x)): s (1 - s) 2u + s u + s u
<= 2.5u -> 3u; softplus log1pf(expf(x)): the exp error moves it by at most 2u, log1pf by 4u * softplus, which the
C_TOL * S term (S contains std) covers -> 4u absolute; the recovery -expm1f(-x) <= 4u.

Decisions.  The ELU branch (x > 0) and softplus's x > 20 branch are taken in fp32.  Both functions are continuous with a
continuous first derivative across the branch point to far below the bound: |x - expm1(x)| <= x^2 / 2, which for a
pre-activation the two sides could disagree on (|x| <= C_TOL * S, S = O(1)) is O(1e-12); softplus(20) - 20 = 2.1e-9
against ulp(20) = 1.9e-6; ELU' through the saved output is y > 0 ? 1 : y + 1, continuous at y = 0.  So a differing
decision cannot produce an error above the bound and NO element is left out of any comparison (count 0 in every case).
`near_decision_fraction` reports the share of pre-activations within DECISION_MARGIN of a branch point; the CPU tests
confirm on the float64 reference that it is below 0.1 % for every case.
"""
from __future__ import annotations

from collections import namedtuple

import torch
import torch.nn.functional as F

from tests.dense_ref import ACT_ALLOW, C_TOL, elu64, elu_grad_from_out64
from tests.reduce_ref import SOFTPLUS_ALLOW, TINY, cat_probs_ref

U = 2.0 ** -24
SIGMOID_ALLOW = 4 * U      # derivation in the module docstring
TANH_ALLOW = 8 * U         # derivation in the module docstring
DECISION_MARGIN = 1e-6
D64 = torch.float64

Allow = namedtuple("Allow", "act softplus sigmoid tanh")
HW = Allow(ACT_ALLOW, SOFTPLUS_ALLOW, SIGMOID_ALLOW, TANH_ALLOW)
EXACT = Allow(4 * U, 4 * U, 3 * U, 4 * U)

ACT_RAW_INIT_STD = float(torch.log(torch.exp(torch.tensor(5.0)) - 1))
ACT_MIN_STD = 1e-4
ACT_MEAN_SCALE = 5.0
ALL = slice(None)


def f32(x: float) -> float:
    """A Python float as the kernel receives it (a C float argument)."""
    return float(torch.tensor(x, dtype=torch.float32))


def to64(d):
    return {k: (v.double() if torch.is_tensor(v) else
                [w.double() for w in v] if isinstance(v, (list, tuple)) else v) for k, v in d.items()}


# ---- shapes, parameters, inputs ----------------------------------------------------------------------------------------

Dims = namedtuple("Dims", "T B Be S A Hd")      # imagination: T = Hm, B = N


ACTOR_KINDS = (None, "regular", "peaked", "saturated")
PEAK_FACTOR = 10.0          # factor 30 reaches norm - max = -73, factor 60 leaves ratios64's domain (-80)
SAT_LEAD = 120.0            # expf(-104) is already 0 in fp32; 120 leaves room for the spread of the other logits
SAT_GATE, SAT_W = 100.0, 2.0


def sat_class(A: int) -> int:
    return A - 1


def sat_rows(B: int, device="cpu"):
    """The rows the `saturated` variant saturates: the even ones."""
    return torch.arange(B, device=device) % 2 == 0


def plant_saturated(d, W):
    """The weight side of the `saturated` variant of the Categorical actor.  A bias is shared by all rows, so raising
    b_a4[k] alone would saturate every row; the rows are told apart by a gate instead.  Belief unit 0 is carried
    unchanged through every step (its update gate is sigmoid(40) = 1 in fp32: h_0[t] = 0 * n + 1 * h_0[t-1]) and holds
    +0.9 on the even rows, -0.9 on the odd ones (make_imagine_inputs).  Actor unit 0 of every hidden layer reads only
    the gate: ELU(100 * h_0) = 90 on even rows, -1 on odd rows (exp(-90) is below half an ulp of 1), then ELU of the unit
    itself: 90 / ELU^3(-1) = -0.37.  Class k = A - 1 reads it with weight 2 and no other class reads it: on even rows
    class k leads every other logit by 180 minus their O(1) spread (`discrete_actor_layers` asserts >= SAT_LEAD on the
    float64 logits), on odd rows it moves by -0.75 and the row stays regular."""
    Be, k = d.Be, sat_class(d.A)
    W["W_ih"][Be], W["W_hh"][Be], W["b_ih"][Be], W["b_hh"][Be] = 0.0, 0.0, 40.0, 0.0
    W["W_a0"][0], W["b_a"][0][0] = 0.0, 0.0
    W["W_a0"][0, 0] = SAT_GATE
    for l in range(3):
        W["W_a"][l][0], W["W_a"][l][:, 0], W["b_a"][l + 1][0] = 0.0, 0.0, 0.0
        W["W_a"][l][0, 0] = 1.0
    W["W_a4"][:, 0] = 0.0
    W["W_a4"][k, 0] = SAT_W


def make_weights(d: Dims, seed: int, device="cpu", imagine: bool = False, actor=None):
    """Random fp32 parameters in the PyTorch (out, in) layout; fan-in scaling keeps pre-activations O(1).
    actor (the Categorical actor's variants): 'peaked' multiplies the A logit rows of W_a4 / b_a4 by PEAK_FACTOR (entropy
    mean 1.4 / 2.3 at A = 17 / 64 instead of ln A - 0.1); 'saturated': plant_saturated."""
    assert actor in ACTOR_KINDS, actor
    W = _make_weights(d, seed, imagine)
    if actor == "peaked":
        W["W_a4"][:d.A] *= PEAK_FACTOR
        W["b_a4"][:d.A] *= PEAK_FACTOR
    elif actor == "saturated":
        plant_saturated(d, W)
    return {k: ([w.to(device) for w in v] if isinstance(v, list) else v.to(device)) for k, v in W.items()}


def _make_weights(d: Dims, seed: int, imagine: bool):
    device = "cpu"
    g = torch.Generator().manual_seed(seed)

    def w(n, k, gain=1.0):
        return (torch.randn(n, k, generator=g) * (gain / k ** 0.5)).to(device)

    def b(n):
        return (torch.randn(n, generator=g) * 0.1).to(device)

    W = dict(W_e=w(d.Be, d.S + d.A), b_e=b(d.Be), W_ih=w(3 * d.Be, d.Be), W_hh=w(3 * d.Be, d.Be), b_ih=b(3 * d.Be),
             b_hh=b(3 * d.Be), W_1=w(d.Hd, d.Be), b_1=b(d.Hd), W_2=w(2 * d.S, d.Hd), b_2=b(2 * d.S))
    if imagine:
        W.update(W_a0=w(d.Hd, d.Be + d.S), W_a=[w(d.Hd, d.Hd) for _ in range(3)], b_a=[b(d.Hd) for _ in range(4)],
                 W_a4=w(2 * d.A, d.Hd), b_a4=b(2 * d.A))
    return W


NONTERM_KINDS = ("none", "ones", "zeros")


def make_observe_inputs(d: Dims, seed: int, device="cpu", nonterm="zeros", zero_init=False):
    g = torch.Generator().manual_seed(seed + 1000)
    r = lambda *s: torch.randn(*s, generator=g)
    I = dict(init_belief=torch.tanh(r(d.B, d.Be)), init_state=r(d.B, d.S), actions=r(d.T, d.B, d.A),
             pre_emb=0.5 * r(d.T, d.B, d.Hd), eps_post=r(d.T, d.B, d.S))
    if zero_init:
        I["init_belief"].zero_(); I["init_state"].zero_()
    if nonterm == "none":
        I["nonterm"] = None
    else:
        nt = torch.ones(d.T, d.B)
        if nonterm == "zeros":          # t = 0, mid-sequence and t = T-1, in different rows (wrapping over small batches)
            for i, t in enumerate(sorted({0, d.T // 2, d.T - 1})):
                nt[t, (3 * i) % d.B] = 0.0
                nt[t, (d.B - 1 - i) % d.B] = 0.0
        I["nonterm"] = nt
    return {k: (v.to(device) if v is not None else None) for k, v in I.items()}


def make_observe_grads(d: Dims, seed: int, device="cpu", dpm=True, dps=True):
    g = torch.Generator().manual_seed(seed + 2000)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    return dict(dfeat=r(d.T, d.B, d.Be + d.S), dpost_mean=r(d.T, d.B, d.S) if dpm else None,
                dpost_std=r(d.T, d.B, d.S) if dps else None)


def exp1(g, *shape):
    return torch.empty(*shape).exponential_(generator=g).clamp_min(1e-6)


def set_sat_gate(start_feat):
    """Belief unit 0 of the `saturated` variant: +0.9 on the even rows, -0.9 on the odd ones (plant_saturated)."""
    start_feat[:, 0] = torch.where(sat_rows(start_feat.shape[0], start_feat.device), 0.9, -0.9).to(start_feat.dtype)


def make_imagine_inputs(d: Dims, seed: int, device="cpu", discrete=False, saturated=False):
    """discrete: eps_action holds the Exp(1) draws of the Categorical actor's sampler."""
    g = torch.Generator().manual_seed(seed + 3000)
    r = lambda *s: torch.randn(*s, generator=g)
    sf = torch.cat([torch.tanh(r(d.B, d.Be)), r(d.B, d.S)], 1)
    I = dict(start_feat=sf, eps_action=exp1(g, d.T, d.B, d.A) if discrete else r(d.T, d.B, d.A), eps_prior=r(d.T, d.B, d.S))
    if saturated:
        set_sat_gate(sf)
    return {k: v.to(device) for k, v in I.items()}


DISCRETE_VARIANTS = ("peaked", "saturated", "duplicate")     # at A = 17 and A = 64; "regular" at every shape
ACTOR_DUP = {17: (3, 11), 64: (5, 37)}      # inside one 16-lane group; across the xor-32 stage of disc_sample's butterfly


def plant_actor_duplicate(d, W, eps_action):
    """The duplicate-class case of the Categorical actor (scan_cat_ref.plant_duplicate for the prior's factors): class `hi`
    gets the W_a4 row, the bias (raised by 3.0, so that the pair wins often) and the draws of class `lo`.  Their p / q tie
    bit for bit; the first maximum, `lo`, must be the class sampled."""
    lo, hi = ACTOR_DUP[d.A]
    W["b_a4"][lo] += 3.0
    W["W_a4"][hi], W["b_a4"][hi] = W["W_a4"][lo], W["b_a4"][lo]
    eps_action[..., hi] = eps_action[..., lo]
    return lo, hi


def actor_duplicate_check(d, norm, action):
    """Bit-equal log-probabilities of the planted pair, and never the higher index sampled.  Returns how often the pair won."""
    lo, hi = ACTOR_DUP[d.A]
    assert torch.equal(norm[..., lo], norm[..., hi]), "the log-probabilities of two identical classes differ in bits"
    k = action.argmax(-1)
    assert not bool((k == hi).any()), f"class {hi} sampled although class {lo} ties with it"
    assert not bool((action[..., hi] != 0).any()), f"action entry {hi} nonzero although class {lo} ties with it"
    return int((k == lo).sum())


def make_imagine_grads(d: Dims, seed: int, device="cpu", ent_weight=True):
    """dfeat, arbitrary numbers for slots 2, 3 of sv_act_stats (read by the backward as given) and the weights."""
    g = torch.Generator().manual_seed(seed + 4000)
    r = lambda *s: torch.randn(*s, generator=g).to(device)
    return dict(dfeat=r(d.T, d.B, d.Be + d.S), slot2=r(d.T, d.B, d.A), slot3=r(d.T, d.B, d.A),
                ent_weight=(torch.rand(d.T, d.B, generator=g).to(device) + 0.5) if ent_weight else None)


def make_discrete_case(d, seed, variant="regular", device="cpu", weights=None, inputs=None):
    """Weights and inputs of one case of the Categorical actor: (W, I, saturated rows or None, planted pair or None).
    `weights` / `inputs`: make_weights / make_imagine_inputs of the latent kind (default: the Gaussian ones)."""
    assert variant in ("regular",) + DISCRETE_VARIANTS, variant
    W = (weights or make_weights)(d, seed, device, imagine=True, actor=variant if variant in ("peaked", "saturated") else None)
    I = (inputs or make_imagine_inputs)(d, seed, device, discrete=True, saturated=variant == "saturated")
    dup = plant_actor_duplicate(d, W, I["eps_action"]) if variant == "duplicate" else None
    return W, I, (sat_rows(d.B, device) if variant == "saturated" else None), dup


# ---- layer pieces ------------------------------------------------------------------------------------------------------

def lin(x, W, b=None, extra=None):
    pre, S = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        pre, S = pre + b, S + b.abs()
    if extra is not None:
        pre, S = pre + extra, S + extra.abs()
    return pre, S


def dgrad(dn, W, saved, AL):
    """(dn W) * ELU'(saved): reference, S, allow (dense_ref.dgrad_ref with the build's allowance)."""
    acc, S = dn @ W, dn.abs() @ W.abs()
    f = elu_grad_from_out64(saved)
    return acc * f, S * f + (acc * f).abs(), AL.act * acc.abs()


def gru_layers(W, x, h_prev, K, t, AL, Be):
    gi, Sgi = lin(x, W["W_ih"], W["b_ih"])
    gh, Sgh = lin(h_prev, W["W_hh"], W["b_hh"])
    g = K["sv_gates"][t]
    for i in (0, 1):
        c = slice(i * Be, (i + 1) * Be)
        v = torch.sigmoid(gi[:, c] + gh[:, c])
        yield "sv_gates", t, c, v, v * (1 - v) * (Sgi[:, c] + Sgh[:, c]) + v, AL.sigmoid
    c2 = slice(2 * Be, 3 * Be)
    yield "sv_gates", t, slice(3 * Be, 4 * Be), gh[:, c2], Sgh[:, c2], 0.0
    rk, nhk = g[:, :Be], g[:, 3 * Be:]
    n = torch.tanh(gi[:, c2] + rk * nhk)
    yield "sv_gates", t, c2, n, (1 - n * n) * (Sgi[:, c2] + (rk * nhk).abs()) + n.abs(), AL.tanh
    zk, nk = g[:, Be:2 * Be], g[:, c2]
    yield "feat", t, slice(0, Be), (1 - zk) * nk + zk * h_prev, ((1 - zk) * nk).abs() + (zk * h_prev).abs() + nk.abs(), 0.0


def head_layers(W, q, eps, min_std, K, t, AL, S_, Be, mean_name, std_name):
    out, So = lin(q, W["W_2"], W["b_2"])
    mean, Sm = out[:, :S_], So[:, :S_]
    raw = out[:, S_:]
    if K.get(mean_name) is not None:
        yield mean_name, t, ALL, mean, Sm, 0.0
        mean, Sm = K[mean_name][t], K[mean_name][t].abs()
    std = F.softplus(raw, beta=1, threshold=20) + min_std
    yield std_name, t, ALL, std, torch.sigmoid(raw) * So[:, S_:] + std, AL.softplus
    sk = K[std_name][t]
    yield "feat", t, slice(Be, Be + S_), mean + sk * eps, Sm + (sk * eps).abs() + mean.abs(), 0.0


# ---- observe forward ---------------------------------------------------------------------------------------------------

def observe_fwd_layers(d: Dims, W, I, K, min_std, AL=HW):
    """W, I float64 (to64); K: float64 tensors [T, B, width] named as in bd_observe_fwd_args."""
    ms = f32(min_std)
    for t in range(d.T):
        h_prev = K["feat"][t - 1][:, :d.Be] if t else I["init_belief"]
        s_prev = K["feat"][t - 1][:, d.Be:] if t else I["init_state"]
        s = s_prev * I["nonterm"][t][:, None] if I.get("nonterm") is not None else s_prev
        yield "sv_s", t, ALL, s, s.abs(), 0.0
        pre, S = lin(torch.cat([K["sv_s"][t], I["actions"][t]], 1), W["W_e"], W["b_e"])
        yield "sv_x", t, ALL, elu64(pre), S, AL.act
        yield from gru_layers(W, K["sv_x"][t], h_prev, K, t, AL, d.Be)
        pre, S = lin(K["feat"][t][:, :d.Be], W["W_1"], W["b_1"], I["pre_emb"][t])
        yield "sv_q", t, ALL, elu64(pre), S, AL.act
        yield from head_layers(W, K["sv_q"][t], I["eps_post"][t], ms, K, t, AL, d.S, d.Be, "post_mean", "post_std")


OBS_FWD_TENSORS = dict(feat=lambda d: d.Be + d.S, post_mean=lambda d: d.S, post_std=lambda d: d.S, sv_s=lambda d: d.S,
                       sv_x=lambda d: d.Be, sv_gates=lambda d: 4 * d.Be, sv_q=lambda d: d.Hd)
OBS_BWD_TENSORS = dict(d_embed_pre=lambda d: d.Be, d_gi=lambda d: 3 * d.Be, d_gh=lambda d: 3 * d.Be,
                       d_q1_pre=lambda d: d.Hd, d_q2_out=lambda d: 2 * d.S)


# ---- observe backward --------------------------------------------------------------------------------------------------

def gate_grads(dh, Sdh, Adh, g, hprev, Be):
    """GRU gate gradients from the total belief gradient (observe.hip step 3): dict name -> (value, S, A)."""
    r, z, n, hn = g[:, :Be], g[:, Be:2 * Be], g[:, 2 * Be:3 * Be], g[:, 3 * Be:]
    fn = (1 - z) * (1 - n * n)
    vni = dh * fn
    Sni = Sdh * fn + 2 * dh.abs() + vni.abs()
    fr = hn * r * (1 - r)
    vr = vni * fr
    Sr = Sni * fr.abs() + (vni * hn * r).abs() + vr.abs()
    fz = (hprev - n) * z * (1 - z)
    vz = dh * fz
    Sz = Sdh * fz.abs() + (dh * (hprev - n)).abs() + (dh.abs() * (hprev.abs() + n.abs()) * z * (1 - z)) + vz.abs()
    return dict(r=(vr, Sr, Adh * (fn * fr).abs()), z=(vz, Sz, Adh * fz.abs()), ni=(vni, Sni, Adh * fn),
                nh=(vni * r, Sni * r + (vni * r).abs(), Adh * fn * r))


def sigmoid_recovery(std, ms):
    """1 - exp(-(std - min_std)) and the magnitude of its fp32 input rounding (observe.hip step 1)."""
    x = std - ms
    return -torch.expm1(-x), (std.abs() + abs(ms)) * torch.exp(-x)


def observe_bwd_layers(d: Dims, W, I, K, G, min_std, AL=HW):
    """I: forward inputs plus the forward's tensors the backward reads (feat, post_std, sv_x, sv_gates, sv_q), float64;
    G: dfeat / dpost_mean / dpost_std (None allowed); K: the five d_* tensors."""
    ms = f32(min_std)
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
        dfs, eps = G["dfeat"][t][:, Be:], I["eps_post"][t]
        dpm = G["dpost_mean"][t] if G.get("dpost_mean") is not None else z0
        dps = G["dpost_std"][t] if G.get("dpost_std") is not None else z0
        dst = ds + dfs
        Sdst = Sds + dfs.abs() + dst.abs()
        dm, dsd = dst + dpm, dst * eps + dps
        sig, Sx = sigmoid_recovery(I["post_std"][t], ms)
        yield "d_q2_out", t, slice(0, S_), dm, Sdst + dpm.abs() + dm.abs(), 0.0
        yield ("d_q2_out", t, slice(S_, 2 * S_), dsd * sig,
               (Sdst * eps.abs() + dps.abs() + dsd.abs()) * sig + dsd.abs() * Sx + (dsd * sig).abs(), AL.softplus * dsd.abs())
        yield ("d_q1_pre", t, ALL) + dgrad(K["d_q2_out"][t], W["W_2"], I["sv_q"][t], AL)
        dq = K["d_q1_pre"][t]
        dfh = G["dfeat"][t][:, :Be]
        dh = dq @ W["W_1"] + dhc + dfh
        Sdh = dq.abs() @ W["W_1"].abs() + Sdhc + dfh.abs() + dh.abs()
        hprev = I["feat"][t - 1][:, :Be] if t else I["init_belief"]
        gg = gate_grads(dh, Sdh, 0.0, I["sv_gates"][t], hprev, Be)
        for name, third in (("d_gi", "ni"), ("d_gh", "nh")):
            for i, k in enumerate(("r", "z", third)):
                yield name, t, slice(i * Be, (i + 1) * Be), gg[k][0], gg[k][1], 0.0
        yield ("d_embed_pre", t, ALL) + dgrad(K["d_gi"][t], W["W_ih"], I["sv_x"][t], AL)
        dgh, z = K["d_gh"][t], I["sv_gates"][t][:, Be:2 * Be]
        dhc = dh * z + dgh @ W["W_hh"]
        Sdhc = Sdh * z + (dh * z).abs() + dgh.abs() @ W["W_hh"].abs() + dhc.abs()


# ---- imagination forward -----------------------------------------------------------------------------------------------

def img_fwd_tensors(d: Dims, discrete=False):
    """discrete (the Categorical actor): sv_act_stats is A wide and holds norm, `entropy` is written by the scan, there is
    no sv_act_us."""
    t = dict(feat=d.Be + d.S, prior_mean=d.S, prior_std=d.S, action=d.A, sv_x=d.Be, sv_gates=4 * d.Be, sv_p=d.Hd)
    t.update(dict(sv_act_stats=d.A, entropy=1) if discrete else dict(sv_act_stats=4 * d.A, sv_act_us=2 * d.A))
    t.update({f"sv_actor{l}": d.Hd for l in range(4)})
    return t


def actor_layers(d, W, x, I, K, t, AL=HW):
    """The tanh-Normal actor of one imagination step from its input x = [h; s] through `action` (shared with
    scan_cat_ref.py: the Categorical scan runs the same actor on [h; one-hot s])."""
    init, amin, scale = f32(ACT_RAW_INIT_STD), f32(ACT_MIN_STD), f32(ACT_MEAN_SCALE)
    A = d.A
    for l in range(4):
        pre, S = lin(x, W["W_a0"] if l == 0 else W["W_a"][l - 1], W["b_a"][l])
        yield f"sv_actor{l}", t, ALL, elu64(pre), S, AL.act
        x = K[f"sv_actor{l}"][t]
    out, So = lin(x, W["W_a4"], W["b_a4"])
    th = torch.tanh(out[:, :A] / scale)
    yield "sv_act_stats", t, slice(0, A), th, (1 - th * th) * (So[:, :A] + out[:, :A].abs()) / scale + th.abs(), AL.tanh
    pre, Sp = out[:, A:] + init, So[:, A:] + abs(init) + (out[:, A:] + init).abs()
    sg = torch.sigmoid(pre)
    yield "sv_act_stats", t, slice(A, 2 * A), sg, sg * (1 - sg) * Sp + sg, AL.sigmoid
    st = K["sv_act_stats"][t]
    mean = scale * st[:, :A]
    yield "sv_act_stats", t, slice(2 * A, 3 * A), mean, mean.abs(), 0.0
    sd = F.softplus(pre, beta=1, threshold=20) + amin
    yield "sv_act_stats", t, slice(3 * A, 4 * A), sd, sg * Sp + sd, AL.softplus
    mk, sk, eps = st[:, 2 * A:3 * A], st[:, 3 * A:], I["eps_action"][t]
    u = mk + sk * eps
    Su = mk.abs() + (sk * eps).abs() + u.abs()
    if K.get("sv_act_us") is not None:
        yield "sv_act_us", t, slice(0, A), u, Su, 0.0
        yield "sv_act_us", t, slice(A, 2 * A), sk, 0.0 * sk, 0.0       # the same bits as slot 3
        u, Su = K["sv_act_us"][t][:, :A], 0.0 * u
    a = torch.tanh(u)
    yield "action", t, ALL, a, (1 - a * a) * Su + a.abs(), AL.tanh


# ---- the Categorical actor (discrete_actions = 1), shared by both latent kinds ---------------------------------------------

def ratios64(logits, q, D, C):
    """softmax(l)_c / q_c per factor in float64 and d_c = l_c - max l (scan_cat_ref.py: "The sample")."""
    l = logits.double().reshape(-1, D, C)
    d = l - l.max(-1, keepdim=True).values
    assert float(d.min()) > -80.0 and float(q.min()) >= 1e-30, "ratios outside the normal range: the margin does not hold"
    return torch.softmax(l, -1) / q.double().reshape(-1, D, C), d


def first_max(logits, q, D, C):
    """argmax of the float64 ratios, the first maximum winning (the chained reference's sampler)."""
    return ratios64(logits, q, D, C)[0].argmax(-1)


def jacobian(logits, g, Sg, Ag, D, C):
    """Straight-through softmax Jacobian per factor as a (value, S, A) triple: p (g - sum_c p g), p from `logits`."""
    sh = g.shape
    p, Sp, _ = cat_probs_ref(logits.reshape(-1, D, C))
    g, Sg = g.reshape(-1, D, C), Sg.reshape(-1, D, C)
    Ag = Ag.reshape(-1, D, C) if torch.is_tensor(Ag) else Ag + 0.0 * g
    dot = (p * g).sum(-1, keepdim=True)
    Sdot = (Sp * g.abs() + p * Sg).sum(-1, keepdim=True) + (p * g).abs().sum(-1, keepdim=True)
    v = p * (g - dot)
    Sv = Sp * (g - dot).abs() + p * (Sg + Sdot + (g - dot).abs()) + v.abs()
    Av = p * (Ag + (p * Ag).sum(-1, keepdim=True)) + TINY * (g.abs() + dot.abs())
    return v.reshape(sh), Sv.reshape(sh), Av.reshape(sh)


def discrete_actor_layers(d, W, x, I, K, t, AL=HW, chain=False, sat=None):
    """The Categorical actor (discrete_actions = 1, csrc/bd_discrete.h; tests/discrete_oracle.py's discrete_head): the A
    outputs `out`, norm = out - logsumexp(out) (saved as sv_act_stats [.. x A]), p = softmax(norm), k = argmax(p / q) with
    q = eps_action, action = (onehot(k) + p) - p, entropy = -sum p norm.
    - norm: d lse = sum_c p_c d out_c <= max_c S_out, the fp32 exponentials, their sum over A <= 64 classes and the
      logarithm move lse by less than (A + 6) u <= 8 C_TOL, the two additions round by u |lse| and u |norm|.
    - action: the sampled class is read from the kernel's action (its entry above 0.5) and checked by `sample_check` on
      the kernel's norm (one factor of A classes, libm margin); every other entry is (0 + p) - p = 0 exactly, the hot
      entry fl(fl(1 + p) - p) lies within 2u (1 + p) <= 4u of 1.
    - entropy from the kernel's norm: p carries cat_probs_ref's S_p.
    sat (bool [N], the `saturated` variant): rows whose leading logit is at least SAT_LEAD above every other one
    (asserted here on the float64 logits).  expf(-104) is 0 in fp32, so the kernel's numbers of such a row are determined
    without a margin: s = 1 + 0, norm_k = 0, p = onehot(k) exactly, action = onehot(k) with hot entry
    fl(fl(1 + 1) - 1) = 1, entropy = -(1 * 0 + sum 0 * norm) = 0.  Action and entropy of these rows are yielded with
    S = 0 and no allowance: an exact comparison (norm keeps its bound).  The float64 values they replace are below 1e-49."""
    for l in range(4):
        pre, S = lin(x, W["W_a0"] if l == 0 else W["W_a"][l - 1], W["b_a"][l])
        yield f"sv_actor{l}", t, ALL, elu64(pre), S, AL.act
        x = K[f"sv_actor{l}"][t]
    out, So = lin(x, W["W_a4"][:d.A], W["b_a4"][:d.A])
    lse = out.logsumexp(-1, keepdim=True)
    yield "sv_act_stats", t, ALL, out - lse, So + So.max(-1, keepdim=True).values + out.abs() + 2 * lse.abs() + (out - lse).abs() + 8, 0.0
    nk = K["sv_act_stats"][t]
    reg = torch.ones(out.shape[0], dtype=torch.bool, device=out.device) if sat is None else ~sat
    if sat is not None:
        top = out[sat].topk(2, -1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= SAT_LEAD, f"t={t}: a saturated row leads by less than {SAT_LEAD}"
    if chain:
        k = out.argmax(-1)
        k[reg] = first_max(nk[reg], I["eps_action"][t][reg], 1, d.A)[:, 0]
        K["action"][t] = F.one_hot(k, d.A).to(D64)
    hot = (K["action"][t] > 0.5).to(D64)
    assert bool((hot.sum(-1) == 1).all()), f"action[t={t}]: not one class per row"
    hot = torch.where(reg[:, None], hot, F.one_hot(out.argmax(-1), d.A).to(D64))
    yield "action", t, ALL, hot, 0.0 * hot, 4 * U * hot * reg[:, None]
    p, Sp, _ = cat_probs_ref(nk)
    H = -(p * nk).sum(-1, keepdim=True) * reg[:, None]
    yield "entropy", t, ALL, H, ((Sp * nk.abs() + (p * nk).abs()).sum(-1, keepdim=True) + H.abs()) * reg[:, None], 0.0


def discrete_actor_tail(d, I, K, G, dentropy, sat=None):
    """d_actor_out [.. x A] of the Categorical actor from the d loss / d action triple:
    p (g - p.g) + dent (-p (norm + H)), p and H from the saved norm (bd_discrete.h disc_head_grad).
    sat: the saturated rows (discrete_actor_layers).  There p = onehot(k) exactly, so p.g = g_k, p_k (g_k - p.g) = 0,
    p_c (...) = 0 for every other class and p (norm + H) = 0 (norm_k = H = 0): every entry is exactly 0, yielded with
    S = 0 and no allowance."""
    dent0 = f32(dentropy)

    def tail(t, dA):
        nk = I["sv_act_stats"][t]
        v, Sv, Av = jacobian(nk, dA[0], dA[1], dA[2], 1, d.A)
        p, Sp, _ = cat_probs_ref(nk)
        H = -(p * nk).sum(-1, keepdim=True)
        SH = (Sp * nk.abs() + (p * nk).abs()).sum(-1, keepdim=True) + H.abs()
        dent = dent0 * G["ent_weight"][t][:, None] if G.get("ent_weight") is not None else dent0
        e = -dent * p * (nk + H)
        Se = abs(dent) * (Sp * (nk + H).abs() + p * (nk.abs() + SH + (nk + H).abs())) + 2 * e.abs()
        reg = 1.0 if sat is None else (~sat)[:, None].to(D64)
        yield "d_actor_out", t, ALL, (v + e) * reg, (Sv + Se + (v + e).abs()) * reg, Av * reg
    return tail


def saturated_exact(d, Kf, Kb, sat, tag=""):
    """The exact statements about the saturated rows, spelled out on the tensors ([T x N x width]; Kb may be None)."""
    hot = F.one_hot(torch.tensor(sat_class(d.A)), d.A).to(Kf["action"].dtype).to(Kf["action"].device)
    assert bool((Kf["action"][:, sat] == hot).all()), f"{tag}saturated rows: the action is not the one-hot of class {sat_class(d.A)} with 1"
    assert bool((Kf["entropy"][:, sat].abs() == 0).all()), f"{tag}saturated rows: |entropy| != 0"
    assert bool((Kf["sv_act_stats"][:, sat][..., sat_class(d.A)] == 0).all()), f"{tag}saturated rows: norm of the leading class != 0"
    if Kb is not None:
        assert bool((Kb["d_actor_out"][:, sat] == 0).all()), f"{tag}saturated rows: d_actor_out != 0"
    return int(sat.sum()) * d.T


def imagine_fwd_layers(d: Dims, W, I, K, min_std, AL=HW, discrete=False, chain=False, sat=None):
    """bd_imagine_forward_scan with sv_act_stats given; tanh-Normal actor, or the Categorical one (discrete; chain: the
    action is set from the float64 ratios, the chained reference).  K may lack prior_mean / sv_act_us (NULL)."""
    ms = f32(min_std)
    Be = d.Be
    for t in range(d.T):
        fp = K["feat"][t - 1] if t else I["start_feat"]
        h_prev, s_prev = fp[:, :Be], fp[:, Be:]
        if discrete:
            yield from discrete_actor_layers(d, W, fp, I, K, t, AL, chain, sat)
        else:
            yield from actor_layers(d, W, fp, I, K, t, AL)
        pre, S = lin(torch.cat([s_prev, K["action"][t]], 1), W["W_e"], W["b_e"])
        yield "sv_x", t, ALL, elu64(pre), S, AL.act
        yield from gru_layers(W, K["sv_x"][t], h_prev, K, t, AL, Be)
        pre, S = lin(K["feat"][t][:, :Be], W["W_1"], W["b_1"])
        yield "sv_p", t, ALL, elu64(pre), S, AL.act
        yield from head_layers(W, K["sv_p"][t], I["eps_prior"][t], ms, K, t, AL, d.S, Be, "prior_mean", "prior_std")


# ---- imagination backward ----------------------------------------------------------------------------------------------

def _mm(v, S, A, W):
    return v @ W, S @ W.abs() + v.abs() @ W.abs(), A @ W.abs()


def gauss_head_carry(W, I, min_std, AL):
    """The Gaussian prior head of the imagination backward: (t, d state triple) -> the (value, S, A) triple of
    d loss / d sv_p before ELU'."""
    ms = f32(min_std)

    def head(t, dm, Sdm, Adm):
        eps = I["eps_prior"][t]
        sig, Sx = sigmoid_recovery(I["prior_std"][t], ms)
        dr = dm * eps * sig
        Sdr = Sdm * eps.abs() * sig + (dm * eps).abs() * Sx + 2 * dr.abs()
        Adr = Adm * eps.abs() * sig + AL.softplus * (dm * eps).abs()
        return _mm(torch.cat([dm, dr], 1), torch.cat([Sdm, Sdr], 1), torch.cat([Adm, Adr], 1), W["W_2"])
    return head


def actor_pre_layers(W, I, K, t, AL, W_out):
    """d_actor_pre3..0 of step t, each from the kernel's own gradient of the layer above (d_actor_out first, through
    W_out: W_a4, or its A logit rows for the Categorical actor)."""
    dn, Wn = K["d_actor_out"][t], W_out
    for l in (3, 2, 1, 0):
        yield (f"d_actor_pre{l}", t, ALL) + dgrad(dn, Wn, I[f"sv_actor{l}"][t], AL)
        dn, Wn = K[f"d_actor_pre{l}"][t], W["W_a"][l - 1] if l else None


def imagine_bwd_layers(d: Dims, W, I, K, G, dentropy, min_std, AL=HW, actor_pre=True, head=None, actor_tail=None,
                       discrete=False, sat=None):
    """`head`: the prior head's backward (default: the Gaussian one; scan_cat_ref.py passes the Categorical one).
    `actor_tail(t, dA)`: the layers from the d loss / d action triple up to d_actor_out (default: the tanh-Normal actor
    below; discrete_actor_tail: the Categorical one, whose d_actor_pre chain starts from the A logit rows of W_a4).
    discrete (with sat, the saturated rows): actor_tail = discrete_actor_tail.
    I: forward inputs and tensors (start_feat, feat, prior_std, action, eps_*, sv_actor0..3, sv_act_stats with the
    caller's slots 2, 3, sv_x, sv_gates, sv_p), float64; G: dfeat, ent_weight (or None); K: d_actor_out and, with
    actor_pre, d_actor_pre0..3 (written by the scan or by the caller's bd_mlp_backward: the same contract)."""
    dent0 = f32(dentropy)
    if discrete and actor_tail is None:
        actor_tail = discrete_actor_tail(d, I, K, G, dentropy, sat)
    head = head or gauss_head_carry(W, I, min_std, AL)
    Be, S_, A = d.Be, d.S, d.A
    dev = W["W_e"].device
    zb, zs = torch.zeros(d.B, Be, dtype=D64, device=dev), torch.zeros(d.B, S_, dtype=D64, device=dev)
    dhc, dsc = (zb, zb, zb), (zs, zs, zs)
    Wes, Wea = W["W_e"][:, :S_], W["W_e"][:, S_:]
    for t in reversed(range(d.T)):
        dfs, dfh = G["dfeat"][t][:, Be:], G["dfeat"][t][:, :Be]
        dm = dsc[0] + dfs
        Sdm, Adm = dsc[1] + dfs.abs() + dm.abs(), dsc[2]
        acc = head(t, dm, Sdm, Adm)
        f = elu_grad_from_out64(I["sv_p"][t])
        dP = (acc[0] * f, acc[1] * f + (acc[0] * f).abs(), acc[2] * f + AL.act * acc[0].abs())
        m = _mm(*dP, W["W_1"])
        dh = m[0] + dhc[0] + dfh
        Sdh, Adh = m[1] + dhc[1] + dfh.abs() + dh.abs(), m[2] + dhc[2]
        fprev = I["feat"][t - 1] if t else I["start_feat"]
        g = I["sv_gates"][t]
        gg = gate_grads(dh, Sdh, Adh, g, fprev[:, :Be], Be)
        cat3 = lambda ks: tuple(torch.cat([gg[k][i] for k in ks], 1) for i in range(3))
        z = g[:, Be:2 * Be]
        mh = _mm(*cat3(("r", "z", "nh")), W["W_hh"])
        dhc = (dh * z + mh[0], Sdh * z + (dh * z).abs() + mh[1] + (dh * z + mh[0]).abs(), Adh * z + mh[2])
        mx = _mm(*cat3(("r", "z", "ni")), W["W_ih"])
        f = elu_grad_from_out64(I["sv_x"][t])
        dE = (mx[0] * f, mx[1] * f + (mx[0] * f).abs(), mx[2] * f + AL.act * mx[0].abs())
        dsc = _mm(*dE, Wes)
        dA = _mm(*dE, Wea)
        if actor_tail is not None:
            yield from actor_tail(t, dA)
            if actor_pre:
                yield from actor_pre_layers(W, I, K, t, AL, W["W_a4"][:A])
            continue
        act, epa, st = I["action"][t], I["eps_action"][t], I["sv_act_stats"][t]
        th, sg, s2, s3 = st[:, :A], st[:, A:2 * A], st[:, 2 * A:3 * A], st[:, 3 * A:]
        fa = 1 - act * act
        dxa, Sxa, Axa = dA[0] * fa, dA[1] * fa + dA[0].abs() + (dA[0] * fa).abs(), dA[2] * fa
        dent = dent0 * G["ent_weight"][t][:, None] if G.get("ent_weight") is not None else dent0
        dmean, dstd = dxa + dent * s2, dxa * epa + dent * s3
        Smean = Sxa + 2 * abs(dent * s2) + dmean.abs()
        Sstd = Sxa * epa.abs() + (dxa * epa).abs() + 2 * abs(dent * s3) + dstd.abs()
        ft = 1 - th * th
        yield "d_actor_out", t, slice(0, A), dmean * ft, Smean * ft + dmean.abs() + (dmean * ft).abs(), Axa * ft
        yield "d_actor_out", t, slice(A, 2 * A), dstd * sg, Sstd * sg + (dstd * sg).abs(), Axa * epa.abs() * sg
        if actor_pre:
            yield from actor_pre_layers(W, I, K, t, AL, W["W_a4"])


# ---- drivers -----------------------------------------------------------------------------------------------------------

def check_layers(layers, K, report=None, tag=""):
    """Compare every yielded layer; the failure names tensor, step, row and column.  report[name] = worst err / bound."""
    for name, t, sl, ref, S, allow in layers:
        got = K[name][t][:, sl]
        err = (got - ref).abs()
        bound = C_TOL * S + allow
        bad = ~(err <= bound)
        if bool(bad.any()):
            r, c = (int(i) for i in bad.nonzero()[0])
            col = c + (sl.start or 0)
            raise AssertionError(f"{tag}{name}[t={t}, row={r}, col={col}]: {int(bad.sum())} of {got.numel()} out of tolerance; "
                                 f"got {float(got[r, c])!r}, ref {float(ref[r, c])!r}, err {float(err[r, c]):.3e}, "
                                 f"bound {float(bound[r, c]):.3e}")
        if report is not None:
            pos = bound > 0
            assert bool((err[~pos] == 0).all()), f"{tag}{name}[t={t}]: nonzero error where the bound is zero"
            if bool(pos.any()):
                report[name] = max(report.get(name, 0.0), float((err[pos] / bound[pos]).max()))


def fill_layers(layers, K):
    """Write every yielded reference into K: the per-step reference chained over the whole sequence."""
    for name, t, sl, ref, _S, _allow in layers:
        K[name][t][:, sl] = ref


def empty_set(widths, d: Dims, device="cpu"):
    return {k: torch.zeros(d.T, d.B, (w(d) if callable(w) else w), dtype=D64, device=device) for k, w in widths.items()}


def near_decision_fraction(pres) -> float:
    """Largest share, over the given pre-activation tensors, of elements within DECISION_MARGIN of a branch point."""
    return max(float((p.abs() < DECISION_MARGIN).double().mean()) for p in pres)


# ---- host dispatch, restated (observe_cluster.hip pick_cluster, observe_ksplit.hip ksplit_ok, bd_scan_layout.h) --------------------

K_WAVES, K_MAX_CLUSTER, K_LOCAL_BLOCKS = 8, 16, 2
K_THREADS, K_FRAG, K_HEAD_MAX_N, K_MAX_LDS = K_WAVES * 64, 256, 64, 160 * 1024
K_SPLIT_PARTIAL = K_WAVES * 2 * 2 * 256
K_SPLIT_SCRATCH = K_SPLIT_PARTIAL + 2 * 16 * K_HEAD_MAX_N
ENGINE_MAX_WGS = 128


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def pick_cluster(B: int, Be: int) -> int:
    Nb, tiles = cdiv(Be, 16), cdiv(B, 16)
    C = Nb if tiles * Nb <= 256 else cdiv(Nb, K_LOCAL_BLOCKS)
    C = max(C, 1)
    return C if (C <= K_MAX_CLUSTER and tiles * C <= 256) else 0


def ksplit_ok(Be: int, S: int, A: int, Hd: int, C: int) -> bool:
    return (C == cdiv(Be, 16) and C <= 2 * K_WAVES and cdiv(Hd, 16) <= C and cdiv(S, 16) <= 4 and cdiv(A, 16) <= 2 and
            S <= K_HEAD_MAX_N and 16 * S <= K_THREADS and 2 * cdiv(S, 16) <= K_WAVES)


def observe_forms(B, Be, S, A, Hd):
    """Forms that accept the shape: 'single' (observe.hip), 'ksplit', 'round1' (the cluster call with set_ksplit(0))."""
    forms = ["single"]
    C = pick_cluster(B, Be)
    if C > 0 and S <= K_HEAD_MAX_N:
        if ksplit_ok(Be, S, A, Hd, C):
            forms.append("ksplit")
        forms.append("round1")
    return forms


def lds_bytes(entry: str, Be, S, A, Hd, discrete: bool = False) -> int:
    """Dynamic LDS of every entry point; the CPU test holds it to the library at every table shape (bd_scan_lds_bytes).
    discrete: the imagination forward with the Categorical actor keeps only the logits image of the four action regions
    (bd_scan_layout.h ImagineFwdLds); the library's query describes the tanh-Normal layout, so the CPU test holds this
    figure to the "needs N B of LDS" refusal of a shape above 160 KiB instead."""
    h, s, a, hd = cdiv(Be, 16), cdiv(S, 16), cdiv(A, 16), cdiv(Hd, 16)
    if entry == "observe_fwd":
        n = (3 * h + hd + s + a) * K_FRAG + 16 * S + K_SPLIT_SCRATCH
    elif entry == "observe_bwd":
        n = (6 * h + hd + 2 * s) * K_FRAG + 16 * S + K_SPLIT_SCRATCH
    elif entry == "cluster_fwd":
        n = (3 * h + hd + s + a) * K_FRAG + 16 * S + max(K_WAVES * K_LOCAL_BLOCKS * 4 * 64 * 4, K_SPLIT_SCRATCH)
    elif entry == "cluster_bwd":
        n = (6 * h + hd + 2 * s) * K_FRAG + 16 * S + max(K_WAVES * K_LOCAL_BLOCKS * 2 * 64 * 4, K_SPLIT_PARTIAL)
    elif entry == "ksplit_fwd":
        n = ((s + a) * K_FRAG + ((16 * S + 3) & ~3) + 2 * K_WAVES * 256 + (K_WAVES // (2 * s)) * 2 * 16 * s * 16 +
             2 * h * K_FRAG + K_WAVES * 4 * 256)
    elif entry == "ksplit_bwd":
        n = 2 * s * K_FRAG + (K_WAVES // s) * ((16 * S + 3) & ~3) + 2 * K_WAVES * 256
    elif entry == "imagine_fwd":
        n = (3 * h + 2 * hd + s + a) * K_FRAG + (16 if discrete else 3 * 16 + K_WAVES * 16 * 3) * A + K_SPLIT_SCRATCH
    elif entry == "imagine_bwd":
        n = (6 * h + 3 * hd + 2 * s + 2 * a) * K_FRAG + 16 * S + K_SPLIT_PARTIAL
    else:
        raise ValueError(entry)
    return 4 * n


# ---- the GPU shape tables (the CPU tests assert form and LDS side of every entry) ---------------------------------------
# (T, B, Be, S, A, Hd), cluster size, default cluster form ('ksplit' / 'round1' / None)
OBSERVE_SHAPES = {
    "configs1": (Dims(3, 50, 200, 30, 6, 200), 13, "ksplit"),
    "b1": (Dims(2, 1, 40, 10, 3, 32), 3, "ksplit"),
    "b15": (Dims(2, 15, 40, 10, 3, 32), 3, "ksplit"),
    "b16": (Dims(2, 16, 40, 10, 3, 32), 3, "ksplit"),
    "b17_T7": (Dims(7, 17, 40, 10, 3, 32), 3, "ksplit"),
    "b17_T1": (Dims(1, 17, 40, 10, 3, 32), 3, "ksplit"),
    "ragged42": (Dims(3, 19, 42, 10, 3, 30), 3, "ksplit"),
    "ragged46": (Dims(3, 19, 46, 9, 2, 35), 3, "ksplit"),
    "a17": (Dims(2, 20, 40, 10, 17, 32), 3, "ksplit"),
    "a32": (Dims(2, 20, 40, 10, 32, 32), 3, "ksplit"),
    "s32": (Dims(2, 20, 40, 32, 3, 32), 3, "ksplit"),
    "s33": (Dims(2, 20, 40, 33, 3, 32), 3, "round1"),
    "s64": (Dims(2, 20, 40, 64, 3, 32), 3, "round1"),
    "s65": (Dims(2, 20, 40, 65, 3, 32), 3, None),            # the cluster forward rejects S > 64: single form only
    "hd_gt_be": (Dims(2, 20, 48, 10, 3, 80), 3, "round1"),
    "b320": (Dims(2, 320, 200, 30, 6, 200), 7, "round1"),    # two belief blocks per member, 140 workgroups
    "be300": (Dims(2, 16, 300, 10, 3, 32), 0, None),         # 19 belief blocks: no cluster; the backward fills the CU's LDS
    "biglds": (Dims(2, 16, 256, 30, 6, 256), 16, "ksplit"),  # above 64 KiB in the single and round-1 forms
}
# dynamic LDS above 64 KiB (the kernel must be opted in, allow_big_lds)?  entry point -> shape names on the far side; every
# other shape of the table is below.  Only the single-workgroup entry points have such a line: the cluster launchers opt
# in unconditionally (the round-1 forward's gate-partial scratch alone is 64 KiB).
OBSERVE_BIG_LDS = {
    "observe_fwd": {"configs1", "b320", "be300", "biglds"},
    "observe_bwd": {"configs1", "b320", "be300", "biglds", "hd_gt_be", "s32", "s33", "s64", "s65"},
}
IMAGINE_SHAPES = {
    "n1_h1": Dims(1, 1, 40, 10, 1, 32),
    "n17_h2": Dims(2, 17, 40, 10, 6, 32),
    "n17_h14": Dims(14, 17, 40, 10, 6, 32),
    "a17": Dims(2, 17, 40, 10, 17, 32),
    "ragged42": Dims(3, 19, 42, 10, 3, 30),
    "ragged46": Dims(3, 19, 46, 9, 2, 35),
    "n2450": Dims(2, 2450, 200, 30, 6, 200),
}
IMAGINE_BIG_LDS = {"imagine_fwd": {"n17_h2", "n17_h14", "a17", "n2450"}, "imagine_bwd": {"n2450"}}


# ---- the Categorical actor (discrete_actions = 1) in the imagination scan -------------------------------------------------
# A = 2 / 16: one column block of the logits GEMM, part of it / all of it; 17: a second block with one column; 33: a third;
# 64: no invalid lane.  n1_a1: one row, one class (norm = 0, p = 1, H = 0, gradient 0).  n32_a17: N a multiple of 16.
DISCRETE_SHAPES = {
    **{f"a{A}": Dims(3, 19, 40, 10, A, 32) for A in (2, 16, 17, 33, 64)},
    "n1_a1": Dims(1, 1, 40, 10, 1, 32),
    "n32_a17": Dims(2, 32, 40, 10, 17, 32),
    "ragged_a18": Dims(3, 19, 42, 9, 18, 30),
}
DISCRETE_EXACT = (("a17", "regular"), ("a64", "peaked"))      # the cases of the -DBD_EXACT_MATH twin
# the seeds of the GPU tests that sample (the Categorical scans, the Categorical actor: its cases use the last one); the
# CPU tests assert the ambiguous share of each on the float64 reference
SEEDS = (11, 12, 24)


def discrete_cases(shapes):
    """(shape name, variant) of every GPU case of the Categorical actor."""
    return [(n, "regular") for n in shapes] + [(n, v) for n in ("a17", "a64") for v in DISCRETE_VARIANTS]
