"""CPU tests of tests/scan_ref.py: the per-step float64 references of the observe and imagination scans chain to the
oracle and to autograd; an fp32 emulation of the kernels' order of operations passes every tolerance at every shape of
the GPU tables; planted faults fail; the host dispatch (cluster size, form, LDS side, rejections) matches the tables.  The
Categorical actor (discrete_actions = 1) in the imagination scan: chain against autograd, emulation at every GPU case,
planted faults, and the ambiguous share of its draws on the float64 reference."""
import ctypes as C
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O
from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.discrete_oracle import FLOAT_MIN, discrete_head

D64 = torch.float64


# ---- an emulation of the kernels' order of operations in plain torch (any dtype; optional planted fault) ---------------

def _cast(d, dtype):
    return {k: (v.to(dtype) if torch.is_tensor(v) else [w.to(dtype) for w in v] if isinstance(v, list) else v)
            for k, v in d.items()}


def _gru(W, x, h, Be, fault, keep):
    gi = x @ W["W_ih"].t() + W["b_ih"]
    gh = h @ W["W_hh"].t() + W["b_hh"]
    keep += [gi, gh]
    r = torch.sigmoid(gi[:, :Be] + gh[:, :Be])
    z = torch.sigmoid(gi[:, Be:2 * Be] + gh[:, Be:2 * Be])
    nh = gh[:, 2 * Be:]
    n = torch.tanh(gi[:, 2 * Be:] + r * nh)
    hn = (1 - z) * n + z * h
    slot3 = nh - W["b_hh"][2 * Be:] if fault == "no_bhn" else nh
    return hn, torch.cat([r, z, n, slot3], 1)


def _head(W, q, eps, ms, fault):
    out = (q[:, :-1] @ W["W_2"][:, :-1].t() if fault == "drop_col_hd" else q @ W["W_2"].t()) + W["b_2"]
    S_ = out.shape[1] // 2
    std = F.softplus(out[:, S_:]) + ms
    return out, out[:, :S_], std, out[:, :S_] + std * eps


def emu_observe_fwd(d, W, I, min_std, dtype, fault=None):
    W, I = _cast(W, dtype), _cast(I, dtype)
    ms = min_std if dtype == D64 else R.f32(min_std)
    h, s = I["init_belief"], I["init_state"]
    K = {k: [] for k in R.OBS_FWD_TENSORS}
    pres = dict(pre_e=[], gi=[], gh=[], q1=[], out=[])
    for t in range(d.T):
        if I["nonterm"] is not None and fault != "fwd_mask_dropped":
            s = s * I["nonterm"][t][:, None]
        sa = torch.cat([s, I["actions"][t]], 1)
        pre_e = (sa[:, 1:] @ W["W_e"][:, 1:].t() if fault == "drop_col_s" else sa @ W["W_e"].t()) + W["b_e"]
        x = F.elu(pre_e)
        if fault == "zero_last_row" and t == d.T - 1:
            x = torch.cat([x[:-1], 0 * x[-1:]], 0)
        keep = []
        hn, gates = _gru(W, x, h, d.Be, fault, keep)
        q1 = (hn[:, :-1] @ W["W_1"][:, :-1].t() if fault == "drop_col_be" else hn @ W["W_1"].t()) + W["b_1"] + I["pre_emb"][t]
        q = F.elu(q1)
        eps = I["eps_post"][(t + 1) % d.T] if fault == "eps_wrong_step" else I["eps_post"][t]
        out, mean, std, st = _head(W, q, eps, ms, fault)
        for k, v in dict(feat=torch.cat([hn, st], 1), post_mean=mean, post_std=std, sv_s=s, sv_x=x, sv_gates=gates, sv_q=q).items():
            K[k].append(v)
        for k, v in dict(pre_e=pre_e, gi=keep[0], gh=keep[1], q1=q1, out=out).items():
            pres[k].append(v)
        h, s = hn, st
    return {k: torch.stack(v) for k, v in K.items()}, pres


def _elug(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def _gate_bwd(dh, g, hprev, Be):
    r, z, n, hn = g[:, :Be], g[:, Be:2 * Be], g[:, 2 * Be:3 * Be], g[:, 3 * Be:]
    vni = dh * (1 - z) * (1 - n * n)
    vr = vni * hn * r * (1 - r)
    vz = dh * (hprev - n) * z * (1 - z)
    return torch.cat([vr, vz, vni], 1), torch.cat([vr, vz, vni * r], 1), dh * z


def emu_observe_bwd(d, W, I, G, min_std, dtype, fault=None):
    W, I, G = _cast(W, dtype), _cast(I, dtype), _cast(G, dtype)
    ms = min_std if dtype == D64 else R.f32(min_std)
    Be, S_ = d.Be, d.S
    K = {k: [None] * d.T for k in R.OBS_BWD_TENSORS}
    dhc, ds = torch.zeros(d.B, Be, dtype=dtype), torch.zeros(d.B, S_, dtype=dtype)
    for t in reversed(range(d.T)):
        eps = I["eps_post"][t - 1] if fault == "bwd_eps_step" else I["eps_post"][t]
        dst = ds + G["dfeat"][t][:, Be:]
        dm = dst + (G["dpost_mean"][t] if G["dpost_mean"] is not None else 0)
        sig = 1 - torch.exp(-(I["post_std"][t] - (0.0 if fault == "no_min_std" else ms)))
        dps = G["dpost_std"][t] if G["dpost_std"] is not None else 0
        dr = dst * eps * sig + dps if fault == "dps_after" else (dst * eps + dps) * sig
        d2 = torch.cat([dm, dr], 1)
        dq = (d2 @ W["W_2"]) * _elug(I["sv_q"][t])
        dh = dq @ W["W_1"] + dhc + G["dfeat"][t][:, :Be]
        hprev = I["feat"][t - 1][:, :Be] if t else I["init_belief"]
        if fault == "hprev_t":
            hprev = I["feat"][t][:, :Be]
        if fault == "no_init" and t == 0:
            hprev = 0 * hprev
        dgi, dgh, carry = _gate_bwd(dh, I["sv_gates"][t], hprev, Be)
        if fault == "bwd_zero_last_row":
            dgi = torch.cat([dgi[:-1], 0 * dgi[-1:]], 0)
        de = ((dgi[:, :-1] @ W["W_ih"][:-1] if fault == "bwd_drop_col" else dgi @ W["W_ih"])) * _elug(I["sv_x"][t])
        dhc = carry + dgh @ W["W_hh"]
        ds = de @ W["W_e"][:, :S_]
        if I["nonterm"] is not None:
            ds = ds * I["nonterm"][t - 1 if fault == "mask_step" else t][:, None]
        for k, v in dict(d_embed_pre=de, d_gi=dgi, d_gh=dgh, d_q1_pre=dq, d_q2_out=d2).items():
            K[k][t] = v
    return {k: torch.stack(v) for k, v in K.items()}


def emu_discrete_head(out, q, fault=None):
    """The Categorical actor's row pass (csrc/bd_discrete.h) in the dtype of `out`: (action, entropy [N x 1], norm, the
    action as the embed layer reads it).  Without a fault it is tests/discrete_oracle.discrete_head itself."""
    A = out.shape[1]
    if fault is None:
        a, ent, norm, _k = discrete_head(out, q)
        return a, ent[:, None], norm, a
    o = torch.cat([out[:, :16], 0 * out[:, 16:]], 1) if fault == "cols16_dropped" else out     # logit image columns >= 16 unwritten
    if fault == "no_max":                   # exp(out) instead of exp(out - max)
        lse = torch.log(torch.exp(o).sum(-1, keepdim=True))
    elif fault == "lane63_invalid":         # lane < A - 1: the last class never enters a reduction
        lse = o[:, :A - 1].logsumexp(-1, keepdim=True)
    else:
        lse = o.logsumexp(-1, keepdim=True)
    norm = o - lse
    p = F.softmax(norm, -1)
    if fault == "lane63_invalid":
        p = torch.cat([F.softmax(norm[:, :A - 1], -1), 0 * p[:, A - 1:]], 1)
    r = p / q
    k = (A - 1 - r.flip(-1).argmax(-1)) if fault == "sampler_ge" else r.argmax(-1)       # r >= best: the LAST maximum wins
    a = (F.one_hot(k, A).to(p.dtype) + p) - p
    ent = -(torch.clamp(norm, min=FLOAT_MIN) * p).sum(-1, keepdim=True)
    ae = torch.cat([a[:, :16], 0 * a[:, 16:]], 1) if fault == "af16_dropped" else a       # action fragment columns >= 16 unwritten
    return a, ent, norm, ae


def emu_discrete_grad(norm, dA, dent, fault=None):
    """d_actor_out of the Categorical actor from the saved norm (bd_discrete.h disc_rows_bwd)."""
    if fault == "ent_dropped":
        dent = 0 * dent
    elif fault == "ent_sign":
        dent = -dent
    p = torch.softmax(norm, -1)
    H = -(p * norm).sum(-1, keepdim=True)
    return p * (dA - (p * dA).sum(-1, keepdim=True)) + dent * (-p * (norm + H))


def emu_imagine_fwd(d, W, I, min_std, dtype, with_us=True, with_mean=True, discrete=False, fault=None):
    W, I = _cast(W, dtype), _cast(I, dtype)
    exact = dtype == D64
    ms, init, amin, scale = [(v if exact else R.f32(v)) for v in (min_std, R.ACT_RAW_INIT_STD, R.ACT_MIN_STD, R.ACT_MEAN_SCALE)]
    Be, A = d.Be, d.A
    fp = I["start_feat"]
    names = list(R.img_fwd_tensors(d, discrete))
    K = {k: [] for k in names}
    pres = {f"a{l}": [] for l in range(4)}
    pres.update(out=[], mean=[], std=[])
    for t in range(d.T):
        x = fp.detach()
        step = {}
        for l in range(4):
            pre = x @ (W["W_a0"] if l == 0 else W["W_a"][l - 1]).t() + W["b_a"][l]
            pres[f"a{l}"].append(pre)
            x = F.elu(pre)
            step[f"sv_actor{l}"] = x
        out = x @ W["W_a4"].t() + W["b_a4"]
        if discrete:
            out = out[:, :A]
            a, ent, norm, ae = emu_discrete_head(out, I["eps_action"][t], fault)
            step.update(sv_act_stats=norm, entropy=ent)
            mean = sd = out
        else:
            th = torch.tanh(out[:, :A] / scale)
            mean = scale * th
            pre_s = out[:, A:] + init
            sd = F.softplus(pre_s) + amin
            u = mean + sd * I["eps_action"][t]
            a = ae = torch.tanh(u)
            step.update(sv_act_stats=torch.cat([th, torch.sigmoid(pre_s), mean, sd], 1), sv_act_us=torch.cat([u, sd], 1))
        xe = F.elu(torch.cat([fp[:, Be:], ae], 1) @ W["W_e"].t() + W["b_e"])
        hn, gates = _gru(W, xe, fp[:, :Be], Be, None, [])
        p = F.elu(hn @ W["W_1"].t() + W["b_1"])
        _o, pm, ps, st = _head(W, p, I["eps_prior"][t], ms, None)
        fp = torch.cat([hn, st], 1)
        step.update(feat=fp, prior_mean=pm, prior_std=ps, action=a, sv_x=xe, sv_gates=gates, sv_p=p)
        for k in names:
            K[k].append(step[k])
        for k, v in dict(out=out, mean=mean, std=sd).items():
            pres[k].append(v)
    K = {k: torch.stack(v) for k, v in K.items()}
    if not with_us and not discrete:
        K["sv_act_us"] = None
    if not with_mean:
        K["prior_mean"] = None
    return K, pres


def emu_imagine_bwd(d, W, I, G, dentropy, min_std, dtype, fault=None, discrete=False):
    W, I, G = _cast(W, dtype), _cast(I, dtype), _cast(G, dtype)
    ms = min_std if dtype == D64 else R.f32(min_std)
    dent0 = dentropy if dtype == D64 else R.f32(dentropy)
    Be, S_, A = d.Be, d.S, d.A
    K = {"d_actor_out": [None] * d.T, **{f"d_actor_pre{l}": [None] * d.T for l in range(4)}}
    dhc, ds = torch.zeros(d.B, Be, dtype=dtype), torch.zeros(d.B, S_, dtype=dtype)
    for t in reversed(range(d.T)):
        dm = ds + G["dfeat"][t][:, Be:]
        dr = dm * I["eps_prior"][t] * (1 - torch.exp(-(I["prior_std"][t] - ms)))
        dP = (torch.cat([dm, dr], 1) @ W["W_2"]) * _elug(I["sv_p"][t])
        dh = dP @ W["W_1"] + dhc + G["dfeat"][t][:, :Be]
        fprev = I["feat"][t - 1] if t else I["start_feat"]
        dgi, dgh, carry = _gate_bwd(dh, I["sv_gates"][t], fprev[:, :Be], Be)
        dhc = carry + dgh @ W["W_hh"]
        dE = (dgi @ W["W_ih"]) * _elug(I["sv_x"][t])
        ds = dE @ W["W_e"][:, :S_]
        dA = dE @ W["W_e"][:, S_:]
        st, act = I["sv_act_stats"][t], I["action"][t]
        dent = dent0 * G["ent_weight"][t][:, None] if (G["ent_weight"] is not None and fault != "no_ent_weight") else dent0
        if discrete:        # the hidden layers below: the caller's bd_mlp_backward from d_actor_out through W_a4's A logit rows
            dn, Wn = emu_discrete_grad(st, dA, dent, fault), W["W_a4"][:A]
        else:
            dxa = dA if fault == "no_tanh_grad" else dA * (1 - act * act)
            dmean = dxa + dent * st[:, 2 * A:3 * A]
            dstd = dxa * I["eps_action"][t] + dent * st[:, 3 * A:]
            dn, Wn = torch.cat([dmean * (1 - st[:, :A] ** 2), dstd * st[:, A:2 * A]], 1), W["W_a4"]
        K["d_actor_out"][t] = dn
        for l in (3, 2, 1, 0):
            dn = (dn @ Wn) * _elug(I[f"sv_actor{l}"][t])
            K[f"d_actor_pre{l}"][t] = dn
            Wn = W["W_a"][l - 1] if l else None
    return {k: torch.stack(v) for k, v in K.items()}


# ---- helpers ------------------------------------------------------------------------------------------------------------

def k64(K):
    return {k: (v.double().clone() if v is not None else None) for k, v in K.items()}


def observe_bwd_inputs(I, Kf):
    return dict(I, **{k: Kf[k] for k in ("feat", "post_std", "sv_x", "sv_gates", "sv_q")})


def imagine_bwd_inputs(I, Kf, G):
    J = dict(I, **{k: v for k, v in Kf.items() if k != "sv_act_us"})
    st = Kf["sv_act_stats"].clone()
    A = st.shape[-1] // 4
    st[..., 2 * A:3 * A], st[..., 3 * A:] = G["slot2"].to(st.dtype), G["slot3"].to(st.dtype)
    J["sv_act_stats"] = st
    return J


def oracle_sd(W, d, E=0, seed=5):
    g = torch.Generator().manual_seed(seed)
    W_emb = torch.randn(d.Hd, max(E, 1), generator=g, dtype=D64) * 0.3
    sd = {"fc_embed_state_action.0.weight": W["W_e"], "fc_embed_state_action.0.bias": W["b_e"],
          "rnn.weight_ih": W["W_ih"], "rnn.bias_ih": W["b_ih"], "rnn.weight_hh": W["W_hh"], "rnn.bias_hh": W["b_hh"]}
    for which, first in (("belief_posterior", torch.cat([W["W_1"].double(), W_emb], 1)), ("belief_prior", W["W_1"])):
        sd.update({f"{which}.model.0.weight": first, f"{which}.model.0.bias": W["b_1"],
                   f"{which}.model.2.weight": W["W_2"], f"{which}.model.2.bias": W["b_2"]})
    return {k: v.double() for k, v in sd.items()}, W_emb


def _leaves(W):
    """The weights as autograd leaves, so that every pre-activation of the emulation carries a graph."""
    leaf = lambda v: v.clone().requires_grad_(True)
    return {k: ([leaf(w) for w in v] if isinstance(v, list) else leaf(v)) for k, v in W.items()}


def rel_close(a, b, tol=1e-10):
    a, b = a.detach(), b.detach()
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), float((a - b).abs().max())


# ---- the reference chains to the oracle and to autograd (float64 against float64) -----------------------------------------

@pytest.mark.parametrize("nonterm", R.NONTERM_KINDS)
def test_observe_reference_equals_oracle_and_autograd(monkeypatch, nonterm):
    monkeypatch.setattr(R, "f32", lambda x: x)
    d = R.Dims(5, 7, 22, 6, 3, 19)
    W = R.to64(R.make_weights(d, 3))
    I = R.to64(R.make_observe_inputs(d, 3, nonterm=nonterm))
    sd, W_emb = oracle_sd(W, d, E=4)
    emb = torch.randn(d.T, d.B, 4, dtype=D64, generator=torch.Generator().manual_seed(9))
    I["pre_emb"] = emb @ W_emb.t()
    G = R.to64(R.make_observe_grads(d, 3))
    # forward: per-step reference, chained
    Kf = R.empty_set(R.OBS_FWD_TENSORS, d)
    R.fill_layers(R.observe_fwd_layers(d, W, I, Kf, 0.1), Kf)
    nt = I["nonterm"][:, :, None] if I["nonterm"] is not None else None
    bel, _, _, post, (qm, qs) = O.transition_forward(sd, I["init_state"], I["actions"], I["init_belief"], emb, nt,
                                                     torch.zeros(d.T, d.B, d.S, dtype=D64), I["eps_post"])
    rel_close(Kf["feat"][..., :d.Be], bel); rel_close(Kf["feat"][..., d.Be:], post)
    rel_close(Kf["post_mean"], qm); rel_close(Kf["post_std"], qs)
    # the emulation in float64 is the oracle's function too; autograd through it gives the pre-activation gradients
    Ke, pres = emu_observe_fwd(d, _leaves(W), I, 0.1, D64)
    for k in Kf:
        rel_close(Ke[k], Kf[k])
    loss = (Ke["feat"] * G["dfeat"]).sum() + (Ke["post_mean"] * G["dpost_mean"]).sum() + (Ke["post_std"] * G["dpost_std"]).sum()
    flat = [p for k in ("pre_e", "gi", "gh", "q1", "out") for p in pres[k]]
    grads = torch.autograd.grad(loss, flat)
    ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in enumerate(("d_embed_pre", "d_gi", "d_gh", "d_q1_pre", "d_q2_out"))}
    Kb = R.empty_set(R.OBS_BWD_TENSORS, d)
    R.fill_layers(R.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G, 0.1), Kb)
    for k in Kb:
        rel_close(Kb[k], ag[k].detach())


@pytest.mark.parametrize("ent_weight", [True, False])
def test_imagine_reference_equals_oracle_and_autograd(monkeypatch, ent_weight):
    monkeypatch.setattr(R, "f32", lambda x: x)
    d = R.Dims(4, 5, 22, 6, 3, 19)
    W = R.to64(R.make_weights(d, 4, imagine=True))
    I = R.to64(R.make_imagine_inputs(d, 4))
    G = R.to64(R.make_imagine_grads(d, 4, ent_weight=ent_weight))
    Kf = R.empty_set(R.img_fwd_tensors(d), d)
    R.fill_layers(R.imagine_fwd_layers(d, W, I, Kf, 0.1), Kf)
    sd, _ = oracle_sd(W, d)
    actor = {"model.0.weight": W["W_a0"], "model.8.weight": W["W_a4"], "model.8.bias": W["b_a4"]}
    actor.update({f"model.{2 * l}.weight": W["W_a"][l - 1] for l in (1, 2, 3)})
    actor.update({f"model.{2 * l}.bias": W["b_a"][l] for l in range(4)})
    P = {"transition_model": sd, "actor": actor}
    sf = I["start_feat"]
    bel, sts, (pm, ps), _ent = O.imagine_ahead(P, sf[:, d.Be:], sf[:, :d.Be], d.T + 1, I["eps_action"],
                                               torch.zeros(d.T, 1, d.B, d.A, dtype=D64), I["eps_prior"])
    rel_close(Kf["feat"][..., :d.Be], bel); rel_close(Kf["feat"][..., d.Be:], sts)
    rel_close(Kf["prior_mean"], pm); rel_close(Kf["prior_std"], ps)
    m, s = O.actor_forward(sf[:, :d.Be], sf[:, d.Be:], actor)
    rel_close(Kf["sv_act_stats"][0][:, 2 * d.A:3 * d.A], m); rel_close(Kf["sv_act_stats"][0][:, 3 * d.A:], s)
    Ke, pres = emu_imagine_fwd(d, _leaves(W), I, 0.1, D64)
    for k in Kf:
        rel_close(Ke[k], Kf[k])
    dent = -0.37
    w = G["ent_weight"][:, :, None] if ent_weight else 1.0
    loss = (Ke["feat"] * G["dfeat"]).sum() + (dent * w * (torch.stack(pres["mean"]) * G["slot2"] + torch.stack(pres["std"]) * G["slot3"])).sum()
    flat = [p for k in ("out", "a0", "a1", "a2", "a3") for p in pres[k]]
    grads = torch.autograd.grad(loss, flat)
    ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in
          enumerate(("d_actor_out", "d_actor_pre0", "d_actor_pre1", "d_actor_pre2", "d_actor_pre3"))}
    Kb = R.empty_set({"d_actor_out": 2 * d.A, **{f"d_actor_pre{l}": d.Hd for l in range(4)}}, d)
    R.fill_layers(R.imagine_bwd_layers(d, W, imagine_bwd_inputs(I, Kf, G), Kb, G, dent, 0.1), Kb)
    for k in Kb:
        rel_close(Kb[k], ag[k].detach())


# ---- an fp32 emulation passes every tolerance at every shape of the GPU tables ------------------------------------------

def _observe_emulated(d, seed, min_std=0.1, nonterm="zeros", fwd_fault=None, bwd_fault=None, dpm=True, dps=True):
    W, I = R.make_weights(d, seed), R.make_observe_inputs(d, seed, nonterm=nonterm)
    G = R.make_observe_grads(d, seed, dpm=dpm, dps=dps)
    with torch.no_grad():
        Kf, pres = emu_observe_fwd(d, W, I, min_std, torch.float32, fwd_fault)
        Kb = emu_observe_bwd(d, W, observe_bwd_inputs(I, Kf), G, min_std, torch.float32, bwd_fault)
    return R.to64(W), R.to64(I), R.to64(G), k64(Kf), k64(Kb), pres


def _check_observe(d, W, I, G, Kf, Kb, min_std=0.1, report=None):
    R.check_layers(R.observe_fwd_layers(d, W, I, Kf, min_std), Kf, report)
    R.check_layers(R.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G, min_std), Kb, report)


@pytest.mark.parametrize("name", list(R.OBSERVE_SHAPES))
def test_fp32_emulation_of_observe_passes(name):
    d = R.OBSERVE_SHAPES[name][0]
    for seed, ms, nt, dpm, dps in ((1, 0.1, "zeros", True, True), (2, 0.25, "none", False, True), (3, 0.1, "ones", True, False)):
        W, I, G, Kf, Kb, pres = _observe_emulated(d, seed, ms, nt, dpm=dpm, dps=dps)
        rep = {}
        _check_observe(d, W, I, G, Kf, Kb, ms, rep)
        assert max(rep.values()) < 1.0
        frac = R.near_decision_fraction([p.double() for k in ("pre_e", "q1") for p in pres[k]])
        assert frac <= 1e-3, frac


def _imagine_emulated(d, seed, dent=-0.37, ent_weight=True, fault=None, with_us=True, with_mean=True):
    W, I = R.make_weights(d, seed, imagine=True), R.make_imagine_inputs(d, seed)
    G = R.make_imagine_grads(d, seed, ent_weight=ent_weight)
    with torch.no_grad():
        Kf, pres = emu_imagine_fwd(d, W, I, 0.1, torch.float32, with_us, with_mean)
        full, _ = emu_imagine_fwd(d, W, I, 0.1, torch.float32)
        Kb = emu_imagine_bwd(d, W, imagine_bwd_inputs(I, full, G), G, dent, 0.1, torch.float32, fault)
    return R.to64(W), R.to64(I), R.to64(G), k64(Kf), k64(Kb), k64(full), pres


@pytest.mark.parametrize("name", list(R.IMAGINE_SHAPES))
def test_fp32_emulation_of_imagine_passes(name):
    d = R.IMAGINE_SHAPES[name]
    for seed, ew, us, mean in ((1, True, True, True), (2, False, False, False)):
        W, I, G, Kf, Kb, full, pres = _imagine_emulated(d, seed, ent_weight=ew, with_us=us, with_mean=mean)
        rep = {}
        R.check_layers(R.imagine_fwd_layers(d, W, I, Kf, 0.1), Kf, rep)
        R.check_layers(R.imagine_bwd_layers(d, W, imagine_bwd_inputs(I, full, G), Kb, G, -0.37, 0.1), Kb, rep)
        assert max(rep.values()) < 1.0
        assert R.near_decision_fraction([p.double() for l in range(4) for p in pres[f"a{l}"]]) <= 1e-3


# ---- planted faults fail ------------------------------------------------------------------------------------------------

FAULT_SHAPE = R.Dims(4, 19, 42, 10, 3, 30)     # ragged Be, Hd and S, a partly filled second tile


@pytest.mark.parametrize("fault", ["fwd_mask_dropped", "zero_last_row", "drop_col_be", "drop_col_hd", "drop_col_s", "no_bhn",
                                   "eps_wrong_step"])
def test_planted_forward_fault_fails(fault):
    W, I, G, Kf, Kb, _ = _observe_emulated(FAULT_SHAPE, 1, fwd_fault=fault)
    with pytest.raises(AssertionError):
        R.check_layers(R.observe_fwd_layers(FAULT_SHAPE, W, I, Kf, 0.1), Kf)


@pytest.mark.parametrize("fault", ["mask_step", "hprev_t", "no_init", "bwd_zero_last_row", "bwd_drop_col", "dps_after",
                                   "bwd_eps_step", "no_min_std"])
def test_planted_backward_fault_fails(fault):
    d = FAULT_SHAPE
    W, I, G, Kf, Kb, _ = _observe_emulated(d, 1, bwd_fault=fault)
    R.check_layers(R.observe_fwd_layers(d, W, I, Kf, 0.1), Kf)
    with pytest.raises(AssertionError):
        R.check_layers(R.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G, 0.1), Kb)


@pytest.mark.parametrize("fault", ["no_tanh_grad", "no_ent_weight"])
def test_planted_imagine_fault_fails(fault):
    d = R.Dims(3, 19, 42, 10, 3, 30)
    W, I, G, Kf, Kb, full, _ = _imagine_emulated(d, 1, fault=fault)
    with pytest.raises(AssertionError):
        R.check_layers(R.imagine_bwd_layers(d, W, imagine_bwd_inputs(I, full, G), Kb, G, -0.37, 0.1), Kb)


# ---- the Categorical actor (discrete_actions = 1) in the Gaussian-latent imagination scan -----------------------------------

def share_ok(amb, n):
    return amb <= 1e-3 * n


def _discrete_emulated(d, seed, variant, ew=True, fault=None):
    W, I, sat, dup = R.make_discrete_case(d, seed, variant)
    G = R.make_imagine_grads(d, seed, ent_weight=ew)
    with torch.no_grad():
        Kf, pres = emu_imagine_fwd(d, W, I, 0.1, torch.float32, discrete=True, fault=fault)
        Kb = emu_imagine_bwd(d, W, dict(I, **Kf), G, -0.37, 0.1, torch.float32, fault, discrete=True)
    return R.to64(W), R.to64(I), R.to64(G), k64(Kf), k64(Kb), sat, dup, pres


def _check_discrete(d, W, I, G, Kf, Kb, sat, dup, rep=None):
    """Every check the GPU test makes of a case; returns (ambiguous draws, draws, times the planted pair won)."""
    R.check_layers(R.imagine_fwd_layers(d, W, I, Kf, 0.1, discrete=True, sat=sat), Kf, rep)
    counts = RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"], sat, dup)
    R.check_layers(R.imagine_bwd_layers(d, W, dict(I, **Kf), Kb, G, -0.37, 0.1, discrete=True, sat=sat), Kb, rep)
    if sat is not None:
        assert R.saturated_exact(d, Kf, Kb, sat) > 0
    return counts


@pytest.mark.parametrize("name,variant", R.discrete_cases(R.DISCRETE_SHAPES))
def test_fp32_emulation_of_the_discrete_actor_passes(name, variant):
    """Every GPU case of the Categorical actor: the fp32 emulation passes every bound, the margin of every draw and the
    exact statements of the saturated rows; its ambiguous share is within the cap; the planted pair wins somewhere."""
    d = R.DISCRETE_SHAPES[name]
    for ew in (True, False):
        W, I, G, Kf, Kb, sat, dup, pres = _discrete_emulated(d, R.SEEDS[2], variant, ew)
        rep = {}
        amb, n, won = _check_discrete(d, W, I, G, Kf, Kb, sat, dup, rep)
        assert max(rep.values()) < 1.0, rep
        # (one class: every gradient is exactly zero under a zero bound, which the report does not list)
        assert set(rep) >= ({"sv_act_stats", "action", "entropy", "d_actor_out", "d_actor_pre0", "d_actor_pre3"} if d.A > 1 else {"action"}), rep
        assert share_ok(amb, n) and n == d.T * (d.B if sat is None else int((~sat).sum())), (amb, n)
        assert won is None or won > 0, "the planted pair never won: the case checks nothing"
        assert R.near_decision_fraction([p.double() for l in range(4) for p in pres[f"a{l}"]]) <= 1e-3


@pytest.mark.parametrize("variant", ["regular", "peaked", "saturated"])
def test_discrete_actor_reference_equals_autograd(monkeypatch, variant):
    """The chained float64 reference of the Categorical actor in the Gaussian-latent scan equals the float64 emulation
    (tests/discrete_oracle.discrete_head) and autograd through it, d_actor_pre0..3 included (1e-10)."""
    monkeypatch.setattr(R, "f32", lambda x: x)
    d = R.Dims(4, 6, 22, 6, 5, 19)
    for ew in (True, False):
        W, I, sat, _ = R.make_discrete_case(d, 4, variant)
        W, I, G = R.to64(W), R.to64(I), R.to64(R.make_imagine_grads(d, 4, ent_weight=ew))
        Kc = R.empty_set(R.img_fwd_tensors(d, True), d)
        R.fill_layers(R.imagine_fwd_layers(d, W, I, Kc, 0.1, discrete=True, chain=True, sat=sat), Kc)
        Ke, pres = emu_imagine_fwd(d, _leaves(W), I, 0.1, D64, discrete=True)
        for k in Kc:
            rel_close(Ke[k], Kc[k])
        w = G["ent_weight"][:, :, None] if ew else 1.0
        loss = (Ke["feat"] * G["dfeat"]).sum() + (-0.37 * w * Ke["entropy"]).sum()
        grads = torch.autograd.grad(loss, [p for k in ("out", "a0", "a1", "a2", "a3") for p in pres[k]])
        ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in
              enumerate(("d_actor_out", "d_actor_pre0", "d_actor_pre1", "d_actor_pre2", "d_actor_pre3"))}
        Kb = R.empty_set({"d_actor_out": d.A, **{f"d_actor_pre{l}": d.Hd for l in range(4)}}, d)
        R.fill_layers(R.imagine_bwd_layers(d, W, dict(I, **Kc), Kb, G, -0.37, 0.1, discrete=True, sat=sat), Kb)
        for k in Kb:
            rel_close(Kb[k], ag[k][..., :d.A] if k == "d_actor_out" else ag[k])
        if variant == "peaked":
            assert float(Kc["entropy"].mean()) < 0.75 * float(torch.log(torch.tensor(float(d.A))))


# fault -> (shape, variant) at which the reference's checks must see it.  no_max sits at `saturated`, not `peaked`: expf
# overflows above 88.7 and the peaked logits stay below 16 (exp(out) without the maximum is then the same number to
# rounding and passes every bound, as it should), while the saturated rows' leading logit is near 180: inf - inf.
DISCRETE_FAULTS = {"ent_dropped": ("a17", "regular"),         # the entropy term of d_actor_out dropped
                   "ent_sign": ("a17", "peaked"),             # dentropy with the wrong sign
                   "cols16_dropped": ("a17", "regular"),      # classes >= 16 of the logits image never written
                   "lane63_invalid": ("a64", "regular"),      # lane 63 treated as invalid
                   "no_max": ("a64", "saturated"),            # the maximum not subtracted before the exponential
                   "af16_dropped": ("a17", "regular")}        # action fragment columns >= 16 not fed to the embed layer


@pytest.mark.parametrize("fault", list(DISCRETE_FAULTS))
def test_planted_discrete_actor_fault_fails(fault):
    name, variant = DISCRETE_FAULTS[fault]
    d = R.DISCRETE_SHAPES[name]
    W, I, G, Kf, Kb, sat, dup, _ = _discrete_emulated(d, R.SEEDS[2], variant, fault=fault)
    with pytest.raises(AssertionError):
        _check_discrete(d, W, I, G, Kf, Kb, sat, dup)


@pytest.mark.parametrize("name", ["a17", "a64"])
def test_planted_last_maximum_fails_the_actor_duplicate_check(name):
    """`>=` for `>` in disc_sample: invisible to the margin (the two classes tie), caught by the duplicate-class case."""
    d = R.DISCRETE_SHAPES[name]
    W, I, G, Kf, Kb, sat, dup, _ = _discrete_emulated(d, R.SEEDS[2], "duplicate", fault="sampler_ge")
    R.check_layers(R.imagine_fwd_layers(d, W, I, Kf, 0.1, discrete=True), Kf)
    RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"])       # the margin alone does not see it
    with pytest.raises(AssertionError):
        RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"], dup=dup)


@pytest.mark.parametrize("name,variant", R.discrete_cases(R.DISCRETE_SHAPES))
def test_ambiguous_share_of_the_float64_reference(name, variant):
    """On the chained float64 reference alone: at most 0.1 % of the actor's draws have a runner-up within the margin of
    the best, for every case of the Categorical actor and every seed, under both margins."""
    d = R.DISCRETE_SHAPES[name]
    for seed in R.SEEDS:
        W, I, sat, dup = R.make_discrete_case(d, seed, variant)
        W, I = R.to64(W), R.to64(I)
        K = R.empty_set(R.img_fwd_tensors(d, True), d)
        R.fill_layers(R.imagine_fwd_layers(d, W, I, K, 0.1, discrete=True, chain=True, sat=sat), K)
        for path in ("hw", "libm"):
            amb, n, won = RC.actor_checks(d, K["sv_act_stats"], I["eps_action"], K["action"], sat, dup, path=path)
            assert share_ok(amb, n) and n > 0, (name, variant, seed, path, amb, n)
            assert won is None or won > 0


def test_discrete_actor_shapes_fit_and_the_lds_mirror_matches_the_refusal():
    """With the Categorical actor the forward keeps one of its four action regions (bd_scan_layout.h ImagineFwdLds), which
    is what lets A = 64 run at all; bd_scan_lds_bytes describes the tanh-Normal layout, so the mirror's discrete figure is
    held to the "needs N B of LDS" refusal of shapes above 160 KiB."""
    import re
    from big_dreamer_amd import _cabi as cabi
    for name, d in R.DISCRETE_SHAPES.items():
        assert R.lds_bytes("imagine_fwd", d.Be, d.S, d.A, d.Hd, discrete=True) <= R.K_MAX_LDS, name
        assert R.lds_bytes("imagine_bwd", d.Be, d.S, d.A, d.Hd) <= R.K_MAX_LDS, name
    d = R.DISCRETE_SHAPES["a64"]
    assert R.lds_bytes("imagine_fwd", d.Be, d.S, d.A, d.Hd) > R.K_MAX_LDS      # the tanh-Normal actor does not fit there
    for Be, S, A, Hd in ((1000, 30, 64, 200), (1200, 10, 17, 32)):
        for disc in (0, 1):
            f = _fake_imagine_fwd(cabi, N=20, Hm=2, Be=Be, S=S, A=A, Hd=Hd, discrete_actions=disc)
            want = R.lds_bytes("imagine_fwd", Be, S, A, Hd, discrete=bool(disc))
            assert want > R.K_MAX_LDS and cabi.lib.bd_imagine_forward_scan(C.byref(f), None) != 0
            m = re.search(rb"needs (\d+) B of LDS", cabi.lib.bd_last_error())
            assert m and int(m.group(1)) == want, (Be, S, A, Hd, disc, cabi.lib.bd_last_error(), want)


# ---- host checks (no launch) --------------------------------------------------------------------------------------------

def _fake_imagine_fwd(cabi, **dims):
    f = _fake_ptrs(cabi.ImagineFwdArgs(), ("sv_act_us",) if dims.get("discrete_actions") else ())
    f.n_samples = 1
    for k, v in dims.items():
        setattr(f, k, v)
    for i in range(3):
        f.w_a[i] = 4096
    for i in range(4):
        f.b_a[i] = 4096
    return f


def test_dispatch_tables_match_the_library():
    from big_dreamer_amd import _cabi as cabi
    for B in (1, 15, 16, 17, 50, 64, 320, 2450, 5000):
        for Be in (16, 40, 42, 46, 48, 200, 256, 257, 300, 600):
            assert cabi.lib.bd_observe_cluster_size(B, Be) == R.pick_cluster(B, Be), (B, Be)
    def lib_lds(kernel, d, **kw):          # the library's own figure: the total of the layout kernel and launcher share
        dims = dict(dict(Be=d.Be, S=d.S, D=0, C=0, A=d.A, Hd=d.Hd, Cm=0), **kw)
        return cabi.lib.bd_scan_lds_bytes(cabi.SCAN_KERNELS[kernel], *(dims[k] for k in ("Be", "S", "D", "C", "A", "Hd", "Cm")))

    for name, (d, Cn, form) in R.OBSERVE_SHAPES.items():
        assert R.pick_cluster(d.B, d.Be) == Cn, name
        for kernel, entry in (("observe_fwd", "observe_fwd"), ("observe_bwd", "observe_bwd"), ("observe_cfwd", "cluster_fwd"),
                              ("observe_cbwd", "cluster_bwd")) + ((("observe_kfwd", "ksplit_fwd"), ("observe_kbwd", "ksplit_bwd"))
                                                                  if form == "ksplit" else ()):
            assert lib_lds(kernel, d) == R.lds_bytes(entry, d.Be, d.S, d.A, d.Hd), (name, kernel)
        forms = R.observe_forms(d.B, d.Be, d.S, d.A, d.Hd)
        assert (forms[1] if len(forms) > 1 else None) == form, (name, forms)
        tiles = R.cdiv(d.B, 16)
        assert tiles * Cn <= R.ENGINE_MAX_WGS or name == "b320", name      # the engine's cap; b320 is the stated exception
        if name == "b320":
            assert tiles * Cn == 140 and R.cdiv(R.cdiv(d.Be, 16), Cn) == 2
        for entry in ("observe_fwd", "observe_bwd"):
            lds = R.lds_bytes(entry, d.Be, d.S, d.A, d.Hd)
            assert lds <= R.K_MAX_LDS, (name, entry, lds)
            assert (lds > 64 * 1024) == (name in R.OBSERVE_BIG_LDS[entry]), (name, entry, lds)
        if Cn and form:
            for entry in ("cluster_fwd", "cluster_bwd"):
                assert R.lds_bytes(entry, d.Be, d.S, d.A, d.Hd) <= R.K_MAX_LDS, (name, entry)
    for entry, big in list(R.OBSERVE_BIG_LDS.items()) + list(R.IMAGINE_BIG_LDS.items()):
        table = R.OBSERVE_SHAPES if entry.startswith("observe") else R.IMAGINE_SHAPES
        assert big and set(table) - big, entry             # a shape on each side of the 64 KiB line
    for name, d in R.IMAGINE_SHAPES.items():
        for entry in ("imagine_fwd", "imagine_bwd"):
            lds = R.lds_bytes(entry, d.Be, d.S, d.A, d.Hd)
            assert lds <= R.K_MAX_LDS and (lds > 64 * 1024) == (name in R.IMAGINE_BIG_LDS[entry]), (name, entry, lds)
            assert lib_lds(entry, d) == lds, (name, entry)
    forms = {f for d, _, _ in R.OBSERVE_SHAPES.values() for f in R.observe_forms(d.B, d.Be, d.S, d.A, d.Hd)}
    assert forms == {"single", "ksplit", "round1"}
    # the query rejects what it cannot describe, with the reason
    d = R.OBSERVE_SHAPES["b16"][0]
    assert cabi.lib.bd_scan_lds_bytes(len(cabi.SCAN_KERNELS), d.Be, d.S, 0, 0, d.A, d.Hd, 0) == 0
    assert b"unknown kernel" in cabi.lib.bd_last_error()
    assert cabi.lib.bd_scan_lds_bytes(-1, d.Be, d.S, 0, 0, d.A, d.Hd, 0) == 0 and b"unknown kernel" in cabi.lib.bd_last_error()
    assert lib_lds("observe_fwd", d, S=0) == 0 and b"bad dims" in cabi.lib.bd_last_error()


def _fake_ptrs(args, skip=()):
    for name, typ in args._fields_:
        if typ is C.c_void_p and name not in skip:
            setattr(args, name, 4096)
    return args


def test_rejecting_paths_return_without_a_launch():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib

    def fwd(S=10, **kw):
        a = _fake_ptrs(cabi.ObserveFwdArgs(), kw.pop("null", ()))
        a.T, a.B, a.Be, a.S, a.A, a.Hd = 2, 20, 40, S, 3, 32
        return a

    def bwd(**kw):
        b = _fake_ptrs(cabi.ObserveBwdArgs(), kw.pop("null", ()))
        b.T, b.B, b.Be, b.S, b.A, b.Hd = 2, 20, 40, 10, 3, 32
        return b

    need = lib.bd_observe_cluster_ws_floats(20, 40)
    assert need > 0
    # S > 64 on the cluster entry point
    assert lib.bd_observe_forward_cluster(C.byref(fwd(S=65)), 4096, need, None) != 0
    assert b"state width" in lib.bd_last_error()
    # a workspace that is too small, a missing workspace
    assert lib.bd_observe_forward_cluster(C.byref(fwd()), 4096, need - 1, None) != 0
    assert b"workspace too small" in lib.bd_last_error()
    assert lib.bd_observe_backward_cluster(C.byref(bwd()), 4096, need - 1, None) != 0
    assert b"workspace too small" in lib.bd_last_error()
    assert lib.bd_observe_forward_cluster(C.byref(fwd()), None, need, None) != 0
    # a shape without a cluster
    a = fwd(); a.Be = 300
    assert lib.bd_observe_cluster_size(20, 300) == 0 and lib.bd_observe_forward_cluster(C.byref(a), 4096, 1 << 24, None) != 0
    assert b"do not fit" in lib.bd_last_error()
    # NULL required pointers, every entry point
    for null in ("w_hn", "init_state", "eps_post", "post_std"):
        assert lib.bd_observe_forward(C.byref(fwd(null=(null,))), None) != 0, null
        assert lib.bd_observe_forward_cluster(C.byref(fwd(null=(null,))), 4096, need, None) != 0, null
    for null in ("wt_q2s", "sv_gates", "dfeat", "d_gh"):
        assert lib.bd_observe_backward(C.byref(bwd(null=(null,))), None) != 0, null
        assert lib.bd_observe_backward_cluster(C.byref(bwd(null=(null,))), 4096, need, None) != 0, null
    f = _fake_ptrs(cabi.ImagineFwdArgs())
    f.N, f.Hm, f.Be, f.S, f.A, f.Hd, f.n_samples = 17, 2, 40, 65, 3, 32, 1
    for i in range(3):
        f.w_a[i] = 4096
    for i in range(4):
        f.b_a[i] = 4096
    assert lib.bd_imagine_forward_scan(C.byref(f), None) != 0 and b"width above" in lib.bd_last_error()
    f.S, f.feat = 10, None
    assert lib.bd_imagine_forward_scan(C.byref(f), None) != 0 and b"missing outputs" in lib.bd_last_error()
    g = _fake_ptrs(cabi.ImagineBwdArgs(), ("d_actor_out",))
    g.N, g.Hm, g.Be, g.S, g.A, g.Hd = 17, 2, 40, 10, 3, 32
    for i in range(3):
        g.wt_a[i] = 4096
    assert lib.bd_imagine_backward(C.byref(g), None) != 0 and b"missing outputs" in lib.bd_last_error()
    # A = 65: one lane per class does not reach class 64; both entry points say so themselves, for either actor (without a GPU
    # every call fails: the message shows that this check came first)
    for disc in (0, 1):
        f = _fake_imagine_fwd(cabi, N=17, Hm=2, Be=40, S=10, A=65, Hd=32, discrete_actions=disc)
        assert lib.bd_imagine_forward_scan(C.byref(f), None) != 0 and b"action width above 64" in lib.bd_last_error(), lib.bd_last_error()
        assert lib.bd_imagine_forward(C.byref(f), None) != 0 and b"action width above 64" in lib.bd_last_error(), lib.bd_last_error()
        g = _fake_ptrs(cabi.ImagineBwdArgs(), ("d_actor_pre",) if disc else ())
        g.N, g.Hm, g.Be, g.S, g.A, g.Hd, g.discrete_actions = 17, 2, 40, 10, 65, 32, disc
        for i in range(3):
            g.wt_a[i] = 4096
        assert lib.bd_imagine_backward(C.byref(g), None) != 0 and b"action width 65 above 64" in lib.bd_last_error(), lib.bd_last_error()
    assert lib.bd_observe_cluster_set_ksplit(7) != 0 and b"set_ksplit" in lib.bd_last_error()
    assert lib.bd_observe_cluster_set_ksplit(-1) == 0


def test_engine_falls_back_to_the_single_form_above_64_state_columns():
    """bd_observe_forward_cluster rejects S > 64 while observe.hip takes it: DreamerEngine._cluster_ok must say no."""
    from big_dreamer_amd.engine import DreamerEngine
    stub = lambda S: types.SimpleNamespace(use_obs_cluster=True, d=types.SimpleNamespace(Be=40, S=S))
    assert DreamerEngine._cluster_ok(stub(64), 20) is True
    assert DreamerEngine._cluster_ok(stub(65), 20) is False
