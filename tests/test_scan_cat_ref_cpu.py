"""CPU tests of tests/scan_cat_ref.py: the per-step float64 references of the Categorical observe and imagination scans
chain to the oracle and to autograd (straight-through estimator as in the oracle); an fp32 emulation of the kernels' order
of operations passes every tolerance at every shape of the GPU tables with an ambiguous-sample share of at most 0.1 %;
planted faults fail at the shape named for them; the mirror of the host dispatch equals the library and the tables; the
rejecting paths return non-zero from host-side argument checks."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O
from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests import test_scan_ref_cpu as GC

D64 = torch.float64
_cast, _gru, _elug, _gate_bwd, k64, rel_close, _leaves = GC._cast, GC._gru, GC._elug, GC._gate_bwd, GC.k64, GC.rel_close, GC._leaves


# ---- an emulation of the kernels' order of operations in plain torch (any dtype; optional planted fault) ---------------

def _probs(l, D, C, dtype, path):
    """softmax per factor in the kernel's order: C == 32 one exponential and a reciprocal, otherwise the library's
    two-pass normalised form (bd_categorical.h)."""
    l = l.reshape(-1, D, C)
    m = l.max(-1, keepdim=True).values
    if dtype == D64:
        return torch.softmax(l, -1)
    if path == "hw":
        e = torch.exp(l - m)
        return e * (1 / e.sum(-1, keepdim=True))
    lse = m + torch.log(torch.exp(l - m).sum(-1, keepdim=True))
    e = torch.exp((l - lse) - (m - lse))
    return e * (1 / e.sum(-1, keepdim=True))


def _sample(l, q, D, C, dtype, path, fault=None):
    l, q = l.reshape(-1, D, C), q.reshape(-1, D, C)
    m = l.max(-1, keepdim=True).values
    if dtype == D64:
        r = torch.softmax(l, -1) / q
    elif path == "hw":
        r = torch.exp(l - m) * (1 / q)
    else:
        lse = m + torch.log(torch.exp(l - m).sum(-1, keepdim=True))
        e = torch.exp((l - lse) - (m - lse))
        r = (e / e.sum(-1, keepdim=True)) / q
    if fault == "sampler_ge":               # r >= best: the LAST maximum wins
        return C - 1 - r.flip(-1).argmax(-1)
    return r.argmax(-1)


def _hot(idx, C, dtype):
    return F.one_hot(idx, C).to(dtype).reshape(idx.shape[0], -1)


def _state_in(d, idx_hist, init, t, dtype, fault):
    """The dense state a layer of step t reads, from the indices of the steps before."""
    if t == 0:
        s = init
        if fault == "zero_as_class0":
            s = s.clone().reshape(-1, d.D, d.C)
            s[..., 0] += (s.abs().sum(-1) == 0).to(dtype)
            s = s.reshape(-1, d.S)
        return s
    idx = idx_hist[t - 2] if (fault == "stale_sidx" and t >= 2) else idx_hist[t - 1]
    if fault == "wrap128":                  # a signed byte read back with sign extension: the gather leaves the factor
        idx = torch.where(idx >= 128, idx - 128, idx)
    s = _hot(idx, d.C, dtype)
    if fault == "gather_rem" and d.D % 8:
        s = s.clone()
        s[:, (d.D - d.D % 8) * d.C:] = 0
    return s


def emu_observe_fwd(d, W, I, dtype, fault=None, exact=False, st=False):
    W, I = _cast(W, dtype), _cast(I, dtype)
    path = RC.sample_path(d.C, exact)
    h = I["init_belief"]
    K = {k: [] for k in list(RC.OBS_FWD_TENSORS) + ["sidx"]}
    pres = dict(pre_e=[], gi=[], gh=[], q1=[], out=[])
    state = None
    for t in range(d.T):
        s = _state_in(d, K["sidx"], I["init_state"], t, dtype, fault)
        if st and t:
            s = state                        # float64 autograd: the straight-through state carries the graph
        if I["nonterm"] is not None and fault != "fwd_nonterm":
            s = s * I["nonterm"][t][:, None]
        pre_e = torch.cat([s, I["actions"][t]], 1) @ W["W_e"].t() + W["b_e"]
        x = F.elu(pre_e)
        keep = []
        hn, gates = _gru(W, x, h, d.Be, None, keep)
        q1 = hn @ W["W_1"].t() + W["b_1"] + I["pre_emb"][t]
        q = F.elu(q1)
        out = q @ W["W_2"].t() + W["b_2"]
        idx = _sample(out.detach(), I["q_post"][t], d.D, d.C, dtype, path, fault)
        hot = _hot(idx, d.C, dtype)
        if st:
            p = torch.softmax(out.reshape(-1, d.D, d.C), -1).reshape(-1, d.S)
            state = hot + (p - p.detach())
        sv_s = s if fault not in ("gather_rem", "wrap128", "stale_sidx", "zero_as_class0") else (
            (_hot(K["sidx"][t - 1], d.C, dtype) if t else I["init_state"]) *
            (I["nonterm"][t][:, None] if I["nonterm"] is not None else 1))
        for k, v in dict(feat=torch.cat([hn, state if st else hot], 1), post_logits=out, sv_s=sv_s, sv_x=x, sv_gates=gates,
                         sv_q=q, sidx=idx).items():
            K[k].append(v)
        for k, v in dict(pre_e=pre_e, gi=keep[0], gh=keep[1], q1=q1, out=out).items():
            pres[k].append(v)
        h = hn
    return {k: torch.stack(v) for k, v in K.items()}, pres


def emu_observe_bwd(d, W, I, G, dtype, fault=None, exact=False):
    W, I, G = _cast(W, dtype), _cast(I, dtype), _cast(G, dtype)
    path = RC.sample_path(d.C, exact)
    Be, S_ = d.Be, d.S
    geo = RC.cat_geo(d.D, d.C)
    K = {k: [None] * d.T for k in RC.OBS_BWD_TENSORS}
    dhc, ds = torch.zeros(d.B, Be, dtype=dtype), torch.zeros(d.B, S_, dtype=dtype)
    W2 = W["W_2"]
    if fault == "chunk1_w2":                # chunk 1 contracts with chunk 0's rows of W_2
        W2 = W2.clone()
        n = min(256, S_ - 256)
        W2[256:256 + n] = W["W_2"][:n]
    for t in reversed(range(d.T)):
        g = (ds + G["dfeat"][t][:, Be:]).reshape(-1, d.D, d.C)
        p = _probs(I["post_logits"][t], d.D, d.C, dtype, path)
        dot = (p * g).sum(-1, keepdim=True)
        v = (p * (1 - dot) if fault == "jac_one_minus" else p * (g - dot)).reshape(-1, S_)
        d2 = v + G["dpost_logits"][t] if (G["dpost_logits"] is not None and fault != "dpl_ignored") else v
        dl = d2
        if fault == "last_chunk_skipped":   # the factors of the last, partial chunk never reach d hidden
            dl = d2.clone()
            dl[:, (geo.NCH - 1) * geo.CW:] = 0
        dq = (dl @ W2) * _elug(I["sv_q"][t])
        dh = dq @ W["W_1"] + dhc + G["dfeat"][t][:, :Be]
        hprev = I["feat"][t - 1][:, :Be] if t else I["init_belief"]
        dgi, dgh, carry = _gate_bwd(dh, I["sv_gates"][t], hprev, Be)
        de = (dgi @ W["W_ih"]) * _elug(I["sv_x"][t])
        dhc = carry + dgh @ W["W_hh"]
        ds = de @ W["W_e"][:, :S_]
        if I["nonterm"] is not None and fault != "bwd_nonterm":
            ds = ds * I["nonterm"][t][:, None]
        for k, val in dict(d_embed_pre=de, d_gi=dgi, d_gh=dgh, d_q1_pre=dq, d_q2_out=d2).items():
            K[k][t] = val
    return {k: torch.stack(v) for k, v in K.items()}


def emu_imagine_fwd(d, W, I, dtype, fault=None, exact=False, st=False, discrete=False):
    W, I = _cast(W, dtype), _cast(I, dtype)
    path = RC.sample_path(d.C, exact)
    f64 = dtype == D64
    init, amin, scale = [(v if f64 else R.f32(v)) for v in (R.ACT_RAW_INIT_STD, R.ACT_MIN_STD, R.ACT_MEAN_SCALE)]
    Be, A = d.Be, d.A
    h, s = I["start_feat"][:, :Be], I["start_feat"][:, Be:]
    names = list(RC.img_fwd_tensors(d, discrete)) + ["sidx"]
    K = {k: [] for k in names}
    pres = {f"a{l}": [] for l in range(4)}
    pres.update(out=[], mean=[], std=[])
    for t in range(d.T):
        x = torch.cat([h, 0 * s if fault == "actor_gather" else s], 1).detach()
        step = {}
        for l in range(4):
            pre = x @ (W["W_a0"] if l == 0 else W["W_a"][l - 1]).t() + W["b_a"][l]
            pres[f"a{l}"].append(pre)
            x = F.elu(pre)
            step[f"sv_actor{l}"] = x
        out = x @ W["W_a4"].t() + W["b_a4"]
        if discrete:         # the Categorical actor as tests/discrete_oracle.py states it (or with a planted fault)
            out = out[:, :A]
            a, ent, norm, ae = GC.emu_discrete_head(out, I["eps_action"][t], fault)
            step.update(sv_act_stats=norm, entropy=ent)
            th = mean = pre_s = sd = u = out
        else:
            th = torch.tanh(out[:, :A] / scale)
            mean = scale * th
            pre_s = out[:, A:] + init
            sd = F.softplus(pre_s) + amin
            u = mean + sd * I["eps_action"][t]
            a = ae = torch.tanh(u)
        xe = F.elu(torch.cat([s, ae], 1) @ W["W_e"].t() + W["b_e"])
        hn, gates = _gru(W, xe, h, Be, None, [])
        pp = F.elu(hn @ W["W_1"].t() + W["b_1"])
        lg = pp @ W["W_2"].t() + W["b_2"]
        idx = _sample(lg.detach(), I["q_prior"][t], d.D, d.C, dtype, path)
        hot = _hot(idx, d.C, dtype)
        if st:
            p = torch.softmax(lg.reshape(-1, d.D, d.C), -1).reshape(-1, d.S)
            hot = hot + (p - p.detach())
        h, s = hn, hot
        step.update(feat=torch.cat([hn, hot], 1), prior_logits=lg, action=a, sv_x=xe, sv_gates=gates, sv_p=pp, sidx=idx)
        if not discrete:
            step.update(sv_act_stats=torch.cat([th, torch.sigmoid(pre_s), mean, sd], 1), sv_act_us=torch.cat([u, sd], 1))
        for k in names:
            K[k].append(step[k])
        for k, v in dict(out=out, mean=mean, std=sd).items():
            pres[k].append(v)
    return {k: torch.stack(v) for k, v in K.items()}, pres


def emu_imagine_bwd(d, W, I, G, dentropy, dtype, exact=False, discrete=False, fault=None):
    W, I, G = _cast(W, dtype), _cast(I, dtype), _cast(G, dtype)
    path = RC.sample_path(d.C, exact)
    dent0 = dentropy if dtype == D64 else R.f32(dentropy)
    Be, S_, A = d.Be, d.S, d.A
    K = {"d_actor_out": [None] * d.T, **{f"d_actor_pre{l}": [None] * d.T for l in range(4)}}
    dhc, ds = torch.zeros(d.B, Be, dtype=dtype), torch.zeros(d.B, S_, dtype=dtype)
    for t in reversed(range(d.T)):
        g = (ds + G["dfeat"][t][:, Be:]).reshape(-1, d.D, d.C)
        p = _probs(I["prior_logits"][t], d.D, d.C, dtype, path)
        dl = (p * (g - (p * g).sum(-1, keepdim=True))).reshape(-1, S_)
        dP = (dl @ W["W_2"]) * _elug(I["sv_p"][t])
        dh = dP @ W["W_1"] + dhc + G["dfeat"][t][:, :Be]
        fprev = I["feat"][t - 1] if t else I["start_feat"]
        dgi, dgh, carry = _gate_bwd(dh, I["sv_gates"][t], fprev[:, :Be], Be)
        dhc = carry + dgh @ W["W_hh"]
        dE = (dgi @ W["W_ih"]) * _elug(I["sv_x"][t])
        ds = dE @ W["W_e"][:, :S_]
        dA = dE @ W["W_e"][:, S_:]
        st, act = I["sv_act_stats"][t], I["action"][t]
        dent = dent0 * G["ent_weight"][t][:, None] if G["ent_weight"] is not None else dent0
        if discrete:        # the hidden layers below: the caller's bd_mlp_backward from d_actor_out through W_a4's A logit rows
            dn, Wn = GC.emu_discrete_grad(st, dA, dent, fault), W["W_a4"][:A]
        else:
            dxa = dA * (1 - act * act)
            dmean = dxa + dent * st[:, 2 * A:3 * A]
            dstd = dxa * I["eps_action"][t] + dent * st[:, 3 * A:]
            dn, Wn = torch.cat([dmean * (1 - st[:, :A] ** 2), dstd * st[:, A:2 * A]], 1), W["W_a4"]
        K["d_actor_out"][t] = dn
        for l in (3, 2, 1, 0):
            dn = (dn @ Wn) * _elug(I[f"sv_actor{l}"][t])
            K[f"d_actor_pre{l}"][t] = dn
            Wn = W["W_a"][l - 1] if l else None
    return {k: torch.stack(v) for k, v in K.items() if v[0] is not None}


# ---- helpers ------------------------------------------------------------------------------------------------------------

def k64i(K):
    return {k: (v.clone() if v.dtype == torch.long else v.double().clone()) for k, v in K.items()}


def observe_bwd_inputs(I, Kf):
    return dict(I, **{k: Kf[k] for k in ("feat", "post_logits", "sv_x", "sv_gates", "sv_q")})


imagine_bwd_inputs = GC.imagine_bwd_inputs


def share_ok(amb, n):
    return amb <= 1e-3 * n


# ---- the reference chains to the oracle and to autograd (float64 against float64) -----------------------------------------

@pytest.mark.parametrize("nonterm,init", [("zeros", "mixed"), ("none", "onehot"), ("ones", "zeros")])
def test_observe_reference_equals_oracle_and_autograd(monkeypatch, nonterm, init):
    monkeypatch.setattr(R, "f32", lambda x: x)
    d = RC.CDims(5, 7, 22, 3, 5, 3, 19)
    W = R.to64(RC.make_weights(d, 3))
    I = R.to64(RC.make_observe_inputs(d, 3, nonterm=nonterm, init=init))
    sd, W_emb = GC.oracle_sd(W, d, E=4)
    emb = torch.randn(d.T, d.B, 4, dtype=D64, generator=torch.Generator().manual_seed(9))
    I["pre_emb"] = emb @ W_emb.t()
    G = R.to64(RC.make_observe_grads(d, 3))
    Kf = RC.empty_set(RC.OBS_FWD_TENSORS, d)
    R.fill_layers(RC.observe_fwd_layers(d, W, I, Kf, chain=True), Kf)
    nt = I["nonterm"][:, :, None] if I["nonterm"] is not None else None
    bel, _, _, post, (ql,) = O.transition_forward(sd, I["init_state"], I["actions"], I["init_belief"], emb, nt,
                                                  torch.ones(d.T, d.B, d.S, dtype=D64), I["q_post"], (d.D, d.C))
    rel_close(Kf["feat"][..., :d.Be], bel)
    assert torch.equal(Kf["feat"][..., d.Be:], post.detach()), "chained one-hot states differ from the oracle's"
    rel_close(Kf["post_logits"], ql.reshape(d.T, d.B, d.S))
    # the emulation in float64 (straight-through state, as the oracle writes it) is the oracle's function too
    Ke, pres = emu_observe_fwd(d, _leaves(W), I, D64, st=True)
    for k in Kf:
        if k == "sidx":
            assert torch.equal(Ke[k], Kf[k])
        else:
            rel_close(Ke[k], Kf[k])
    loss = (Ke["feat"] * G["dfeat"]).sum() + (Ke["post_logits"] * G["dpost_logits"]).sum()
    flat = [p for k in ("pre_e", "gi", "gh", "q1", "out") for p in pres[k]]
    grads = torch.autograd.grad(loss, flat)
    ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in enumerate(("d_embed_pre", "d_gi", "d_gh", "d_q1_pre", "d_q2_out"))}
    Kb = R.empty_set(RC.OBS_BWD_TENSORS, d)
    R.fill_layers(RC.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G), Kb)
    for k in Kb:
        rel_close(Kb[k], ag[k].detach())


@pytest.mark.parametrize("ent_weight,start", [(True, "mixed"), (False, "onehot")])
def test_imagine_reference_equals_oracle_and_autograd(monkeypatch, ent_weight, start):
    monkeypatch.setattr(R, "f32", lambda x: x)
    d = RC.CDims(4, 5, 22, 3, 5, 3, 19)
    W = R.to64(RC.make_weights(d, 4, imagine=True))
    I = R.to64(RC.make_imagine_inputs(d, 4, start=start))
    G = R.to64(RC.make_imagine_grads(d, 4, ent_weight=ent_weight))
    Kf = RC.empty_set(RC.img_fwd_tensors(d), d)
    R.fill_layers(RC.imagine_fwd_layers(d, W, I, Kf, chain=True), Kf)
    sd, _ = GC.oracle_sd(W, d)
    actor = {"model.0.weight": W["W_a0"], "model.8.weight": W["W_a4"], "model.8.bias": W["b_a4"]}
    actor.update({f"model.{2 * l}.weight": W["W_a"][l - 1] for l in (1, 2, 3)})
    actor.update({f"model.{2 * l}.bias": W["b_a"][l] for l in range(4)})
    sf = I["start_feat"]
    bel, sts, (pl,), _ent = O.imagine_ahead({"transition_model": sd, "actor": actor}, sf[:, d.Be:], sf[:, :d.Be], d.T + 1,
                                            I["eps_action"], torch.zeros(d.T, 1, d.B, d.A, dtype=D64), I["q_prior"], (d.D, d.C))
    rel_close(Kf["feat"][..., :d.Be], bel)
    assert torch.equal(Kf["feat"][..., d.Be:], sts.detach())
    rel_close(Kf["prior_logits"], pl.reshape(d.T, d.B, d.S))
    Ke, pres = emu_imagine_fwd(d, _leaves(W), I, D64, st=True)
    for k in Kf:
        if k == "sidx":
            assert torch.equal(Ke[k], Kf[k])
        else:
            rel_close(Ke[k], Kf[k])
    dent = -0.37
    w = G["ent_weight"][:, :, None] if ent_weight else 1.0
    loss = (Ke["feat"] * G["dfeat"]).sum() + (dent * w * (torch.stack(pres["mean"]) * G["slot2"] + torch.stack(pres["std"]) * G["slot3"])).sum()
    flat = [p for k in ("out", "a0", "a1", "a2", "a3") for p in pres[k]]
    grads = torch.autograd.grad(loss, flat)
    ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in
          enumerate(("d_actor_out", "d_actor_pre0", "d_actor_pre1", "d_actor_pre2", "d_actor_pre3"))}
    Kb = R.empty_set({"d_actor_out": 2 * d.A, **{f"d_actor_pre{l}": d.Hd for l in range(4)}}, d)
    R.fill_layers(RC.imagine_bwd_layers(d, W, imagine_bwd_inputs(I, Kf, G), Kb, G, dent), Kb)
    for k in Kb:
        rel_close(Kb[k], ag[k].detach())


# ---- an fp32 emulation passes every tolerance at every shape of the GPU tables ------------------------------------------

def _observe_emulated(d, seed, nonterm="zeros", init="mixed", dpl=True, fwd_fault=None, bwd_fault=None, exact=False,
                      bias_high=False):
    W = RC.make_weights(d, seed, bias_high=bias_high)
    I, G = RC.make_observe_inputs(d, seed, nonterm=nonterm, init=init), RC.make_observe_grads(d, seed, dpl=dpl)
    with torch.no_grad():
        Kf, pres = emu_observe_fwd(d, W, I, torch.float32, fwd_fault, exact)
        Kb = emu_observe_bwd(d, W, observe_bwd_inputs(I, Kf), G, torch.float32, bwd_fault, exact)
    return R.to64(W), R.to64(I), R.to64(G), k64i(Kf), k64(Kb), pres


def _check_observe(d, W, I, G, Kf, Kb, report=None, AL=R.HW, exact=False):
    R.check_layers(RC.observe_fwd_layers(d, W, I, Kf, AL), Kf, report)
    amb = 0
    for t in range(d.T):
        amb += RC.sample_check(Kf["post_logits"][t], I["q_post"][t], Kf["sidx"][t], d.D, d.C, RC.sample_path(d.C, exact),
                               f"t={t} ")[0]
    R.check_layers(RC.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G, AL), Kb, report)
    return amb


@pytest.mark.parametrize("name", list(RC.OBSERVE_SHAPES))
def test_fp32_emulation_of_observe_passes(name):
    d = RC.OBSERVE_SHAPES[name][0]
    nt, init, dpl = RC.observe_variant(name)
    for seed in RC.SEEDS:
        for exact in (False, True):
            W, I, G, Kf, Kb, pres = _observe_emulated(d, seed, nt, init, dpl, exact=exact, bias_high=name == "c256_d2")
            rep = {}
            amb = _check_observe(d, W, I, G, Kf, Kb, rep, R.EXACT if exact else R.HW, exact)
            assert max(rep.values()) < 1.0, rep
            assert share_ok(amb, d.T * d.B * d.D), (name, seed, amb)
        assert R.near_decision_fraction([p.double() for k in ("pre_e", "q1") for p in pres[k]]) <= 1e-3
        if name == "c256_d2":
            assert int((Kf["sidx"] >= 128).sum()) > 0.5 * Kf["sidx"].numel()


def _imagine_emulated(d, seed, ent_weight=True, fault=None, start="mixed", exact=False, bias_high=False):
    W, I = RC.make_weights(d, seed, imagine=True, bias_high=bias_high), RC.make_imagine_inputs(d, seed, start=start)
    G = RC.make_imagine_grads(d, seed, ent_weight=ent_weight)
    with torch.no_grad():
        Kf, pres = emu_imagine_fwd(d, W, I, torch.float32, fault, exact)
        Kb = emu_imagine_bwd(d, W, imagine_bwd_inputs(I, Kf, G), G, -0.37, torch.float32, exact)
    return R.to64(W), R.to64(I), R.to64(G), k64i(Kf), k64(Kb), pres


def _check_imagine(d, W, I, G, Kf, Kb, report=None, AL=R.HW, exact=False):
    R.check_layers(RC.imagine_fwd_layers(d, W, I, Kf, AL), Kf, report)
    amb = sum(RC.sample_check(Kf["prior_logits"][t], I["q_prior"][t], Kf["sidx"][t], d.D, d.C, RC.sample_path(d.C, exact))[0]
              for t in range(d.T))
    R.check_layers(RC.imagine_bwd_layers(d, W, imagine_bwd_inputs(I, Kf, G), Kb, G, -0.37, AL), Kb, report)
    return amb


@pytest.mark.parametrize("name", list(RC.IMAGINE_SHAPES))
def test_fp32_emulation_of_imagine_passes(name):
    d = RC.IMAGINE_SHAPES[name]
    for seed, ew, start in ((RC.SEEDS[2], True, "mixed"), (23, False, "onehot")):
        W, I, G, Kf, Kb, pres = _imagine_emulated(d, seed, ew, start=start, bias_high=name == "c256_d2")
        rep = {}
        amb = _check_imagine(d, W, I, G, Kf, Kb, rep)
        assert max(rep.values()) < 1.0, rep
        assert share_ok(amb, d.T * d.B * d.D), (name, seed, amb)
        assert R.near_decision_fraction([p.double() for l in range(4) for p in pres[f"a{l}"]]) <= 1e-3


def test_discrete_actor_reference_equals_autograd_and_emulation_passes(monkeypatch):
    """discrete_actions = 1: the float64 chain equals autograd through tests/discrete_oracle.discrete_head (1e-10), and
    the fp32 emulation passes every bound at the GPU shape."""
    d = RC.IMAGINE_SHAPES["discrete"]
    for ew in (True, False):
        W, I = RC.make_weights(d, RC.SEEDS[2], imagine=True), RC.make_imagine_inputs(d, RC.SEEDS[2], start="mixed", discrete=True)
        G = RC.make_imagine_grads(d, RC.SEEDS[2], ent_weight=ew)
        with torch.no_grad():
            Kf, _ = emu_imagine_fwd(d, W, I, torch.float32, discrete=True)
            Kb = emu_imagine_bwd(d, W, dict(I, **Kf), G, -0.37, torch.float32, discrete=True)
        W6, I6, G6, Kf6, Kb6 = R.to64(W), R.to64(I), R.to64(G), k64i(Kf), k64(Kb)
        rep = {}
        R.check_layers(RC.imagine_fwd_layers(d, W6, I6, Kf6, discrete=True), Kf6, rep)
        for t in range(d.T):
            k = Kf6["action"][t].argmax(-1, keepdim=True)
            RC.sample_check(Kf6["sv_act_stats"][t], I6["eps_action"][t], k, 1, d.A, "libm")
        R.check_layers(RC.imagine_bwd_layers(d, W6, dict(I6, **Kf6), Kb6, G6, -0.37, actor_pre=False, discrete=True), Kb6, rep)
        assert max(rep.values()) < 1.0, rep
        with torch.no_grad():       # a fault the bound must see: the entropy term dropped
            bad = k64(emu_imagine_bwd(d, W, dict(I, **Kf), G, 0.0, torch.float32, discrete=True))
        with pytest.raises(AssertionError):
            R.check_layers(RC.imagine_bwd_layers(d, W6, dict(I6, **Kf6), bad, G6, -0.37, actor_pre=False, discrete=True), bad)
    monkeypatch.setattr(R, "f32", lambda x: x)
    Kc = RC.empty_set(RC.img_fwd_tensors(d, True), d)
    R.fill_layers(RC.imagine_fwd_layers(d, W6, I6, Kc, chain=True, discrete=True), Kc)
    Ke, pres = emu_imagine_fwd(d, _leaves(W6), I6, D64, st=True, discrete=True)
    for k in Kc:
        assert torch.equal(Ke[k], Kc[k]) if k == "sidx" else rel_close(Ke[k], Kc[k]) is None, k
    w = G6["ent_weight"][:, :, None] if G6["ent_weight"] is not None else 1.0
    loss = (Ke["feat"] * G6["dfeat"]).sum() + (-0.37 * w * Ke["entropy"]).sum()
    grads = torch.autograd.grad(loss, [p for k in ("out", "a0", "a1", "a2", "a3") for p in pres[k]])
    ag = {k: torch.stack(grads[i * d.T:(i + 1) * d.T]) for i, k in
          enumerate(("d_actor_out", "d_actor_pre0", "d_actor_pre1", "d_actor_pre2", "d_actor_pre3"))}
    Kb = R.empty_set({"d_actor_out": d.A, **{f"d_actor_pre{l}": d.Hd for l in range(4)}}, d)
    R.fill_layers(RC.imagine_bwd_layers(d, W6, dict(I6, **Kc), Kb, G6, -0.37, discrete=True), Kb)
    for k in Kb:        # d_actor_pre0..3: the chain the caller's bd_mlp_backward runs from d_actor_out
        rel_close(Kb[k], ag[k][..., :d.A] if k == "d_actor_out" else ag[k])


# ---- the Categorical actor at its own shapes and variants (scan_ref.DISCRETE_VARIANTS) -----------------------------------------

def _discrete_emulated(d, seed, variant, ew=True, fault=None, exact=False):
    W, I, sat, dup = RC.make_discrete_case(d, seed, variant)
    G = RC.make_imagine_grads(d, seed, ent_weight=ew)
    with torch.no_grad():
        Kf, pres = emu_imagine_fwd(d, W, I, torch.float32, fault, exact, discrete=True)
        Kb = emu_imagine_bwd(d, W, dict(I, **Kf), G, -0.37, torch.float32, exact, discrete=True, fault=fault)
    return R.to64(W), R.to64(I), R.to64(G), k64i(Kf), k64(Kb), sat, dup, pres


def _check_discrete(d, W, I, G, Kf, Kb, sat, dup, rep=None):
    """Every check the GPU test makes of a case; returns (ambiguous draws, draws, times the planted pair won), the prior's
    factors counted with the actor's draws."""
    R.check_layers(RC.imagine_fwd_layers(d, W, I, Kf, discrete=True, sat=sat), Kf, rep)
    amb, n, won = RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"], sat, dup)
    for t in range(d.T):
        a, m, _ = RC.sample_check(Kf["prior_logits"][t], I["q_prior"][t], Kf["sidx"][t], d.D, d.C, RC.sample_path(d.C))
        amb, n = amb + a, n + m
    R.check_layers(RC.imagine_bwd_layers(d, W, dict(I, **Kf), Kb, G, -0.37, discrete=True, sat=sat), Kb, rep)
    if sat is not None:
        assert R.saturated_exact(d, Kf, Kb, sat) > 0
    return amb, n, won


@pytest.mark.parametrize("name,variant", R.discrete_cases(RC.DISCRETE_SHAPES))
def test_fp32_emulation_of_the_discrete_actor_passes(name, variant):
    d = RC.DISCRETE_SHAPES[name]
    for ew in (True, False):
        W, I, G, Kf, Kb, sat, dup, pres = _discrete_emulated(d, RC.SEEDS[2], variant, ew)
        rep = {}
        amb, n, won = _check_discrete(d, W, I, G, Kf, Kb, sat, dup, rep)
        assert max(rep.values()) < 1.0, rep
        assert set(rep) >= ({"sv_act_stats", "action", "entropy", "d_actor_out", "d_actor_pre0", "d_actor_pre3"} if d.A > 1 else {"action"}), rep
        assert share_ok(amb, n) and n == d.T * ((d.B if sat is None else int((~sat).sum())) + d.B * d.D), (amb, n)
        assert won is None or won > 0, "the planted pair never won: the case checks nothing"
        assert R.near_decision_fraction([p.double() for l in range(4) for p in pres[f"a{l}"]]) <= 1e-3


@pytest.mark.parametrize("fault", list(GC.DISCRETE_FAULTS))
def test_planted_discrete_actor_fault_fails(fault):
    name, variant = GC.DISCRETE_FAULTS[fault]
    d = RC.DISCRETE_SHAPES[name]
    W, I, G, Kf, Kb, sat, dup, _ = _discrete_emulated(d, RC.SEEDS[2], variant, fault=fault)
    with pytest.raises(AssertionError):
        _check_discrete(d, W, I, G, Kf, Kb, sat, dup)


@pytest.mark.parametrize("name", ["a17", "a64"])
def test_planted_last_maximum_fails_the_actor_duplicate_check(name):
    d = RC.DISCRETE_SHAPES[name]
    W, I, G, Kf, Kb, sat, dup, _ = _discrete_emulated(d, RC.SEEDS[2], "duplicate", fault="sampler_ge")
    R.check_layers(RC.imagine_fwd_layers(d, W, I, Kf, discrete=True), Kf)
    RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"])       # the margin alone does not see it
    with pytest.raises(AssertionError):
        RC.actor_checks(d, Kf["sv_act_stats"], I["eps_action"], Kf["action"], dup=dup)


@pytest.mark.parametrize("name", list(RC.OBSERVE_SHAPES) + ["img:" + n for n in RC.IMAGINE_SHAPES] +
                         [f"disc:{n}:{v}" for n, v in R.discrete_cases(RC.DISCRETE_SHAPES)])
def test_ambiguous_share_of_the_float64_reference(name):
    """On the chained float64 reference alone: at most 0.1 % of the draws -- the prior's or posterior's factors and, with
    the Categorical actor, the actor's draws, counted together as the GPU tests count them -- have a runner-up within the
    margin of the best, for every shape and variant of the tables and every seed the GPU tests use."""
    img, dcase = name.startswith("img:"), name.startswith("disc:")
    d = RC.DISCRETE_SHAPES[name.split(":")[1]] if dcase else RC.IMAGINE_SHAPES[name[4:]] if img else RC.OBSERVE_SHAPES[name][0]
    high = name.endswith("c256_d2")
    for seed in RC.SEEDS:
        sat = dup = None
        if img or dcase:
            disc = dcase or name == "img:discrete"
            if dcase:
                W, I, sat, dup = RC.make_discrete_case(d, seed, name.split(":")[2])
                W, I = R.to64(W), R.to64(I)
            else:
                W, I = R.to64(RC.make_weights(d, seed, imagine=True, bias_high=high)), R.to64(RC.make_imagine_inputs(d, seed, discrete=disc))
            K = RC.empty_set(RC.img_fwd_tensors(d, disc), d)
            R.fill_layers(RC.imagine_fwd_layers(d, W, I, K, chain=True, discrete=disc, sat=sat), K)
            lg, q = K["prior_logits"], I["q_prior"]
        else:
            nt, init, _ = RC.observe_variant(name)
            W, I = R.to64(RC.make_weights(d, seed, bias_high=high)), R.to64(RC.make_observe_inputs(d, seed, nonterm=nt, init=init))
            K = RC.empty_set(RC.OBS_FWD_TENSORS, d)
            R.fill_layers(RC.observe_fwd_layers(d, W, I, K, chain=True), K)
            lg, q = K["post_logits"], I["q_post"]
        for path in ("hw", "libm"):
            amb, n = sum(RC.sample_check(lg[t], q[t], K["sidx"][t], d.D, d.C, path)[0] for t in range(d.T)), d.T * d.B * d.D
            if img and disc or dcase:
                a, m, won = RC.actor_checks(d, K["sv_act_stats"], I["eps_action"], K["action"], sat, dup, path=path)
                assert m == d.T * (d.B if sat is None else int((~sat).sum())) and (won is None or won > 0), (name, seed, m, won)
                amb, n = amb + a, n + m
            assert share_ok(amb, n), (name, seed, path, amb, n)


# ---- planted faults fail, each at the shape named for it ---------------------------------------------------------------

FWD_FAULTS = {"fwd_nonterm": "c16_d20",       # nonterminal factor dropped from the forward gather
              "gather_rem": "c32_d12",        # the gather's remainder loop (D % 8 factors) dropped
              "wrap128": "c256_d2",           # class index wrapped at 128
              "zero_as_class0": "c16_d20",    # the zero initial state treated as class 0
              "stale_sidx": "t7"}             # the gather reads sidx of step t - 2
BWD_FAULTS = {"bwd_nonterm": "c16_d20",       # nonterminal factor dropped from the backward carry
              "chunk1_w2": "c32_d12",         # chunk 1 reading chunk 0's W_2 rows
              "last_chunk_skipped": "c16_d20",  # the last partial chunk's factors skipped
              "dpl_ignored": "c32_d12",       # dpost_logits ignored
              "jac_one_minus": "c5_d3"}       # 1 - sum instead of g - sum_c p g


@pytest.mark.parametrize("fault", list(FWD_FAULTS))
def test_planted_forward_fault_fails(fault):
    name = FWD_FAULTS[fault]
    d = RC.OBSERVE_SHAPES[name][0]
    W, I, G, Kf, Kb, _ = _observe_emulated(d, 11, "zeros", "mixed", fwd_fault=fault, bias_high=name == "c256_d2")
    with pytest.raises(AssertionError):
        R.check_layers(RC.observe_fwd_layers(d, W, I, Kf), Kf)


@pytest.mark.parametrize("fault", list(BWD_FAULTS))
def test_planted_backward_fault_fails(fault):
    d = RC.OBSERVE_SHAPES[BWD_FAULTS[fault]][0]
    W, I, G, Kf, Kb, _ = _observe_emulated(d, 11, "zeros", "mixed", bwd_fault=fault)
    R.check_layers(RC.observe_fwd_layers(d, W, I, Kf), Kf)
    with pytest.raises(AssertionError):
        R.check_layers(RC.observe_bwd_layers(d, W, observe_bwd_inputs(I, Kf), Kb, G), Kb)


def test_planted_actor_gather_fault_fails():
    d = RC.IMAGINE_SHAPES["c16_d20"]
    W, I, G, Kf, Kb, _ = _imagine_emulated(d, RC.SEEDS[2], fault="actor_gather", start="onehot")
    with pytest.raises(AssertionError):
        R.check_layers(RC.imagine_fwd_layers(d, W, I, Kf), Kf)


@pytest.mark.parametrize("name", ["c16_d20", "c32_d12"])
def test_planted_last_maximum_fails_the_duplicate_class_check(name):
    """`>=` instead of `>` in the sampler: invisible to the margin (both classes tie), caught by the duplicate-class case."""
    d = RC.OBSERVE_SHAPES[name][0]
    W, I = RC.make_weights(d, 11), RC.make_observe_inputs(d, 11)
    RC.plant_duplicate(d, W, I["q_post"])
    with torch.no_grad():
        good, _ = emu_observe_fwd(d, W, I, torch.float32)
        bad, _ = emu_observe_fwd(d, W, I, torch.float32, "sampler_ge")
    assert RC.duplicate_check(d, good["post_logits"], good["sidx"]) > 0
    for t in range(d.T):        # the margin alone does not see it
        RC.sample_check(bad["post_logits"][t], I["q_post"][t], bad["sidx"][t], d.D, d.C, RC.sample_path(d.C))
    with pytest.raises(AssertionError):
        RC.duplicate_check(d, bad["post_logits"], bad["sidx"])


# ---- host checks (no launch) --------------------------------------------------------------------------------------------

def test_tables_and_mirror_match_the_library():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    for B in (1, 16, 17, 40, 100, 257, 4100):
        for Be in (16, 40, 42, 200, 256, 520):
            for D, Cc in ((32, 32), (12, 32), (3, 32), (20, 16), (16, 64), (2, 256), (136, 2), (3, 5), (7, 9), (16, 1), (4, 16),
                          (8, 32), (64, 4), (16, 16)):
                for max_wgs in (16, 128, 256, 1000):
                    Cm = RC.pick_cat_cluster(B, Be, D, Cc, max_wgs)
                    assert lib.bd_observe_cat_cluster_size(B, Be, D, Cc, max_wgs) == Cm, (B, Be, D, Cc, max_wgs)
                    for Hd in (16, 200):
                        for cm in {Cm, 4, 16} - {0}:
                            assert lib.bd_observe_cat_cluster_ws_floats(B, Be, Hd, D, cm) == RC.cluster_ws_floats(B, Be, Hd, D, cm)
    def lib_lds(kernel, d, Cm=0, **kw):    # the library's own figure: the total of the layout kernel and launcher share
        dims = dict(dict(Be=d.Be, S=0, D=d.D, C=d.C, A=d.A, Hd=d.Hd, Cm=Cm), **kw)
        return lib.bd_scan_lds_bytes(cabi.SCAN_KERNELS[kernel], *(dims[k] for k in ("Be", "S", "D", "C", "A", "Hd", "Cm")))

    seen = {}
    for name, (d, Cm, chunks, last, math_, staging, gather, rem) in RC.OBSERVE_SHAPES.items():
        assert RC.accepts(d.D, d.C, d.Hd), name
        assert RC.pick_cat_cluster(d.B, d.Be, d.D, d.C, 256) == Cm, name
        p = RC.paths(d.D, d.C, d.Be, d.Hd)
        assert (p["chunks"], p["last"], p["math"], p["staging"], p["gather"], p["rem"]) == (chunks, last, math_, staging, gather, rem), (name, p)
        sizes = RC.cluster_sizes(d.B, d.Be, d.D, d.C, d.Hd)
        assert (sizes[0] if sizes else 0) == Cm, (name, sizes)
        for entry in ("observe_fwd", "observe_bwd"):
            lds = RC.lds_bytes(entry, d.Be, d.D, d.C, d.A, d.Hd)
            assert lds <= RC.K_MAX_LDS and (lds > 64 * 1024) == (name in RC.OBSERVE_BIG_LDS[entry]), (name, entry, lds)
            assert lib_lds("observe_cat_" + entry[8:], d) == lds, (name, entry)
        for cm in sizes:
            for entry in ("cluster_fwd", "cluster_bwd"):
                lds = RC.lds_bytes(entry, d.Be, d.D, d.C, d.A, d.Hd, cm)
                assert lds <= RC.K_MAX_LDS, (name, entry, cm)
                assert lib_lds("observe_cat_c" + entry[8:], d, cm) == lds, (name, entry, cm)
        nt, init, dpl = RC.observe_variant(name)
        for kind in ("cluster" if Cm else None, "generic" if math_ == "generic" else None):
            if kind:
                seen.setdefault(kind, set()).update({("nt", nt), ("init", init), ("dpl", dpl)})
    every = {("nt", k) for k in R.NONTERM_KINDS} | {("init", k) for k in RC.INIT_KINDS} | {("dpl", True), ("dpl", False)}
    assert seen["cluster"] == every and seen["generic"] == every, seen
    assert {RC.OBSERVE_SHAPES[n][1] for n in RC.OBSERVE_SHAPES} >= {0, 4, 8, 16}
    assert RC.cluster_sizes(18, 64, 32, 32, 48) == [16, 8] and RC.cluster_sizes(16, 48, 8, 32, 256) == [8, 4]
    for name, d in RC.IMAGINE_SHAPES.items():
        assert RC.accepts(d.D, d.C, d.Hd), name
        for entry in ("imagine_fwd", "imagine_bwd"):
            lds = RC.lds_bytes(entry, d.Be, d.D, d.C, d.A, d.Hd)
            assert lds <= RC.K_MAX_LDS and (lds > 64 * 1024) == (name in RC.IMAGINE_BIG_LDS[entry]), (name, entry, lds)
            assert lib_lds("imagine_cat_" + entry[8:], d) == lds, (name, entry)
    # a28: the entropy partial sums decide the size of the forward's shared region
    d = RC.IMAGINE_SHAPES["a28"]
    assert RC.K_WAVES * 16 * d.A * 3 == 10752 > max(RC.K_SPLIT_SCRATCH, RC.full_image(d.D, d.C)) == 10240
    assert [RC.lds_bytes(e, d.Be, d.D, d.C, d.A, d.Hd) for e in ("imagine_fwd", "imagine_bwd")] == [63232, 59392]
    # the query rejects what it cannot describe, with the reason
    d = RC.OBSERVE_SHAPES["c32_d12"][0]
    assert lib.bd_scan_lds_bytes(len(cabi.SCAN_KERNELS), d.Be, 0, d.D, d.C, d.A, d.Hd, 4) == 0 and b"unknown kernel" in lib.bd_last_error()
    assert lib_lds("observe_cat_cfwd", d, 8) == 0 and b"does not divide D=12" in lib.bd_last_error()
    assert lib_lds("observe_cat_cbwd", d, 0) == 0 and b"does not divide" in lib.bd_last_error()
    t = RC.IMAGINE_SHAPES["tile_loop"]
    assert RC.cdiv(t.B, 16) == 257 and RC.cat_grid(t.B) == 129        # workgroups walk two tiles, the last one walks one
    assert RC.cat_grid(4096) == 256 and RC.cat_grid(4900) == 154


def test_lds_formulas_of_the_mirror_match_the_library():
    """Every entry point rejects a shape above 160 KiB with "needs N B of LDS": N must be the mirror's figure."""
    import re
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    shapes = [dict(Be=520, D=32, C=32, A=6, Hd=256), dict(Be=1000, D=12, C=32, A=3, Hd=200), dict(Be=900, D=20, C=16, A=17, Hd=30),
              dict(Be=1200, D=3, C=5, A=2, Hd=20)]
    single = [("observe_fwd", lib.bd_observe_cat_forward, cabi.ObserveCatFwdArgs, dict(T=2, B=20)),
              ("observe_bwd", lib.bd_observe_cat_backward, cabi.ObserveCatBwdArgs, dict(T=2, B=20)),
              ("imagine_fwd", lib.bd_imagine_cat_forward, cabi.ImagineCatFwdArgs, dict(N=20, Hm=2, n_samples=1)),
              ("imagine_bwd", lib.bd_imagine_cat_backward, cabi.ImagineCatBwdArgs, dict(N=20, Hm=2))]
    for sh in shapes:
        for entry, fn, typ, extra in single:
            want = RC.lds_bytes(entry, sh["Be"], sh["D"], sh["C"], sh["A"], sh["Hd"])
            assert want > RC.K_MAX_LDS
            assert fn(C.byref(_fake(typ(), dict(sh, **extra))), None) != 0
            m = re.search(rb"needs (\d+) B of LDS", lib.bd_last_error())
            assert m and int(m.group(1)) == want, (entry, sh, lib.bd_last_error(), want)
    for sh, Cm in ((dict(Be=512, D=32, C=32, A=6, Hd=256), 16), (dict(Be=250, D=16, C=64, A=3, Hd=256), 8)):
        assert RC.cluster_ok(20, sh["Be"], sh["D"], sh["C"], sh["Hd"], Cm)
        for entry, fn, typ in (("cluster_fwd", lib.bd_observe_cat_forward_cluster, cabi.ObserveCatFwdArgs),
                               ("cluster_bwd", lib.bd_observe_cat_backward_cluster, cabi.ObserveCatBwdArgs)):
            want = RC.lds_bytes(entry, sh["Be"], sh["D"], sh["C"], sh["A"], sh["Hd"], Cm)
            if want <= RC.K_MAX_LDS:
                continue
            assert fn(C.byref(_fake(typ(), dict(sh, T=2, B=20))), Cm, 4096, 1 << 28, None) != 0
            m = re.search(rb"needs (\d+) B of LDS", lib.bd_last_error())
            assert m and int(m.group(1)) == want, (entry, sh, lib.bd_last_error(), want)


def _fake(args, dims, null=()):
    GC._fake_ptrs(args, null)
    for k, v in dims.items():
        setattr(args, k, v)
    for arr in ("w_a", "b_a", "wt_a"):
        if hasattr(args, arr):
            for i in range(len(getattr(args, arr))):
                getattr(args, arr)[i] = 4096
    return args


def test_rejecting_paths_return_without_a_launch():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    base = dict(T=2, B=20, Be=40, D=4, C=16, A=3, Hd=32)
    img = dict(N=20, Hm=2, Be=40, D=4, C=16, A=3, Hd=32)
    entries = [(lib.bd_observe_cat_forward, cabi.ObserveCatFwdArgs, base), (lib.bd_observe_cat_backward, cabi.ObserveCatBwdArgs, base),
               (lib.bd_imagine_cat_forward, cabi.ImagineCatFwdArgs, dict(img, n_samples=1)),
               (lib.bd_imagine_cat_backward, cabi.ImagineCatBwdArgs, img)]
    # 30 x 10: S > 256 and 256 % C != 0; 33 x 8: S = 264 > 256 is no multiple of 16 (17 x 16 = 272 is one, and is accepted)
    bad = [dict(D=30, C=10), dict(D=33, C=8), dict(D=2, C=257), dict(Hd=257)]
    assert RC.accepts(17, 16, 32)
    for fn, typ, dims in entries:
        for b in bad:
            assert not RC.accepts(dict(dims, **b)["D"], dict(dims, **b)["C"], dict(dims, **b)["Hd"])
            assert fn(C.byref(_fake(typ(), dict(dims, **b))), None) != 0, (fn.__name__, b)
            assert b"unsupported" in lib.bd_last_error() or b"hidden width" in lib.bd_last_error()
    need = lib.bd_observe_cat_cluster_ws_floats(20, 40, 32, 4, 4)
    for fn, typ in ((lib.bd_observe_cat_forward_cluster, cabi.ObserveCatFwdArgs), (lib.bd_observe_cat_backward_cluster, cabi.ObserveCatBwdArgs)):
        for b in bad:
            assert fn(C.byref(_fake(typ(), dict(base, **b))), 4, 4096, 1 << 26, None) != 0, (fn.__name__, b)
        assert not RC.cluster_ok(20, 40, 4, 16, 32, 8) and not RC.cluster_ok(20, 40, 4, 16, 32, 3)
        for cm in (8, 3):         # 8: groups of half a factor's columns do not exist (4 % 8 != 0); 3 does not divide D
            assert fn(C.byref(_fake(typ(), base)), cm, 4096, 1 << 26, None) != 0
            assert b"cluster size" in lib.bd_last_error()
        assert fn(C.byref(_fake(typ(), base)), 4, 4096, need - 1, None) != 0 and b"workspace too small" in lib.bd_last_error()
        assert fn(C.byref(_fake(typ(), base)), 4, None, need, None) != 0
    f = _fake(cabi.ImagineCatFwdArgs(), dict(img, n_samples=1, discrete_actions=1))
    assert lib.bd_imagine_cat_forward(C.byref(f), None) != 0 and b"sv_act_us" in lib.bd_last_error()
    g = _fake(cabi.ImagineCatBwdArgs(), dict(img, discrete_actions=1))
    assert lib.bd_imagine_cat_backward(C.byref(g), None) != 0 and b"d_actor_pre" in lib.bd_last_error()
    # A = 65: one lane per class does not reach class 64; both entry points say so themselves, for either actor (without a GPU
    # every call fails: the message shows that this check came first)
    for disc in (0, 1):
        f = _fake(cabi.ImagineCatFwdArgs(), dict(img, A=65, n_samples=1, discrete_actions=disc), null=("sv_act_us",) if disc else ())
        assert lib.bd_imagine_cat_forward(C.byref(f), None) != 0 and b"action width 65 above 64" in lib.bd_last_error(), lib.bd_last_error()
        g = _fake(cabi.ImagineCatBwdArgs(), dict(img, A=65, discrete_actions=disc), null=("d_actor_pre",) if disc else ())
        assert lib.bd_imagine_cat_backward(C.byref(g), None) != 0 and b"action width 65 above 64" in lib.bd_last_error(), lib.bd_last_error()
