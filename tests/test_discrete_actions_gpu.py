"""GPU tests of the Categorical actor (action_distribution="Categorical", DESIGN.md "Discrete actions"): one imagination
forward and backward against the CPU restatement (tests/discrete_oracle.py) on both latent families, two whole train
steps at rho in {-1, 0, 0.5}, the pipelined schedule against the serial one, the launches left out at rho = 0, the
bd_actor_reinforce_cat kernel against autograd, get_action / update_belief_and_act, and the drop-in surface."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from big_dreamer_amd import synth
from oracle import dreamer_oracle as O
from tests.discrete_oracle import DISCRETE_GOLDEN, DiscreteOracleDreamer, discrete_head, oracle_hp
from tests.helpers import assert_close, check_fingerprints, load_golden

pytestmark = pytest.mark.gpu

SLOT = 11
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _disc(d, A):
    return dataclasses.replace(d, A=A, discrete_actions=True)


# (dims, seed, engine hp, restatement hp)
_CASES = {
    "tiny": (_disc(synth.TINY, 6), 0, {}, {}),
    "tiny_a18": (_disc(synth.TINY, 18), 1, {}, {}),
    "cat_tiny": (_disc(synth.CAT_TINY, 6), 51, dict(free_nats=0.0), dict(free_nats=0.0, categorical=(3, 5))),
    "cat_tiny_a18": (_disc(synth.CAT_TINY, 18), 52, dict(free_nats=0.0), dict(free_nats=0.0, categorical=(3, 5))),
    "tiny_pixel": (_disc(synth.TINY_PIXEL, 6), 4, {}, {}),
    "tiny_discount": (_disc(synth.TINY_DISCOUNT, 6), 9, {}, {}),
    "small": (_disc(synth.SMALL, 18), 3, {}, {}),
    # entropy_weight = 0.1: the entropy term of the actor gradient (and its discount weights) well above the tolerances
    "tiny_a18_ent": (_disc(synth.TINY, 18), 5, dict(entropy_weight=0.1), dict(entropy_weight=0.1)),
    "tiny_discount_ent": (_disc(synth.TINY_DISCOUNT, 6), 10, dict(entropy_weight=0.1), dict(entropy_weight=0.1)),
}


# ------------------------------------------------------------------------------------------ one imagination
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("family", ["gauss", "cat"])
def test_imagination_forward_vs_restatement(A, family):
    """The scans' discrete head forward: one-hot indices exactly, entropies and action values within 1e-6 (the backward:
    test_scan_backward_d_actor_out_vs_restatement)."""
    from big_dreamer_amd.engine import DreamerEngine
    base = synth.SMALL if family == "gauss" else synth.CAT_TINY
    d = dataclasses.replace(base, A=A, B=11, discrete_actions=True)      # N = T * B rows: two 16-row tiles and a ragged one
    seed = 7 * A + (family == "cat")
    P = synth.make_params(d, seed)
    eng = DreamerEngine(d, {}, "cuda", params=P)
    N, Hm = d.N, d.Hm
    g = torch.Generator().manual_seed(seed)
    start = torch.randn(N, d.Be + d.S, generator=g)
    if d.categorical:
        idx = torch.randint(d.cat_C, (N, d.cat_D), generator=g)
        start[:, d.Be:] = F.one_hot(idx, d.cat_C).float().reshape(N, d.S)
    noise = synth.make_noise(d, seed)
    nz = _dev({"action": noise["action"], "img_prior": noise["img_prior"]})
    sidx = idx.to(torch.uint8).cuda().contiguous() if d.categorical else None
    ifeat, ent, act = eng.imagine(start.cuda(), N, Hm, nz, save=True, start_sidx=sidx)
    torch.cuda.synchronize()
    # restatement with autograd through the actor head outputs
    Pt = {m: {k: torch.tensor(v) for k, v in sd.items()} for m, sd in P.items()}
    cat = (d.cat_D, d.cat_C) if d.categorical else None
    outs, acts, ents, ks, feats = [], [], [], [], []
    belief, state = start[:, :d.Be], start[:, d.Be:]
    tm = Pt["transition_model"]
    for t in range(Hm):
        out = O.mlp(torch.cat([belief, state], 1), Pt["actor"]).detach().requires_grad_(True)
        a, h, norm, k = discrete_head(out, torch.as_tensor(noise["action"][t]))
        outs.append(out); acts.append(a); ents.append(h); ks.append(k)
        belief = O.gru_cell(O.embed_state_action(state, a, tm), belief, tm)
        if cat:
            state, _ = O.categorical_belief(belief, O._sub(tm, "belief_prior"),
                                            torch.as_tensor(noise["img_prior"][t]).reshape(-1, *cat), *cat)
        else:
            state, _, _ = O.gaussian_belief(belief, tm, "belief_prior", torch.as_tensor(noise["img_prior"][t]))
        belief, state = belief.detach(), state.detach()      # forward comparison only: the backward below is per step
        feats.append(torch.cat([belief, state], 1))
    got_act = act.view(Hm, N, A).cpu()
    want_act = torch.stack(acts).detach()
    assert torch.equal(got_act.argmax(-1), torch.stack(ks)), "one-hot indices"
    assert_close("action", got_act.numpy(), want_act.numpy(), 1e-6, 0)
    assert_close("entropy", ent.view(Hm, N).cpu().numpy(), torch.stack(ents).detach().numpy(), 1e-6, 1e-6)
    assert_close("feat", ifeat.view(Hm, N, -1).cpu().numpy(), torch.stack(feats).numpy(), 2e-5, 2e-5)


# ------------------------------------------------------------------------------------------ the scans' backward
@pytest.mark.parametrize("A", [2, 6, 18])
@pytest.mark.parametrize("family", ["gauss", "cat", "discount"])
@pytest.mark.parametrize("rho", [-1, 0.0, 0.5])
def test_scan_backward_d_actor_out_vs_restatement(A, family, rho):
    """d_actor_out as the engine leaves it after one train step (the scan's softmax Jacobian + entropy term, then
    bd_actor_reinforce_cat for rho != -1; rho = 0: the REINFORCE kernel alone) against the restatement's autograd
    d actor_loss / d out, within 1e-6.  entropy_weight = 0.1 makes the entropy term (and, with use_discount, its
    ent_weight factor) ~1e-3 of each entry: dropping it, flipping it or ignoring ent_weight fails here."""
    from big_dreamer_amd.engine import DreamerEngine
    base = {"gauss": synth.TINY, "cat": synth.CAT_TINY, "discount": synth.TINY_DISCOUNT}[family]
    d = dataclasses.replace(base, A=A, B=11, discrete_actions=True)     # N = 44 rows: two 16-row tiles and a ragged one
    seed = 3 * A + len(family)
    hp = dict(entropy_weight=0.1, gradient_mixing=rho, **(dict(free_nats=0.0) if d.categorical else {}))
    P = synth.make_params(d, seed)
    batch, nz = synth.make_batch(d, seed), synth.make_noise(d, seed)
    eng = DreamerEngine(d, hp, "cuda", params=P)
    od = DiscreteOracleDreamer(P, oracle_hp(d, hp))
    od.train_step(batch, nz)
    eng.train_step(_dev(batch), _dev(nz))
    torch.cuda.synchronize()
    # per-decision scale: d_actor_out is d (mean over the Mi = Hm * N decisions) / d out; times Mi, entries are O(1e-3)
    Mi = d.Hm * d.N
    got = eng._buf["d_actor_out"].view(d.Hm, d.N, A).cpu().numpy() * Mi
    want = od.last["d_actor_out"].numpy() * Mi
    assert_close("d_actor_out * Mi", got, want, 1e-6, 1e-4)
    # the entropy term is far above that tolerance: the restatement without it differs by much more
    od0 = DiscreteOracleDreamer(P, oracle_hp(d, dict(hp, entropy_weight=0.0)))
    od0.train_step(batch, nz)
    with pytest.raises(AssertionError):
        assert_close("d_actor_out * Mi without entropy", od0.last["d_actor_out"].numpy() * Mi, want, 1e-6, 1e-4)


# ------------------------------------------------------------------------------------------ pinned by the reference
@pytest.mark.parametrize("name", sorted(DISCRETE_GOLDEN))
def test_train_steps_vs_reference_golden(name):
    """Two whole train steps against the reference's own run (tools/gen_discrete_golden.py): logs, clipped gradients,
    gradient norms and post-Adam weights, at the tolerances of the restatement comparison below."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp = DISCRETE_GOLDEN[name]
    g = load_golden(name)
    P, batch = synth.make_params(d, seed), synth.make_batch(d, seed)
    check_fingerprints(g, P, batch, synth.make_noise(d, seed))
    eng = DreamerEngine(d, hp, "cuda", params=P)
    db = _dev(batch)
    mods = ("transition_model", "observation_model", "reward_model", "encoder") + \
        (("discount_model",) if d.use_discount else ())
    for step in range(2):
        logs = eng.train_step(db, _dev(synth.make_noise(d, seed + step)))
        if step == 0:
            eng.update_critic()
        torch.cuda.synchronize()
        for k in [k.split(".log.")[1] for k in g if k.startswith(f"step{step}.log.")]:
            tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
            assert_close(f"s{step}.{k}", logs[k], g[f"step{step}.log.{k}"], *tol)
        assert_close(f"s{step}.grad_norms", np.array([logs["grad_norm_model"], logs["grad_norm_actor"],
                                                      logs["grad_norm_critic"]]), g[f"step{step}.grad_norms"], 1e-6, 1e-3)
        for mod in mods + ("actor", "critic"):
            for k in [n.split(".", 3)[3] for n in g if n.startswith(f"step{step}.grad.{mod}.")]:
                want = g[f"step{step}.grad.{mod}.{k}"]
                scale = float(np.abs(want).max()) + 1e-12
                assert_close(f"s{step}.grad.{mod}.{k}", eng.G(mod, k).detach().cpu().numpy().reshape(want.shape), want,
                             2e-3 * scale + 1e-9, 2e-3)
        for mod in mods + ("actor", "critic", "critic_target"):
            for k in [n.split(".", 3)[3] for n in g if n.startswith(f"step{step}.param.{mod}.")]:
                want = g[f"step{step}.param.{mod}.{k}"]
                assert_close(f"s{step}.param.{mod}.{k}", eng.W(mod, k).detach().cpu().numpy().reshape(want.shape), want,
                             2e-5, 1e-5)


# ------------------------------------------------------------------------------------------ the REINFORCE kernel
@pytest.mark.parametrize("A", [2, 18, 64])
@pytest.mark.parametrize("weighted", [False, True])
def test_actor_reinforce_cat_kernel_vs_autograd(A, weighted):
    from big_dreamer_amd import _cabi
    lib, ptr = _cabi.lib, _cabi.ptr
    Hm, N = 3, 211
    g = torch.Generator().manual_seed(A + 100 * int(weighted))
    rows = Hm * N
    f64 = dict(generator=g, dtype=torch.float64)
    out = (torch.randn(rows, A, **f64) * 2.0).float().double()
    norm32 = (out - out.logsumexp(-1, keepdim=True)).float()
    k = torch.randint(A, (rows,), generator=g)
    p32 = torch.softmax(norm32.double(), -1).float()
    action = ((F.one_hot(k, A).float() + p32) - p32)
    ret = torch.randn(rows, **f64).float().double()
    base0 = torch.randn(N, **f64).float().double()
    value = torch.randn(rows, **f64).float().double()
    w = (torch.rand(rows, **f64) * 0.99).float().double() if weighted else torch.ones(rows, dtype=torch.float64)
    rho, inv, dent = 0.3, 1.0 / rows, -1e-2 / rows
    adv = ret - torch.cat([base0, value[:rows - N]])
    c = -(1 - rho) * inv * w * adv
    x = norm32.double().clone().requires_grad_(True)      # (norm is out up to a constant: the same gradient)
    norm = x - x.logsumexp(-1, keepdim=True)
    lp = norm.gather(1, k[:, None]).squeeze(1)
    p = torch.softmax(norm, -1)
    H = -(p * norm).sum(-1)
    g_rf, = torch.autograd.grad((c * lp).sum(), x, retain_graph=True)
    g_ent, = torch.autograd.grad((dent * w * H).sum(), x)
    ref_sum = float((w * adv * lp.detach()).sum())
    d0 = torch.randn(rows, A, **f64).float()
    cu = lambda t: t.float().cuda().contiguous()
    dev = dict(act=cu(action), st=cu(norm32), ret=cu(ret), base0=cu(base0), value=cu(value), w=cu(w))
    ws = torch.zeros(int(lib.bd_reduce_ws_floats()), device="cuda")
    results = {}
    for write in (0, 1):
        dout = d0.clone().cuda()
        sc = torch.zeros(16, device="cuda")
        _cabi.check(lib.bd_actor_reinforce_cat(ptr(dev["act"]), ptr(dev["st"]), ptr(dev["ret"]), ptr(dev["base0"]),
                                               ptr(dev["value"]), ptr(dev["w"]) if weighted else None, Hm, N, A, rho,
                                               inv, dent, write, ptr(dout), ptr(sc), SLOT, ptr(ws), _cabi.stream()))
        torch.cuda.synchronize()
        results[write] = (dout.cpu().double(), sc.cpu())
    want = {0: d0.double() + g_rf, 1: g_rf + g_ent}
    for write, (got, sc) in results.items():
        scale = float(want[write].abs().max())
        assert_close(f"d_actor_out(write={write})", got.numpy(), want[write].numpy(), 2e-5 * scale, 1e-4)
        assert_close("slot", float(sc[SLOT]), ref_sum, 1e-5 * float((w * adv * lp.detach()).abs().sum()), 1e-5)
        assert float(sc[:SLOT].abs().sum()) == 0 and float(sc[SLOT + 1:].abs().sum()) == 0
    assert torch.equal(results[0][1], results[1][1]), "the sum must not depend on the mode"


# ------------------------------------------------------------------------------------------ whole train steps
_STEP_CASES = [("tiny", -1), ("tiny", 0.0), ("tiny", 0.5), ("tiny_a18", -1), ("tiny_a18", 0.5), ("cat_tiny", -1),
               ("cat_tiny", 0.0), ("cat_tiny", 0.5), ("cat_tiny_a18", -1), ("tiny_pixel", -1), ("tiny_discount", -1),
               ("tiny_discount", 0.5), ("small", -1), ("tiny_a18_ent", -1), ("tiny_a18_ent", 0.5), ("tiny_discount_ent", -1),
               ("tiny_discount_ent", 0.0)]


@pytest.mark.parametrize("name,rho", _STEP_CASES)
def test_train_steps_vs_restatement(name, rho):
    """Two whole train steps: logs, clipped gradients, gradient norms and post-Adam weights against the restatement, at
    the tolerances of test_gradient_mixing_gpu.test_train_steps_vs_restatement."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, ohp = _CASES[name]
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
    od = DiscreteOracleDreamer(P, dict(ohp, planning_horizon=d.H, gradient_mixing=rho))
    db = _dev(batch)
    for step in range(2):
        nz = synth.make_noise(d, seed + step)
        assert "entropy" not in nz
        ologs = od.train_step(batch, nz)
        logs = eng.train_step(db, _dev(nz))
        if step == 0:
            od.update_critic()
            eng.update_critic()
        torch.cuda.synchronize()
        assert set(ologs) <= set(logs)
        for k, v in ologs.items():
            tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
            assert_close(f"s{step}.{k}", logs[k], v, *tol)
        gn = od.last["grad_norms"]
        assert_close(f"s{step}.grad_norms", np.array([logs["grad_norm_model"], logs["grad_norm_actor"],
                                                      logs["grad_norm_critic"]]),
                     np.array([gn["model"], gn["actor"], gn["critic"]]), 1e-6, 1e-3)
        coef = min(1.0, od.hp["grad_clip_norm"] / (gn["actor"] + 1e-6))
        for i, k in enumerate(od.P["actor"]):
            want = od.last["actor_grads"][i].numpy() * coef
            scale = float(np.abs(want).max()) + 1e-12
            assert_close(f"s{step}.grad.actor.{k}", eng.G("actor", k).detach().cpu().numpy(), want, 2e-3 * scale + 1e-9,
                         2e-3)
        for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
            for k, p in od.P[mod].items():
                assert_close(f"s{step}.param.{mod}.{k}", eng.W(mod, k).detach().cpu().numpy(), p.detach().numpy(), 2e-5,
                             1e-5)


def _weights_equal(a, b):
    for grp in ("model", "actor", "critic", "critic_target"):
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat), grp
        if ga.grad is not None:
            assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp


@pytest.mark.parametrize("name", ["small", "cat_tiny_a18"])
@pytest.mark.parametrize("rho", [-1, 0.0])
def test_pipelined_schedule_is_bit_identical_to_serial(name, rho):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _CASES[name]
    P = synth.make_params(d, seed)
    engs = []
    for pipe in (True, False):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.pipeline = pipe
        engs.append(eng)
    steps = 4
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    torch.cuda.synchronize()
    logs = []
    for eng in engs:
        for i in range(steps):
            eng.train_step(batches[i], noises[i], sync_logs="lazy")
            if i == 1:
                eng.update_critic()
        logs.append(eng.logs())
        torch.cuda.synchronize()
    for i, a in enumerate(engs):
        _weights_equal(a, engs[1])
        assert logs[i] == logs[1], i
    assert np.isfinite(list(logs[0].values())).all()


@pytest.mark.parametrize("name", ["small", "cat_tiny"])
def test_rho_zero_runs_no_imagination_backward(name):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _CASES[name]
    P = synth.make_params(d, seed)
    spans = {}
    for rho in (-1, 0.0):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.enable_timers(True)
        eng.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed)))
        torch.cuda.synchronize()
        spans[rho] = set(eng.timer_summary())
    assert {"imagine_bwd", "img_heads_bwd"} <= spans[-1] and "actor_reinforce" not in spans[-1]
    assert not {"imagine_bwd", "img_heads_bwd"} & spans[0.0], spans[0.0]
    assert {"imagine_fwd", "actor_reinforce", "actor_hidden_bwd", "wgrad_actor"} <= spans[0.0]


def test_perf_mode_noise_trains():
    """Perf mode (no explicit noise): Exp(1) action draws from the engine's generator, finite logs, one-hot actions."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _CASES["cat_tiny_a18"]
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    for i in range(3):
        logs = eng.train_step(_dev(synth.make_batch(d, seed + i)))
    torch.cuda.synchronize()
    assert np.isfinite(list(logs.values())).all(), logs
    assert float(eng.make_noise(d.B, "bh")["action"].min()) >= 0.0
    act = eng._buf["action"]
    assert torch.equal((act > 0.5).sum(-1), torch.ones(act.shape[0], dtype=torch.long, device=act.device))


# ------------------------------------------------------------------------------------------ drop-in surface
def _params(algo, A, extra=()):
    from big_dreamer_amd.config import load_config
    d = synth.SMALL
    ov = [f"belief_size={d.Be}", f"hidden_size={d.Hd}", f"embedding_size={d.E}", f"batch_size={d.B}",
          f"seq_len={d.L}", f"planning_horizon={d.H}", "experience_size=400", "seed_steps=120", "max_episode_length=40",
          "action_distribution=Categorical", f"synthetic_env_action_size={A}", f"algorithm={algo}"] + list(extra)
    if algo == "dreamerV2":
        ov += ["latent_distribution=Categorical", "discrete_latent_dimensions=4", "discrete_latent_classes=5",
               "state_size=20"]
    else:
        ov += [f"state_size={d.S}"]
    return load_config(ov)


@pytest.mark.parametrize("algo,A", [("dreamer", 6), ("dreamerV2", 18)])
def test_surface_trains_acts_and_checkpoints(algo, A, tmp_path):
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import Env, SyntheticDiscreteEnv
    params = _params(algo, A)
    env = Env(params)
    assert isinstance(env, SyntheticDiscreteEnv) and env.action_size == A
    cls = DreamerV2 if algo == "dreamerV2" else Dreamer
    torch.manual_seed(0)
    agent = cls(params, env)
    assert agent.dims.discrete_actions and agent.actor.model[-2].weight.shape[0] == A
    np.random.seed(0)
    agent.randomly_initialize_replay_buffer()
    for _ in range(2):
        logs = agent.train_step()
        assert all(np.isfinite(v) for v in logs.values()), logs
    agent.update_critic()
    S = agent.state_size
    Be = agent.belief_size
    # get_action: sample (one-hot up to the straight-through rounding), mode, exact entropy
    belief, state = torch.randn(5, Be).cuda(), torch.zeros(5, S).cuda()
    act, ent = agent.get_action(belief, state)
    assert torch.equal((act > 0.5).sum(-1).cpu(), torch.ones(5, dtype=torch.long))
    assert float((act - F.one_hot(act.argmax(-1), A).float()).abs().max()) < 1e-6
    mode, ent2 = agent.get_action(belief, state, deterministic=True)
    logits = agent.actor.model(torch.cat([belief, state], 1))
    _, dist = agent.actor(belief, state)
    assert torch.equal(mode.argmax(-1), logits.argmax(-1)) and torch.equal(mode, F.one_hot(mode.argmax(-1), A).float())
    assert_close("entropy", ent.cpu().numpy(), dist.entropy().cpu().numpy(), 1e-5, 1e-5)
    assert torch.equal(ent, ent2)
    # explicit Exp(1) draws: the kernel's sample is argmax(p / q)
    q = torch.empty(5, A, device="cuda").exponential_()
    act3, _ = agent.get_action(belief, state, _noise={"action": q})
    assert torch.equal(act3.argmax(-1), (dist.probs / q).argmax(-1))
    # update_belief_and_act with exploration: one-hot rows; action_noise = 1 makes every row random
    obs = env.reset()
    b0, s0, a0 = torch.zeros(1, Be).cuda(), torch.zeros(1, S).cuda(), torch.zeros(1, A).cuda()
    for explore in (False, True):
        _, _, a, _, reward, _ = agent.update_belief_and_act(env, b0, s0, a0, obs, explore=explore)
        assert a.shape == (1, A) and int((a > 0.5).sum()) == 1 and np.isfinite(reward)
    agent.action_noise = 1.0
    nz = {"prior": torch.zeros(1, S).cuda(), "post": torch.zeros(1, S).cuda(),
          "action": torch.ones(1, A).cuda(), "explore_u": torch.zeros(1).cuda(), "explore_k": torch.tensor([A - 1]).cuda()}
    if agent.dims.categorical:
        nz["prior"], nz["post"] = torch.ones(1, S).cuda(), torch.ones(1, S).cuda()
    _, _, a, _, _, _ = agent.update_belief_and_act(env, b0, s0, a0, obs, explore=True, _noise=nz)
    assert torch.equal(a.cpu(), F.one_hot(torch.tensor([A - 1]), A).float())
    # checkpoint round trip, bit for bit; a Gaussian actor does not load into the Categorical agent
    path = str(tmp_path / "ckpt.pt")
    agent.save(path)
    torch.manual_seed(1)
    other = cls(dict(params, models=path), Env(params))
    for key in ("actor", "critic", "transition_model"):
        for (k, v), (k2, v2) in zip(getattr(agent, key).state_dict().items(), getattr(other, key).state_dict().items()):
            assert k == k2 and torch.equal(v.cpu(), v2.cpu()), (key, k)
    sd = torch.load(path, weights_only=True)
    W = sd["actor"]["model.8.weight"]
    sd["actor"]["model.8.weight"] = torch.cat([W, W], 0)
    sd["actor"]["model.8.bias"] = torch.cat([sd["actor"]["model.8.bias"]] * 2)
    with pytest.raises(RuntimeError, match="size mismatch"):
        other.actor.load_state_dict(sd["actor"])


def test_main_runs_with_categorical_actions():
    """python src/main.py algorithm=dreamerV2 action_distribution=Categorical ..., tiny sizes, a handful of updates."""
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), "algorithm=dreamerV2", "action_distribution=Categorical",
           "synthetic_env_action_size=18", "latent_distribution=Categorical", "discrete_latent_dimensions=4",
           "discrete_latent_classes=5", "state_size=20", "belief_size=32", "hidden_size=32", "embedding_size=64",
           "batch_size=6", "seq_len=8", "planning_horizon=5", "experience_size=500", "seed_steps=100",
           "max_episode_length=30", "train_steps=140", "log_freq=10", "collect_interval=2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Initialized with" in out.stdout and "actor_loss" in out.stdout
