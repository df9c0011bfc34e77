"""GPU: the world-model heads (reward_head=twohot, symlog_observations=true; DESIGN.md, "World-model heads on any scale")
through the engine and the agent -- two whole train steps against the CPU restatement (tests/wm_heads_oracle.py), the
symlog switch against an agent fed transformed observations (exact), open-loop prediction against its composition by hand,
the replay under the Collector, any-scale inputs, the default path against an agent built without the keys, the pipelined
schedule against the serial one, the diagnostics, Dreamer.reward, checkpoint / resume with refused mismatches, and the
command line."""
import dataclasses
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests.helpers import CASES, CAT_CASES, assert_close
from tests.twohot_oracle import decode
from tests.wm_heads_oracle import WmHeadsDiscreteOracleDreamer, WmHeadsOracleDreamer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = dict(lo=-1.5, hi=6.0, count=3.0, skipped=0.0)          # scale 7.5
REWARD_SCALE, OBS_SCALE = 300.0, 50.0


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _case(name, reward=None, critic=None, symlog=False):
    """(dims, seed, engine hp, restatement hp).  reward / critic: (K, Z) of a two-hot head, None = the width-1 head."""
    if name == "tiny_cat_actor":
        d, seed, hp = dataclasses.replace(synth.TINY, A=6, discrete_actions=True), 0, {}
    elif name in CAT_CASES:
        d, seed, hp, _ = CAT_CASES[name]
    else:
        d, seed, hp, _ = CASES[name]
    hp = dict(hp, entropy_weight=0.1)
    ohp = dict(hp, critic_head="normal", symlog_observations=bool(symlog))
    if reward is not None:
        d = dataclasses.replace(d, reward_head="twohot", reward_bins=reward[0], reward_bin_range=reward[1])
        ohp.update(reward_head="twohot", reward_bins=reward[0], reward_bin_range=reward[1])
    if critic is not None:
        d = dataclasses.replace(d, critic_head="twohot", critic_bins=critic[0], critic_bin_range=critic[1])
        ohp.update(critic_head="twohot", critic_bins=critic[0], critic_bin_range=critic[1])
    if symlog:
        d = dataclasses.replace(d, symlog_obs=True)
    if d.categorical:
        ohp["categorical"] = (d.cat_D, d.cat_C)
    return d, seed, hp, ohp


def _scaled(batch, symlog):
    """The batch with rewards x 300 and, where symlog is on, observations x 50 (so that it is far from the identity)."""
    out = dict(batch, rewards=batch["rewards"] * np.float32(REWARD_SCALE))
    if symlog:
        out["observations"] = batch["observations"] * np.float32(OBS_SCALE)
    return out


# ------------------------------------------------------------------------------------------ against the restatement
# (case, rho, reward (K, Z), critic (K, Z), percentile, symlog)
_STEP_CASES = [
    ("tiny", -1, (255, 20.0), None, False, False),
    ("tiny", 0.5, (7, 20.0), None, False, False),
    ("small", -1, (7, 20.0), None, False, False),
    ("cat_tiny", -1, (255, 20.0), None, False, False),
    ("tiny_cat_actor", 0.5, (255, 20.0), None, False, False),
    ("tiny_discount", -1, (255, 20.0), None, False, False),
    ("tiny", 0.5, (31, 10.0), (255, 20.0), True, False),         # differing K and Z: a mixed-up dimension shows
    ("tiny", -1, None, None, False, True),                       # symlog_observations alone
    ("tiny", 0.5, (31, 10.0), (255, 20.0), True, True),          # everything on
    ("tiny_pixel", -1, (7, 20.0), None, False, False),           # the smallest pixel case of the suite: the reward head only
]


@pytest.mark.parametrize("name,rho,reward,critic,pct,symlog", _STEP_CASES)
def test_train_steps_vs_restatement(name, rho, reward, critic, pct, symlog):
    """Two whole train steps: logs, clipped gradients, gradient norms and post-Adam weights of every parameter tensor
    against the CPU restatement at the tolerances of test_twohot_gpu.test_train_steps_vs_restatement."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, ohp = _case(name, reward, critic, symlog)
    rn = dict(return_normalization="percentile", return_norm_decay=0.5) if pct else {}
    P = synth.make_params(d, seed)
    RK = reward[0] if reward else 1
    assert P["reward_model"]["model.8.weight"].shape[0] == RK
    batch = _scaled(synth.make_batch(d, seed), symlog)
    eng = DreamerEngine(d, dict(hp, gradient_mixing=rho, **rn), "cuda", params=P)
    if reward is not None:
        assert not eng.heads_fused and eng.behaviour_plan(d.Hm, d.N) == (d.Hm,)
    cls = WmHeadsDiscreteOracleDreamer if d.discrete_actions else WmHeadsOracleDreamer
    od = cls(P, dict(ohp, planning_horizon=d.H, gradient_mixing=rho, **rn))
    if pct:
        eng.load_return_norm_state(PRESET)
        od.rn_state = dict(PRESET)
    db = _dev(batch)
    obs_before = db["observations"].clone()
    rep = []

    def rel(tag, got, want, atol, rtol):
        got, want = np.asarray(got, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
        rep.append(f"{tag:28s} max|err|={np.abs(got - want).max():.3e}  max|ref|={np.abs(want).max():.3e}")
        assert_close(tag, got, want, atol, rtol)

    try:
        for step in range(2):
            nz = synth.make_noise(d, seed + step)
            ologs = od.train_step(batch, nz)
            logs = eng.train_step(db, _dev(nz))
            if step == 0:
                od.update_critic()
                eng.update_critic()
            torch.cuda.synchronize()
            eng.cluster_status(d.B)
            assert set(ologs) <= set(logs) and "reward_loss" in ologs
            for k, v in ologs.items():
                tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                rel(f"s{step}.{k}", logs[k], v, *tol)
            rel(f"s{step}.returns", eng._buf[f"p{step & 1}_returns" if eng.pipeline else "returns"].cpu().numpy(),
                od.last["returns"].numpy().reshape(-1), 2e-5, 5e-5)
            gn = od.last["grad_norms"]
            rel(f"s{step}.grad_norms", [logs["grad_norm_model"], logs["grad_norm_actor"], logs["grad_norm_critic"]],
                [gn["model"], gn["actor"], gn["critic"]], 1e-6, 1e-3)
            coef = {k: min(1.0, od.hp["grad_clip_norm"] / (gn[k] + 1e-6)) for k in gn}
            groups = {"model": (od.model_modules, od.last["model_grads"]), "actor": (("actor",), od.last["actor_grads"]),
                      "critic": (("critic",), od.last["critic_grads"])}
            for grp, (mods, grads) in groups.items():
                i = 0
                for mod in mods:
                    for k in od.P[mod]:
                        want = grads[i].numpy() * coef[grp]
                        scale = float(np.abs(want).max()) + 1e-12
                        rel(f"s{step}.grad.{mod}.{k}", eng.G(mod, k).detach().cpu().numpy(), want, 2e-3 * scale + 1e-9,
                            2e-3)
                        i += 1
            for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
                for k, p in od.P[mod].items():
                    rel(f"s{step}.param.{mod}.{k}", eng.W(mod, k).detach().cpu().numpy(), p.detach().numpy(), 2e-5, 1e-5)
        assert eng.W("reward_model", "model.8.weight").shape == (RK, d.Hd)
        assert torch.equal(db["observations"], obs_before)          # the caller's batch is never modified
    finally:
        print("\n".join(rep[-200:]))


# ------------------------------------------------------------------------------------------ exact wiring
def _weights_equal(a, b, groups=("model", "actor", "critic", "critic_target")):
    for grp in groups:
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat), grp
        if ga.grad is not None:
            assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp


def _symlog_dev(x):
    from big_dreamer_amd import _cabi as cabi
    x = x.contiguous()
    out = torch.empty_like(x)
    cabi.check(cabi.lib.bd_symlog(x.data_ptr(), x.numel(), out.data_ptr(), cabi.stream()))
    return out


def _symexp_dev(x):
    from big_dreamer_amd import _cabi as cabi
    x = x.contiguous()
    out = torch.empty_like(x)
    cabi.check(cabi.lib.bd_symexp(x.data_ptr(), x.numel(), out.data_ptr(), cabi.stream()))
    return out


@pytest.mark.parametrize("name", ["tiny", "small", "cat_tiny"])
def test_the_switch_is_symlog_of_the_engines_input_train_steps(name):
    """An engine with symlog_observations=true on raw observations and one without it on bd_symlog of them: the same
    logs and weights after two train steps, bit for bit (small: the composed encoder tail is off at these row counts,
    so force it on there)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name, (31, 10.0))
    P = synth.make_params(d, seed)
    a = DreamerEngine(dataclasses.replace(d, symlog_obs=True), hp, "cuda", params=P)
    b = DreamerEngine(d, hp, "cuda", params=P)
    if name == "small":
        a.encoder_composed = b.encoder_composed = True
    for step in range(2):
        batch = _dev(_scaled(synth.make_batch(d, seed + step), True))
        nz = _dev(synth.make_noise(d, seed + step))
        la = a.train_step(batch, nz)
        lb = b.train_step(dict(batch, observations=_symlog_dev(batch["observations"])), nz)
        torch.cuda.synchronize()
        assert la == lb, (la, lb)
    _weights_equal(a, b)
    assert "obs_symlog" in a._buf and "obs_symlog" not in b._buf


def _agent(extra, seed, models=None, drop_keys=False, d=synth.SMALL):
    from big_dreamer_amd.config import REWARD_HEAD_KEYS, load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from tests.test_checkpoint_gpu import ScriptedEnv, _overrides
    params = load_config(_overrides(d, list(extra)) + ([f"models={models}"] if models else []))
    if drop_keys:
        for k in REWARD_HEAD_KEYS + ("symlog_observations",):
            del params[k]
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    random.seed(seed + 2)
    cls = DreamerV2 if params["algorithm"] == "dreamerV2" else Dreamer
    return cls(params, ScriptedEnv(d))


_CAT = ["algorithm=dreamerV2", "latent_distribution=Categorical", f"discrete_latent_dimensions={synth.CAT_TINY.cat_D}",
        f"discrete_latent_classes={synth.CAT_TINY.cat_C}"]


@pytest.mark.parametrize("latents,fused", [("gaussian", True), ("gaussian", False), ("categorical", True), ("categorical", False)])
def test_the_switch_is_symlog_of_the_agents_input_acting(latents, fused, monkeypatch):
    """Belief, state and action of three chained update_belief_and_act calls under injected noise: the agent with the
    switch on raw observations equals the agent without it on bd_symlog of them, on the fused and the composed route."""
    cat = latents == "categorical"
    d, extra = (synth.CAT_TINY, _CAT) if cat else (synth.SMALL, [])
    monkeypatch.setenv("BD_ACT_FUSED", "1" if fused else "0")
    monkeypatch.setenv("BD_ACT_FUSED_CAT", "1" if fused else "0")
    a = _agent(extra + ["symlog_observations=true"], 5, d=d)
    b = _agent(extra, 5, d=d)
    assert a.dims.symlog_obs and not b.dims.symlog_obs
    assert (a.act_fused_cat if cat else a.act_fused) == fused and (b.act_fused_cat if cat else b.act_fused) == fused
    _weights_equal(a.engine, b.engine)
    g = torch.Generator().manual_seed(11)
    draw = (lambda *s: torch.empty(*s).exponential_(generator=g).cuda()) if cat else (lambda *s: torch.randn(*s, generator=g).cuda())
    S, A, B = a.state_size, a.action_size, 8           # eight rows: the environment is stepped with row 0's action only
    carry_a = carry_b = (torch.zeros(B, a.belief_size).cuda(), torch.zeros(B, S).cuda(), torch.zeros(B, A).cuda())
    moved = False
    for t in range(3):
        obs = (torch.randn(B, a.dims.O, generator=g) * OBS_SCALE).cuda()
        nz = {"prior": torch.ones(B, S).cuda(), "post": draw(B, S), "action": torch.randn(B, A, generator=g).cuda(),
              "entropy": torch.randn(a.dims.n_entropy, B, A, generator=g).cuda(), "explore": torch.randn(B, A, generator=g).cuda()}
        raw = obs.clone()
        out_a = [x.clone() for x in a.update_belief_and_act(a.env, *carry_a, obs, explore=True, _noise=nz)[:3]]
        assert torch.equal(obs, raw)                            # the uploaded observation is never modified
        out_b = [x.clone() for x in b.update_belief_and_act(b.env, *carry_b, _symlog_dev(obs), explore=True, _noise=nz)[:3]]
        for n, x, y in zip(("belief", "state", "action"), out_a, out_b):
            assert tuple(x.shape)[0] == B and torch.equal(x, y), (t, n)
        off = [x.clone() for x in b.update_belief_and_act(b.env, *carry_b, obs, explore=True, _noise=nz)[:3]]
        moved |= any(not torch.equal(x, y) for x, y in zip(off[1:], out_a[1:]))     # (the belief of step t does not read obs t)
        carry_a, carry_b = tuple(out_a), tuple(out_b)
    assert moved, "the transform did not change the decision: the test shows nothing"


def test_open_loop_is_symlog_open_loop_symexp_error():
    """With the switch on, open_loop = symlog -> the existing open loop -> bd_symexp -> bd_openl_error on raw truth."""
    from tests.test_checkpoint_gpu import _fill
    a = _agent(["symlog_observations=true"], 5)
    b = _agent([], 5)
    _weights_equal(a.engine, b.engine)
    _fill(a.buffer, a.dims)
    batch = [x.clone() for x in a.buffer.sample(3, 6)]
    batch[0] = batch[0] * OBS_SCALE
    L, n = batch[1].shape[:2]
    T, c = L - 1, 2
    g = torch.Generator().manual_seed(5)
    noise = {"post": torch.randn(c, n, a.state_size, generator=g).cuda(), "prior": torch.randn(T - c, n, a.state_size, generator=g).cuda()}
    raw = batch[0].clone()
    res = a.open_loop(batch=batch, context=c, _noise=noise)
    assert torch.equal(batch[0], raw)
    by_hand = b.open_loop(batch=[_symlog_dev(batch[0].cuda())] + batch[1:], context=c, _noise=noise)
    assert torch.equal(res["beliefs"], by_hand["beliefs"]) and torch.equal(res["states"], by_hand["states"])
    model = _symexp_dev(b.observation_model(by_hand["beliefs"], by_hand["states"]))
    want = b.engine.openl_error(batch[0][1:].cuda().contiguous(), model, T, n, a.dims.O, False).cpu().numpy()
    assert np.array_equal(res["openl_obs_mse"], want) and np.isfinite(want).all() and (want > 0).all()
    assert not np.array_equal(by_hand["openl_obs_mse"], want)           # the curve is in observation units, not symlog units
    assert res["openl_mse_context"] == float(want[:c].mean()) and res["openl_mse_open"] == float(want[c:].mean())
    # observation_model as a module returns the prediction in symlog space
    assert torch.equal(a.observation_model(res["beliefs"], res["states"]), b.observation_model(res["beliefs"], res["states"]))


def test_the_replay_keeps_raw_observations_under_the_collector():
    from big_dreamer_amd.collect import Collector
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    from big_dreamer_amd.env import Env, VecEnv
    from tests.test_collect_gpu import TINY
    params = load_config(TINY + ["collect_envs=3", "symlog_observations=true", "reward_head=twohot"])
    torch.manual_seed(3)
    agent = Dreamer(params, VecEnv(Env, params, 3))
    buf = agent.buffer
    collector = Collector(agent, agent.env)
    collector.seed(24)
    buf.sync_device()
    seen, idx0 = [], buf.idx
    for _ in range(5):
        seen.append(torch.as_tensor(collector.observation).float().reshape(3, -1).numpy().copy())
        collector.step()
    torch.cuda.synchronize()
    bits = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)
    for e in range(3):
        for k, obs in enumerate(seen):
            row = e * buf.lane_size + idx0 + k
            assert np.array_equal(bits(buf.observations[row].reshape(-1)), bits(obs[e])), (e, k)
    assert np.array_equal(bits(buf._dev["observations"].cpu().numpy()), bits(buf.observations))
    assert "act_obs_symlog" in agent.engine._buf or not agent.act_fused


# ------------------------------------------------------------------------------------------ any scale
def test_any_scale_leaves_the_engine_step_finite():
    """rewards x 1e30 and observations x 1e30 with both switches on (and the two-hot critic): two engine steps give finite
    logs, weights and grad_norm_model."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case("tiny", (31, 10.0), (255, 20.0), True)
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    batch = synth.make_batch(d, seed)
    batch = _dev(dict(batch, rewards=batch["rewards"] * np.float32(1e30), observations=batch["observations"] * np.float32(1e30)))
    for step in range(2):
        logs = eng.train_step(batch, _dev(synth.make_noise(d, seed + step)))
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in logs.values()), logs
        assert np.isfinite(logs["grad_norm_model"])
    for grp in ("model", "actor", "critic"):
        assert torch.isfinite(eng.groups[grp].flat).all(), grp


def test_the_planner_refuses_a_twohot_reward_head():
    """DreamerEngine.plan scores candidates with a width-1 reward model: with reward_head=twohot it raises instead of
    reading logit 0 of the K-wide layer."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case("tiny", (7, 20.0))
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    B, H, cand = 2, 3, 16
    with pytest.raises(ValueError, match="reward_head=twohot.*width-1"):
        eng.plan(torch.zeros(B, d.Be).cuda(), torch.zeros(B, d.S).cuda(), H, 1, cand, 4,
                 torch.zeros(1, H, B, cand, d.A).cuda(), torch.zeros(1, H, B * cand, d.S).cuda())


# ------------------------------------------------------------------------------------------ the default path
def test_defaults_given_explicitly_are_an_agent_built_without_the_keys():
    from tests.test_checkpoint_gpu import Own, _assert_groups_equal, _fill
    a = _agent(["reward_head=normal", "reward_bins=255", "reward_bin_range=20.0", "symlog_observations=false"], 5)
    b = _agent([], 5, drop_keys=True)
    assert a.dims == b.dims and a.dims.reward_out == 1 and a.engine.heads_fused == b.engine.heads_fused
    _assert_groups_equal(a, b)
    for ag in (a, b):
        _fill(ag.buffer, ag.dims)
    own_a, own_b = Own(a), Own(b)
    for _ in range(3):
        la, lb = own_a.run(lambda: dict(a.train_step())), own_b.run(lambda: dict(b.train_step()))
        assert la == lb, (la, lb)
    _assert_groups_equal(a, b)
    assert sorted(a.engine._buf) == sorted(b.engine._buf)
    assert all(a.engine._buf[k].shape == b.engine._buf[k].shape for k in a.engine._buf)
    assert not any("row_loss" in k or "_val" in k or "logits" in k or "symlog" in k for k in a.engine._buf)


# ------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("name,rho", [("small", -1), ("small", 0.1), ("cat_tiny", -1)])
def test_pipelined_schedule_is_bit_identical_to_serial(name, rho):
    """Four un-synchronised steps with both switches on, pipelined / serial / pipelined with the held-back optimiser steps:
    every weight, Adam moment and logged scalar."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name, (31, 10.0), None, True)
    P = synth.make_params(d, seed)
    engs = []
    for pipe, defer in ((True, False), (False, False), (True, True)):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.pipeline, eng.defer_opt = pipe, defer
        engs.append(eng)
    steps = 4
    batches = [_dev(_scaled(synth.make_batch(d, seed + 10 * i), True)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    torch.cuda.synchronize()
    logs, lazy = [], []
    for eng in engs:
        for i in range(steps):
            lz = eng.train_step(batches[i], noises[i], sync_logs="lazy")
            if i == 1:
                eng.update_critic()
        lazy.append(dict(lz))
        logs.append(eng.logs())
        torch.cuda.synchronize()
    for i, a in enumerate(engs):
        _weights_equal(a, engs[1])
        assert logs[i] == logs[1], i
        assert lazy[i] == lazy[1] == logs[1], i
    assert np.isfinite(list(logs[0].values())).all()


# ------------------------------------------------------------------------------------------ diagnostics and the surface
_TH = ["reward_head=twohot", "reward_bins=31", "reward_bin_range=10.0"]


def test_diagnostics_read_decoded_rewards():
    """reward_pred_* and imag_reward_* of a diagnosed step against Dreamer.reward on the step's own features (the model
    learning rate is 0, so the weights the step used are the agent's)."""
    from tests.test_checkpoint_gpu import _fill
    a = _agent(_TH + ["symlog_observations=true", "model_learning_rate=0", "diagnostics_interval=1"], 5)
    _fill(a.buffer, a.dims)
    logs = dict(a.train_step())
    torch.cuda.synchronize()
    e, d = a.engine, a.dims
    tag = "p0_" if e.pipeline else ""
    for key, buf in (("reward_pred", tag + "feat"), ("imag_reward", tag + "ifeat")):
        feat = e._buf[buf]
        r = a.reward(feat[:, :d.Be].contiguous(), feat[:, d.Be:].contiguous()).double().cpu().numpy()
        assert r.shape == (feat.shape[0], 1)
        assert abs(logs[key + "_mean"] - r.mean()) <= 2e-5 * max(1.0, abs(r.mean())), key
        assert abs(logs[key + "_std"] - r.std()) <= 2e-5 * max(1.0, r.std()), key
        logits = a.reward_model(feat[:, :d.Be].contiguous(), feat[:, d.Be:].contiguous())
        assert logits.shape == (feat.shape[0], 31)
    assert abs(logs["imag_reward_max"] - float(r.max())) <= 2e-5 * max(1.0, abs(r.max()))
    assert abs(logs["reward_loss"] - np.log(31)) < 1.0             # a cross-entropy at a fresh head, not the Normal's


def test_reward_decodes_the_logits():
    from oracle import dreamer_oracle as O
    a = _agent(_TH, 5)
    d = a.dims
    g = torch.Generator().manual_seed(0)
    belief, state = torch.randn(4, 9, d.Be, generator=g).cuda(), torch.randn(4, 9, d.S, generator=g).cuda()
    logits = a.reward_model(belief, state)
    assert logits.shape == (4, 9, 31)
    r = a.reward(belief, state)
    assert r.shape == (4, 9, 1)
    sd = {k: p.detach().cpu() for k, p in a.reward_model.state_dict().items()}
    want = decode(O.dense_on_features(belief.cpu(), state.cpu(), sd), 10.0)
    assert_close("reward", r.cpu().numpy(), want.numpy(), 2e-5, 5e-5)
    n = _agent([], 5)
    assert torch.equal(n.reward(belief, state), n.reward_model(belief, state)) and n.reward(belief, state).shape == (4, 9, 1)


def test_resume_is_bit_identical_and_mismatches_are_refused(tmp_path):
    from tests.test_checkpoint_gpu import Own, _assert_groups_equal, _fill
    on = _TH + ["symlog_observations=true"]
    a = _agent(on, 5)
    _fill(a.buffer, a.dims)
    for _ in range(2):
        la = dict(a.train_step())
    assert np.isfinite(la["reward_loss"])
    models, replay = str(tmp_path / "models_2.pth"), str(tmp_path / "experience_2.npz")
    a.save(models, extra={"step": 2})
    a.buffer.save(replay)
    own_a = Own(a)
    saved = torch.load(models, map_location="cpu", weights_only=True)
    assert saved["run_state"]["reward_head"] == {"kind": "twohot", "bins": 31, "range": 10.0}
    assert saved["run_state"]["symlog_observations"] is True
    assert saved["reward_model"]["model.8.weight"].shape[0] == 31
    b = _agent(on, 99, models=models)
    b.buffer.load(replay)
    assert b.load_run_state(models) == {"step": 2}
    own_b = Own(b)
    _assert_groups_equal(a, b)
    for _ in range(2):
        la, lb = own_a.run(lambda: dict(a.train_step())), own_b.run(lambda: dict(b.train_step()))
        assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
    _assert_groups_equal(a, b)
    # another K, another Z, the width-1 head: refused with both heads named, before anything is copied
    sym = ["symlog_observations=true"]
    for extra in (["reward_head=twohot", "reward_bins=7", "reward_bin_range=10.0"] + sym, ["reward_head=twohot", "reward_bins=31"] + sym,
                  sym):
        with pytest.raises(ValueError, match="reward head .*twohot.*31.* does not match"):
            _agent(extra, 7, models=models)
    with pytest.raises(ValueError, match="symlog_observations=True does not match .*symlog_observations=False"):
        _agent(_TH, 7, models=models)
    plain = _agent([], 5)
    _fill(plain.buffer, plain.dims)
    dict(plain.train_step())
    default = str(tmp_path / "models_default.pth")
    plain.save(default, extra={"step": 1})
    rs = torch.load(default, map_location="cpu", weights_only=True)["run_state"]
    assert "reward_head" not in rs and "symlog_observations" not in rs
    with pytest.raises(ValueError, match="'kind': 'normal'.* does not match .*twohot"):
        _agent(_TH, 7, models=default)
    with pytest.raises(ValueError, match="symlog_observations=False does not match .*symlog_observations=True"):
        _agent(sym, 7, models=default)
    fresh = _agent(on, 11)
    before = fresh.fingerprint()
    with pytest.raises(ValueError):
        fresh.load({"models": default})
    assert fresh.fingerprint() == before            # nothing was copied


_CLI = ["state_size=8", "belief_size=32", "hidden_size=32", "embedding_size=64", "batch_size=6", "seq_len=8",
        "planning_horizon=5", "experience_size=500", "seed_steps=100", "max_episode_length=30", "log_freq=10", "collect_interval=2"]


def test_main_trains_with_both_switches():
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), "reward_head=twohot", "symlog_observations=true",
           "train_steps=140", *_CLI]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Initialized with" in out.stdout and "'reward_loss': " in out.stdout


@pytest.mark.parametrize("extra,msg", [(["algorithm=planet", "reward_head=twohot"], "PlaNet"),
                                       (["algorithm=planet", "symlog_observations=true"], "PlaNet"),
                                       (["pixel_observation=true", "symlog_observations=true"], "pixel")])
def test_main_refuses(extra, msg):
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), *extra, "train_steps=10", *_CLI]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "ValueError" in out.stderr and msg in out.stderr, out.stderr[-2000:]
