"""GPU: the evaluation policy through the acting path -- the fused step (csrc/act.hip: action_mode / latent_mean of
bd_act_args) for the four (latent, actor) configurations against tests/act_ref.py / tests/act_cat_ref.py and the selection
reference tests/act_mode_ref.py, bitwise against the sampling step where the two must coincide; the fused against the
composed route of update_belief_and_act; Dreamer.evaluate's reproducibility; the CLI; a checkpoint round trip.

Exact comparisons of sampled classes rest on the margin condition tests/test_act_mode_ref_cpu.py asserts for these inputs."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import act_cat_ref as CR
from tests import act_mode_ref as R
from tests.helpers import assert_close
from tests.test_act_step_cat_gpu import AGENT_KINDS, _agent_inputs, _min_gap
from tests.test_act_step_gpu import StubEnv, _load, _tiny_agent, cu

pytestmark = pytest.mark.gpu

TOL = 2e-5              # beliefs, Gaussian states, actor statistics, tanh-Normal actions (tests/test_act_step_gpu.TOL)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = ("action_mode", "latent_mean", "n_mode", "eps_mode", "stream_mode", "act_stats_out", "mode_index_out")


# ---------------------------------------------------------------------------------------------- the fused step
@pytest.fixture(scope="module")
def cases():
    """Per configuration, built on first use: engine, parameters, data, and the float64 decisions by (B, form, state_mean)."""
    from big_dreamer_amd.engine import DreamerEngine
    made = {}

    def get(name):
        if name not in made:
            d, seed = R.fused_cases()[name]
            P = synth.make_params(d, R.FUSED_PARAM_SEED)
            made[name] = (DreamerEngine(d, None, "cuda", params=P), P, CR.make_data(d, seed), {})
        return made[name]
    return get


def _ref(case, B, form, state_mean):
    eng, P, data, memo = case
    key = (B, form, state_mean)
    if key not in memo:
        memo[key] = R.policy_ref(P, eng.d, data, B, form, state_mean)
    return memo[key]


class Runner:
    """One decision (call 0 of the case's data) on the first B rows through Engine.act_step / act_step_cat."""

    def __init__(self, eng, data, B, form):
        self.eng, self.d, self.B = eng, eng.d, B
        self.ins = (cu(data["belief"][:B]), cu(data["state"][:B]), cu(data["action"][:B]))
        self.kw = {"obs": cu(data["obs"][0, :B])} if form == "obs" else {"embedding": cu(data["emb"][0, :B])}
        self.post, self.act, self.exp = cu(data["post"][0, :B]), cu(data["act"][0, :B]), cu(data["exp"][0, :B])
        self.step = eng.act_step_cat if (self.d.categorical or self.d.discrete_actions) else eng.act_step

    def __call__(self, action_mode="sample", state_mean=False, noise=(), explore=False):
        """-> ((belief, state, action) clones, act_stats clone or None, mode index clone or None)"""
        out = self.step(*self.ins, explore=explore, action_noise=CR.ACTION_NOISE, noise=None if noise is None else dict(noise),
                        action_mode=action_mode, state_mean=state_mean, **self.kw)
        keep = lambda t: None if t is None else t.clone()
        return tuple(t.clone() for t in out), keep(self.eng.last_act_stats), keep(self.eng.last_act_mode_index)


def _same(x, y, what):
    for name, s, t in zip(("belief", "state", "action"), x, y):
        assert torch.equal(s, t), f"{what}: {name} differs (max {float((s - t).abs().max()):.3e})"


@pytest.mark.parametrize("form", ["obs", "emb"])
@pytest.mark.parametrize("B", R.FUSED_B)
@pytest.mark.parametrize("name", list(R.fused_cases()))
def test_fused_step_with_a_policy(cases, name, B, form):
    case = cases(name)
    eng, P, data, _ = case
    d = eng.d
    run = Runner(eng, data, B, form)
    zero_or_one = torch.ones_like(run.post) if d.categorical else torch.zeros_like(run.post)
    greedy_q = torch.ones_like(run.act) if d.discrete_actions else torch.zeros_like(run.act)

    # "mean": belief', state', statistics and action against float64
    mean_run, stats, index = run("mean", False, {"post": run.post})
    hb, hs, ha, info, m64, s64 = _ref(case, B, form, False)
    assert info["min_gap"] > CR.MIN_GAP
    assert_close(f"{name} belief", mean_run[0].cpu().numpy(), hb, TOL, TOL)
    if d.categorical:
        assert np.array_equal(mean_run[1].cpu().numpy(), hs.astype(np.float32))
    else:
        assert_close(f"{name} state", mean_run[1].cpu().numpy(), hs, TOL, TOL)
    assert index is None
    if d.discrete_actions:
        assert stats is None
        assert np.array_equal(mean_run[2].cpu().numpy(), ha.astype(np.float32)), "the exact one-hot of argmax p"
        _same(run("mode", False, {"post": run.post})[0], mean_run, "Categorical actor: mode and mean")
        fed = run("sample", False, {"post": run.post, "action": greedy_q})[0]          # q = 1: (onehot + p) - p of the same class
        assert torch.equal(fed[2].argmax(1), mean_run[2].argmax(1)) and torch.equal(fed[1], mean_run[1])
    else:
        assert tuple(stats.shape) == (B, 2 * d.A)
        assert_close(f"{name} act_stats mean", stats[:, :d.A].cpu().numpy(), m64, TOL, TOL)
        assert_close(f"{name} act_stats std", stats[:, d.A:].cpu().numpy(), s64, TOL, TOL)
        assert_close(f"{name} action", mean_run[2].cpu().numpy(), ha, TOL, TOL)
        # "mean" is the sampling step fed eps_action = 0, bit for bit
        _same(run("sample", False, {"post": run.post, "action": greedy_q})[0], mean_run, '"mean" against eps_action = 0')

    # state_mean is the run fed zero (ones) posterior noise, bit for bit, under every action mode; and float64
    sm = run("sample", True, {"action": run.act})
    _same(run("sample", False, {"post": zero_or_one, "action": run.act})[0], sm[0], "state_mean against fed noise")
    sm_mean = run("mean", True, {})
    _same(run("mean", False, {"post": zero_or_one})[0], sm_mean[0], "state_mean, mean action")
    hb, hs, ha, info, _, _ = _ref(case, B, form, True)
    assert info["min_gap"] > CR.MIN_GAP
    assert torch.equal(sm_mean[0][0], mean_run[0]), "the belief takes no noise"
    if d.categorical:
        assert np.array_equal(sm_mean[0][1].cpu().numpy(), hs.astype(np.float32))
    else:
        assert_close(f"{name} state_mean state", sm_mean[0][1].cpu().numpy(), hs, TOL, TOL)
    if d.discrete_actions:
        assert np.array_equal(sm_mean[0][2].cpu().numpy(), ha.astype(np.float32))
    else:
        assert_close(f"{name} state_mean action", sm_mean[0][2].cpu().numpy(), ha, TOL, TOL)

    if d.discrete_actions:
        return
    # "mode": the index admissible for the kernel's OWN statistics, the action that index' draw
    m, s = stats[:, :d.A].cpu(), stats[:, d.A:].cpu()
    eps = R.eps_for_stats(m, s, d.n_entropy, seed=500 + B)
    assert bool(R.regular_or_saturated(m, s, eps).all())
    mode_run, stats2, index = run("mode", False, {"post": run.post, "mode": eps})
    assert torch.equal(stats2, stats) and torch.equal(mode_run[0], mean_run[0]) and torch.equal(mode_run[1], mean_run[1])
    assert index.dtype == torch.int32 and tuple(index.shape) == (B,)
    multi = R.check(index, mode_run[2], m, s, eps, TOL, tag=f"{name} B={B} {form}: ")
    print(f"{name} B={B} {form}: {multi} of {B} rows with more than one admissible index")
    assert multi <= R.MULTI_CAP * B
    # exploration on top, as in the sampling step
    noisy = run("mode", False, {"post": run.post, "mode": eps, "explore": run.exp}, explore=True)
    want = torch.clamp(mode_run[2] + CR.ACTION_NOISE * run.exp, -1, 1)
    assert torch.equal(noisy[2], index) and float((noisy[0][2] - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("name", list(R.fused_cases()))
def test_zeroed_tail_is_the_sampling_step(cases, name, monkeypatch):
    """With the new fields zero the three outputs are the sampling step's: the engine's call (whose block names the
    act_mode stream, nothing else of the tail) against a second launch of the same block with the whole tail zeroed, as a
    caller that never heard of the fields leaves it."""
    from big_dreamer_amd import _cabi as cabi
    from big_dreamer_amd import engine as engine_module
    eng, P, data, _ = cases(name)
    B, seen = 17, []

    class Recorder:
        def __getattr__(self, key):
            real = getattr(cabi.lib, key)
            if key not in ("bd_act_step", "bd_act_step_cat"):
                return real

            def call(ref, stream):
                seen.append((real, cabi.ActArgs.from_buffer_copy(bytes(ref._obj))))
                return real(ref, stream)
            return call

    run = Runner(eng, data, B, "obs")
    monkeypatch.setattr(engine_module, "lib", Recorder())
    for explore in (False, True):
        first = run("sample", False, {"post": run.post, "action": run.act, "explore": run.exp}, explore=explore)[0]
        real, block = seen[-1]
        assert block.action_mode == 0 and block.latent_mean == 0 and block.act_stats_out is None
        for key in TAIL:
            setattr(block, key, None if key in ("eps_mode", "act_stats_out", "mode_index_out") else 0)
        out = [torch.full_like(t, float("nan")) for t in first]
        block.belief_out, block.state_out, block.action_out = (t.data_ptr() for t in out)
        cabi.check(real(C.byref(block), cabi.stream()))
        torch.cuda.synchronize()
        _same(out, first, f"explore={explore}: zeroed tail")


@pytest.mark.parametrize("name", ["gauss_tanh", "cat3x5_tanh"])
def test_in_kernel_mode_draws_are_the_rng_fill_stream(cases, name):
    from big_dreamer_amd import _cabi as cabi
    eng, P, data, _ = cases(name)
    d, B = eng.d, 17
    eng.set_noise_seed(4321)
    run = Runner(eng, data, B, "obs")
    k = eng._rng_step.get("act", 0)
    own = run("mode", False, None, explore=True)
    assert eng._rng_step["act"] == k + 1, "the decision counter advances by one per call, mode draws included"
    shapes = [("post", "act_post", (B, d.S), cabi.BD_RNG_EXPONENTIAL if d.categorical else cabi.BD_RNG_NORMAL),
              ("mode", "act_mode", (d.n_entropy, B, d.A), cabi.BD_RNG_NORMAL), ("explore", "act_explore", (B, d.A), cabi.BD_RNG_NORMAL)]
    r = cabi.RngFillArgs()
    r.n, r.seed, r.step = len(shapes), eng.rng_seed, k
    bufs = {}
    for i, (key, stream, shape, kind) in enumerate(shapes):
        t = bufs[key] = torch.zeros(*shape, device="cuda")
        r.t[i] = cabi.RngTensor(t.data_ptr(), t.numel(), kind, eng.RNG_STREAMS[stream])
    cabi.check(cabi.lib.bd_rng_fill(C.byref(r), cabi.stream()))
    fed = run("mode", False, bufs, explore=True)
    _same(fed[0], own[0], "in-kernel draws against bd_rng_fill's")
    assert torch.equal(fed[1], own[1]) and torch.equal(fed[2], own[2])
    assert eng._rng_step["act"] == k + 1, "explicit noise consumes no counter step"
    nxt = run("mode", False, None, explore=True)
    assert not torch.equal(nxt[0][2], own[0][2]) and torch.equal(nxt[0][0], own[0][0])


# ---------------------------------------------------------------------------------------------- fused against composed
KINDS = dict(AGENT_KINDS, gauss_tanh=(synth.TINY, []))


@pytest.mark.parametrize("kind", list(KINDS))
def test_fused_and_composed_routes_agree(kind, monkeypatch):
    """update_belief_and_act with the same injected noise on both routes, within the tolerance the two routes are already
    held to (tests/test_act_step_gpu.py, tests/test_act_step_cat_gpu.py); rows of the mode with more than one admissible
    index are the exception: counted, printed, under the same cap."""
    d, extra = KINDS[kind]
    switch = "BD_ACT_FUSED" if kind == "gauss_tanh" else "BD_ACT_FUSED_CAT"
    B = 17
    env = StubEnv(d, batched=B)
    agent = _tiny_agent(d, extra, env=env)
    _load(agent, synth.make_params(d, 3))
    ins, obs, nz = _agent_inputs(d, B, 21)
    q1 = torch.ones(B, d.S).cuda() if d.categorical else torch.zeros(B, d.S).cuda()
    greedy = torch.ones(B, d.A).cuda()

    def both(**kw):
        monkeypatch.setenv(switch, "1")
        assert agent.act_fused or agent.act_fused_cat
        fused = [t.clone() for t in agent.update_belief_and_act(env, *ins, obs, _noise=nz, **kw)[:3]]
        stats = agent.engine.last_act_stats
        stats = None if stats is None else stats.clone()
        assert np.array_equal(env.got[-1], fused[2].cpu().numpy())
        monkeypatch.setenv(switch, "0")
        assert not agent.act_fused and not agent.act_fused_cat
        composed = [t.clone() for t in agent.update_belief_and_act(env, *ins, obs, _noise=nz, **kw)[:3]]
        assert np.array_equal(env.got[-1], composed[2].cpu().numpy())
        return fused, composed, stats

    def compare(tag, fused, composed, skip_rows=None):
        assert_close(f"{tag} belief", fused[0].cpu().numpy(), composed[0].cpu().numpy(), TOL, TOL)
        if d.categorical:
            assert torch.equal(fused[1], composed[1]), f"{tag}: one-hot states differ"
        else:
            assert_close(f"{tag} state", fused[1].cpu().numpy(), composed[1].cpu().numpy(), TOL, TOL)
        if d.discrete_actions:
            assert torch.equal(fused[2], composed[2]) and bool(((fused[2] == 0) | (fused[2] == 1)).all()) and \
                bool((fused[2].sum(1) == 1).all()), f"{tag}: exact one-hot actions"
        else:
            keep = torch.ones(B, dtype=torch.bool) if skip_rows is None else ~skip_rows
            assert_close(f"{tag} action", fused[2].cpu().numpy()[keep.numpy()], composed[2].cpu().numpy()[keep.numpy()], TOL, TOL)

    # the samplers of these inputs are decided outside the kernels' rounding (float64, current weights)
    for post in (nz["post"], q1):
        assert _min_gap(agent, d, ins, obs, dict(nz, post=post, action=greedy if d.discrete_actions else nz["action"])) > CR.MIN_GAP
    fused, composed, stats = both(action_mode="mean", state_mean=True)
    compare(f"{kind} mean, state_mean", fused, composed)
    fused, composed, stats = both(action_mode="mean", state_mean=False)
    compare(f"{kind} mean", fused, composed)
    if d.discrete_actions:
        fused, composed, _ = both(action_mode="mode", state_mean=False)
        compare(f"{kind} mode", fused, composed)
        return
    m, s = stats[:, :d.A].cpu(), stats[:, d.A:].cpu()
    nz["mode"] = R.eps_for_stats(m, s, d.n_entropy, seed=77).cuda()
    assert bool(R.regular_or_saturated(m, s, nz["mode"].cpu()).all())
    fused, composed, stats2 = both(action_mode="mode", state_mean=False)
    assert torch.equal(stats2, stats)
    multi = R.admissible(m, s, nz["mode"].cpu()).sum(0) > 1
    print(f"{kind}: {int(multi.sum())} of {B} rows with more than one admissible index")
    assert int(multi.sum()) <= R.MULTI_CAP * B
    R.check(_index_of(fused[2], m, s, nz["mode"].cpu()), fused[2], m, s, nz["mode"].cpu(), TOL, tag=f"{kind} fused: ")
    compare(f"{kind} mode", fused, composed, skip_rows=multi)
    with pytest.raises(ValueError, match="action_mode"):
        agent.update_belief_and_act(env, *ins, obs, _noise=nz, action_mode="best")


def _index_of(action, mean, sd, eps):
    """The draw an action is: per row the j whose float64 tanh(mean + sd e_j) is nearest."""
    y = torch.tanh(mean.double().unsqueeze(0) + sd.double().unsqueeze(0) * eps.double())
    return (y - action.double().cpu().unsqueeze(0)).abs().amax(-1).argmin(0)


# ---------------------------------------------------------------------------------------------- evaluate, CLI, checkpoint
def test_evaluate_is_reproducible_with_a_deterministic_policy(monkeypatch):
    from tests.test_evaluate_gpu import _agent, _reseed
    monkeypatch.delenv("BD_ACT_FUSED", raising=False)
    agent = _agent()
    assert agent.act_fused and agent.params["eval_action"] == "sample" and agent.params["eval_state_mean"] is False
    _reseed(agent)
    one = agent.evaluate(episodes=3, action_mode="mean", state_mean=True)
    two = agent.evaluate(episodes=3, action_mode="mean", state_mean=True)
    assert np.isfinite(one["returns"]).all() and np.array_equal(one["returns"], two["returns"])
    a, b = agent.evaluate(episodes=3), agent.evaluate(episodes=3, action_mode="sample", state_mean=False)
    assert not np.array_equal(a["returns"], b["returns"]), "sampled evaluations of one agent returned the same"
    assert not np.array_equal(a["returns"], one["returns"])
    monkeypatch.setenv("BD_ACT_FUSED", "0")                 # the composed route: as reproducible
    three = agent.evaluate(episodes=3, action_mode="mean", state_mean=True)
    four = agent.evaluate(episodes=3, action_mode="mean", state_mean=True)
    assert np.array_equal(three["returns"], four["returns"])
    assert np.abs(three["returns"] - one["returns"]).max() <= 1e-3 * np.abs(one["returns"]).max()
    mode = agent.evaluate(episodes=3, action_mode="mode")   # runs; its draws are the engine's
    assert np.isfinite(mode["returns"]).all()
    # the config keys are the defaults of evaluate()
    agent.params["eval_action"], agent.params["eval_state_mean"] = "mean", True
    monkeypatch.delenv("BD_ACT_FUSED", raising=False)
    assert np.array_equal(agent.evaluate(episodes=3)["returns"], one["returns"])
    with pytest.raises(ValueError, match="action_mode"):
        agent.evaluate(episodes=3, action_mode="best")


def test_planet_evaluates_with_the_defaults_only():
    from tests.test_evaluate_gpu import _agent
    agent = _agent(["algorithm=planet", "MPC.optimisation_iters=2", "MPC.candidates=32", "MPC.top_candidates=4"], cls="planet")
    with pytest.raises(ValueError, match="PlaNet plans"):
        agent.evaluate(episodes=2, action_mode="mode")


def test_cli_evaluates_with_the_mode():
    from tests.test_evaluate_gpu import EVAL_KEYS, TINY
    cli = TINY + ["seed_steps=48", "train_steps=51", "log_freq=10", "collect_interval=2", "experience_size=300",
                  "test_episodes=3", "test_interval=5", "evaluation=true", "eval_action=mode"]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *cli], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    for key in EVAL_KEYS:
        values = re.findall(rf"^{key} : (\S+)$", out.stdout, flags=re.M)
        assert len(values) >= 1 and all(math.isfinite(float(v)) for v in values), (key, values)
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *cli[:-1], "eval_action=best"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "eval_action" in bad.stderr


@pytest.mark.parametrize("fused", ["1", "0"])
def test_checkpoint_round_trip_after_mode_decisions(fused, tmp_path, monkeypatch):
    """Two decisions with action_mode = "mode" on Philox draws (the act_mode stream shares the decision counter), save,
    rebuild from the file, two more decisions on each: bit-identical, and the counters agree."""
    from big_dreamer_amd import checkpoint as ck
    from tests.test_checkpoint_gpu import Own, _agent, _start
    monkeypatch.setenv("BD_ACT_FUSED", fused)

    def decide(agent, carry):
        belief, state, action, obs = carry
        belief, state, action, nxt, _, _ = agent.update_belief_and_act(agent.env, belief, state, action, obs, explore=True,
                                                                       action_mode="mode")
        return belief.clone(), state.clone(), action.clone(), nxt

    a = _agent("state", 5)
    assert a.act_fused == (fused == "1")
    own_a = Own(a)
    carry = _start(a)
    for _ in range(2):
        carry = own_a.run(decide, a, carry)
    models = ck.models_path(str(tmp_path), 0)
    own_a.run(lambda: a.save(models, extra={"step": 0, "collect_envs": 1}))
    noise = a.engine.noise_state()
    assert noise["step"]["act"] == 2
    b = _agent("state", 99, models=models)
    b.load_run_state(models)
    own_b = Own(b)
    assert b.engine.noise_state() == noise
    ca = cb = carry
    b.env.t = a.env.t
    for _ in range(2):
        ca, cb = own_a.run(decide, a, ca), own_b.run(decide, b, cb)
        for x, y in zip(ca[:3], cb[:3]):
            assert torch.equal(x, y)
    assert a.engine.noise_state() == b.engine.noise_state() and a.engine.noise_state()["step"]["act"] == 4
