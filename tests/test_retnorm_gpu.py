"""GPU: percentile return normalisation (ActorCritic.return_normalization=percentile; DESIGN.md, "Return normalisation")
through the engine and the agent -- two whole train steps against the CPU restatement (tests/retnorm_oracle.py), the
running range against tests/retnorm_ref.py applied to the engine's own returns, what must not change against an engine
without it, the pipelined schedule against the serial one, checkpoint / resume and the command line."""
import dataclasses
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import retnorm_ref
from tests.helpers import CASES, CAT_CASES, assert_close
from tests.retnorm_oracle import RetnormDiscreteOracleDreamer, RetnormOracleDreamer

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRESET = dict(lo=-1.5, hi=6.0, count=3.0, skipped=0.0)          # scale 7.5
ON = dict(return_normalization="percentile")
RN_KEYS = {"return_scale", "return_p_low", "return_p_high"}


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _case(name):
    """(dims, seed, engine hp, restatement hp); entropy_weight 0.1 puts the entropy term -- which is NOT divided by the
    scale -- well above the tolerances."""
    if name == "tiny_cat_actor":
        d = dataclasses.replace(synth.TINY, A=6, discrete_actions=True)
        return d, 0, dict(entropy_weight=0.1), dict(entropy_weight=0.1)
    if name in CAT_CASES:
        d, seed, hp, _ = CAT_CASES[name]
        hp = dict(hp, entropy_weight=0.1)
        return d, seed, hp, dict(hp, categorical=(d.cat_D, d.cat_C))
    d, seed, hp, _ = CASES[name]
    hp = dict(hp, entropy_weight=0.1)
    return d, seed, hp, dict(hp)


def _returns_of(eng, step):
    """The lambda-returns train step number `step` left (double-buffered by step parity when pipelined)."""
    return eng._buf[f"p{step & 1}_returns" if eng.pipeline else "returns"].cpu().numpy()


def _state_after(state, returns, hp):
    k = retnorm_ref.ranks(returns.size, hp.get("return_norm_low", 0.05), hp.get("return_norm_high", 0.95))
    return retnorm_ref.update(state, returns, *k, hp.get("return_norm_decay", 0.99))


def _assert_state(got, want):
    for key in ("lo", "hi"):
        assert abs(got[key] - want[key]) <= 1e-12 * abs(want[key]), (key, got, want)
    assert got["count"] == want["count"] and got["skipped"] == want["skipped"], (got, want)


# ------------------------------------------------------------------------------------------ against the restatement
_STEP_CASES = [("tiny", -1), ("small", -1), ("tiny", 0.5), ("tiny", 0.0), ("tiny_discount", 0.1), ("cat_tiny", -1),
               ("tiny_cat_actor", 0.5)]


@pytest.mark.parametrize("name,rho", _STEP_CASES)
def test_train_steps_vs_restatement(name, rho):
    """Two whole train steps from a preset range (scale 7.5) with decay 0.5: logs, clipped gradients, gradient norms and
    post-Adam weights against the CPU restatement at the tolerances of
    test_gradient_mixing_gpu.test_train_steps_vs_restatement; after each step the device state against retnorm_ref applied
    to the engine's own returns."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, ohp = _case(name)
    rn = dict(ON, return_norm_decay=0.5)
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    eng = DreamerEngine(d, dict(hp, gradient_mixing=rho, **rn), "cuda", params=P)
    eng.load_return_norm_state(PRESET)
    assert eng.return_norm_state() == PRESET
    cls = RetnormDiscreteOracleDreamer if d.discrete_actions else RetnormOracleDreamer
    od = cls(P, dict(ohp, planning_horizon=d.H, gradient_mixing=rho, **rn))
    od.rn_state = dict(PRESET)
    db = _dev(batch)
    rep = []
    state = dict(PRESET)

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
            assert set(ologs) <= set(logs) and RN_KEYS <= set(ologs)
            assert logs["return_scale"] == float(retnorm_ref.scale(state, 1.0))          # exactly: the state the step used
            assert logs["return_p_low"] == float(np.float32(state["lo"]))
            assert logs["return_p_high"] == float(np.float32(state["hi"]))
            for k, v in ologs.items():
                tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                rel(f"s{step}.{k}", logs[k], v, *tol)
            want = _state_after(state, _returns_of(eng, step), rn)
            state = eng.return_norm_state()             # (the next step's scale is that of the DEVICE's state)
            _assert_state(state, want)
            assert state["count"] == 4.0 + step
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
    finally:
        print("\n".join(rep[-200:]))


# ------------------------------------------------------------------------------------------ what must not change
def _weights_equal(a, b, groups=("model", "actor", "critic", "critic_target")):
    for grp in groups:
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat), grp
        if ga.grad is not None:
            assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp


def _two_steps(d, seed, hp, between=None):
    from big_dreamer_amd.engine import DreamerEngine
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    logs = []
    for step in range(2):
        logs.append(eng.train_step(_dev(synth.make_batch(d, seed + step)), _dev(synth.make_noise(d, seed + step))))
        torch.cuda.synchronize()
        if between is not None and step == 0:
            between(eng)
    return eng, logs


@pytest.mark.parametrize("name,rho", [("small", -1), ("tiny", 0.5), ("tiny_discount", 0.1), ("cat_tiny", 0.0)])
def test_only_the_actor_sees_the_scale(name, rho):
    """Against an engine with 'none' on the same inputs: the world model (weights, gradients, Adam moments) is
    bit-identical after both steps, the critic after step 0 (step 1's imagination runs with another actor); 'none' given
    explicitly is an engine built without the key; and from the empty range with floor 1 the scale of step 0 is exactly 1, so
    step 0's actor update is bit-identical too (the seed is dconst / 1, the REINFORCE factor grad_scale / 1)."""
    d, seed, hp, _ = _case(name)
    hp = dict(hp, gradient_mixing=rho)
    snap = {}

    def keep(tag):
        def f(eng):
            snap[tag] = {g: (eng.groups[g].flat.clone(), eng.groups[g].m.clone(), eng.groups[g].v.clone())
                         for g in ("actor", "critic")}
        return f

    plain, logs_plain = _two_steps(d, seed, hp, keep("plain"))
    none, logs_none = _two_steps(d, seed, dict(hp, return_normalization="none"), keep("none"))
    on, logs_on = _two_steps(d, seed, dict(hp, **ON), keep("on"))
    assert plain._rn is None and none._rn is None and on._rn is not None
    _weights_equal(plain, none)
    assert logs_plain == logs_none and not RN_KEYS & set(logs_plain[0])
    assert set(logs_on[0]) == set(logs_plain[0]) | RN_KEYS
    _weights_equal(plain, on, groups=("model",))
    for g in ("actor", "critic"):
        for x, y in zip(snap["plain"][g], snap["on"][g]):
            assert torch.equal(x, y), g
    assert logs_on[0]["return_scale"] == 1.0 and logs_on[0]["return_p_low"] == 0.0
    assert {k: v for k, v in logs_on[0].items() if k not in RN_KEYS} == logs_plain[0]
    # step 1 divides by the range of step 0's returns
    st = _state_after(retnorm_ref.empty_state(), _returns_of(on, 0), {})
    assert logs_on[1]["return_scale"] == float(retnorm_ref.scale(st, 1.0))
    assert logs_on[1]["return_p_low"] == float(np.float32(st["lo"])) and logs_on[1]["return_p_high"] == float(np.float32(st["hi"]))
    for k in ("observation_loss", "reward_loss", "kl_loss", "model_loss", "grad_norm_model"):
        assert logs_on[1][k] == logs_plain[1][k], k
    assert plain.return_norm_state() == retnorm_ref.empty_state()
    with pytest.raises(ValueError):
        plain.load_return_norm_state(PRESET)


def test_a_large_scale_changes_the_actor_update():
    """The switch does something: with a preset range the actor's step differs from 'none', the critic's does not."""
    d, seed, hp, _ = _case("small")
    plain, _ = _two_steps(d, seed, hp)
    from big_dreamer_amd.engine import DreamerEngine
    eng = DreamerEngine(d, dict(hp, **ON), "cuda", params=synth.make_params(d, seed))
    eng.load_return_norm_state(PRESET)
    logs = eng.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed)))
    torch.cuda.synchronize()
    ref = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    rlogs = ref.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed)))
    torch.cuda.synchronize()
    assert torch.equal(eng.groups["critic"].flat, ref.groups["critic"].flat)
    assert torch.equal(eng.groups["model"].flat, ref.groups["model"].flat)
    assert not torch.equal(eng.groups["actor"].grad, ref.groups["actor"].grad)
    assert logs["value_loss"] == rlogs["value_loss"] and logs["actor_loss"] != rlogs["actor_loss"]
    assert logs["return_scale"] == 7.5


# ------------------------------------------------------------------------------------------ schedules
@pytest.mark.parametrize("name,rho,plan", [("small", -1, None), ("small", -1, (2, 2, 1)), ("small", 0.1, None)])
def test_pipelined_schedule_is_bit_identical_to_serial(name, rho, plan):
    """Four un-synchronised steps, pipelined / serial / pipelined with the held-back optimiser steps: every weight, Adam
    moment, logged scalar and the running range.  plan (2, 2, 1): the chunked behaviour chain, which behaviour_plan
    grants at rho = -1 (the seed fill precedes the first chunk)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name)
    P = synth.make_params(d, seed)
    engs = []
    for pipe, defer in ((True, False), (False, False), (True, True)):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho, return_norm_decay=0.5, **ON), "cuda", params=P)
        eng.pipeline, eng.defer_opt, eng.bh_chunks = pipe, defer, plan
        engs.append(eng)
    steps = 4
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    torch.cuda.synchronize()
    logs, lazy, states = [], [], []
    for eng in engs:
        for i in range(steps):
            lz = eng.train_step(batches[i], noises[i], sync_logs="lazy")
            if i == 1:
                eng.update_critic()
        lazy.append(dict(lz))
        logs.append(eng.logs())
        states.append(eng.return_norm_state())
        torch.cuda.synchronize()
    if plan is not None:
        assert all(e._bh_plan_used == plan for e in engs), "the chunk plan is not in force"
    for i, a in enumerate(engs):
        _weights_equal(a, engs[1])
        assert logs[i] == logs[1], i
        assert lazy[i] == lazy[1] == logs[1], i
        assert states[i] == states[1], i
    assert RN_KEYS <= set(logs[0]) and np.isfinite(list(logs[0].values())).all()
    assert states[0]["count"] == 4.0 and states[0]["skipped"] == 0.0 and logs[0]["return_scale"] >= 1.0


# ------------------------------------------------------------------------------------------ checkpoint and surface
def _agent(extra, seed, models=None):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    from tests.test_checkpoint_gpu import ScriptedEnv, _overrides
    d = synth.SMALL
    params = load_config(_overrides(d, list(extra)) + ([f"models={models}"] if models else []))
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    random.seed(seed + 2)
    return Dreamer(params, ScriptedEnv(d))


_PCT = ["ActorCritic.return_normalization=percentile", "ActorCritic.return_norm_decay=0.5", "ActorCritic.return_norm_floor=0.01"]


def test_resume_continues_the_range(tmp_path):
    """Save after two steps, resume in a fresh agent: the next burst of two steps is bit-identical to the uninterrupted
    run, the range included."""
    from tests.test_checkpoint_gpu import Own, _assert_groups_equal, _fill
    a = _agent(_PCT, 5)
    _fill(a.buffer, a.dims)
    for _ in range(2):
        la = dict(a.train_step())
    assert RN_KEYS <= set(la)
    models, replay = str(tmp_path / "models_2.pth"), str(tmp_path / "experience_2.npz")
    a.save(models, extra={"step": 2})
    a.buffer.save(replay)
    own_a = Own(a)
    saved = torch.load(models, map_location="cpu", weights_only=True)["run_state"]["return_norm"]
    assert saved == a.return_norm_state() and saved["count"] == 2.0
    b = _agent(_PCT, 99, models=models)
    b.buffer.load(replay)
    assert b.return_norm_state() == retnorm_ref.empty_state()
    assert b.load_run_state(models) == {"step": 2}
    own_b = Own(b)
    assert b.return_norm_state() == saved
    _assert_groups_equal(a, b)
    for _ in range(2):
        la, lb = own_a.run(lambda: dict(a.train_step())), own_b.run(lambda: dict(b.train_step()))
        assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
    assert la["return_scale"] != 0.01                       # the range, not the floor
    _assert_groups_equal(a, b)
    assert a.return_norm_state() == b.return_norm_state() and a.return_norm_state()["count"] == 4.0


def test_default_checkpoint_has_no_range_and_loads_as_the_empty_state(tmp_path):
    from tests.test_checkpoint_gpu import _fill
    a = _agent([], 5)
    _fill(a.buffer, a.dims)
    dict(a.train_step())
    models = str(tmp_path / "models_1.pth")
    a.save(models, extra={"step": 1})
    assert "return_norm" not in torch.load(models, map_location="cpu", weights_only=True)["run_state"]
    assert a.return_norm_state() == retnorm_ref.empty_state()
    b = _agent(_PCT, 99, models=models)
    b.load_return_norm_state(PRESET)
    b.load_run_state(models)
    assert b.return_norm_state() == retnorm_ref.empty_state()
    _fill(b.buffer, b.dims)
    assert dict(b.train_step())["return_scale"] == float(np.float32(0.01))


def test_main_prints_the_scale():
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), "ActorCritic.return_normalization=percentile",
           "state_size=8", "belief_size=32", "hidden_size=32", "embedding_size=64", "batch_size=6", "seq_len=8",
           "planning_horizon=5", "experience_size=500", "seed_steps=100", "max_episode_length=30", "train_steps=140",
           "log_freq=10", "collect_interval=2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Initialized with" in out.stdout and "'return_scale': " in out.stdout and "'return_p_high': " in out.stdout
