"""GPU: the two-hot critic (ActorCritic.critic_head=twohot; DESIGN.md, "Two-hot critic") through the engine and the
agent -- two whole train steps against the CPU restatement (tests/twohot_oracle.py), 'normal' given explicitly against an
agent built without the keys, the pipelined schedule against the serial one, the K-wide polyak update, Dreamer.value,
checkpoint / resume with refused mismatches, and the command line."""
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
from tests.twohot_oracle import TwohotDiscreteOracleDreamer, TwohotOracleDreamer, decode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = dict(lo=-1.5, hi=6.0, count=3.0, skipped=0.0)          # scale 7.5


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _case(name, K, Z=20.0):
    """(dims with the two-hot head, seed, engine hp, restatement hp), as tests/test_retnorm_gpu._case."""
    if name == "tiny_cat_actor":
        d, seed, hp = dataclasses.replace(synth.TINY, A=6, discrete_actions=True), 0, {}
    elif name in CAT_CASES:
        d, seed, hp, _ = CAT_CASES[name]
    else:
        d, seed, hp, _ = CASES[name]
    d = dataclasses.replace(d, critic_head="twohot", critic_bins=K, critic_bin_range=Z)
    hp = dict(hp, entropy_weight=0.1)
    ohp = dict(hp, critic_bins=K, critic_bin_range=Z)
    if d.categorical:
        ohp["categorical"] = (d.cat_D, d.cat_C)
    return d, seed, hp, ohp


# ------------------------------------------------------------------------------------------ against the restatement
_STEP_CASES = [("tiny", -1, 255, False), ("tiny", 0.0, 255, False), ("tiny", 0.5, 7, False), ("small", -1, 7, False),
               ("cat_tiny", -1, 255, False), ("tiny_cat_actor", 0.5, 255, False), ("tiny_discount", 0.1, 255, False),
               ("tiny_discount", -1, 7, False), ("tiny", 0.5, 255, True), ("small", -1, 7, True)]


@pytest.mark.parametrize("name,rho,K,pct", _STEP_CASES)
def test_train_steps_vs_restatement(name, rho, K, pct):
    """Two whole train steps: logs, clipped gradients, gradient norms and post-Adam weights of every parameter tensor
    against the CPU restatement at the tolerances of test_retnorm_gpu.test_train_steps_vs_restatement.  pct: percentile
    return normalisation from a preset range (scale 7.5) on top."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, ohp = _case(name, K)
    rn = dict(return_normalization="percentile", return_norm_decay=0.5) if pct else {}
    P = synth.make_params(d, seed)
    assert P["critic"]["model.8.weight"].shape[0] == K
    batch = synth.make_batch(d, seed)
    eng = DreamerEngine(d, dict(hp, gradient_mixing=rho, **rn), "cuda", params=P)
    assert not eng.heads_fused and eng.behaviour_plan(d.Hm, d.N) == (d.Hm,)
    cls = TwohotDiscreteOracleDreamer if d.discrete_actions else TwohotOracleDreamer
    od = cls(P, dict(ohp, planning_horizon=d.H, gradient_mixing=rho, **rn))
    if pct:
        eng.load_return_norm_state(PRESET)
        od.rn_state = dict(PRESET)
    db = _dev(batch)
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
            assert set(ologs) <= set(logs) and "value_loss" in ologs
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
        assert eng.W("critic", "model.8.weight").shape == (K, d.Hd)
    finally:
        print("\n".join(rep[-200:]))


def test_the_head_changes_the_critic_update_and_the_diagnostics_read_decoded_values():
    """The switch does something -- the value loss is a cross-entropy (about log K at a fresh critic), not the Normal's --
    and a diagnosed step logs the decoded critic values."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case("small", 255)
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed), diagnostics_interval=1)
    logs = dict(eng.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed))))
    torch.cuda.synchronize()
    assert abs(logs["value_loss"] - np.log(255)) < 0.5
    keys = [k for k in logs if k.startswith("critic_value") or k.startswith("imag_value") or k == "value_explained_variance"]
    assert keys and all(np.isfinite(logs[k]) for k in keys), keys
    mean_key = [k for k in keys if k.startswith("critic_value") and "mean" in k]
    if mean_key:        # decoded values of a fresh head are of order 1, not logits' sums
        assert abs(logs[mean_key[0]]) < 5.0


# ------------------------------------------------------------------------------------------ schedules
def _weights_equal(a, b, groups=("model", "actor", "critic", "critic_target")):
    for grp in groups:
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat), grp
        if ga.grad is not None:
            assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp


@pytest.mark.parametrize("name,rho,K", [("small", -1, 255), ("small", 0.1, 7), ("tiny_discount", 0.0, 255), ("cat_tiny", -1, 7)])
def test_pipelined_schedule_is_bit_identical_to_serial(name, rho, K):
    """Four un-synchronised steps, pipelined / serial / pipelined with the held-back optimiser steps: every weight, Adam
    moment and logged scalar."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name, K)
    P = synth.make_params(d, seed)
    engs = []
    for pipe, defer in ((True, False), (False, False), (True, True)):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.pipeline, eng.defer_opt = pipe, defer
        engs.append(eng)
    steps = 4
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
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


def test_update_critic_averages_the_wide_target():
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case("tiny", 7)
    eng = DreamerEngine(d, dict(hp, polyak_avg=0.25), "cuda", params=synth.make_params(d, seed))
    eng.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed)))
    torch.cuda.synchronize()
    tgt0 = {k: eng.W("critic_target", k).clone() for k in eng.state_dict("critic_target")}
    assert tgt0["model.8.weight"].shape == (7, d.Hd) and not torch.equal(tgt0["model.8.weight"], eng.W("critic", "model.8.weight"))
    eng.update_critic()
    torch.cuda.synchronize()
    for k, t0 in tgt0.items():
        want = 0.25 * eng.W("critic", k).double() + 0.75 * t0.double()
        assert (eng.W("critic_target", k).double() - want).abs().max() <= 2e-7 * max(1.0, float(want.abs().max())), k


# ------------------------------------------------------------------------------------------ the agent
def _agent(extra, seed, models=None, drop_keys=False):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    from big_dreamer_amd.engine import CRITIC_HEAD_KEYS
    from tests.test_checkpoint_gpu import ScriptedEnv, _overrides
    d = synth.SMALL
    params = load_config(_overrides(d, list(extra)) + ([f"models={models}"] if models else []))
    if drop_keys:
        for k in CRITIC_HEAD_KEYS:
            del params["ActorCritic"][k]
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    random.seed(seed + 2)
    return Dreamer(params, ScriptedEnv(d))


_TH = ["ActorCritic.critic_head=twohot", "ActorCritic.critic_bins=31", "ActorCritic.critic_bin_range=10.0"]


def test_normal_given_explicitly_is_an_agent_built_without_the_keys():
    from tests.test_checkpoint_gpu import Own, _assert_groups_equal, _fill
    a = _agent(["ActorCritic.critic_head=normal"], 5)
    b = _agent([], 5, drop_keys=True)
    assert a.dims == b.dims and a.dims.critic_out == 1 and a.engine.heads_fused == b.engine.heads_fused
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
    assert not any("row_loss" in k or "_val" in k or "logits" in k for k in a.engine._buf)


def test_value_decodes_the_logits():
    a = _agent(_TH, 5)
    d = a.dims
    g = torch.Generator().manual_seed(0)
    belief, state = torch.randn(4, 9, d.Be, generator=g).cuda(), torch.randn(4, 9, d.S, generator=g).cuda()
    for target in (False, True):
        mod = a.critic_target if target else a.critic
        logits = mod(belief, state)
        assert logits.shape == (4, 9, 31)
        v = a.value(belief, state, target=target)
        assert v.shape == (4, 9, 1)
        sd = {k: p.detach().cpu() for k, p in mod.state_dict().items()}
        from oracle import dreamer_oracle as O
        want = decode(O.dense_on_features(belief.cpu(), state.cpu(), sd), 10.0)
        assert_close(f"value target={target}", v.cpu().numpy(), want.numpy(), 2e-5, 5e-5)
    n = _agent([], 5)
    bn, sn = belief[..., :n.dims.Be], state[..., :n.dims.S]
    assert torch.equal(n.value(bn, sn), n.critic(bn, sn)) and n.value(bn, sn, target=True).shape == (4, 9, 1)


def test_resume_is_bit_identical_and_mismatched_heads_are_refused(tmp_path):
    from tests.test_checkpoint_gpu import Own, _assert_groups_equal, _fill
    a = _agent(_TH, 5)
    _fill(a.buffer, a.dims)
    for _ in range(2):
        la = dict(a.train_step())
    assert np.isfinite(la["value_loss"])
    models, replay = str(tmp_path / "models_2.pth"), str(tmp_path / "experience_2.npz")
    a.save(models, extra={"step": 2})
    a.buffer.save(replay)
    own_a = Own(a)
    saved = torch.load(models, map_location="cpu", weights_only=True)
    assert saved["run_state"]["critic_head"] == {"kind": "twohot", "bins": 31, "range": 10.0}
    assert saved["critic"]["model.8.weight"].shape[0] == 31
    b = _agent(_TH, 99, models=models)
    b.buffer.load(replay)
    assert b.load_run_state(models) == {"step": 2}
    own_b = Own(b)
    _assert_groups_equal(a, b)
    for _ in range(2):
        la, lb = own_a.run(lambda: dict(a.train_step())), own_b.run(lambda: dict(b.train_step()))
        assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
    _assert_groups_equal(a, b)
    # another K, another Z, the width-1 critic: refused with both heads named, before anything is copied
    for extra in (["ActorCritic.critic_head=twohot", "ActorCritic.critic_bins=7", "ActorCritic.critic_bin_range=10.0"],
                  ["ActorCritic.critic_head=twohot", "ActorCritic.critic_bins=31"], []):
        with pytest.raises(ValueError, match="critic head .*twohot.*31.* does not match"):
            _agent(extra, 7, models=models)
    plain = _agent([], 5)
    _fill(plain.buffer, plain.dims)
    dict(plain.train_step())
    default = str(tmp_path / "models_default.pth")
    plain.save(default, extra={"step": 1})
    assert "critic_head" not in torch.load(default, map_location="cpu", weights_only=True)["run_state"]
    with pytest.raises(ValueError, match="'kind': 'normal'.* does not match .*twohot"):
        _agent(_TH, 7, models=default)
    fresh = _agent(_TH, 11)
    before = fresh.fingerprint()
    with pytest.raises(ValueError):
        fresh.load({"models": default})
    assert fresh.fingerprint() == before            # nothing was copied


def test_main_trains_with_the_twohot_critic():
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), "ActorCritic.critic_head=twohot",
           "ActorCritic.return_normalization=percentile", "state_size=8", "belief_size=32", "hidden_size=32",
           "embedding_size=64", "batch_size=6", "seq_len=8", "planning_horizon=5", "experience_size=500", "seed_steps=100",
           "max_episode_length=30", "train_steps=140", "log_freq=10", "collect_interval=2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Initialized with" in out.stdout and "'value_loss': " in out.stdout and "'return_scale': " in out.stdout
