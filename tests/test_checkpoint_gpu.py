"""GPU: checkpoint and resume ("Checkpoint and resume").  An agent rebuilt from models_<step>.pth, experience_<step>.npz
and load_run_state continues exactly where the original stands: the same kernels run on the same inputs with the same Philox
counters, so every comparison is exact (torch.equal, == on the log dicts) and there is no tolerance anywhere in this file."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import checkpoint as ck
from big_dreamer_amd import synth
from big_dreamer_amd.config import load_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, SIZE = 200, 300                                  # a partly filled ring: rows [0, 200) of 300


def _overrides(d, extra=()):
    return [f"belief_size={d.Be}", f"state_size={d.S}", f"hidden_size={d.Hd}", f"embedding_size={d.E}",
            f"batch_size={d.B}", f"seq_len={d.L}", f"planning_horizon={d.H}", f"experience_size={SIZE}", *extra]


# name -> (dims, overrides, what to set in the environment of the process)
CASES = {
    "state": (synth.SMALL, [], {"BD_ACT_FUSED": None}),                                   # the fused acting step (default)
    "pixel": (synth.TINY_PIXEL, ["pixel_observation=true"], {}),
    "categorical": (synth.CAT_TINY, ["algorithm=dreamerV2", "latent_distribution=Categorical",
                                     f"discrete_latent_dimensions={synth.CAT_TINY.cat_D}",
                                     f"discrete_latent_classes={synth.CAT_TINY.cat_C}", "action_distribution=Categorical"],
                    {"BD_ACT_FUSED_CAT": "1"}),                                           # bd_act_step_cat
    "planet": (synth.TINY, ["algorithm=planet", "MPC.candidates=32", "MPC.top_candidates=8", "MPC.optimisation_iters=2"], {}),
}


class ScriptedEnv:
    """Returns fixed observations whatever the action; keeps the actions it was given."""

    def __init__(self, d, seed=3):
        self.action_size, self.observation_size = d.A, d.O
        rng = np.random.Generator(np.random.PCG64(seed))
        shape = (8, 1, 3, 64, 64) if d.pixel else (8, 1, d.O)
        obs = rng.random(shape, dtype=np.float32) - 0.5 if d.pixel else rng.standard_normal(shape, dtype=np.float32)
        self.script, self.t, self.got = torch.from_numpy(obs), 0, []

    def step(self, action):
        self.got.append(action.clone())
        self.t += 1
        return self.script[self.t % 8], -0.25 * self.t, False


def _agent(case, seed, models=None):
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.planet import Planet
    d, extra, _ = CASES[case]
    params = load_config(_overrides(d, extra) + ([f"models={models}"] if models else []))
    torch.manual_seed(seed)
    np.random.seed(seed + 1)
    random.seed(seed + 2)
    cls = {"planet": Planet, "dreamer": Dreamer, "dreamerV2": DreamerV2}[params["algorithm"]]
    return cls(params, ScriptedEnv(d))


def _fill(buf, d, seed=2):
    """Rows [0, ROWS) from synth.make_replay (pixels: 5-bit quantised uint8 frames, discrete actions: one-hot)."""
    rep = synth.make_replay(d, rows=ROWS, seed=seed)
    if d.pixel:
        rng = np.random.Generator(np.random.PCG64(seed + 50))
        rep["observations"] = (rng.integers(0, 32, size=(ROWS, 3, 64, 64)) * 8).astype(np.uint8)
    if d.discrete_actions:
        rep["actions"] = np.eye(d.A, dtype=np.float32)[rep["actions"].argmax(-1)]
    for k, v in rep.items():
        getattr(buf, k)[:ROWS] = v
    buf.idx, buf.full, buf.steps, buf.episodes = ROWS, False, ROWS, 4
    buf.mark_dirty()


def _set_env(monkeypatch, case):
    for k, v in CASES[case][2].items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _decide(agent, carry, explore=True):
    """One update_belief_and_act on the scripted environment from `carry` = (belief, state, action, observation)."""
    belief, state, action, obs = carry
    belief, state, action, nxt, _, _ = agent.update_belief_and_act(agent.env, belief, state, action, obs, explore=explore)
    return belief.clone(), state.clone(), action.clone(), nxt


def _start(agent):
    dev = agent.device
    return (torch.zeros(1, agent.belief_size, device=dev), torch.zeros(1, agent.state_size, device=dev),
            torch.zeros(1, agent.action_size, device=dev), agent.env.script[0])


def _groups(agent):
    names = ("model",) if type(agent).__name__ == "Planet" else ("model", "actor", "critic")
    torch.cuda.synchronize()
    out = {}
    for g in names:
        grp = agent.engine.groups[g]
        out[g] = (grp.flat.clone(), grp.m.clone(), grp.v.clone(), int(grp.step))
    out["critic_target"] = (agent.engine.groups["critic_target"].flat.clone(),)
    return out


def _assert_groups_equal(a, b):
    ga, gb = _groups(a), _groups(b)
    for g in ga:
        for x, y in zip(ga[g], gb[g]):
            assert (x == y) if isinstance(x, int) else torch.equal(x, y), g


class Own:
    """Two agents in one process share the process's generators (numpy for the replay's index draws, torch's device
    generator for the composed acting path), two runs do not.  ``Own(agent).run(f)`` calls f with the generators where this
    agent's last call left them, so each agent sees the stream of draws it would see alone in a process."""

    def __init__(self, agent):
        self.agent, self.state = agent, ck.capture_generators(agent.device)

    def run(self, f, *args):
        ck.restore_generators(self.state, self.agent.device)
        out = f(*args)
        self.state = ck.capture_generators(self.agent.device)
        return out


def _run_until_checkpoint(case, tmp_path):
    """Agent `a` under seed 5: three train steps on Philox noise, two decisions, then models_3.pth and experience_3.npz.
    Returns Own(a) as of the save, the episode in flight and the two paths."""
    a = _agent(case, 5)
    _fill(a.buffer, a.dims)
    for _ in range(3):
        dict(a.train_step())
    carry = _start(a)
    for _ in range(2):
        carry = _decide(a, carry)
    models, replay = ck.models_path(str(tmp_path), 3), ck.experience_path(str(tmp_path), 3)
    a.save(models, extra={"step": 3, "collect_envs": 1})
    a.buffer.save(replay)
    return Own(a), carry, models, replay


@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_exact_at_the_api(case, tmp_path, monkeypatch):
    _set_env(monkeypatch, case)
    own_a, carry, models, replay = _run_until_checkpoint(case, tmp_path)
    a = own_a.agent
    if case == "state":
        assert a.act_fused
    if case == "categorical":
        assert a.act_fused_cat
    # the whole file loads with the loader that executes nothing from it, and still holds every key of the old layout
    d = torch.load(models, map_location="cpu", weights_only=True)
    assert set(d) >= {"transition_model", "observation_model", "reward_model", "encoder", "model_optimizer", "actor",
                      "critic", "critic_target", "actor_optimizer", "value_optimizer", "run_state"}
    assert d["run_state"]["extra"] == {"step": 3, "collect_envs": 1}
    noise = a.engine.noise_state()
    assert d["run_state"]["noise"] == noise and noise["seed"] is not None and noise["step"]["wm"] == 3
    if case != "planet" and (a.act_fused or a.act_fused_cat):
        assert noise["step"]["act"] == 2                 # the two decisions drew from the acting streams
    if a.dims.pixel:
        assert a.buffer._pix_step == 3 and a.buffer._pix_seed is not None

    b = _agent(case, 99, models=models)                  # other weights, other generators: everything comes from the files
    b.buffer.load(replay)
    assert b.load_run_state(models) == {"step": 3, "collect_envs": 1}
    own_b = Own(b)
    assert b.engine.noise_state() == noise
    assert (b.buffer._pix_step, b.buffer._pix_seed) == (a.buffer._pix_step, a.buffer._pix_seed)
    _assert_groups_equal(a, b)

    ca = cb = carry                                      # the caller owns the episode in flight: both go on from a's,
    b.env.t = a.env.t                                    # on a scripted environment at the same point of its script
    for _ in range(2):
        la, lb = own_a.run(lambda: dict(a.train_step())), own_b.run(lambda: dict(b.train_step()))
        assert la == lb and all(np.isfinite(v) for v in la.values()), (la, lb)
        ca, cb = own_a.run(_decide, a, ca), own_b.run(_decide, b, cb)
        for x, y in zip(ca[:3], cb[:3]):
            assert torch.equal(x, y)
        assert torch.equal(a.env.got[-1], b.env.got[-1])
    _assert_groups_equal(a, b)
    assert a.engine.noise_state() == b.engine.noise_state()
    assert a.engine.noise_state() != noise


def test_resume_needs_the_run_state(tmp_path, monkeypatch):
    """Weights, optimisers and replay alone -- what the parent of this change restores -- do not give the next step."""
    _set_env(monkeypatch, "state")
    own_a, _, models, replay = _run_until_checkpoint("state", tmp_path)
    a = own_a.agent
    c = _agent("state", 99, models=models)
    c.buffer.load(replay)
    _assert_groups_equal(a, c)
    lc = dict(c.train_step())
    la = own_a.run(lambda: dict(a.train_step()))
    assert la != lc, la


def test_models_alone_leaves_generators_and_noise_alone(tmp_path, monkeypatch):
    _set_env(monkeypatch, "state")
    a, models = _run_until_checkpoint("state", tmp_path)[0].agent, ck.models_path(str(tmp_path), 3)
    b = _agent("state", 99)
    b.engine.set_noise_seed(1234)
    b.engine._rng_step["wm"] = 11

    def snapshot():
        g = ck.capture_generators(b.device)
        return (g["torch_cpu"], g["torch_device"], g["numpy"]["keys"], g["python"]["words"], g["numpy"]["pos"],
                b.engine.noise_state())

    before = snapshot()
    b.load({"models": models})
    after = snapshot()
    for x, y in zip(before, after):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
    _assert_groups_equal(a, b)                           # ... and the weights and optimisers did arrive


def test_checkpoint_without_run_state_cannot_be_resumed(tmp_path, monkeypatch):
    _set_env(monkeypatch, "state")
    a, models = _run_until_checkpoint("state", tmp_path)[0].agent, ck.models_path(str(tmp_path), 3)
    d = torch.load(models, map_location="cpu", weights_only=True)
    del d["run_state"]
    old = str(tmp_path / "old_layout.pth")
    torch.save(d, old)
    b = _agent("state", 99, models=old)                  # models= still loads it
    _assert_groups_equal(a, b)
    before = b.engine.noise_state()
    with pytest.raises(ValueError, match="run_state"):
        b.load_run_state(old)
    assert b.engine.noise_state() == before


def test_extra_must_be_flat(tmp_path):
    a = _agent("state", 5)
    with pytest.raises(ValueError, match="extra"):
        a.save(str(tmp_path / "m.pth"), extra={"step": [1]})
    assert os.listdir(tmp_path) == []


# ---------------------------------------------------------------------------------------------- the CLI
TINY = ["belief_size=32", "hidden_size=32", "embedding_size=64", "state_size=6", "synthetic_env_action_size=2",
        "synthetic_env_observation_size=3", "batch_size=3", "seq_len=4", "planning_horizon=4", "experience_size=100",
        "max_episode_length=8", "action_repeat=2", "environment_steps_per_update=1", "collect_interval=1", "log_freq=1",
        "seed_steps=24"]
K = 28                                                   # the checkpointed step: seed phase ends at 24, k + 3 = 31
LOSSES = ("observation_loss", "reward_loss", "kl_loss", "model_loss", "actor_loss", "policy_entropy", "value_loss")


def _main(*extra, cwd=None):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *TINY, *extra], capture_output=True, text=True,
                         timeout=300, cwd=cwd)
    return out


def _log_lines(stdout):
    """{step: {loss: text as printed}} of the loop's log lines."""
    out = {}
    for line in stdout.splitlines():
        m = re.match(r"^(\d+) \{(.*)\}$", line)
        if m:
            out[int(m.group(1))] = {k: re.search(rf"'{k}': ([^,}}]+)", m.group(2)).group(1) for k in LOSSES}
    return out


def test_cli_checkpoint_and_resume(tmp_path):
    ckdir = tmp_path / "ck"
    cwd = tmp_path / "cwd"
    cwd.mkdir()
    u = _main(f"train_steps={K + 3}", cwd=str(cwd))
    assert u.returncode == 0, u.stderr[-2000:]
    assert os.listdir(cwd) == [] and not ckdir.exists()              # none of the new keys: no file anywhere
    assert "Initialized with 3 episodes and 24 steps" in u.stdout
    lu = _log_lines(u.stdout)
    assert sorted(lu) == list(range(24, K + 3))
    a = _main(f"train_steps={K + 1}", f"checkpoint_dir={ckdir}", f"checkpoint_interval={K}", "checkpoint_experience=true",
              cwd=str(cwd))
    assert a.returncode == 0, a.stderr[-2000:]
    assert sorted(os.listdir(ckdir)) == [f"experience_{K}.npz", f"models_{K}.pth"] and os.listdir(cwd) == []
    la = _log_lines(a.stdout)
    assert la == {s: lu[s] for s in range(24, K + 1)}                # checkpointing changes nothing a run computes
    b = _main("resume=true", f"models={ckdir}/models_{K}.pth", f"experience_replay={ckdir}/experience_{K}.npz",
              f"train_steps={K + 3}", cwd=str(cwd))
    assert b.returncode == 0, b.stderr[-2000:]
    assert "Initialized with" not in b.stdout
    lb = _log_lines(b.stdout)
    assert sorted(lb) == [K + 1, K + 2]
    first = [l for l in b.stdout.splitlines() if re.match(r"^\d+ \{", l)][0]
    assert first.startswith(f"{K + 1} ")
    assert lb[K + 1] == lu[K + 1], (lb[K + 1], lu[K + 1])
    # resume=true without models= is refused
    r = _main("resume=true", f"train_steps={K + 3}", cwd=str(cwd))
    assert r.returncode != 0 and "resume=true needs models=" in r.stderr


def test_cli_checkpoint_and_resume_collect_envs(tmp_path):
    """collect_envs=4: one iteration is four steps, [48, 52), [52, 56), [56, 60), [60, 64), ...; the multiples of 10 fall into
    the first and the fourth, whose checkpoints carry the iteration's first step; checkpoint_keep=1 leaves the newer."""
    ckdir = tmp_path / "ck"
    common = ["collect_envs=4", "checkpoint_interval=10", "seed_steps=48"]       # six rows per lane: more than seq_len
    u = _main(*common, "train_steps=72")
    a = _main(*common, "train_steps=64", f"checkpoint_dir={ckdir}", "checkpoint_experience=true", "checkpoint_keep=1")
    assert u.returncode == 0 and a.returncode == 0, u.stderr[-2000:] + a.stderr[-2000:]
    assert sorted(os.listdir(ckdir)) == ["experience_60.npz", "models_60.pth"]
    resume = ["resume=true", f"models={ckdir}/models_60.pth", f"experience_replay={ckdir}/experience_60.npz", "train_steps=72"]
    b = _main(*common, *resume)
    assert b.returncode == 0, b.stderr[-2000:]
    assert "Initialized with" not in b.stdout
    lu, lb = _log_lines(u.stdout), _log_lines(b.stdout)
    assert sorted(lb) == [64, 68] and lb[64] == lu[64], (lb, lu)
    r = _main("collect_envs=2", "checkpoint_interval=10", "seed_steps=48", *resume)
    assert r.returncode != 0 and "collect_envs=4" in r.stderr and "collect_envs=2" in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- two ranks
def test_two_ranks_checkpoint_and_resume(tmp_path):
    """Two processes on one GPU (gloo): save is collective and issues the held-back actor / critic updates; a second pair
    of processes loads the per-rank files and reproduces the first pair's next step on both ranks."""
    env = dict(os.environ, CK_DIR=str(tmp_path), OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for phase, port in (("first", 29641), ("second", 29642)):
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "tests", "checkpoint_dp_worker.py")]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=dict(env, CK_PHASE=phase), cwd=ROOT)
        assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
        for r in (0, 1):
            assert f"CKPT_DP_OK phase={phase} rank={r}" in out.stdout, out.stdout[-1500:]
        if phase == "first":
            assert sorted(n for n in os.listdir(tmp_path) if not n.startswith("after_")) == [
                "experience_2_rank0.npz", "experience_2_rank1.npz", "models_2_rank0.pth", "models_2_rank1.pth"]
