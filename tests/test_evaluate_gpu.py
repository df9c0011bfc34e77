"""GPU: evaluation episodes -- the frame kernel alone (csrc/video.hip: bd_eval_frame) bit for bit against
tests/eval_ref.py's frame_reference, Dreamer.evaluate / Planet.evaluate against the reference-shaped loop run by hand
with update_belief_and_act (src/main.py:199-272) under the same seeds, and the CLI's evaluation=true / test=true."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.eval_ref import frame_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVAL_KEYS = ("Eval_min_return", "Eval_avg_return", "Eval_max_return", "Eval_std_return")


# ---------------------------------------------------------------------------------------------- the kernel alone
def _frame_values(rng, shape):
    """Random values reaching past both clip bounds, with the exact bin edges k / 256 - 0.5, their fp32 neighbours on both
    sides and the clip bounds themselves mixed in at random places."""
    v = rng.uniform(-0.75, 0.75, shape).astype(np.float32)
    edges = np.arange(257, dtype=np.float32) / np.float32(256) - np.float32(0.5)
    special = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(1)),
                              np.array([-0.5, 0.5, -3.0, 7.0, 0.0, -0.0], np.float32)])
    flat = v.reshape(-1)
    flat[rng.choice(flat.size, special.size, replace=False)] = special
    return v


@pytest.mark.parametrize("n", [1, 3, 7])
def test_eval_frame_kernel_is_bit_identical_to_the_reference(n):
    from big_dreamer_amd import _cabi as cabi
    from big_dreamer_amd.evaluate import frame_shape
    rng = np.random.default_rng(40 + n)
    obs = _frame_values(rng, (n, 3, 64, 64))                    # NCHW, as uploaded for the encoder
    dec = _frame_values(rng, (n, 64, 64, 3))                    # NHWC, as the conv stack leaves it
    want = frame_reference(obs, dec.transpose(0, 3, 1, 2))
    assert want.shape == frame_shape(n) and want.max() == 255 and want.min() == 0
    video = torch.full((3,) + frame_shape(n), 0xFF, dtype=torch.uint8, device="cuda")
    o, d = torch.from_numpy(obs).cuda(), torch.from_numpy(dec).cuda()
    cabi.check(cabi.lib.bd_eval_frame(o.data_ptr(), d.data_ptr(), n, video.data_ptr(), 3, 1, cabi.stream()))
    got = video.cpu().numpy()
    assert (got[0] == 0xFF).all() and (got[2] == 0xFF).all()     # the neighbouring frames are untouched
    assert np.array_equal(got[1], want), int((got[1] != want).sum())
    # argument checks come back as error codes, before any launch
    for bad in ((None, d.data_ptr(), n, video.data_ptr(), 3, 1), (o.data_ptr(), d.data_ptr(), 0, video.data_ptr(), 3, 1),
                (o.data_ptr(), d.data_ptr(), n, video.data_ptr(), 3, 3), (o.data_ptr(), d.data_ptr(), n, video.data_ptr(), 3, -1),
                (o.data_ptr(), d.data_ptr(), n, video.data_ptr() + 1, 3, 1)):
        assert cabi.lib.bd_eval_frame(*bad, cabi.stream()) != 0
    assert np.array_equal(video.cpu().numpy(), got)


# ---------------------------------------------------------------------------------------------- agents
TINY = ["belief_size=32", "hidden_size=32", "embedding_size=64", "state_size=6", "synthetic_env_action_size=2",
        "synthetic_env_observation_size=3", "batch_size=3", "seq_len=4", "planning_horizon=4", "experience_size=100",
        "max_episode_length=8", "action_repeat=2"]


def _agent(extra=(), cls="dreamer", seed=3):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import Env
    from big_dreamer_amd.planet import Planet
    params = load_config(TINY + list(extra))
    torch.manual_seed(seed)                                      # the weights: PyTorch's default initialisation
    return {"dreamer": Dreamer, "dreamerV2": DreamerV2, "planet": Planet}[cls](params, Env(params))


def _reseed(agent, seed=11):
    torch.manual_seed(seed)
    agent.engine.set_noise_seed(seed)


def _hand_loop(agent, n, frames=False):
    """src/main.py:199-272 as written there, on this library's EnvBatcher."""
    from big_dreamer_amd.env import Env, EnvBatcher
    p, dev = agent.params, agent.device
    envs = EnvBatcher(Env, p, n)
    observation = envs.reset()
    total, video, steps = np.zeros((n,)), [], 0
    belief = torch.zeros(n, p["belief_size"], device=dev)
    state = torch.zeros(n, agent.state_size, device=dev)
    action = torch.zeros(n, agent.env.action_size, device=dev)
    for _ in range(p["max_episode_length"] // p["action_repeat"]):
        belief, state, action, next_observation, reward, done = agent.update_belief_and_act(
            envs, belief, state, action, observation.to(device=dev))
        total += reward.numpy()
        steps += 1
        if frames:
            video.append(frame_reference(observation.numpy(), agent.observation_model(belief, state).cpu().numpy()))
        observation = next_observation
        if done.sum().item() == n:
            break
    envs.close()
    return total, belief.clone(), steps, video


def _evaluate_and_compare(agent, n, monkeypatch, video=False):
    """evaluate() under a seed, then the hand-run loop under the same seed: returns and final belief bit for bit."""
    last, inner = {}, agent.update_belief_and_act

    def recording(*a, **kw):
        out = inner(*a, **kw)
        last["belief"] = out[0].clone()
        return out

    _reseed(agent)
    with monkeypatch.context() as m:
        m.setattr(agent, "update_belief_and_act", recording)
        res = agent.evaluate(episodes=n, video=video)
    _reseed(agent)
    total, belief, steps, frames = _hand_loop(agent, n, frames=video)
    assert res["steps"] == steps
    assert res["returns"].shape == (n,) and np.array_equal(res["returns"], total), (res["returns"], total)
    assert torch.equal(last["belief"], belief)
    assert np.isfinite(total).all() and len(set(total.tolist())) > 1        # the episodes differ: sampled actions
    assert res["Eval_avg_return"] == total.mean() and res["Eval_std_return"] == total.std()
    assert res["Eval_min_return"] == total.min() and res["Eval_max_return"] == total.max()
    return res, frames


@pytest.mark.parametrize("fused", ["1", "0"])
def test_evaluate_state_agent_equals_the_hand_run_loop(fused, monkeypatch):
    monkeypatch.setenv("BD_ACT_FUSED", fused)
    agent = _agent()
    assert (agent.belief_size, agent.hidden_size, agent.embedding_size, agent.state_size, agent.action_size,
            agent.env.observation_size) == (32, 32, 64, 6, 2, 3)
    res, _ = _evaluate_and_compare(agent, 3, monkeypatch)
    assert res["steps"] == 4 and res["video"] is None
    assert agent.evaluate(episodes=3, video=True)["video"] is None          # video is for pixel observations only


def test_evaluate_pixel_agent_video_equals_the_hand_built_frames(monkeypatch):
    agent = _agent(["pixel_observation=true", "embedding_size=1024", "max_episode_length=6"])
    res, frames = _evaluate_and_compare(agent, 7, monkeypatch, video=True)
    assert res["steps"] == 3 and len(frames) == 3
    assert res["video"].dtype == np.uint8 and res["video"].shape == (3, 3, 134, 652)
    for t in range(3):
        assert np.array_equal(res["video"][t], frames[t]), (t, int((res["video"][t] != frames[t]).sum()))
    assert len({f.tobytes() for f in frames}) == 3                           # the frames differ from step to step
    assert agent.evaluate(episodes=7)["video"] is None


@pytest.mark.parametrize("fused", ["0", "1"])
def test_evaluate_categorical_agent_equals_the_hand_run_loop(fused, monkeypatch):
    monkeypatch.setenv("BD_ACT_FUSED_CAT", fused)
    agent = _agent(["algorithm=dreamerV2", "latent_distribution=Categorical", "discrete_latent_dimensions=3",
                    "discrete_latent_classes=5", "action_distribution=Categorical", "synthetic_env_action_size=3"],
                   cls="dreamerV2")
    assert agent.state_size == 15 and agent.action_size == 3
    res, _ = _evaluate_and_compare(agent, 3, monkeypatch)
    assert res["steps"] == 4


def test_evaluate_planet_equals_the_hand_run_loop(monkeypatch):
    agent = _agent(["algorithm=planet", "MPC.optimisation_iters=2", "MPC.candidates=32", "MPC.top_candidates=4"], cls="planet")
    assert agent.planning_horizon == 4
    res, _ = _evaluate_and_compare(agent, 2, monkeypatch)
    assert res["steps"] == 4


# ---------------------------------------------------------------------------------------------- the CLI
CLI = TINY + ["seed_steps=48", "train_steps=61", "log_freq=10", "collect_interval=2", "experience_size=300",
              "test_episodes=3", "test_interval=5"]


def _main(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *CLI, *extra], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_cli_evaluation_switch():
    off = _main()
    assert "Eval_" not in off and "model_loss" in off
    on = _main("evaluation=true")
    first = int(re.search(r"Initialized with \d+ episodes and (\d+) steps", on).group(1))
    crossed = sum(1 for step in range(first, 61) if step % 5 == 0)
    assert crossed >= 2
    for key in EVAL_KEYS:
        values = re.findall(rf"^{key} : (\S+)$", on, flags=re.M)
        assert len(values) == crossed, (key, values)
        assert all(np.isfinite(float(v)) for v in values)
    assert "model_loss" in on


def test_cli_test_mode_evaluates_a_saved_checkpoint_and_exits(tmp_path):
    agent = _agent()
    path = str(tmp_path / "models.pth")
    agent.save(path)
    out = _main("test=true", f"models={path}")
    for key in EVAL_KEYS:
        assert len(re.findall(rf"^{key} : \S+$", out, flags=re.M)) == 1, out
    assert "Initialized with" not in out and "model_loss" not in out          # no replay fill, no training log line
