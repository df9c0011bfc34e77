"""CPU: the evaluation loop's host side -- EnvBatcher against the reference's own record (tests/golden/env_batcher.npz, made
by tests/gen_golden_eval.py), the video frame's geometry (tests/eval_ref.py: frame_reference, the statement bd_eval_frame is
held to on the GPU), evaluate.run_evaluation under a stub agent, and the two new configuration keys."""
import numpy as np
import pytest
import torch

from tests.eval_ref import (SCRIPT_FINISH, SCRIPT_N, SCRIPT_STEPS, ScriptedEnv, StubAgent, frame_geometry, frame_reference,
                            quantise, script_actions, script_params, script_reward)
from tests.helpers import load_golden


# ---------------------------------------------------------------------------------------------- EnvBatcher
def test_env_batcher_matches_the_reference_record():
    from big_dreamer_amd.env import EnvBatcher
    g = load_golden("env_batcher")
    params = script_params()
    batch = EnvBatcher(ScriptedEnv, params, SCRIPT_N)
    assert batch.n == int(g["n"]) and len(batch.envs) == SCRIPT_N
    assert batch.dones == g["initial_dones"].tolist() == [True] * SCRIPT_N
    first = batch.reset()
    assert str(first.dtype) == str(g["reset.dtype"]) and tuple(first.shape) == g["reset"].shape
    assert np.array_equal(first.numpy(), g["reset"])
    assert batch.dones == [False] * SCRIPT_N
    for t in range(1, SCRIPT_STEPS + 1):
        o, r, d = batch.step(script_actions(t))
        for name, got in (("observations", o), ("rewards", r), ("dones", d)):
            want = g[name][t - 1]
            assert str(got.dtype) == str(g[name + ".dtype"]), (name, t, got.dtype)
            assert tuple(got.shape) == want.shape, (name, t, tuple(got.shape))
            assert np.array_equal(got.numpy(), want), (name, t, got, want)
        assert [bool(x) for x in batch.dones] == g["sticky"][t - 1].tolist()
    # every environment was stepped at every call, finished ones included, each with its own row of the actions
    assert np.array_equal(np.stack([np.stack(e.actions) for e in batch.envs]), g["actions_seen"])
    batch.close()
    assert params["closed"] == int(g["closed"]) == SCRIPT_N


def test_env_batcher_record_shows_the_semantics():
    """The record itself: the blanking mask is `dones` BEFORE the call (the finishing step keeps its values), dones stick."""
    g = load_golden("env_batcher")
    for i, fin in enumerate(SCRIPT_FINISH):
        for t in range(1, SCRIPT_STEPS + 1):
            blank = fin and t > fin
            assert g["rewards"][t - 1, i] == (0.0 if blank else script_reward(i, t))
            assert (g["observations"][t - 1, i] == 0).all() == bool(blank)
            assert g["dones"][t - 1, i] == int(bool(fin) and t >= fin)


# ---------------------------------------------------------------------------------------------- frame geometry
SHAPES = {1: (3, 64, 128), 3: (3, 68, 392), 5: (3, 68, 652), 7: (3, 134, 652), 10: (3, 134, 652)}


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_frame_geometry(n):
    from big_dreamer_amd.evaluate import frame_shape
    assert frame_shape(n) == SHAPES[n]
    GH, GW, origins = frame_geometry(n)
    assert (3, GH, GW) == SHAPES[n] and len(origins) == n
    xmaps = min(5, n)
    for k, (r, c) in enumerate(origins):
        assert (r, c) == ((0, 0) if n == 1 else ((k // xmaps) * 66 + 2, (k % xmaps) * 130 + 2))
    # hand-built input: tile k is the constant pair (real 2k + 1, predicted 2k + 2) as bytes; everything else is 0
    level = lambda b: np.float32((b + 0.5) / 256 - 0.5)                     # the middle of byte b's bin
    obs = np.stack([np.full((3, 64, 64), level(2 * k + 1), np.float32) for k in range(n)])
    dec = np.stack([np.full((3, 64, 64), level(2 * k + 2), np.float32) for k in range(n)])
    frame = frame_reference(obs, dec)
    assert frame.shape == SHAPES[n] and frame.dtype == np.uint8
    covered = np.zeros(frame.shape, bool)
    for k, (r, c) in enumerate(origins):
        assert (frame[:, r:r + 64, c:c + 64] == 2 * k + 1).all() and (frame[:, r:r + 64, c + 64:c + 128] == 2 * k + 2).all()
        assert not covered[:, r:r + 64, c:c + 128].any()                    # tiles do not overlap
        covered[:, r:r + 64, c:c + 128] = True
    assert (frame[~covered] == 0).all() and int(covered.sum()) == n * 3 * 64 * 128
    if n > 1:       # two padding bytes round every tile
        for r, c in origins:
            assert not covered[:, r - 2:r, :].any() and not covered[:, :, c - 2:c].any()
        assert not covered[:, GH - 2:, :].any() and not covered[:, :, GW - 2:].any()


def test_frame_channels_and_orientation():
    """Not a constant: channel, row and column of both halves land where make_grid(cat(dim=3)) puts them."""
    rng = np.random.default_rng(0)
    obs = rng.uniform(-0.5, 0.5, (3, 3, 64, 64)).astype(np.float32)
    dec = rng.uniform(-0.5, 0.5, (3, 3, 64, 64)).astype(np.float32)
    frame = frame_reference(obs, dec)
    for k, c, y, x in ((0, 0, 0, 0), (1, 2, 63, 5), (2, 1, 17, 63)):
        assert frame[c, 2 + y, 2 + 130 * k + x] == quantise(obs[k, c, y, x])
        assert frame[c, 2 + y, 2 + 130 * k + 64 + x] == quantise(dec[k, c, y, x])


def test_quantise_is_postprocess_observation_at_8_bits():
    edges = (np.arange(257, dtype=np.float32) / np.float32(256)) - np.float32(0.5)          # k / 256 - 0.5: exact in fp32
    assert np.array_equal(quantise(edges[:256]), np.arange(256, dtype=np.uint8))
    # fp32 arithmetic: the largest float below an edge may round onto it in `v + 0.5` (the spacing of v is finer than that of
    # the sum), so it lands in either bin -- never further; just below 0 it does round up (0.5 - 1e-45 is 0.5)
    below = quantise(np.nextafter(edges[1:256], np.float32(-1))).astype(int)
    assert ((below == np.arange(255)) | (below == np.arange(1, 256))).all() and below[127] == 128
    assert quantise(np.float32(0.5)) == 255 and quantise(np.float32(7.0)) == 255 and quantise(np.float32(-3.0)) == 0
    v = np.random.default_rng(1).uniform(-0.7, 0.7, 1000).astype(np.float32)
    want = np.clip(np.floor((v + 0.5) * 2 ** 8) * 2 ** (8 - 8), 0, 2 ** 8 - 1).astype(np.uint8)    # src/utils.py:333-337
    assert np.array_equal(quantise(v), want)


# ---------------------------------------------------------------------------------------------- run_evaluation
def _run(finish, max_steps, **kw):
    from big_dreamer_amd.env import EnvBatcher
    from big_dreamer_amd.evaluate import run_evaluation
    params = script_params(finish)
    agent = kw.pop("agent", None) or StubAgent()
    envs = EnvBatcher(ScriptedEnv, params, len(finish))
    return run_evaluation(agent, envs, max_steps, **kw), agent, params


def _sum(i, last):
    return sum(script_reward(i, t) for t in range(1, last + 1))


def test_run_evaluation_runs_the_full_length_when_one_env_never_finishes():
    res, agent, params = _run(SCRIPT_FINISH, SCRIPT_STEPS)
    assert res["steps"] == SCRIPT_STEPS == len(agent.calls)
    want = np.array([_sum(0, 2), _sum(1, 4), _sum(2, SCRIPT_STEPS), _sum(3, 2)])       # rewards up to and including `done`
    assert res["returns"].shape == (SCRIPT_N,) and np.array_equal(res["returns"], want)
    assert res["Eval_min_return"] == want.min() and res["Eval_max_return"] == want.max()
    assert res["Eval_avg_return"] == want.mean()
    assert res["Eval_std_return"] == want.std() == np.sqrt(((want - want.mean()) ** 2).mean())    # population std (ddof 0)
    assert res["Eval_std_return"] != want.std(ddof=1)
    for k in ("Eval_min_return", "Eval_avg_return", "Eval_max_return", "Eval_std_return"):
        assert type(res[k]) is float
    assert res["video"] is None
    assert set(res) == {"Eval_min_return", "Eval_avg_return", "Eval_max_return", "Eval_std_return", "returns", "steps", "video"}
    assert params["closed"] >= SCRIPT_N                                              # the envs were closed


def test_run_evaluation_stops_once_every_env_is_done():
    finish = (2, 4, 3, 2)
    res, agent, _ = _run(finish, 50)
    assert res["steps"] == 4 == len(agent.calls)
    assert np.array_equal(res["returns"], np.array([_sum(i, f) for i, f in enumerate(finish)]))


def test_run_evaluation_start_state_and_call_protocol():
    res, agent, _ = _run(SCRIPT_FINISH, 3)
    assert res["steps"] == 3
    first = agent.calls[0]
    assert tuple(first["belief"].shape) == (SCRIPT_N, agent.belief_size) and not first["belief"].any()
    assert tuple(first["state"].shape) == (SCRIPT_N, agent.state_size) and not first["state"].any()      # agent.state_size columns
    assert tuple(first["action"].shape) == (SCRIPT_N, agent.action_size) and not first["action"].any()
    assert np.array_equal(first["observation"].numpy(), load_golden("env_batcher")["reset"])
    # what a call returns is what the next one gets
    second = agent.calls[1]
    assert (second["belief"] == 1).all() and (second["state"] == 2).all() and torch.equal(second["action"], script_actions(1))
    assert np.array_equal(second["observation"].numpy(), load_golden("env_batcher")["observations"][0])
    assert all(c["explore"] is False for c in agent.calls)
    assert agent.modes == ["eval", "act", "act", "act", "train"]


def test_run_evaluation_passes_noise_only_when_given():
    res, agent, _ = _run(SCRIPT_FINISH, 2, agent=StubAgent(takes_noise=False))          # a Planet-like signature: no _noise keyword
    assert res["steps"] == 2 and all(c["kw"] == {} for c in agent.calls)
    seen = []
    noise = lambda t: seen.append(t) or {"post": t}
    res, agent, _ = _run(SCRIPT_FINISH, 3, _noise=noise)
    assert seen == [0, 1, 2]
    assert [c["kw"] for c in agent.calls] == [{"_noise": {"post": t}} for t in range(3)]


# ---------------------------------------------------------------------------------------------- configuration
def test_config_keys():
    from big_dreamer_amd.config import load_config
    p = load_config([])
    assert p["evaluation"] is False and p["eval_video_dir"] == ""
    assert p["test"] is False and p["test_interval"] == 25 and p["test_episodes"] == 10 and p["log_video_freq"] == -1
    q = load_config(["evaluation=true", "eval_video_dir=videos", "test=true"])
    assert q["evaluation"] is True and q["eval_video_dir"] == "videos" and q["test"] is True
