"""GPU: collecting from N environments at once -- the append kernel alone (csrc/replay.hip: bd_replay_append) against numpy on
state observations and on pixels, the laned ExperienceReplay's device mirror against its host arrays, the Collector on a
real agent, and the CLI's collect_envs.  Every comparison is bit-exact: each path is a copy or the fp32 operation sequence of
ExperienceReplay.append."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 40                                                    # rows of the kernel tests' mirror


def _bits(x):
    """The bytes of an array: equality of these is bit equality (NaN payloads and signed zeros included)."""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.uint8)


def _quantise(o, bits):
    """The expression of ExperienceReplay.append (big_dreamer_amd/memory.py) on a float32 array."""
    assert o.dtype == np.float32
    return np.clip(np.floor((o + 0.5) * 2 ** bits) * 2 ** (8 - bits), 0, 2 ** 8 - 1).astype(np.uint8)


class _Mirror:
    """A sentinel-filled device mirror of SIZE rows with its expected numpy twin."""

    def __init__(self, width, A, bits):
        self.width, self.A, self.bits = width, A, bits
        if bits:
            obs = (np.arange(SIZE * width) % 251).astype(np.uint8).reshape(SIZE, width)
        else:
            obs = -1000.0 - np.arange(SIZE * width, dtype=np.float32).reshape(SIZE, width)
        self.want = {"obs": obs, "act": -2000.0 - np.arange(SIZE * A, dtype=np.float32).reshape(SIZE, A),
                     "rew": -3000.0 - np.arange(SIZE, dtype=np.float32), "non": -4000.0 - np.arange(SIZE, dtype=np.float32)}
        self.dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in self.want.items()}

    def append(self, rows, obs, act, rew, non):
        """One bd_replay_append call, and the same transitions written into the numpy twin."""
        from big_dreamer_amd import _cabi as cabi
        n = len(rows)
        t = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (np.asarray(rows, np.int32), obs, act, rew, non)]
        args = cabi.ReplayAppendArgs(n=n, size=SIZE, rows=t[0].data_ptr(), obs=t[1].data_ptr(), obs_width=self.width,
                                     bit_depth=self.bits, dst_obs=self.dev["obs"].data_ptr(), act=t[2].data_ptr(), A=self.A,
                                     dst_act=self.dev["act"].data_ptr(), reward=t[3].data_ptr(), nonterminal=t[4].data_ptr(),
                                     dst_reward=self.dev["rew"].data_ptr(), dst_nonterminal=self.dev["non"].data_ptr())
        cabi.check(cabi.lib.bd_replay_append(args, cabi.stream()))
        torch.cuda.synchronize()
        for i, row in enumerate(rows):
            if 0 <= row < SIZE:
                self.want["obs"][row] = _quantise(obs[i], self.bits) if self.bits else obs[i]
                self.want["act"][row], self.want["rew"][row], self.want["non"][row] = act[i], rew[i], non[i]

    def check(self):
        """The named rows equal the sources and every other element still holds its sentinel: the twin says both."""
        for k, v in self.want.items():
            got = self.dev[k].cpu().numpy()
            assert np.array_equal(_bits(got), _bits(v)), (k, np.argwhere(got != v)[:5])


def _rows(n):
    """Distinct, unsorted, non-contiguous rows with 0 and 39 among them (one call of n = 1 holds one of the two: the tests
    make a second call for the other)."""
    return [[39], [0, 39, 17], [0, 39, 5, 31, 2, 28, 11, 37, 8, 22, 14, 35, 19, 25, 3, 33, 16]][(1, 3, 17).index(n)]


def _transitions(rng, n, A):
    return (rng.uniform(-1, 1, (n, A)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
            (rng.uniform(0, 1, n) < 0.7).astype(np.float32))


@pytest.mark.parametrize("width,A", [(1, 1), (3, 2), (5, 17)])
@pytest.mark.parametrize("n", [1, 3, 17])
def test_append_kernel_state_observations(n, width, A):
    rng = np.random.default_rng(100 * n + width)
    mirror = _Mirror(width, A, 0)
    calls = [_rows(n)] + ([[0]] if n == 1 else [])
    for rows in calls:
        mirror.append(rows, rng.standard_normal((n, width)).astype(np.float32), *_transitions(rng, n, A))
        mirror.check()
    assert not np.array_equal(mirror.want["rew"][[0, 39]], (-3000.0 - np.arange(SIZE, dtype=np.float32))[[0, 39]])
    # rows outside [0, SIZE) write nothing; the other transitions of the call land
    guarded = [[-1], [SIZE]] if n == 1 else [[-1 if i == 0 else SIZE if i == n - 1 else r for i, r in enumerate(_rows(n))]]
    for rows in guarded:
        before = {k: v.copy() for k, v in mirror.want.items()}
        mirror.append(rows, rng.standard_normal((n, width)).astype(np.float32), *_transitions(rng, n, A))
        mirror.check()
        changed = {int(r) for r in np.flatnonzero(mirror.want["rew"] != before["rew"])}
        assert changed == {r for r in rows if 0 <= r < SIZE}


def _pixel_values(rng, n, bits):
    """Random values in [-0.5, 0.5) with, at random places: every quantisation boundary k / 2^bits - 0.5 and its two float32
    neighbours, +-0.5, +-0.75 and +-2.0 (the clip), +-1e-8.  No NaN: numpy's astype(uint8) of NaN is not defined."""
    v = rng.uniform(-0.5, 0.5, (n, 3 * 64 * 64)).astype(np.float32)
    edges = np.arange(2 ** bits + 1, dtype=np.float32) / np.float32(2 ** bits) - np.float32(0.5)
    special = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(1)),
                              np.array([0.5, -0.5, 0.75, -0.75, 2.0, -2.0, 1e-8, -1e-8], np.float32)])
    for i in range(n):
        v[i, rng.choice(v.shape[1], special.size, replace=False)] = special
    return v


@pytest.mark.parametrize("bits", [1, 5, 8])
@pytest.mark.parametrize("n", [1, 3])
def test_append_kernel_pixels(n, bits):
    rng = np.random.default_rng(10 * n + bits)
    A = 17
    mirror = _Mirror(3 * 64 * 64, A, bits)
    for rows in [_rows(n)] + ([[0]] if n == 1 else []):
        obs = _pixel_values(rng, n, bits)
        want = _quantise(obs, bits)
        assert want.min() == 0 and want.max() == 255 and len(np.unique(want)) >= 2 ** bits       # every level, and the clip
        mirror.append(rows, obs, *_transitions(rng, n, A))
        mirror.check()
    guarded = [[-1], [SIZE]] if n == 1 else [[-1, 12, SIZE]]
    for rows in guarded:
        mirror.append(rows, _pixel_values(rng, n, bits), *_transitions(rng, n, A))
        mirror.check()


# ---------------------------------------------------------------------------------------------- the buffer end to end
@pytest.mark.parametrize("pixel", [False, True])
def test_laned_buffer_keeps_the_mirror_in_step(pixel):
    from big_dreamer_amd.memory import ExperienceReplay
    rng = np.random.default_rng(8)
    lanes, A = 3, 2
    buf = ExperienceReplay(13, A, 5, pixel, 3, "cuda", lanes=lanes)              # 3 lanes x 4 rows, one row unused
    assert buf.lane_size == 4
    for k in ("observations", "actions", "rewards", "nonterminals"):
        getattr(buf, k)[:] = 7
    buf.sync_device()
    shape = (lanes, 3, 64, 64) if pixel else (lanes, 3)
    for call in range(9):                                                        # wraps the 4-row lanes twice
        obs = torch.from_numpy(rng.uniform(-0.5, 0.5, shape).astype(np.float32))
        act = torch.from_numpy(rng.uniform(-1, 1, (lanes, A)).astype(np.float32))
        rew, done = rng.standard_normal(lanes).astype(np.float32), rng.uniform(0, 1, lanes) < 0.3
        kw = {}
        if call % 2 == 0:
            kw = {"observations_device": obs.cuda(), "actions_device": act.cuda()}
        elif call % 4 == 1:
            kw = {"actions_device": act.cuda()}
        buf.append_batch(obs, act, rew, done, **kw)
        for k in ("observations", "actions", "rewards", "nonterminals"):
            assert np.array_equal(_bits(buf._dev[k]), _bits(getattr(buf, k))), (call, k)
    assert buf.full and buf.idx == 1 and buf.steps == 27
    assert (buf.observations[12] == 7).all() and (buf.rewards[12] == 7)          # the remainder row is never written
    np.random.seed(21)
    idxs = np.asarray([buf._sample_idx(3) for _ in range(3)])
    vec = idxs.transpose().reshape(-1)
    np.random.seed(21)
    got = buf.sample(3, 3)
    torch.cuda.synchronize()
    if not pixel:
        assert np.array_equal(_bits(got[0]), _bits(buf.observations[vec].reshape(3, 3, -1)))
    else:
        assert got[0].shape == (3, 3, 3, 64, 64)
    assert np.array_equal(_bits(got[1]), _bits(buf.actions[vec].reshape(3, 3, -1)))
    assert np.array_equal(_bits(got[2]), _bits(buf.rewards[vec].reshape(3, 3)))
    assert np.array_equal(_bits(got[3]), _bits(buf.nonterminals[vec].reshape(3, 3, 1)))


# ---------------------------------------------------------------------------------------------- the Collector on an agent
TINY = ["belief_size=32", "hidden_size=32", "embedding_size=64", "state_size=6", "synthetic_env_action_size=2",
        "synthetic_env_observation_size=3", "batch_size=3", "seq_len=4", "planning_horizon=4", "experience_size=100",
        "max_episode_length=8", "action_repeat=2"]                               # as tests/test_evaluate_gpu.py
LOG_KEYS = {"observation_loss", "reward_loss", "kl_loss", "model_loss", "actor_loss", "policy_entropy", "value_loss"}
CATEGORICAL = ["algorithm=dreamerV2", "latent_distribution=Categorical", "discrete_latent_dimensions=3",
               "discrete_latent_classes=5"]


@pytest.mark.parametrize("extra,fused_cat", [((), "0"), (("pixel_observation=true", "embedding_size=1024"), "0"),
                                             (CATEGORICAL, "1")], ids=["state", "pixel", "categorical"])
def test_collector_on_a_real_agent(extra, fused_cat, monkeypatch):
    from big_dreamer_amd.collect import Collector
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import Env, VecEnv
    monkeypatch.setenv("BD_ACT_FUSED_CAT", fused_cat)
    params = load_config(TINY + list(extra) + ["collect_envs=3"])
    torch.manual_seed(3)
    cls = DreamerV2 if params["algorithm"] == "dreamerV2" else Dreamer
    agent = cls(params, VecEnv(Env, params, 3))
    assert agent.act_fused_cat == (fused_cat == "1")
    buf = agent.buffer
    assert buf.lanes == 3 and buf.lane_size == 33
    collector = Collector(agent, agent.env)
    assert collector.seed(24) == (24, 3) and buf.idx == 4
    buf.sync_device()                                    # from here on append_batch keeps the mirror in step
    ends = []
    for _ in range(12):
        rewards, dones = collector.step()
        ends.append(dones.tolist())
    assert ends == [[k % 4 == 3] * 3 for k in range(12)]                         # 8-step episodes, action_repeat 2
    assert buf.idx == 16 and buf.steps == 48 and buf.episodes == 12 and len(collector.finished_returns) == 9
    torch.cuda.synchronize()
    for k in ("observations", "actions", "rewards", "nonterminals"):
        assert np.array_equal(_bits(buf._dev[k]), _bits(getattr(buf, k))), k
    for e in range(3):
        lane = buf.nonterminals[e * 33:e * 33 + 16, 0]
        assert lane.tolist() == [1.0, 1.0, 1.0, 0.0] * 4, (e, lane)
        assert np.abs(buf.actions[e * 33 + 4:e * 33 + 16]).sum() > 0
    # the rows of the finished environments restart from zero; the others carry their belief on
    assert float(collector.belief.abs().sum()) == 0 and float(collector.action.abs().sum()) == 0
    logs = agent.train_step()
    assert set(logs) >= LOG_KEYS and all(np.isfinite(float(logs[k])) for k in LOG_KEYS), logs


# ---------------------------------------------------------------------------------------------- the CLI
def _main(*extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *TINY, "seed_steps=24", "train_steps=60",
                           "log_freq=10", *extra], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("envs", [3, 1])
def test_cli_collect_envs(envs):
    out = _main(f"collect_envs={envs}")
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Initialized with 3 episodes and 24 steps" in out.stdout, out.stdout
    assert "model_loss" in out.stdout
