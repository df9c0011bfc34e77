"""CPU: collecting from N environments at once -- the laned ExperienceReplay (lanes=1 identity, the laned sampler,
append_batch on the host arrays), VecEnv's auto-reset, the Collector against the reference's single-environment loop
(src/main.py:129-170) with a stub agent, bd_replay_append's argument validation and the collect_envs config key.
Buffers live on "cpu", where no device mirror exists.  Every comparison is bit-exact."""
import numpy as np
import pytest
import torch

ENV = {"synthetic_env_observation_size": 3, "synthetic_env_action_size": 2, "max_episode_length": 8, "action_repeat": 2,
       "seed": 5}


def _buffer(size, lanes=None, pixel=False, A=2, O=3, bits=5):
    from big_dreamer_amd.memory import ExperienceReplay
    kw = {} if lanes is None else {"lanes": lanes}
    return ExperienceReplay(size, A, bits, pixel, O, "cpu", **kw)


def _state(buf):
    return (buf.observations.copy(), buf.actions.copy(), buf.rewards.copy(), buf.nonterminals.copy(), buf.idx, buf.full,
            buf.steps, buf.episodes)


def _same(a, b):
    return all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- lanes = 1 is today's buffer
def test_one_lane_samples_as_the_buffer_without_the_keyword():
    from big_dreamer_amd import synth
    d = synth.TINY
    rep = synth.make_replay(d, rows=64, seed=3)
    for idx, full in ((40, False), (17, True)):
        draws = []
        for lanes in (None, 1):
            buf = _buffer(64, lanes, A=d.A, O=d.O)
            for k, v in rep.items():
                getattr(buf, k)[:] = v
            buf.idx, buf.full = idx, full
            np.random.seed(11)
            draws.append((np.asarray([buf._sample_idx(7) for _ in range(6)]), np.random.randint(1 << 30)))
        assert np.array_equal(draws[0][0], draws[1][0])
        assert draws[0][1] == draws[1][1]                       # np.random was consumed alike


@pytest.mark.parametrize("pixel", [False, True])
def test_append_batch_of_one_row_equals_append(pixel):
    rng = np.random.default_rng(2)
    one, batch = _buffer(5, pixel=pixel), _buffer(5, 1, pixel=pixel)
    for buf in (one, batch):                                    # np.empty storage: give both the same start
        for k in ("observations", "actions", "rewards", "nonterminals"):
            getattr(buf, k)[:] = 0
    for t in range(7):                                          # wraps the 5 rows
        o = torch.from_numpy(rng.uniform(-0.5, 0.5, (1, 3, 64, 64) if pixel else (1, 3)).astype(np.float32))
        a = torch.from_numpy(rng.uniform(-1, 1, 2).astype(np.float32))
        r, done = float(rng.standard_normal()), t in (3, 6)
        one.append(o, a, r, done)
        batch.append_batch(o, a.unsqueeze(0), [r], [done])
        assert _same(_state(one), _state(batch)), t
    assert one.full and one.idx == 2 and one.steps == 7 and one.episodes == 2


# ---------------------------------------------------------------------------------------------- the laned sampler
LANES, LANE_SIZE, L = 4, 12, 5


def _laned_buffer(calls):
    """4 lanes x 12 rows (+ 3 rows no lane owns); the observation of lane e at time t is (e, t, 100 e + t)."""
    buf = _buffer(LANES * LANE_SIZE + 3, LANES)
    buf.observations[:] = -1
    for t in range(calls):
        obs = np.asarray([[e, t, 100 * e + t] for e in range(LANES)], np.float32)
        buf.append_batch(obs, np.full((LANES, 2), t, np.float32), np.arange(LANES) + t / 8, [False] * LANES)
    return buf


@pytest.mark.parametrize("calls", [7, 30])
def test_laned_sampler_draws_chunks_inside_one_lane(calls):
    buf = _laned_buffer(calls)
    assert buf.lane_size == LANE_SIZE and buf.idx == calls % LANE_SIZE and buf.full == (calls >= LANE_SIZE)
    assert buf.steps == LANES * calls
    np.random.seed(4)
    seen = set()
    for _ in range(2000):
        rows = buf._sample_idx(L)
        assert rows.shape == (L,)
        lane, local = rows // LANE_SIZE, rows % LANE_SIZE
        assert (lane == lane[0]).all() and 0 <= lane[0] < LANES            # inside one lane
        assert np.array_equal(local, (local[0] + np.arange(L)) % LANE_SIZE)   # consecutive modulo lane_size
        assert buf.idx not in local[1:]                                     # the write head is not crossed
        if not buf.full:
            assert local.max() < buf.idx
        chunk = buf.observations[rows]                                      # the contents prove the provenance
        assert (chunk[:, 0] == lane[0]).all()
        assert np.array_equal(np.diff(chunk[:, 1]), np.ones(L - 1, np.float32)), chunk
        assert np.array_equal(chunk[:, 2], 100 * chunk[:, 0] + chunk[:, 1])
        seen.add(int(lane[0]))
    assert seen == set(range(LANES))
    assert (buf.observations[LANES * LANE_SIZE:] == -1).all()                # the remainder rows are never written


# ---------------------------------------------------------------------------------------------- error paths
def test_error_paths():
    from big_dreamer_amd.collect import check_collect_envs
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    from big_dreamer_amd.env import Env
    buf = _buffer(24, 3)
    with pytest.raises(ValueError, match="append_batch"):
        buf.append(np.zeros(3, np.float32), np.zeros(2, np.float32), 0.0, False)
    for rows in (1, 2, 4):
        with pytest.raises(ValueError, match="lanes"):
            buf.append_batch(np.zeros((rows, 3), np.float32), np.zeros((rows, 2), np.float32), np.zeros(rows), [False] * rows)
    with pytest.raises(ValueError, match="lanes"):
        buf.append_batch(np.zeros((3, 3), np.float32), np.zeros((3, 2), np.float32), np.zeros(3), [False] * 2)
    assert buf.steps == 0 and buf.idx == 0
    for _ in range(5):
        buf.append_batch(np.zeros((3, 3), np.float32), np.zeros((3, 2), np.float32), np.zeros(3), [False] * 3)
    with pytest.raises(ValueError, match="lanes"):                      # a lane must hold more than one chunk's rows
        buf._sample_idx(5)
    assert buf._sample_idx(4).tolist() in ([0, 1, 2, 3], [8, 9, 10, 11], [16, 17, 18, 19])
    with pytest.raises(ValueError):
        _buffer(2, 3)
    ok = load_config(["seq_len=4", "experience_size=18", "collect_envs=3"])
    assert check_collect_envs(ok) == 3
    bad = load_config(["seq_len=4", "experience_size=17", "collect_envs=3"])
    with pytest.raises(ValueError, match="experience_size"):
        check_collect_envs(bad)
    with pytest.raises(ValueError, match="experience_size"):           # at construction, before anything touches a device
        Dreamer(bad, Env(bad))


# ---------------------------------------------------------------------------------------------- VecEnv
@pytest.mark.parametrize("pixel", [False, True])
def test_vecenv_shapes_seeds_and_auto_reset(pixel):
    from big_dreamer_amd.env import Env, VecEnv
    params = dict(ENV, pixel_observation=pixel)
    n, shape = 3, ((3, 64, 64) if pixel else (3,))
    envs = VecEnv(Env, params, n)
    twins = [Env(dict(params, seed=params["seed"] + e)) for e in range(n)]
    assert envs.n == n and len(envs.envs) == n and envs.action_size == 2
    assert envs.observation_size == ((3, 64, 64) if pixel else 3)
    first = envs.reset()
    assert first.shape == (n,) + shape and first.dtype == torch.float32
    assert not torch.equal(first[0], first[1]) and not torch.equal(first[1], first[2])      # different seeds
    for e, twin in enumerate(twins):
        assert torch.equal(twin.reset()[0], first[e])
    random = envs.sample_random_action()
    assert random.shape == (n, 2) and random.dtype == torch.float32
    for twin in twins:
        twin.sample_random_action()                       # keeps the twins' generators in step
    actions = torch.tensor([[0.25, -0.5], [0.0, 0.125], [-1.0, 1.0]])
    for call in range(1, 6):
        obs, rewards, dones = envs.step(actions)
        assert obs.shape == (n,) + shape and obs.dtype == torch.float32
        assert rewards.shape == (n,) and rewards.dtype == torch.float32
        assert dones.shape == (n,) and dones.dtype == torch.bool
        assert dones.tolist() == [call == 4] * n          # 8 steps at action_repeat 2; True for that call only
        for e, twin in enumerate(twins):
            o, r, d = twin.step(actions[e])
            assert d == (call == 4) and rewards[e].item() == np.float32(r)
            if d:
                o = twin.reset()                          # the row is the reset observation
            assert torch.equal(o[0], obs[e]), (call, e)
    envs.close()


# ---------------------------------------------------------------------------------------------- Collector
class _Stub:
    """An agent for the Collector on the CPU: the action is a fixed function of the observation (exactly rounded
    operations only, so one row and a batch agree bit for bit); records the rows it is given."""
    belief_size, state_size, action_size, action_repeat = 4, 5, 2, 2

    def __init__(self, buffer):
        self.buffer, self.device, self.calls = buffer, torch.device("cpu"), []

    def update_belief_and_act(self, env, belief, posterior_state, action, observation, explore=False):
        self.calls.append((belief.clone(), posterior_state.clone(), action.clone(), explore))
        act = torch.clamp(observation[:, :2] * 0.5 + 0.25, -1, 1)
        batched = hasattr(env, "n") and hasattr(env, "envs")
        next_observation, reward, done = env.step(act if batched else act[0])
        return belief + 1, posterior_state + 2, act, next_observation, reward, done


def _single_environment_loop(e, seed_calls, steps, rows):
    """src/planet.py:136-159 then src/main.py:129-170 alone on environment e (the environment is left running in
    between, as the Collector leaves it)."""
    from big_dreamer_amd.env import Env
    env = Env(dict(ENV, seed=ENV["seed"] + e))
    buf = _buffer(rows)
    stub = _Stub(buf)
    observation = env.reset()
    for _ in range(seed_calls):
        action = env.sample_random_action()
        next_observation, reward, done = env.step(action)
        buf.append(observation, action, reward, done)
        observation = env.reset() if done else next_observation
    belief, state, action = torch.zeros(1, 4), torch.zeros(1, 5), torch.zeros(1, 2)
    returns, episode = [], 0.0
    for _ in range(steps):
        belief, state, action, next_observation, reward, done = stub.update_belief_and_act(
            env, belief, state, action, observation, explore=True)
        buf.append(observation, action[0], reward, done)
        episode += float(np.float32(reward))
        observation = next_observation
        if done:
            returns.append(episode)
            observation, episode = env.reset(), 0.0
            belief.zero_(); state.zero_(); action.zero_()
    return buf, stub, returns


def test_collector_records_per_lane_what_the_single_environment_loop_records():
    from big_dreamer_amd.collect import Collector
    from big_dreamer_amd.env import Env, VecEnv
    n, lane = 3, 20
    agent = _Stub(_buffer(n * lane, n))
    collector = Collector(agent, VecEnv(Env, ENV, n))
    assert collector.seed(36) == (36, 3)                  # 18 transitions = 6 calls; every lane finished one 4-call episode
    assert agent.buffer.idx == 6 and agent.buffer.steps == 18
    dones = []
    for _ in range(10):
        rewards, done = collector.step()
        assert rewards.shape == (n,) and rewards.dtype == torch.float32 and done.dtype == torch.bool
        dones.append(done.tolist())
    assert [d[0] for d in dones] == [False, True, False, False, False, True, False, False, False, True]
    buf = agent.buffer
    assert buf.idx == 16 and not buf.full and buf.steps == 48 and buf.episodes == 3 + 3 * 3
    for e in range(n):
        ref, ref_stub, ref_returns = _single_environment_loop(e, 6, 10, lane)
        rows = slice(e * lane, e * lane + 16)
        assert np.array_equal(buf.observations[rows], ref.observations[:16]), e
        assert np.array_equal(buf.actions[rows], ref.actions[:16]), e
        assert np.array_equal(buf.rewards[rows], ref.rewards[:16]), e
        assert np.array_equal(buf.nonterminals[rows], ref.nonterminals[:16]), e
        assert ref.nonterminals[:16, 0].tolist() == [1, 1, 1, 0] * 4
        for call, (got, want) in enumerate(zip(agent.calls, ref_stub.calls)):      # the rows the agent was handed
            assert got[3] is True and want[3] is True
            for g, w in zip(got[:3], want[:3]):
                assert torch.equal(g[e:e + 1], w), (e, call)
        assert len(ref_returns) == 3
        assert [r for r in collector.finished_returns[e::n]] == [float(r) for r in ref_returns]
    for call, (belief, state, action, _) in enumerate(agent.calls):
        fresh = call == 0 or dones[call - 1][0]
        assert (float(belief.abs().sum()) == 0 and float(state.abs().sum()) == 0 and float(action.abs().sum()) == 0) == fresh
    assert len(collector.finished_returns) == 9


def test_collector_needs_as_many_lanes_as_environments():
    from big_dreamer_amd.collect import Collector
    from big_dreamer_amd.env import Env, VecEnv
    with pytest.raises(ValueError, match="lanes"):
        Collector(_Stub(_buffer(40, 2)), VecEnv(Env, ENV, 3))


# ---------------------------------------------------------------------------------------------- the C ABI's host half
def test_replay_append_rejects_bad_arguments_without_gpu():
    from big_dreamer_amd import _cabi as cabi
    good = dict(n=3, size=40, rows=64, obs=64, obs_width=12, bit_depth=0, dst_obs=64, act=64, A=2, dst_act=64, reward=64,
                nonterminal=64, dst_reward=64, dst_nonterminal=64)              # (addresses are never dereferenced here)
    bad = [{k: None} for k in ("rows", "obs", "dst_obs", "act", "dst_act", "reward", "nonterminal", "dst_reward",
                               "dst_nonterminal")]
    bad += [{"n": 0}, {"n": -1}, {"n": 4097}, {"size": 0}, {"size": -5}, {"A": 0}, {"A": -1}, {"obs_width": 0},
            {"obs_width": -4}, {"bit_depth": -1}, {"bit_depth": 9}, {"bit_depth": 5, "obs_width": 10},
            {"bit_depth": 5, "obs": 64 + 4}, {"bit_depth": 5, "obs": 64 + 8}, {"bit_depth": 8, "dst_obs": 64 + 1},
            {"bit_depth": 1, "dst_obs": 64 + 2}]
    for change in bad:
        args = cabi.ReplayAppendArgs(**dict(good, **change))
        assert cabi.lib.bd_replay_append(args, None) != 0, change
        assert b"bd_replay_append" in cabi.lib.bd_last_error(), change
        with pytest.raises(RuntimeError, match="bd_replay_append"):
            cabi.check(cabi.lib.bd_replay_append(args, None))
    assert cabi.lib.bd_replay_append(None, None) != 0 and b"bd_replay_append" in cabi.lib.bd_last_error()


# ---------------------------------------------------------------------------------------------- config
def test_collect_envs_config_key():
    from big_dreamer_amd.config import load_config
    assert load_config([])["collect_envs"] == 1
    assert load_config(["collect_envs=4"])["collect_envs"] == 4
