"""Environment surface the agent needs (src/planet.py:36,91,147-158): ``action_size``, ``observation_size``,
``reset/step/sample_random_action/close``.  gym / mujoco are not installed in the build image, so the CLI
falls back to a small synthetic control task with the same interface; any object with this interface works.
``EnvBatcher`` (src/env.py:343-394) steps several of them side by side for the evaluation loop, ``VecEnv`` for the collect
loop (auto-reset)."""
from __future__ import annotations

import numpy as np
import torch


class SyntheticEnv:
    """Damped linear system x' = A x + B u + noise, reward = -|x|^2 - 0.1|u|^2, fixed episode length.
    Observations are the state (state-observation mode), actions live in [-1, 1]."""

    def __init__(self, observation_size: int = 3, action_size: int = 1, max_episode_length: int = 1000,
                 action_repeat: int = 2, seed: int = 0):
        self.observation_size, self.action_size = observation_size, action_size
        self._nx = observation_size          # state dimension (the pixel subclass changes observation_size)
        self.max_episode_length, self.action_repeat = max_episode_length, action_repeat
        rng = np.random.default_rng(seed)
        q, _ = np.linalg.qr(rng.standard_normal((observation_size, observation_size)))
        self.A = (0.97 * q).astype(np.float32)
        self.B = (0.3 * rng.standard_normal((observation_size, action_size))).astype(np.float32)
        self.rng = rng
        self.t = 0
        self.x = np.zeros(observation_size, np.float32)

    def reset(self) -> torch.Tensor:
        self.t = 0
        self.x = self.rng.standard_normal(self._nx).astype(np.float32)
        return torch.from_numpy(self.x.copy()).unsqueeze(0)

    def step(self, action):
        return self._advance(self._control(action))

    def _control(self, action) -> np.ndarray:
        return np.asarray(action.detach().cpu().numpy() if isinstance(action, torch.Tensor) else action,
                          dtype=np.float32).reshape(-1)[: self.action_size]

    def _advance(self, u: np.ndarray):
        reward = 0.0
        for _ in range(self.action_repeat):
            self.x = self.A @ self.x + self.B @ u + 0.01 * self.rng.standard_normal(self._nx).astype(np.float32)
            reward += float(-(self.x ** 2).sum() - 0.1 * (u ** 2).sum())
            self.t += 1
            if self.t >= self.max_episode_length:
                break
        done = self.t >= self.max_episode_length
        return torch.from_numpy(self.x.copy()).unsqueeze(0), reward, done

    def sample_random_action(self) -> torch.Tensor:
        return torch.from_numpy(self.rng.uniform(-1, 1, self.action_size).astype(np.float32))

    def close(self) -> None:
        pass


class SyntheticPixelEnv(SyntheticEnv):
    """Same dynamics, observed as a 3x64x64 image in [-0.5, 0.5]: a fixed random linear rendering of the state
    squashed with tanh (stands in for the reference's rendered gym frames, src/env.py:235-317)."""

    def __init__(self, state_size: int = 3, action_size: int = 1, max_episode_length: int = 1000, action_repeat: int = 2,
                 seed: int = 0):
        super().__init__(state_size, action_size, max_episode_length, action_repeat, seed)
        self._render = (self.rng.standard_normal((3 * 64 * 64, state_size)) / np.sqrt(state_size)).astype(np.float32)
        self.state_size = state_size
        self.observation_size = (3, 64, 64)

    def _img(self):
        return torch.from_numpy((0.5 * np.tanh(self._render @ self.x)).astype(np.float32).reshape(1, 3, 64, 64))

    def reset(self):
        self.t = 0
        self.x = self.rng.standard_normal(self.state_size).astype(np.float32)
        return self._img()

    def step(self, action):
        _, reward, done = super().step(action)
        return self._img(), reward, done


class _DiscreteControl:
    """A discrete action set over the continuous dynamics: a one-hot (or straight-through) action vector selects the
    control u = U[argmax(action)] from a fixed table U of A control vectors in [-1, 1]^m (m = control dimension);
    actions are A-vectors, so action_size = A."""

    def _discrete_init(self, n_actions: int, control_size: int) -> None:
        self.control_size = control_size
        self.U = self.rng.uniform(-1, 1, (n_actions, control_size)).astype(np.float32)
        self.action_size = n_actions

    def _control(self, action) -> np.ndarray:
        a = np.asarray(action.detach().cpu().numpy() if isinstance(action, torch.Tensor) else action,
                       dtype=np.float32).reshape(-1)[: self.action_size]
        return self.U[int(np.argmax(a))]

    def sample_random_action(self) -> torch.Tensor:
        out = np.zeros(self.action_size, np.float32)
        out[self.rng.integers(self.action_size)] = 1.0
        return torch.from_numpy(out)


class SyntheticDiscreteEnv(_DiscreteControl, SyntheticEnv):
    """SyntheticEnv with A discrete actions (action_distribution=Categorical, state observations)."""

    def __init__(self, observation_size: int = 3, n_actions: int = 3, max_episode_length: int = 1000,
                 action_repeat: int = 2, seed: int = 0, control_size: int = 1):
        SyntheticEnv.__init__(self, observation_size, control_size, max_episode_length, action_repeat, seed)
        self._discrete_init(n_actions, control_size)


class SyntheticDiscretePixelEnv(_DiscreteControl, SyntheticPixelEnv):
    """SyntheticPixelEnv with A discrete actions (action_distribution=Categorical, 64x64 pixel observations)."""

    def __init__(self, state_size: int = 3, n_actions: int = 3, max_episode_length: int = 1000, action_repeat: int = 2,
                 seed: int = 0, control_size: int = 1):
        SyntheticPixelEnv.__init__(self, state_size, control_size, max_episode_length, action_repeat, seed)
        self._discrete_init(n_actions, control_size)


def Env(params):
    """Factory with the reference's name (src/env.py:320-340)."""
    if params.get("action_distribution", "Gaussian") == "Categorical":
        cls = SyntheticDiscretePixelEnv if params.get("pixel_observation", False) else SyntheticDiscreteEnv
        return cls(int(params.get("synthetic_env_observation_size", 3)), int(params.get("synthetic_env_action_size", 3)),
                   int(params["max_episode_length"]), int(params["action_repeat"]), int(params["seed"]))
    if params.get("pixel_observation", False):
        return SyntheticPixelEnv(int(params.get("synthetic_env_observation_size", 3)),
                                 int(params.get("synthetic_env_action_size", 1)), int(params["max_episode_length"]),
                                 int(params["action_repeat"]), int(params["seed"]))
    return SyntheticEnv(int(params.get("synthetic_env_observation_size", 3)),
                        int(params.get("synthetic_env_action_size", 1)), int(params["max_episode_length"]),
                        int(params["action_repeat"]), int(params["seed"]))


class EnvBatcher:
    """`n` environments stepped side by side (src/env.py:343-394): what the evaluation loop hands to
    ``update_belief_and_act`` in place of a single environment.  An environment that has finished stays finished; from the
    call after the one it finished in, its observation and reward rows are zero."""

    def __init__(self, env_class, env_params, n: int):
        self.n = n
        self.envs = [env_class(env_params) for _ in range(n)]
        self.dones = [True] * n

    def reset(self) -> torch.Tensor:
        observations = [env.reset() for env in self.envs]
        self.dones = [False] * self.n
        return torch.cat(observations)

    def step(self, actions):
        """actions: one row per environment.  Every environment is stepped, finished ones included.  Returns
        (observations concatenated along dim 0, rewards float32 (n,), dones uint8 (n,))."""
        finished = list(self.dones)           # as they were BEFORE this call: the row that finishes now keeps its values
        observations, rewards, dones = zip(*[env.step(action) for env, action in zip(self.envs, actions)])
        self.dones = [bool(d) or prev for d, prev in zip(dones, finished)]
        observations = torch.cat(observations)
        rewards = torch.tensor(rewards, dtype=torch.float32)
        blank = torch.tensor(finished, dtype=torch.bool)
        observations[blank] = 0
        rewards[blank] = 0
        return observations, rewards, torch.tensor(self.dones, dtype=torch.uint8)

    def close(self) -> None:
        for env in self.envs:
            env.close()


class VecEnv:
    """`n` environments stepped side by side for COLLECTING (``collect_envs``): unlike EnvBatcher, an environment that
    finishes is reset in the same call, so every row always carries a live episode.  Environment e is built from
    ``dict(env_params, seed=env_params["seed"] + e)``, so that the synthetic tasks do not run in unison.
    ``update_belief_and_act`` recognises it as a batched environment by ``n`` and ``envs``."""

    def __init__(self, env_class, env_params, n: int):
        self.n = int(n)
        self.envs = [env_class(dict(env_params, seed=env_params["seed"] + e)) for e in range(self.n)]
        self.action_size, self.observation_size = self.envs[0].action_size, self.envs[0].observation_size

    def reset(self) -> torch.Tensor:
        return torch.cat([env.reset() for env in self.envs])

    def sample_random_action(self) -> torch.Tensor:
        return torch.stack([torch.as_tensor(env.sample_random_action()) for env in self.envs])

    def step(self, actions):
        """actions: one row per environment.  Returns (observations (n, ...), rewards float32 (n,), dones bool (n,)).
        An environment that finishes in this call is reset in this call: its observation row is the reset observation (the
        first of its next episode) and its `done` is True for this call only."""
        observations, rewards, dones = [], [], []
        for env, action in zip(self.envs, actions):
            observation, reward, done = env.step(action)
            observations.append(env.reset() if done else observation)
            rewards.append(reward)
            dones.append(bool(done))
        return torch.cat(observations), torch.tensor(rewards, dtype=torch.float32), torch.tensor(dones, dtype=torch.bool)

    def close(self) -> None:
        for env in self.envs:
            env.close()
