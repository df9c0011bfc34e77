"""Collecting from `n` environments at once (``collect_envs``): one decision of ``update_belief_and_act`` serves all of
them, and one ``ExperienceReplay.append_batch`` -- one bd_replay_append launch reading the observation batch and the action
where they already are on the device -- records one transition per lane of the replay buffer.

Per lane the buffer holds exactly what the reference's single-environment loop (src/main.py:129-170) records for that
environment: the observation before the action, the action, its reward, ``not done``, and after a ``done`` the reset
observation as the next row.

``Collector`` needs only ``update_belief_and_act``, ``buffer``, ``device``, ``belief_size``, ``state_size`` and
``action_size`` of the agent, so ``Planet`` works and a stub drives it on the CPU."""
from __future__ import annotations

from typing import Any, Dict, List, Tuple

import numpy as np
import torch


def check_collect_envs(params: Dict[str, Any]) -> int:
    """``collect_envs`` of `params` (default 1), checked against the replay size: every lane must hold one chunk of
    ``seq_len`` rows clear of its write head."""
    n = int(params.get("collect_envs", 1))
    if n < 1:
        raise ValueError(f"collect_envs={n}: at least one environment collects")
    if n == 1:
        return n
    need = n * (int(params["seq_len"]) + 2)
    if int(params["experience_size"]) < need:
        raise ValueError(f"experience_size={params['experience_size']} is too small for collect_envs={n}: each of the {n} "
                         f"replay lanes needs seq_len + 2 = {int(params['seq_len']) + 2} rows ({need} in all)")
    return n


class Collector:
    """The collect half of the training loop for `envs` (a VecEnv of n environments) and `agent`, whose buffer has n
    lanes."""

    def __init__(self, agent, envs):
        self.agent, self.envs, self.n = agent, envs, int(envs.n)
        lanes = getattr(agent.buffer, "lanes", 1)
        if lanes != self.n:
            raise ValueError(f"Collector: {self.n} environments but the agent's replay buffer has {lanes} lanes "
                             "(build the agent with collect_envs equal to the number of environments)")
        dev = agent.device
        self.observation = envs.reset()
        self.belief = torch.zeros(self.n, agent.belief_size, device=dev)
        self.state = torch.zeros(self.n, agent.state_size, device=dev)       # (Categorical latents: dimensions * classes)
        self.action = torch.zeros(self.n, agent.action_size, device=dev)
        self.returns = np.zeros(self.n)
        self.finished_returns: List[float] = []     # returns of the episodes finished so far under step(), oldest first

    def seed(self, seed_steps: int) -> Tuple[int, int]:
        """randomly_initialize_replay_buffer (src/planet.py:136-159) for lanes: random actions on all n environments side
        by side until ``buffer.steps * action_repeat >= seed_steps``.  Returns (env_steps, episodes).  The environments are
        left running, not closed: the collector's observation is the current one."""
        buffer = self.agent.buffer
        repeat = int(getattr(self.agent, "action_repeat", 1))
        while buffer.steps * repeat < seed_steps:
            actions = self.envs.sample_random_action()
            next_observation, rewards, dones = self.envs.step(actions)
            buffer.append_batch(self.observation, actions, rewards, dones)
            self.observation = next_observation
        return buffer.steps * repeat, buffer.episodes

    @torch.no_grad()
    def step(self, explore: bool = True):
        """One decision for all n environments (n environment steps): upload the observation batch once, act, append one
        transition per lane, zero the belief / state / action rows of the environments that finished (their next
        observation is already the reset one).  Returns (rewards float32 (n,), dones bool (n,)).
        Data-parallel runs: this carries the collectives of update_belief_and_act, so every rank calls it."""
        agent, dev = self.agent, self.agent.device
        obs_host = self.observation
        obs_dev = obs_host.to(device=dev)             # the one upload: the encoder and the append kernel both read it
        belief, state, action, next_observation, rewards, dones = agent.update_belief_and_act(
            self.envs, self.belief, self.state, self.action, obs_dev, explore=explore)
        agent.buffer.append_batch(obs_host, action.cpu(), rewards, dones, observations_device=obs_dev, actions_device=action)
        rewards, dones = torch.as_tensor(rewards, dtype=torch.float32), torch.as_tensor(dones, dtype=torch.bool)
        self.returns += rewards.numpy()
        finished = torch.nonzero(dones).reshape(-1)
        if finished.numel():
            for e in finished.tolist():
                self.finished_returns.append(float(self.returns[e]))
                self.returns[e] = 0.0
            where = finished.to(device=dev)
            for t in (belief, state, action):
                t.index_fill_(0, where, 0)
        self.belief, self.state, self.action, self.observation = belief, state, action, next_observation
        return rewards, dones
