#!/usr/bin/env python3
"""CLI with the reference's surface: ``python src/main.py key=value ...`` (reference src/main.py:20-285).

Collect-update loop: every ``environment_steps_per_update`` env steps run ``collect_interval`` train steps
(src/main.py:103-108), critic-target update cadence as at src/main.py:110-112, one env step with exploration
noise (src/main.py:129-143), append to the replay buffer (src/main.py:146), log every ``log_freq``.
``evaluation=true``: every ``test_interval`` steps the test loop (src/main.py:191-283) runs ``test_episodes`` environments
without exploration noise and prints ``Eval_{min,avg,max,std}_return``; ``test=true`` evaluates once and exits.
``openl_freq=k`` (k > 0): every k steps rank 0 runs ``open_loop`` on ``openl_sequences`` replay sequences with ``openl_context``
context steps, prints ``openl_mse_context`` / ``openl_mse_open`` and saves the video as ``Openl_<step>.npy`` in ``eval_video_dir``.
``collect_envs=n`` (n > 1) collects from n environments side by side (big_dreamer_amd/collect.py): one loop iteration is one
decision for all of them = n environment steps, with the same update-to-data ratio.
``sample_on_device=true``: every training batch is drawn and gathered by one launch on the device (the replay's own Philox
stream, keyed by the torch seed) instead of ``np.random`` index draws and an index upload; the draw's counter is saved with
the replay (``experience_<step>.npz``), so a resumed run draws the batches the uninterrupted run draws.
``checkpoint_dir=<dir>``: at the end of every loop iteration whose step is a multiple of ``checkpoint_interval`` (with
``collect_envs=n``: whose n steps hold one) every rank writes ``<dir>/models_<step>.pth`` and, with
``checkpoint_experience=true``, ``<dir>/experience_<step>.npz`` (``_rank<r>`` before the extension in multi-GPU runs), <step>
being the iteration's first step; ``checkpoint_keep=k`` keeps the newest k.  ``experience_replay=<file>`` loads the buffer
instead of running the seed phase.  ``resume=true models=<file>`` continues that run at its saved step plus one iteration
with the same weights, optimisers, noise counters and generator states.  The episode in flight is NOT restored -- an
environment cannot be serialised in general --: the environments are reset and belief, state and action start at zero, so
the first update burst after the resume point is bit-identical to the uninterrupted run's, and the run then goes on from
the same weights, optimiser state, replay and noise position on fresh episodes.
Multi-GPU: launch with ``python -m torch.distributed.run --nproc-per-node N src/main.py ...``; each rank collects
its own experience and the gradients are all-reduced over RCCL (big_dreamer_amd/engine.py).
"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import big_dreamer_amd  # noqa: E402,F401  (first: sets the HIP runtime's queue count before HIP initialises)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from big_dreamer_amd.config import load_config  # noqa: E402


def evaluate(model, params, step, rank):
    """The test half of the reference's loop (src/main.py:191-283).  update_belief_and_act carries collectives in
    data-parallel runs, so every rank evaluates; rank 0 prints and saves."""
    video = (bool(params["pixel_observation"]) and params["log_video_freq"] not in (-1, 0)
             and step % params["log_video_freq"] == 0)
    policy = {}
    if params["eval_action"] != "sample" or params["eval_state_mean"]:      # (a Planet evaluates by planning: defaults only)
        policy = {"action_mode": params["eval_action"], "state_mean": params["eval_state_mean"]}
    result = model.evaluate(episodes=params["test_episodes"], video=video, **policy)
    if rank != 0:
        return
    for key in ("Eval_min_return", "Eval_avg_return", "Eval_max_return", "Eval_std_return"):
        print(f"{key} : {result[key]}", flush=True)
    if result["video"] is not None and params["eval_video_dir"]:
        os.makedirs(params["eval_video_dir"], exist_ok=True)
        np.save(os.path.join(params["eval_video_dir"], f"Eval_rollout_{step}.npy"), result["video"])


def open_loop(model, params, step):
    """Rank 0 only (Dreamer.open_loop issues no collectives): the open-loop prediction error of a fresh replay batch and,
    for pixel observations, its truth / model / error video."""
    result = model.open_loop(sequences=params["openl_sequences"], context=params["openl_context"])
    for key in ("openl_mse_context", "openl_mse_open"):
        print(f"{key} : {result[key]}", flush=True)
    if result["video"] is not None and params["eval_video_dir"]:
        os.makedirs(params["eval_video_dir"], exist_ok=True)
        np.save(os.path.join(params["eval_video_dir"], f"Openl_{step}.npy"), result["video"])


def checkpoint(model, params, step, rank, world, n_envs):
    """models_<step> (always) and experience_<step> (checkpoint_experience) into checkpoint_dir.  Dreamer.save issues the
    held-back optimiser steps of a data-parallel run, a collective: every rank is here at the same point of the loop, and
    writes files of its own (replay contents and generator states differ per rank)."""
    from big_dreamer_amd import checkpoint as ck
    directory = params["checkpoint_dir"]
    os.makedirs(directory, exist_ok=True)
    model.save(ck.models_path(directory, step, rank, world), extra={"step": step, "collect_envs": n_envs})
    if params["checkpoint_experience"]:
        model.buffer.save(ck.experience_path(directory, step, rank, world))
    ck.prune(directory, int(params["checkpoint_keep"]), rank=rank if world > 1 else None)


def fill_replay(model, params, rank, seed_phase):
    """The replay before the loop: experience_replay=<file> loads it, otherwise `seed_phase` collects seed_steps with
    random actions.  Returns the environment steps the buffer stands for, where the loop starts."""
    if params["experience_replay"]:
        model.buffer.load(params["experience_replay"])
        env_steps = model.buffer.steps * params["action_repeat"]       # as the seed phase counts them
        if rank == 0:
            print(f"Loaded {model.buffer.episodes} episodes and {env_steps} steps from {params['experience_replay']}")
        return env_steps
    env_steps, num_episodes = seed_phase()
    if rank == 0:
        print(f"Initialized with {num_episodes} episodes and {env_steps} steps")
    return env_steps


def resume(model, params, n_envs, first_step):
    """The last thing before the loop: with resume=true restore the run state of models= (after it nothing may draw from a
    generator but the loop itself) and return the step the loop continues at, the saved step plus one iteration; else
    `first_step`."""
    if not params["resume"]:
        return first_step
    extra = model.load_run_state(params["models"])
    if "step" not in extra:
        raise ValueError(f"resume=true: {params['models']} was not written by this command line (its run_state has no step)")
    return int(extra["step"]) + n_envs


def collect_many(model, env, params, rank, world):
    """The collect-update loop for ``collect_envs = n > 1``: one iteration is one Collector.step() = n environment steps
    [step, step + n).  Every multiple of ``environment_steps_per_update`` in that range runs one burst of
    ``collect_interval`` train steps, so the update-to-data ratio stays that of the reference; update_critic is called once
    per iteration if any step of the range is not a multiple of ``slow_critic_update_interval`` (the reference's inverted
    cadence, src/main.py:110-112); logging and evaluation fire when a multiple of log_freq / test_interval falls in it."""
    from big_dreamer_amd.collect import Collector
    n = env.n
    collector = Collector(model, env)
    env_steps = fill_replay(model, params, rank, lambda: collector.seed(params["seed_steps"]))
    env_steps = resume(model, params, n, env_steps)
    logs, past, logged = {}, time.time(), env_steps
    slow = params["ActorCritic"]["slow_critic_update_interval"]
    for step in range(env_steps, params["train_steps"], n):
        steps = range(step, step + n)
        for _ in range(sum(1 for s in steps if s % params["environment_steps_per_update"] == 0)):
            t0 = time.time()
            for _ in range(params["collect_interval"]):
                logs = model.train_step()
            logs["weight_update_per_sec"] = params["collect_interval"] / (time.time() - t0)
        if params["algorithm"] != "planet" and any(s % slow for s in steps):
            model.update_critic()
        collector.step(explore=True)
        if collector.finished_returns:
            logs["episode_total_reward"] = collector.finished_returns[-1]
        if any(s % params["log_freq"] == 0 for s in steps) and rank == 0:
            logs["env_update_per_sec"] = (step + n - logged) / max(time.time() - past, 1e-9)
            past, logged = time.time(), step + n
            print(step, {k: (round(v, 5) if isinstance(v, float) else v) for k, v in logs.items()
                         if not isinstance(v, (list, tuple))}, flush=True)      # (list-valued diagnostics are left out)
        if params["evaluation"] and any(s % params["test_interval"] == 0 for s in steps):
            evaluate(model, params, step, rank)
        if params["openl_freq"] > 0 and rank == 0 and any(s % params["openl_freq"] == 0 for s in steps):
            open_loop(model, params, step)
        if params["checkpoint_dir"] and any(s % params["checkpoint_interval"] == 0 for s in steps):
            checkpoint(model, params, step, rank, world, n)
    env.close()


def my_app(argv):
    params = load_config(argv)
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    np.random.seed(params["seed"] + rank)
    torch.manual_seed(params["seed"])                 # identical initial weights on every rank
    random.seed(params["seed"] + rank)
    if params["algorithm"] not in ("planet", "dreamer", "dreamerV2"):     # as src/main.py:73-81
        raise NotImplementedError(f'algorithm {params["algorithm"]} is not yet implemented.')
    from big_dreamer_amd.config import RETURN_NORM_KEYS, check_return_normalization
    check_return_normalization(*(params["ActorCritic"][k] for k in RETURN_NORM_KEYS), algorithm=params["algorithm"])
    from big_dreamer_amd.config import CRITIC_HEAD_KEYS, check_critic_head
    check_critic_head(*(params["ActorCritic"][k] for k in CRITIC_HEAD_KEYS), algorithm=params["algorithm"])
    from big_dreamer_amd.config import REWARD_HEAD_KEYS, check_reward_head, check_symlog_observations
    check_reward_head(*(params[k] for k in REWARD_HEAD_KEYS), algorithm=params["algorithm"])
    check_symlog_observations(params["symlog_observations"], params["pixel_observation"], params["algorithm"])
    from big_dreamer_amd import checkpoint as ck
    for key in ("models", "experience_replay"):                    # multi-GPU: every rank loads its own ..._rank<r> file
        params[key] = ck.for_rank(params[key], rank, world)
    if params["resume"]:
        if not params["models"] or not os.path.exists(params["models"]):
            raise ValueError(f"resume=true needs models=<checkpoint file> (models='{params['models']}')")
        saved = ck.read_run_state(params["models"])["extra"].get("collect_envs", params["collect_envs"])
        if int(saved) != int(params["collect_envs"]):
            raise ValueError(f"resume=true: {params['models']} was saved by a run with collect_envs={saved}, this run has "
                             f"collect_envs={params['collect_envs']}")
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if world > 1:      # (device_id: the communicator is built now, before the engine's streams -- DESIGN.md section 6)
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_stream(torch.cuda.Stream())        # stay off the legacy null stream
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.planet import Planet
    from big_dreamer_amd.env import Env, VecEnv
    n_envs = int(params["collect_envs"])
    env = Env(params) if n_envs == 1 else VecEnv(Env, params, n_envs)
    agent_cls = {"planet": Planet, "dreamer": Dreamer, "dreamerV2": DreamerV2}[params["algorithm"]]
    model = agent_cls(params, env, world_size=world)
    if params.get("replica_sync_at_start", False) and world > 1:
        # every rank becomes a copy of rank 0 as built and loaded (models= may exist on rank 0 only); `resume` below still
        # restores each rank's own run state
        model.sync_replicas(0)
    torch.manual_seed(params["seed"] + rank)
    if params["test"]:                                # evaluate the agent as built (models= loads a checkpoint) and stop
        evaluate(model, params, 0, rank)
        env.close()
        return
    if n_envs > 1:
        collect_many(model, env, params, rank, world)
        return
    env_steps = fill_replay(model, params, rank, model.randomly_initialize_replay_buffer)
    dev = model.device
    observation = env.reset()
    belief = torch.zeros(1, params["belief_size"], device=dev)
    # (the reference sizes this with params["state_size"], src/main.py:94, which is wrong for Categorical latents, where
    # the agent's state_size is dimensions * classes, src/planet.py:56-57)
    posterior_state = torch.zeros(1, model.state_size, device=dev)
    action = torch.zeros(1, env.action_size, device=dev)
    logs, episode_reward, past = {}, 0.0, time.time()
    env_steps = resume(model, params, 1, env_steps)
    for step in range(env_steps, params["train_steps"]):
        if step % params["environment_steps_per_update"] == 0:
            t0 = time.time()
            for _ in range(params["collect_interval"]):
                logs = model.train_step()
            logs["weight_update_per_sec"] = params["collect_interval"] / (time.time() - t0)
        if params["algorithm"] != "planet" and step % params["ActorCritic"]["slow_critic_update_interval"]:
            model.update_critic()                                              # cadence as in the reference (:110-112)
        belief, posterior_state, action, next_observation, reward, done = model.update_belief_and_act(
            env, belief, posterior_state, action, observation, explore=True)
        model.buffer.append(observation, action.cpu()[0], reward, done)
        episode_reward += reward
        observation = next_observation
        if done:
            logs["episode_total_reward"] = episode_reward
            observation, episode_reward = env.reset(), 0.0
            belief.zero_(); posterior_state.zero_(); action.zero_()
        if step % params["log_freq"] == 0 and rank == 0:
            logs["env_update_per_sec"] = params["log_freq"] / max(time.time() - past, 1e-9)
            past = time.time()
            print(step, {k: (round(v, 5) if isinstance(v, float) else v) for k, v in logs.items()
                         if not isinstance(v, (list, tuple))}, flush=True)      # (list-valued diagnostics are left out)
        if params["evaluation"] and step % params["test_interval"] == 0:
            evaluate(model, params, step, rank)
        if params["openl_freq"] > 0 and rank == 0 and step % params["openl_freq"] == 0:
            open_loop(model, params, step)
        if params["checkpoint_dir"] and step % params["checkpoint_interval"] == 0:
            checkpoint(model, params, step, rank, world, 1)
    env.close()


if __name__ == "__main__":
    my_app(sys.argv[1:])
