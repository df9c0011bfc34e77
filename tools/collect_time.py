"""Collect-loop throughput and replay-append cost on the GPU box, config sizes of BASELINE.json: configs[1] on state
observations and configs[2] (64x64 pixels, A = 17).

  * environment steps per second of one collect decision: the CLI's single-environment loop (update_belief_and_act on one
    environment + ExperienceReplay.append: the path of collect_envs=1) and Collector.step() for collect_envs in {1, 4, 16}
    (one decision for all environments + ExperienceReplay.append_batch).  The wall time includes the synthetic environments'
    own stepping on the host.
  * microseconds per appended transition with the device mirror live: append (one environment, four small device
    operations) and append_batch on 4 and 16 lanes, once uploading the host rows and once reading observations_device /
    actions_device (one staging upload + one bd_replay_append launch either way).

Host wall clock between torch.cuda.synchronize() calls, BLOCK decisions / APPEND_BLOCK appends per block; one warm-up block,
then REPEATS timed ones; median and [min, max] over the repeats.  Each case runs on a fresh agent / buffer, all in one process;
the two append_batch variants of a lane count alternate block by block.  Writes
<out_dir>/<tag>_collect_time.json (default out_dir: profiles/).

    python tools/collect_time.py [tag] [out_dir]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd.collect import Collector  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402
from big_dreamer_amd.env import Env, VecEnv  # noqa: E402
from big_dreamer_amd.memory import ExperienceReplay  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "collect"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
REPEATS, BLOCK, APPEND_BLOCK, ROWS = 3, 400, 1000, 4000
CONFIGS = {
    "configs[1] state": [],
    "configs[2] pixel": ["pixel_observation=true", "synthetic_env_action_size=17"],
}


def timed(block):
    """One warm-up block, then REPEATS timed ones: seconds per block."""
    times = []
    for i in range(REPEATS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        block()
        torch.cuda.synchronize()
        if i:
            times.append(time.perf_counter() - t0)
    return times


def summary(times, per_block, scale, name):
    """Rates (scale > 0: per_block / seconds) or costs (scale < 0: seconds / per_block * 1e6)."""
    vals = [per_block / t for t in times] if scale > 0 else [t / per_block * 1e6 for t in times]
    return {f"{name}_median": statistics.median(vals), f"{name}_min": min(vals), f"{name}_max": max(vals)}


def cli_loop(params):
    """The present loop of src/main.py on one environment."""
    env = Env(params)
    agent = Dreamer(params, env)
    agent.seed_steps = 200
    agent.randomly_initialize_replay_buffer()
    agent.buffer.sync_device()
    dev = agent.device
    box = {"observation": env.reset(), "belief": torch.zeros(1, agent.belief_size, device=dev),
           "state": torch.zeros(1, agent.state_size, device=dev), "action": torch.zeros(1, agent.action_size, device=dev)}

    def block():
        for _ in range(BLOCK):
            belief, state, action, next_observation, reward, done = agent.update_belief_and_act(
                env, box["belief"], box["state"], box["action"], box["observation"], explore=True)
            agent.buffer.append(box["observation"], action.cpu()[0], reward, done)
            if done:
                next_observation = env.reset()
                belief.zero_(); state.zero_(); action.zero_()
            box.update(observation=next_observation, belief=belief, state=state, action=action)

    return dict(summary(timed(block), BLOCK, 1, "env_steps_per_s"), act_fused=bool(agent.act_fused))


def collector_loop(params, n):
    params = dict(params, collect_envs=n)
    agent = Dreamer(params, VecEnv(Env, params, n))
    collector = Collector(agent, agent.env)
    collector.seed(200)
    agent.buffer.sync_device()

    def block():
        for _ in range(BLOCK):
            collector.step()

    return dict(summary(timed(block), BLOCK * n, 1, "env_steps_per_s"), act_fused=bool(agent.act_fused))


def append_buffer(pixel, A, lanes):
    buf = ExperienceReplay(ROWS, A, 5, pixel, 3, "cuda", lanes=max(lanes, 1))
    for k in ("observations", "actions", "rewards", "nonterminals"):
        getattr(buf, k)[:] = 0
    buf.sync_device()
    return buf


def append_cost(pixel, A, lanes):
    """lanes = 0: append on the flat ring.  Else append_batch uploading the host rows and append_batch reading the device
    copies, on two buffers, their blocks alternating."""
    rng = np.random.default_rng(0)
    n = max(lanes, 1)
    obs = torch.from_numpy(rng.uniform(-0.5, 0.5, (n, 3, 64, 64) if pixel else (n, 3)).astype(np.float32))
    act = torch.from_numpy(rng.uniform(-1, 1, (n, A)).astype(np.float32))
    rew, done = torch.from_numpy(rng.standard_normal(n).astype(np.float32)), torch.zeros(n, dtype=torch.bool)
    if lanes == 0:
        buf, reward = append_buffer(pixel, A, 0), float(rew[0])

        def block():
            for _ in range(APPEND_BLOCK):
                buf.append(obs, act[0], reward, False)

        return {"append": summary(timed(block), APPEND_BLOCK, -1, "us_per_transition")}
    bufs = (append_buffer(pixel, A, lanes), append_buffer(pixel, A, lanes))
    kws = ({}, {"observations_device": obs.cuda(), "actions_device": act.cuda()})
    times = ([], [])
    for i in range(REPEATS + 1):                       # block 0 of either is the warm-up
        for buf, kw, ts in zip(bufs, kws, times):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(APPEND_BLOCK):
                buf.append_batch(obs, act, rew, done, **kw)
            torch.cuda.synchronize()
            if i:
                ts.append(time.perf_counter() - t0)
    return {f"append_batch_{lanes}": summary(times[0], APPEND_BLOCK * n, -1, "us_per_transition"),
            f"append_batch_{lanes}_device": summary(times[1], APPEND_BLOCK * n, -1, "us_per_transition")}


out = {"what": "collect loop: environment steps per second (cli_loop: update_belief_and_act on one environment + append, the "
               "collect_envs=1 path; collector_N: Collector.step() on N environments) and microseconds per appended "
               "transition with the device mirror live (append; append_batch_N uploading the host rows; "
               "append_batch_N_device reading observations_device / actions_device); median and [min, max] over the repeats",
       "repeats": REPEATS, "decisions_per_block": BLOCK, "appends_per_block": APPEND_BLOCK}
for name, overrides in CONFIGS.items():
    params = load_config(overrides + [f"experience_size={ROWS}"])
    pixel, A = bool(params["pixel_observation"]), int(params["synthetic_env_action_size"])
    res = {}
    torch.manual_seed(0)
    res["cli_loop"] = cli_loop(params)
    print(name, "cli_loop", json.dumps(res["cli_loop"]), flush=True)
    for n in (1, 4, 16):
        torch.manual_seed(0)
        res[f"collector_{n}"] = collector_loop(params, n)
        print(name, f"collector_{n}", json.dumps(res[f"collector_{n}"]), flush=True)
    for n in (0, 1, 4, 16):
        res.update(append_cost(pixel, A, n))
    for k, v in res.items():
        if k.startswith("append"):
            print(name, k, json.dumps(v), flush=True)
    out[name] = res
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_collect_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
