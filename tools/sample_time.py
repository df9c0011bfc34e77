"""Cost of ``ExperienceReplay.sample`` on its two routes -- the host sampler (np.random index draws, pinned index upload, three or
four gather launches) and the device sampler (``device_sampler=True``: one bd_replay_sample_gather launch) -- on the GPU box.

  (a) microseconds of one ``sample(n, L)`` call at four sizes, measured twice: "enqueue" -- the host time of a call as the
      training loop pays it, BLOCK calls back to back with no synchronisation inside the timed region (the device is idle
      at its start and drained after its end) -- and "sync" -- each call followed by torch.cuda.synchronize().
        configs[1]       B = 50, L = 50, state observations (O = 3, A = 1)
        configs[2]       B = 50, L = 50, 64x64 pixels, A = 17
        B=800            B = 800, L = 50, state observations
        lanes=16         B = 50, L = 50, state observations, a ring of 16 lanes
  (b) milliseconds per step of ``Dreamer.train_step`` at configs[1] size in bursts of 5 (five calls, then the last log dict
      is read, as the collect loop does), two agents in the process, one per route.

Every shape is warmed up first; then the two routes alternate block by block, BLOCKS blocks of BLOCK calls (or steps) each;
median and [min, max] over the blocks.  ``device_outside_host_range`` says whether the device route's median lies outside the
host route's own [min, max] in that cell -- only then does a difference count.  Writes <out_dir>/<tag>_sample_time.json
(default out_dir: profiles/).

    python tools/sample_time.py [tag] [out_dir]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402
from big_dreamer_amd.env import Env  # noqa: E402
from big_dreamer_amd.memory import ExperienceReplay  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "sample"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
BLOCKS, BLOCK, BURST, ROWS = 7, 200, 5, 4000
# name -> (n, L, pixel, A, lanes)
SHAPES = {"configs[1] B=50 L=50 state": (50, 50, False, 1, 1), "configs[2] B=50 L=50 pixel": (50, 50, True, 17, 1),
          "B=800 L=50 state": (800, 50, False, 1, 1), "B=50 L=50 state lanes=16": (50, 50, False, 1, 16)}


def fill(buf, seed=0):
    """A full ring of synthetic transitions, head at an arbitrary row."""
    rng = np.random.default_rng(seed)
    if buf.pixel_observation:
        buf.observations[:] = (rng.integers(0, 32, size=buf.observations.shape) * 8).astype(np.uint8)
    else:
        buf.observations[:] = rng.standard_normal(buf.observations.shape, dtype=np.float32)
    buf.actions[:] = rng.uniform(-1, 1, buf.actions.shape).astype(np.float32)
    buf.rewards[:] = rng.standard_normal(buf.rewards.shape, dtype=np.float32)
    buf.nonterminals[:] = 1.0
    buf.idx, buf.full, buf.steps = (buf.lane_size if buf.lanes > 1 else buf.size) // 3, True, buf.size
    buf.mark_dirty()


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def cell(host, device):
    out = {"host": stats(host), "device": stats(device)}
    out["device_outside_host_range"] = not out["host"]["min"] <= out["device"]["median"] <= out["host"]["max"]
    return out


def sample_block(buf, n, L, sync):
    """Microseconds per call of BLOCK calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if sync:
        for _ in range(BLOCK):
            buf.sample(n, L)
            torch.cuda.synchronize()
    else:
        for _ in range(BLOCK):
            buf.sample(n, L)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / BLOCK * 1e6


def burst_block(agent):
    """Milliseconds per step of BLOCK steps in bursts of BURST."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(BLOCK // BURST):
        for _ in range(BURST):
            logs = agent.train_step()
        dict(logs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / BLOCK * 1e3


out = {"what": "ExperienceReplay.sample on the host route and on the device route (device_sampler=True): microseconds per call "
               "as enqueued (no synchronisation in the timed region) and with a synchronisation after every call; "
               "Dreamer.train_step in bursts of 5 at configs[1] size, milliseconds per step; routes alternate block by block; "
               "median and [min, max] over the blocks",
       "blocks": BLOCKS, "calls_per_block": BLOCK, "burst": BURST, "replay_rows": ROWS, "device": torch.cuda.get_device_name(0)}
torch.manual_seed(0)
np.random.seed(0)
buffers = {}
for name, (n, L, pixel, A, lanes) in SHAPES.items():                        # build and warm up every shape first
    pair = [ExperienceReplay(ROWS, A, 5, pixel, 3, "cuda", lanes=lanes, device_sampler=on) for on in (False, True)]
    for buf in pair:
        fill(buf)
        for sync in (False, True):
            sample_block(buf, n, L, sync)
    buffers[name] = pair
sample = {}
for name, (n, L, pixel, A, lanes) in SHAPES.items():
    res = {}
    for kind, sync in (("enqueue_us", False), ("sync_us", True)):
        times = ([], [])
        for _ in range(BLOCKS):
            for buf, ts in zip(buffers[name], times):
                ts.append(sample_block(buf, n, L, sync))
        res[kind] = cell(*times)
    sample[name] = res
    print(name, json.dumps(res), flush=True)
out["sample"] = sample
del buffers

agents = []
for on in (False, True):
    params = load_config([f"experience_size={ROWS}", f"sample_on_device={'true' if on else 'false'}"])
    torch.manual_seed(0)
    agent = Dreamer(params, Env(params))
    fill(agent.buffer)
    burst_block(agent)                                                       # warm-up
    agents.append(agent)
times = ([], [])
for _ in range(BLOCKS):
    for agent, ts in zip(agents, times):
        ts.append(burst_block(agent))
out["train_step_burst_ms_per_step"] = dict(cell(*times), batch_size=int(agents[0].batch_size), seq_len=int(agents[0].seq_len))
print("train_step bursts", json.dumps(out["train_step_burst_ms_per_step"]), flush=True)
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_sample_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
