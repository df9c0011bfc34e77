"""What a checkpoint costs ("Checkpoint and resume"), host wall clock on the GPU box; per figure one warm-up, then
REPEATS timed runs, reported as the median and [min, max]:

  * Dreamer.save at the sizes of BASELINE.json configs[1] (state observations) and configs[2] (64x64 pixels, A = 17): the
    flush of the held-back optimiser steps, the join, the D2H copies of weights and moments, torch.save and the fsync;
  * a burst of BURST train_step() calls with one save in its middle against the same burst without it, configs[1] sizes: what
    a checkpoint costs a running three-stream pipeline (the save drains it, the steps after it fill it again);
  * ExperienceReplay.save / load of 100 000 state rows and of 20 000 pixel rows, with the bytes written and MB/s -- figures
    that belong to the disk of the machine (the directory is <out_dir>/ckpt_tmp) as much as to the code.

Writes <out_dir>/<tag>_checkpoint_time.json (default out_dir: profiles/).

    python tools/checkpoint_time.py [tag] [out_dir]"""
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402
from big_dreamer_amd.env import Env  # noqa: E402
from big_dreamer_amd.memory import ExperienceReplay  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "ckpt"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
tmp = os.path.join(out_dir, "ckpt_tmp")
os.makedirs(tmp, exist_ok=True)
REPEATS, BURST = 3, 50
AGENTS = {
    "configs[1] state": ["experience_size=5000"],
    "configs[2] pixel": ["experience_size=600", "pixel_observation=true", "synthetic_env_action_size=17"],
}


def stats(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def timed(fn, repeats=REPEATS):
    fn()                                                  # warm-up
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def fill(buf, rows, seed=0):
    """`rows` synthetic rows into the head of `buf` (pixels: 5-bit quantised frames)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if buf.pixel_observation:
        buf.observations[:rows] = (rng.integers(0, 32, size=(rows, 3, 64, 64), dtype=np.uint8) * 8)
    else:
        buf.observations[:rows] = rng.standard_normal((rows, buf.observations.shape[1]), dtype=np.float32)
    buf.actions[:rows] = rng.uniform(-1, 1, (rows, buf.actions.shape[1])).astype(np.float32)
    buf.rewards[:rows] = rng.standard_normal(rows, dtype=np.float32)
    buf.nonterminals[:rows] = 1.0
    buf.idx, buf.full, buf.steps = rows % buf.size, rows == buf.size, rows
    buf.mark_dirty()


out = {"what": "host wall time in seconds, median and [min, max] of the repeats after one warm-up", "repeats": REPEATS,
       "burst": BURST, "not_measured": "data-parallel runs (the save's flush is a collective there), the CLI loop as a whole, "
                                       "a cold page cache"}
for name, overrides in AGENTS.items():
    params = load_config(overrides)
    torch.manual_seed(0)
    np.random.seed(0)
    agent = Dreamer(params, Env(params))
    fill(agent.buffer, 500)
    path = os.path.join(tmp, "models_0.pth")
    for _ in range(3):
        agent.train_step()
    res = {"save_seconds": stats(timed(lambda: agent.save(path, extra={"step": 0}))), "file_bytes": os.path.getsize(path)}
    if name == "configs[1] state":

        def burst(save):
            for i in range(BURST):
                agent.train_step()
                if save and i == BURST // 2 - 1:
                    agent.save(path, extra={"step": i})
            agent.engine.join()

        plain, with_save = timed(lambda: burst(False)), timed(lambda: burst(True))
        res["burst_seconds"] = stats(plain)
        res["burst_with_one_save_seconds"] = stats(with_save)
        res["save_costs_the_burst_seconds"] = statistics.median(with_save) - statistics.median(plain)
    out[name] = res
    print(name, json.dumps(res), flush=True)
    del agent

for name, (rows, pixel) in {"replay 100000 state rows": (100_000, False), "replay 20000 pixel rows": (20_000, True)}.items():
    d = synth.CONFIG2
    buf = ExperienceReplay(rows + rows // 4, d.A, 5, pixel, d.O, "cpu")      # a ring larger than what it holds
    fill(buf, rows)
    path = os.path.join(tmp, "experience_0.npz")
    save = timed(lambda: buf.save(path))
    other = ExperienceReplay(rows + rows // 4, d.A, 5, pixel, d.O, "cpu")
    load = timed(lambda: other.load(path))
    size = os.path.getsize(path)
    assert other.steps == rows and np.array_equal(other.observations[:rows], buf.observations[:rows])
    out[name] = {"file_bytes": size, "save_seconds": stats(save), "load_seconds": stats(load),
                 "save_MB_per_s": size / 1e6 / statistics.median(save), "load_MB_per_s": size / 1e6 / statistics.median(load)}
    print(name, json.dumps(out[name]), flush=True)
    del buf, other
shutil.rmtree(tmp, ignore_errors=True)
with open(os.path.join(out_dir, f"{tag}_checkpoint_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
