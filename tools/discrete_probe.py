#!/usr/bin/env python3
"""Steady-state ms/step of the training step with the Categorical actor against the tanh-Normal one at the same action
width ("Discrete actions").

One engine per (config, actor, rho) on fixed device batches with perf-mode noise; after the warm-up, timing events on the
behaviour stream (recorded behind the actor update of the first and the last measured step) give ms/step; each
measurement is repeated.  One JSON line per (config, actor, rho).

    python tools/discrete_probe.py --configs config5_state config2 --A 18 --rho -1 0 --steps 50 --warmup 15 --repeats 3
    (configs[1] = synth.CONFIG2; configs[4] on state observations = synth.CONFIG5_STATE; both with A replaced)
"""
import argparse
import dataclasses
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.engine import DreamerEngine  # noqa: E402

CONFIGS = {"config2": synth.CONFIG2, "config5_state": synth.CONFIG5_STATE, "small": synth.SMALL}


def measure(d, rho: float, steps: int, warmup: int, repeats: int):
    eng = DreamerEngine(d, dict(gradient_mixing=rho), "cuda", params=synth.make_params(d, 0))
    batches = [{k: torch.as_tensor(v).cuda() for k, v in synth.make_batch(d, s).items()} for s in range(4)]
    for i in range(warmup):
        eng.train_step(batches[i % 4], None, sync_logs=False)
    out = []
    for _ in range(repeats):
        eng.join()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(steps + 1):
            eng.train_step(batches[i % 4], None, sync_logs=False)
            if i == 0:
                e0.record(eng._s_bh if eng.pipeline else torch.cuda.current_stream())
        e1.record(eng._s_bh if eng.pipeline else torch.cuda.current_stream())
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    logs = eng.logs()
    assert all(v == v for v in logs.values()), logs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["config5_state", "config2"], choices=sorted(CONFIGS))
    ap.add_argument("--A", type=int, default=18, help="action width (classes of the Categorical actor)")
    ap.add_argument("--rho", nargs="+", type=float, default=[-1.0, 0.0])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name in a.configs:
        for discrete in (False, True):
            d = dataclasses.replace(CONFIGS[name], A=a.A, discrete_actions=discrete)
            for rho in a.rho:
                ms = measure(d, rho, a.steps, a.warmup, a.repeats)
                line = json.dumps({"config": name, "A": a.A, "actor": "Categorical" if discrete else "Gaussian",
                                   "gradient_mixing": rho, "ms_per_step": [round(x, 4) for x in ms],
                                   "min_ms": round(min(ms), 4), "steps": a.steps, "warmup": a.warmup})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
