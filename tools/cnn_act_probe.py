#!/usr/bin/env python3
"""Steady-state ms/step of the pixel training step (BASELINE configs[2]) per cnn_activation_function (README, DESIGN
section 7).  bench.py measures the default (ELU) only.

One engine per activation on fixed device batches with perf-mode noise; after the warm-up, timing events on the behaviour
stream give ms/step; each measurement is repeated.  One JSON line per activation.

    python tools/cnn_act_probe.py --acts ELU ReLU Tanh --steps 30 --warmup 10 --repeats 3
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


def measure(d, steps: int, warmup: int, repeats: int):
    eng = DreamerEngine(d, None, "cuda", params=synth.make_params(d, 0))
    batches = [{k: torch.as_tensor(v).cuda() for k, v in synth.make_batch(d, s).items()} for s in range(2)]
    for i in range(warmup):
        eng.train_step(batches[i % 2], None, sync_logs=False)
    out = []
    for _ in range(repeats):
        eng.join()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for i in range(steps + 1):
            eng.train_step(batches[i % 2], None, sync_logs=False)
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
    ap.add_argument("--acts", nargs="+", default=list(synth.CNN_ACTIVATIONS), choices=synth.CNN_ACTIVATIONS)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for act in a.acts:
        ms = measure(dataclasses.replace(synth.CONFIG3, cnn_act=act), a.steps, a.warmup, a.repeats)
        line = json.dumps({"config": "configs[2]", "cnn_activation_function": act, "ms_per_step": [round(x, 4) for x in ms],
                           "median_ms": round(sorted(ms)[len(ms) // 2], 4), "steps": a.steps, "warmup": a.warmup})
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
