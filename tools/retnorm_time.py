"""Cost of the percentile return normalisation (``ActorCritic.return_normalization=percentile``) on the GPU box.

(a) Milliseconds per step of ``Dreamer.train_step`` in bursts of 5 (five calls, then the last log dict is read, as the collect
loop does) with 'none' and 'percentile' -- two agents built alike, alternating block by block in one process -- at
configs[1] size (state observations), configs[2] size (64x64 pixels, A = 17) and configs[4]'s latents on state observations
(32 x 32 Categorical latents, batch 100).  Every agent is warmed up first; BLOCKS blocks of BLOCK steps per setting; median and
[min, max] over the blocks.  ``inside_none_range`` says whether the 'percentile' median lies inside 'none''s own [min, max].

(b) Microseconds of ``bd_return_range`` alone between two HIP events on an idle device, at M = 37 500 (configs[1]), 75 000
and 600 000 (B = 800) normal draws with the 5 % / 95 % ranks: median and [min, max] of LAUNCHES launches.

Not measured here: more than one rank on RCCL, configs[4] on pixels.
Writes <out_dir>/<tag>_retnorm_time.json (default out_dir: profiles/).

    python tools/retnorm_time.py [tag] [out_dir] [kernel]        ("kernel": part (b) only)"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import big_dreamer_amd  # noqa: E402,F401
from big_dreamer_amd import _cabi, synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer, DreamerV2  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "retnorm"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
kernel_only = "kernel" in sys.argv[3:]
BLOCKS, BLOCK, BURST, ROWS, LAUNCHES = 7, 200, 5, 4000, 50
MODES = ("none", "percentile")
SIZES = {"configs[1]": (synth.CONFIG2, []), "configs[2]": (synth.CONFIG3, []),
         "configs[4] latents, state observations": (synth.CONFIG5_STATE, [
             "batch_size=100", "latent_distribution=Categorical", "discrete_latent_dimensions=32",
             "discrete_latent_classes=32"])}
KERNEL_M = (37500, 75000, 600000)


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
    buf.idx, buf.full, buf.steps = buf.size // 3, True, buf.size
    buf.mark_dirty()


def stats(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def make_agent(d, extra, mode):
    class _Env:
        action_size, observation_size = d.A, (3 if d.pixel else d.O)

    params = load_config([f"experience_size={ROWS}", f"pixel_observation={'true' if d.pixel else 'false'}",
                          f"ActorCritic.return_normalization={mode}", *extra])
    assert (params["batch_size"], params["seq_len"], params["belief_size"]) == (d.B, d.L, d.Be)
    torch.manual_seed(0)
    agent = (DreamerV2 if d.categorical else Dreamer)(params, _Env())
    fill(agent.buffer)
    return agent


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


def measure(d, extra):
    agents = {m: make_agent(d, extra, m) for m in MODES}
    for m in MODES:                                      # warm-up of both
        burst_block(agents[m])
    times = {m: [] for m in MODES}
    for _ in range(BLOCKS):
        for m in MODES:
            times[m].append(burst_block(agents[m]))
    res = {m: stats(v) for m, v in times.items()}
    base, c = res["none"], res["percentile"]
    c["inside_none_range"] = base["min"] <= c["median"] <= base["max"]
    c["median_minus_none_ms"] = c["median"] - base["median"]
    last = dict(agents["percentile"].train_step())
    state = agents["percentile"].return_norm_state()
    return {"train_step_burst_ms_per_step": res, "M": d.Hm * d.T * d.B, "return_scale_last": last["return_scale"],
            "updates": state["count"], "skipped": state["skipped"]}


def kernel_times():
    out = {}
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    rg = torch.zeros(4, device="cuda")
    for M in KERNEL_M:
        x = torch.randn(M, device="cuda")
        k_lo, k_hi = int(math.floor(0.05 * (M - 1))), int(math.floor(0.95 * (M - 1)))
        us = []
        for i in range(LAUNCHES + 5):
            torch.cuda.synchronize()                     # an idle device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _cabi.check(_cabi.lib.bd_return_range(x.data_ptr(), M, k_lo, k_hi, 0.99, 1.0, state.data_ptr(), rg.data_ptr(),
                                                  _cabi.stream()))
            b.record()
            b.synchronize()
            if i >= 5:
                us.append(a.elapsed_time(b) * 1e3)
        out[f"M={M}"] = stats(us)
    return out


out = {"what": __doc__.split("\n\n")[0] + " See tools/retnorm_time.py for what each cell is.",
       "blocks": BLOCKS, "steps_per_block": BLOCK, "burst": BURST, "launches": LAUNCHES,
       "device": torch.cuda.get_device_name(0),
       "not_measured": ["more than one rank on RCCL", "configs[4] on pixels"]}
torch.cuda.set_device(0)
torch.cuda.set_stream(torch.cuda.Stream())               # off the legacy null stream, as src/main.py
np.random.seed(0)
out["bd_return_range_us"] = kernel_times()
print("bd_return_range_us", json.dumps(out["bd_return_range_us"]), flush=True)
if not kernel_only:
    for name, (d, extra) in SIZES.items():
        out[name] = measure(d, extra)
        print(name, json.dumps(out[name]), flush=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_retnorm_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
