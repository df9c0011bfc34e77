"""Cost of the training diagnostics (``diagnostics_interval``) on the GPU box.

Milliseconds per step of ``Dreamer.train_step`` in bursts of 5 (five calls, then the last log dict is read, as the collect loop
does) with diagnostics_interval 0, 1 and 100 on ONE agent (``Dreamer.set_diagnostics``), the three settings alternating block
by block in one process, at configs[1] size (state observations), configs[2] size (64x64 pixels, A = 17) and, with `cat` as
third argument, configs[4]'s latents on state observations (32 x 32 Categorical latents, batch 100).

Every agent is warmed up first; BLOCKS blocks of BLOCK steps per setting; median and [min, max] over the blocks.
``outside_interval0_range`` says whether a setting's median lies outside interval 0's own [min, max] in that cell -- only then
does a difference count.  Not measured here: more than one rank, the kernels' own times by a profiler.
Writes <out_dir>/<tag>_diag_time.json (default out_dir: profiles/).

    python tools/diag_time.py [tag] [out_dir] [cat]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import big_dreamer_amd  # noqa: E402,F401
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "diag"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
BLOCKS, BLOCK, BURST, ROWS = 7, 200, 5, 4000
INTERVALS = (0, 1, 100)
SIZES = {"configs[1]": (synth.CONFIG2, []), "configs[2]": (synth.CONFIG3, [])}
if "cat" in sys.argv[3:]:
    SIZES["configs[4] latents, state observations"] = (synth.CONFIG5_STATE, [
        "batch_size=100", "latent_distribution=Categorical", "discrete_latent_dimensions=32", "discrete_latent_classes=32"])


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


def make_agent(d, extra):
    class _Env:
        action_size, observation_size = d.A, (3 if d.pixel else d.O)

    params = load_config([f"experience_size={ROWS}", f"pixel_observation={'true' if d.pixel else 'false'}", *extra])
    assert (params["batch_size"], params["seq_len"], params["belief_size"]) == (d.B, d.L, d.Be)
    torch.manual_seed(0)
    agent = Dreamer(params, _Env())
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


def measure(agent):
    for k in INTERVALS:                                  # warm-up of every setting
        agent.set_diagnostics(k)
        burst_block(agent)
    times = {k: [] for k in INTERVALS}
    for _ in range(BLOCKS):
        for k in INTERVALS:
            agent.set_diagnostics(k)
            times[k].append(burst_block(agent))
    agent.set_diagnostics(1)
    keys = sorted(k for k in dict(agent.train_step()) if "/" in k or k.startswith(("kl_raw", "post_", "imag_")))
    agent.set_diagnostics(0)
    res = {f"interval_{k}": stats(v) for k, v in times.items()}
    base = res["interval_0"]
    for k in INTERVALS[1:]:
        c = res[f"interval_{k}"]
        c["outside_interval0_range"] = not base["min"] <= c["median"] <= base["max"]
        c["median_minus_interval0_ms"] = c["median"] - base["median"]
    return {"train_step_burst_ms_per_step": res, "diagnostic_keys_seen": len(keys)}


out = {"what": __doc__.split("\n\n")[0] + " See tools/diag_time.py for what each cell is.",
       "blocks": BLOCKS, "steps_per_block": BLOCK, "burst": BURST, "intervals": list(INTERVALS),
       "device": torch.cuda.get_device_name(0),
       "not_measured": ["more than one rank", "kernel times by a profiler"] + ([] if len(SIZES) > 2 else ["configs[4]"])}
torch.cuda.set_device(0)
torch.cuda.set_stream(torch.cuda.Stream())               # off the legacy null stream, as src/main.py
np.random.seed(0)
for name, (d, extra) in SIZES.items():
    agent = make_agent(d, extra)
    out[name] = measure(agent)
    print(name, json.dumps(out[name]), flush=True)
    del agent
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_diag_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
