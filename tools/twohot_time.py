"""Cost of the two-hot critic (``ActorCritic.critic_head=twohot``) on the GPU box.

(a) Milliseconds per step of ``Dreamer.train_step`` in bursts of 5 (five calls, then the last log dict is read, as the collect
loop does) with 'normal' and 'twohot' (K = 255, Z = 20) -- two agents built alike, alternating block by block in one
process -- at configs[1] size (state observations), configs[2] size (64x64 pixels, A = 17) and configs[4]'s latents on state
observations (32 x 32 Categorical latents, batch 100).  Every agent is warmed up first; BLOCKS blocks of BLOCK steps per
setting; median and [min, max] over the blocks.  'twohot' gives up the fused imagined heads and the chunk plan and widens
two layers to K, so it costs step time; nothing is asserted.

(b) Microseconds of each of the three kernels alone between two HIP events on an idle device at rows = 34 300 (configs[1]'s
Hm x N), K = 255: median and [min, max] of LAUNCHES launches, beside the bytes the kernel must move (the logits read once;
the two gradient kernels write as many again; the per-row vectors) and that over the median as a fraction of the 8 TB/s HBM
peak.  A 35 MB operand fits the 256 MB last-level cache, so a repeated launch may be served from there: the figure is
the kernel's rate on a warm device, not a claim about HBM.

Not measured here: more than one rank on RCCL, configs[4] on pixels, K other than 255.
Writes <out_dir>/<tag>_twohot_time.json (default out_dir: profiles/).

    python tools/twohot_time.py [tag] [out_dir] [kernel]        ("kernel": part (b) only)"""
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
from big_dreamer_amd import _cabi, synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer, DreamerV2  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "twohot"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
kernel_only = "kernel" in sys.argv[3:]
BLOCKS, BLOCK, BURST, ROWS, LAUNCHES = 7, 200, 5, 4000, 50
MODES = ("normal", "twohot")
SIZES = {"configs[1]": (synth.CONFIG2, []), "configs[2]": (synth.CONFIG3, []),
         "configs[4] latents, state observations": (synth.CONFIG5_STATE, [
             "batch_size=100", "latent_distribution=Categorical", "discrete_latent_dimensions=32",
             "discrete_latent_classes=32"])}
KERNEL_ROWS, KERNEL_K, KERNEL_Z = 34300, 255, 20.0
HBM_PEAK = 8.0e12


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
                          f"ActorCritic.critic_head={mode}", *extra])
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
    base, c = res["normal"], res["twohot"]
    c["median_minus_normal_ms"] = c["median"] - base["median"]
    c["median_over_normal"] = c["median"] / base["median"]
    last = {m: dict(agents[m].train_step()) for m in MODES}
    return {"train_step_burst_ms_per_step": res, "rows": d.Hm * d.T * d.B,
            "value_loss_last": {m: last[m]["value_loss"] for m in MODES},
            "behaviour_plan": {m: list(agents[m].engine._bh_plan_used) for m in MODES}}


def kernel_times():
    rows, K, Z = KERNEL_ROWS, KERNEL_K, KERNEL_Z
    lib, check = _cabi.lib, _cabi.check
    logits = torch.randn(rows, K, device="cuda")
    dlogits = torch.empty(rows, K, device="cuda")
    target, dv = 50.0 * torch.randn(rows, device="cuda"), torch.randn(rows, device="cuda")
    val, loss = torch.empty(rows, device="cuda"), torch.empty(rows, device="cuda")
    P = lambda t: t.data_ptr()
    mat, vec = 4 * rows * K, 4 * rows
    launches = {
        "bd_twohot_decode": (mat + vec, lambda: lib.bd_twohot_decode(P(logits), K, rows, K, Z, P(val), None, _cabi.stream())),
        "bd_twohot_decode_backward": (2 * mat + vec, lambda: lib.bd_twohot_decode_backward(
            P(logits), K, P(dv), rows, K, Z, P(dlogits), K, _cabi.stream())),
        "bd_twohot_nll": (2 * mat + 2 * vec, lambda: lib.bd_twohot_nll(
            P(logits), K, P(target), None, rows, K, Z, 1.0 / rows, P(dlogits), K, None, P(loss), _cabi.stream())),
    }
    out = {}
    for name, (nbytes, launch) in launches.items():
        us = []
        for i in range(LAUNCHES + 5):
            torch.cuda.synchronize()                     # an idle device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(launch())
            b.record()
            b.synchronize()
            if i >= 5:
                us.append(a.elapsed_time(b) * 1e3)
        s = stats(us)
        s["bytes_moved"] = nbytes
        s["bytes_per_s_at_median"] = nbytes / (s["median"] * 1e-6)
        s["fraction_of_8TBps_hbm_peak"] = s["bytes_per_s_at_median"] / HBM_PEAK
        out[name] = s
    return {"rows": rows, "K": K, "kernels_us": out}


out = {"what": __doc__.split("\n\n")[0] + " See tools/twohot_time.py for what each cell is.",
       "blocks": BLOCKS, "steps_per_block": BLOCK, "burst": BURST, "launches": LAUNCHES,
       "device": torch.cuda.get_device_name(0),
       "not_measured": ["more than one rank on RCCL", "configs[4] on pixels", "K other than 255"]}
torch.cuda.set_device(0)
torch.cuda.set_stream(torch.cuda.Stream())               # off the legacy null stream, as src/main.py
np.random.seed(0)
out["kernels_alone"] = kernel_times()
print("kernels_alone", json.dumps(out["kernels_alone"]), flush=True)
if not kernel_only:
    for name, (d, extra) in SIZES.items():
        out[name] = measure(d, extra)
        print(name, json.dumps(out[name]), flush=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_twohot_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
