"""Latency of one evaluation decision on the GPU box under the three evaluation policies: Dreamer.update_belief_and_act on
the fused route (one bd_act_step / bd_act_step_cat launch) with action_mode = "sample" (the sampling kernel), "mode"
(SampleDist.mode: n_entropy = 100 draws x A log-densities per row, one wave per row, in the same launch) and "mean"
(tanh(mean)), at B = 1 and B = 10, explore off as the evaluation loop runs it, for two agents in ONE process:

    gaussian      BASELINE configs[1] size, Gaussian latents, tanh-Normal actor (A = 1): bd_act_step
    categorical   BASELINE configs[4] size, 32 x 32 Categorical latents, tanh-Normal actor (A = 17): bd_act_step_cat
                  (BD_ACT_FUSED_CAT=1 is set here; it is off by default)

Per agent and batch size: 20 warm-up calls, then 300 timed calls per policy, repeated REPEATS times with the three policies
alternating; the figures are the median and the range [min, max] of the per-call host wall time (incl. the action's D2H
copy) over the repeats.  The kernel's own time per policy comes from HIP events around the launch in a separate pass.
"mode" and "mean" run the evaluation instantiation of the kernel (the sampling kernels carry none of it), so "mean"
against "sample" is the cost of that instantiation and "mode" against "mean" the cost of the selection.
Writes <out_dir>/<tag>_act_mode_latency.json (default out_dir: profiles/).

    python tools/act_mode_latency.py [tag] [out_dir]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "r13"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
WARMUP, CALLS, REPEATS = 20, 300, 7
MODES = ("sample", "mode", "mean")
AGENTS = {
    "gaussian": (synth.CONFIG2, synth.CONFIG2.A, ["experience_size=100"], "BD_ACT_FUSED", "act_fused", "act_step"),
    "categorical": (synth.CONFIG5_STATE, 17,
                    ["experience_size=100", "latent_distribution=Categorical", "discrete_latent_dimensions=32",
                     "discrete_latent_classes=32", "state_size=1024"], "BD_ACT_FUSED_CAT", "act_fused_cat", "act_step_cat"),
}


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def measure(name, B):
    d, A, overrides, switch, fused_attr, span = AGENTS[name]

    class Env:
        action_size, observation_size = A, d.O

        def __init__(self):
            if B > 1:
                self.n, self.envs = B, [None] * B

        def step(self, a):
            return obs0.clone(), 0.0, False

    os.environ[switch] = "1"
    torch.manual_seed(0)
    obs0 = torch.zeros(B, d.O)
    agent = Dreamer(load_config(overrides), Env())
    assert getattr(agent, fused_attr), "this configuration does not take the fused route"
    env = Env()
    belief, state = torch.zeros(B, d.Be).cuda(), torch.zeros(B, d.S).cuda()
    action, obs = torch.zeros(B, A).cuda(), obs0.clone()

    def block(n, mode):
        nonlocal belief, state, action, obs
        t0 = time.perf_counter()
        for _ in range(n):
            belief, state, action, obs, _, _ = agent.update_belief_and_act(env, belief, state, action, obs, explore=False,
                                                                           action_mode=mode)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    times = {m: [] for m in MODES}
    for _ in range(REPEATS):
        for m in MODES:
            block(WARMUP, m)
            times[m].append(block(CALLS, m))
    res = {m: stats(times[m]) for m in MODES}
    for m in MODES:          # the kernel alone: HIP events around the one launch of every call
        agent.engine.enable_timers(True)
        block(CALLS, m)
        ms, _ = agent.engine.timer_summary()[span]
        agent.engine.enable_timers(False)
        res[m]["kernel_us"] = ms * 1e3
    res["mode_minus_mean_kernel_us"] = res["mode"]["kernel_us"] - res["mean"]["kernel_us"]
    res["mean_minus_sample_kernel_us"] = res["mean"]["kernel_us"] - res["sample"]["kernel_us"]
    del agent
    return res


out = {"what": "Dreamer.update_belief_and_act(explore=False, action_mode=...) on the fused route, host wall time per call incl. "
               "the action's D2H copy; us per call: median and [min, max] over the repeats of a 300-call block; kernel_us: HIP "
               "events around the launch",
       "warmup": WARMUP, "calls": CALLS, "repeats": REPEATS}
for name, (d, A, *_rest) in AGENTS.items():
    out[name] = {"model": f"belief={d.Be} state={d.S} hidden={d.Hd} embedding={d.E} action={A} obs={d.O} n_entropy={d.n_entropy}"}
    for B in (1, 10):
        out[name][f"B={B}"] = measure(name, B)
print(json.dumps(out))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_act_mode_latency.json"), "w") as fh:
    json.dump(out, fh, indent=1)
