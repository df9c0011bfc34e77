"""Latency of one collect-loop decision on the GPU box: Dreamer.update_belief_and_act (reference src/planet.py:370-403:
encoder -> one RSSM cell step -> actor sample -> exploration noise -> action.cpu()) at B=1 (collection) and B=10
(evaluation), config-2 model size, on both routes in ONE process: BD_ACT_FUSED=0 (composed from the encoder chain, a
one-step observe scan and a one-step imagination) and BD_ACT_FUSED=1 (one bd_act_step launch).  Per route and batch size:
20 warm-up calls, then 300 timed calls, repeated REPEATS times with the two routes alternating; the figures are the median
and the range (min, max) of the per-call time over the repeats.  The fused kernel's own time comes from HIP events around
the launch in a separate pass (events cost host time); what is left of the fused wall time is host work and the action's
D2H copy.  Writes <out_dir>/<tag>_act_latency.json (default out_dir: profiles/).

    python tools/act_latency.py [tag] [out_dir]"""
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

tag = sys.argv[1] if len(sys.argv) > 1 else "r02"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
WARMUP, CALLS, REPEATS = 20, 300, 7
d = synth.CONFIG2
out = {"what": "Dreamer.update_belief_and_act, host wall time per call incl. the action's D2H copy (the env.step input); "
               "us per call: median and [min, max] over the repeats of a 300-call block",
       "model": "belief=200 state=30 hidden=200 embedding=1024 action=1 obs=3",
       "warmup": WARMUP, "calls": CALLS, "repeats": REPEATS}


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs),
            "range_us": max(xs) - min(xs)}


for B in (1, 10):
    class Env:
        action_size, observation_size = d.A, d.O

        def __init__(self):
            if B > 1:
                self.n, self.envs = B, [None] * B

        def step(self, a):
            return torch.zeros(B, d.O), 0.0, False

    torch.manual_seed(0)
    agent = Dreamer(load_config(["experience_size=100"]), Env())
    env = Env()
    belief, state = torch.zeros(B, d.Be).cuda(), torch.zeros(B, d.S).cuda()
    action, obs = torch.zeros(B, d.A).cuda(), torch.zeros(B, d.O)

    def block(n):
        global belief, state, action, obs
        t0 = time.perf_counter()
        for _ in range(n):
            belief, state, action, obs, _, _ = agent.update_belief_and_act(env, belief, state, action, obs, explore=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    times = {"0": [], "1": []}
    for _ in range(REPEATS):
        for fused in ("0", "1"):
            os.environ["BD_ACT_FUSED"] = fused
            assert agent.act_fused == (fused == "1"), "this configuration does not take the fused route"
            block(WARMUP)
            times[fused].append(block(CALLS))
    res = {"composed": stats(times["0"]), "fused": stats(times["1"])}
    # the kernel alone: HIP events around the one launch of every call
    os.environ["BD_ACT_FUSED"] = "1"
    agent.engine.enable_timers(True)
    block(CALLS)
    ms, n = agent.engine.timer_summary()["act_step"]
    agent.engine.enable_timers(False)
    res["fused_kernel_us"] = ms * 1e3
    res["fused_host_and_d2h_us"] = res["fused"]["median_us"] - ms * 1e3
    res["gain_us"] = res["composed"]["median_us"] - res["fused"]["median_us"]
    res["fused_faster_by_more_than_the_composed_range"] = bool(res["gain_us"] > res["composed"]["range_us"])
    out[f"B={B}"] = res
    del agent
out["default_BD_ACT_FUSED"] = int(all(out[f"B={B}"]["fused_faster_by_more_than_the_composed_range"] for B in (1, 10)))
print(json.dumps(out))
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_act_latency.json"), "w") as fh:
    json.dump(out, fh, indent=1)
