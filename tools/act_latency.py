"""Latency of one collect-loop decision on the GPU box: Dreamer.update_belief_and_act (reference src/planet.py:370-403:
encoder -> one RSSM cell step -> actor sample -> exploration noise -> action.cpu()) at B=1 (collection) and B=10
(evaluation), config-2 model size, on both routes in ONE process: BD_ACT_FUSED=0 (composed from the encoder chain, a
one-step observe scan and a one-step imagination) and BD_ACT_FUSED=1 (one bd_act_step launch).  Per route and batch size:
20 warm-up calls, then 300 timed calls, repeated REPEATS times with the two routes alternating; the figures are the median
and the range (min, max) of the per-call time over the repeats.  The fused kernel's own time comes from HIP events around
the launch in a separate pass (events cost host time); what is left of the fused wall time is host work and the action's
D2H copy.  Writes <out_dir>/<tag>_act_latency.json (default out_dir: profiles/).

--latent categorical (32 x 32 one-hot latents, state_size 1024) and / or --actor categorical (A = 18 classes; with
--latent categorical alone the tanh-Normal actor has A = 17) measure the DreamerV2 configurations at BASELINE configs[4]
size: the fused route is then bd_act_step_cat behind BD_ACT_FUSED_CAT (default 0) and the file is
<tag>_act_cat_latency.json with one block per observation form: "state" (observation form, O = 3, dense encoder in the
kernel) and "pixel" (embedding form: the conv encoder runs first on both routes).

    python tools/act_latency.py [tag] [out_dir] [--latent gaussian|categorical] [--actor tanh|categorical]"""
import argparse
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

ap = argparse.ArgumentParser()
ap.add_argument("tag", nargs="?", default="r02")
ap.add_argument("out_dir", nargs="?", default=os.path.join(ROOT, "profiles"))
ap.add_argument("--latent", choices=("gaussian", "categorical"), default="gaussian")
ap.add_argument("--actor", choices=("tanh", "categorical"), default="tanh")
opt = ap.parse_args()
tag, out_dir = opt.tag, opt.out_dir
WARMUP, CALLS, REPEATS = 20, 300, 7
CAT = opt.latent == "categorical" or opt.actor == "categorical"
SWITCH, FUSED_ATTR, SPAN = (("BD_ACT_FUSED_CAT", "act_fused_cat", "act_step_cat") if CAT else
                            ("BD_ACT_FUSED", "act_fused", "act_step"))
overrides = ["experience_size=100"]
d = synth.CONFIG2
if opt.latent == "categorical":
    overrides += ["latent_distribution=Categorical", "discrete_latent_dimensions=32", "discrete_latent_classes=32",
                  "state_size=1024"]
    d = synth.CONFIG5_STATE
if opt.actor == "categorical":
    overrides += ["action_distribution=Categorical"]
A = 18 if opt.actor == "categorical" else (17 if CAT else d.A)
out = {"what": "Dreamer.update_belief_and_act, host wall time per call incl. the action's D2H copy (the env.step input); "
               "us per call: median and [min, max] over the repeats of a 300-call block",
       "model": f"belief={d.Be} state={d.S} hidden={d.Hd} embedding={d.E} action={A} obs={d.O}",
       "latent": opt.latent, "actor": opt.actor, "switch": SWITCH,
       "warmup": WARMUP, "calls": CALLS, "repeats": REPEATS}


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs),
            "range_us": max(xs) - min(xs)}


def measure(form, dst, B):
    class Env:
        action_size, observation_size = A, d.O

        def __init__(self):
            if B > 1:
                self.n, self.envs = B, [None] * B

        def step(self, a):
            return obs0.clone(), 0.0, False

    torch.manual_seed(0)
    obs0 = torch.zeros(B, 3, 64, 64) if form == "pixel" else torch.zeros(B, d.O)
    agent = Dreamer(load_config(overrides + (["pixel_observation=true"] if form == "pixel" else [])), Env())
    env = Env()
    belief, state = torch.zeros(B, d.Be).cuda(), torch.zeros(B, d.S).cuda()
    action, obs = torch.zeros(B, A).cuda(), obs0.clone()

    def block(n):
        nonlocal belief, state, action, obs
        t0 = time.perf_counter()
        for _ in range(n):
            belief, state, action, obs, _, _ = agent.update_belief_and_act(env, belief, state, action, obs, explore=True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    times = {"0": [], "1": []}
    for _ in range(REPEATS):
        for fused in ("0", "1"):
            os.environ[SWITCH] = fused
            assert getattr(agent, FUSED_ATTR) == (fused == "1"), "this configuration does not take the fused route"
            block(WARMUP)
            times[fused].append(block(CALLS))
    res = {"composed": stats(times["0"]), "fused": stats(times["1"])}
    # the kernel alone: HIP events around the one launch of every call
    os.environ[SWITCH] = "1"
    agent.engine.enable_timers(True)
    block(CALLS)
    ms, n = agent.engine.timer_summary()[SPAN]
    agent.engine.enable_timers(False)
    res["fused_kernel_us"] = ms * 1e3
    res["fused_host_and_d2h_us"] = res["fused"]["median_us"] - ms * 1e3
    res["gain_us"] = res["composed"]["median_us"] - res["fused"]["median_us"]
    res["fused_faster_by_more_than_the_composed_range"] = bool(res["gain_us"] > res["composed"]["range_us"])
    dst[f"B={B}"] = res
    del agent


if CAT:
    res = {"model": out.pop("model"), "switch": out.pop("switch")}
    for form in ("state", "pixel"):
        res[form] = {}
        for B in (1, 10):
            measure(form, res[form], B)
    res["fused_faster_by_more_than_the_composed_range"] = bool(all(
        res[f][f"B={B}"]["fused_faster_by_more_than_the_composed_range"] for f in ("state", "pixel") for B in (1, 10)))
    path = os.path.join(out_dir, f"{tag}_act_cat_latency.json")
    if os.path.exists(path):        # one file for the runs of a round: a block per (latent, actor)
        with open(path) as fh:
            out = dict(json.load(fh), **out)
    out[f"latent={opt.latent} actor={opt.actor}"] = res
    for k in ("latent", "actor"):
        out.pop(k, None)
else:
    for B in (1, 10):
        measure("state", out, B)
    out["default_BD_ACT_FUSED"] = int(all(out[f"B={B}"]["fused_faster_by_more_than_the_composed_range"] for B in (1, 10)))
    for k in ("latent", "actor", "switch"):
        del out[k]
    path = os.path.join(out_dir, f"{tag}_act_latency.json")
print(json.dumps(out))
os.makedirs(out_dir, exist_ok=True)
with open(path, "w") as fh:
    json.dump(out, fh, indent=1)
