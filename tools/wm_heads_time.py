"""Cost of the world-model heads (``reward_head=twohot``, ``symlog_observations=true``) on the GPU box.

(a) Milliseconds per step of ``Dreamer.train_step`` in bursts of 5 (five calls, then the last log dict is read, as the collect
loop does) with the settings 'normal', 'reward_head=twohot' (K = 255, Z = 20), 'symlog_observations=true' and both -- agents
built alike, alternating block by block in one process -- at configs[1] size (state observations), configs[2] size (64x64
pixels, A = 17; the reward head only: symlog is refused on pixels) and configs[4]'s latents on state observations (32 x 32
Categorical latents, batch 100).  Every agent is warmed up first; BLOCKS blocks of BLOCK steps per setting; median and
[min, max] over the blocks.  'reward_head=twohot' gives up the fused imagined heads and the chunk plan and widens the
reward model's last layer to K, so it costs step time; nothing is asserted.

(b) Microseconds of bd_symlog and bd_symexp alone between two HIP events on an idle device at n = 2500 O elements of the
state configuration (the train step's [N x O] target rows at configs[1]): median and [min, max] of LAUNCHES launches.  At
this size the kernel is a launch, not a bandwidth figure.

(c) Microseconds per decision of the fused acting step (``Dreamer.act_step``, in-kernel noise) at B = 1 and B = 10 without
and with symlog_observations, i.e. without and with the extra bd_symlog launch in front of bd_act_step: host wall time per
call with a synchronise behind each, median and [min, max] over ACT_BLOCKS blocks of ACT_CALLS calls.

Not measured here: more than one rank on RCCL, configs[4] on pixels, K other than 255, the composed acting route.
Writes <out_dir>/<tag>_wm_heads_time.json (default out_dir: profiles/).

    python tools/wm_heads_time.py [tag] [out_dir] [quick]        ("quick": parts (b) and (c) only)"""
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

tag = sys.argv[1] if len(sys.argv) > 1 else "wm_heads"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
quick = "quick" in sys.argv[3:]
BLOCKS, BLOCK, BURST, ROWS, LAUNCHES = 7, 200, 5, 4000, 50
ACT_BLOCKS, ACT_CALLS = 7, 200
SETTINGS = {"normal": [], "reward_head=twohot": ["reward_head=twohot"], "symlog_observations=true": ["symlog_observations=true"],
            "both": ["reward_head=twohot", "symlog_observations=true"]}
CAT = ["batch_size=100", "latent_distribution=Categorical", "discrete_latent_dimensions=32", "discrete_latent_classes=32"]
SIZES = {"configs[1]": (synth.CONFIG2, [], tuple(SETTINGS)),
         "configs[2]": (synth.CONFIG3, [], ("normal", "reward_head=twohot")),
         "configs[4] latents, state observations": (synth.CONFIG5_STATE, CAT, tuple(SETTINGS))}
KERNEL_N = 2500 * synth.CONFIG2.O


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


def make_agent(d, extra, setting):
    class _Env:
        action_size, observation_size = d.A, (3 if d.pixel else d.O)

    params = load_config([f"experience_size={ROWS}", f"pixel_observation={'true' if d.pixel else 'false'}",
                          *SETTINGS[setting], *extra])
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


def measure(d, extra, settings):
    agents = {m: make_agent(d, extra, m) for m in settings}
    for m in settings:                                   # warm-up of all
        burst_block(agents[m])
    times = {m: [] for m in settings}
    for _ in range(BLOCKS):
        for m in settings:
            times[m].append(burst_block(agents[m]))
    res = {m: stats(v) for m, v in times.items()}
    base = res["normal"]
    for m in settings[1:]:
        res[m]["median_minus_normal_ms"] = res[m]["median"] - base["median"]
        res[m]["median_over_normal"] = res[m]["median"] / base["median"]
    last = {m: dict(agents[m].train_step()) for m in settings}
    return {"train_step_burst_ms_per_step": res, "rows": d.T * d.B, "imagined_rows": d.Hm * d.T * d.B,
            "reward_loss_last": {m: last[m]["reward_loss"] for m in settings},
            "behaviour_plan": {m: list(agents[m].engine._bh_plan_used) for m in settings}}


def kernel_times():
    n = KERNEL_N
    lib, check = _cabi.lib, _cabi.check
    x, out = 3.0 * torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    res = {}
    for name in ("bd_symlog", "bd_symexp"):
        fn, us = getattr(lib, name), []
        for i in range(LAUNCHES + 5):
            torch.cuda.synchronize()                     # an idle device
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            check(fn(x.data_ptr(), n, out.data_ptr(), _cabi.stream()))
            b.record()
            b.synchronize()
            if i >= 5:
                us.append(a.elapsed_time(b) * 1e3)
        res[name] = dict(stats(us), bytes_moved=8 * n)
    return {"n": n, "kernels_us": res}


def act_times():
    d = synth.CONFIG2
    agents = {m: make_agent(d, [], m) for m in ("normal", "symlog_observations=true")}
    assert all(a.act_fused for a in agents.values())
    out = {}
    for B in (1, 10):
        ins = (torch.zeros(B, d.Be, device="cuda"), torch.zeros(B, d.S, device="cuda"), torch.zeros(B, d.A, device="cuda"))
        obs = 3.0 * torch.randn(B, d.O, device="cuda")
        times = {m: [] for m in agents}

        def block(agent):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(ACT_CALLS):
                agent.act_step(*ins, obs, explore=True)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / ACT_CALLS * 1e6

        for m, a in agents.items():
            block(a)
        for _ in range(ACT_BLOCKS):
            for m, a in agents.items():
                times[m].append(block(a))
        res = {m: stats(v) for m, v in times.items()}
        res["symlog_observations=true"]["median_minus_normal_us"] = (res["symlog_observations=true"]["median"]
                                                                     - res["normal"]["median"])
        out[f"B={B}"] = res
    return {"act_step_us_per_decision": out}


out = {"what": __doc__.split("\n\n")[0] + " See tools/wm_heads_time.py for what each cell is.",
       "blocks": BLOCKS, "steps_per_block": BLOCK, "burst": BURST, "launches": LAUNCHES,
       "act_blocks": ACT_BLOCKS, "act_calls_per_block": ACT_CALLS, "device": torch.cuda.get_device_name(0),
       "not_measured": ["more than one rank on RCCL", "configs[4] on pixels", "K other than 255", "the composed acting route"]}
torch.cuda.set_device(0)
torch.cuda.set_stream(torch.cuda.Stream())               # off the legacy null stream, as src/main.py
np.random.seed(0)
out["kernels_alone"] = kernel_times()
print("kernels_alone", json.dumps(out["kernels_alone"]), flush=True)
out["acting"] = act_times()
print("acting", json.dumps(out["acting"]), flush=True)
if not quick:
    for name, (d, extra, settings) in SIZES.items():
        out[name] = measure(d, extra, settings)
        print(name, json.dumps(out[name]), flush=True)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_wm_heads_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
