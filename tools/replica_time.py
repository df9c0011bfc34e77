"""Cost of the replica watch (``replica_check_interval``) on the GPU box.

  (a) milliseconds per step of ``Dreamer.train_step`` in bursts of 5 (five calls, then the last log dict is read, as the
      collect loop does) at configs[1] size (state observations) and configs[2] size (64x64 pixels, A = 17), with
      replica_check_interval 0, 1 and 100 on ONE agent (``engine.set_replica_check``), the three settings alternating block
      by block:
        plain       one rank: the check is the NaN watch (one bd_fingerprint launch and a D2H copy, no collective)
        rehearsal   BD_FORCE_DP=1 on a one-rank RCCL communicator, as tools/dp_rehearsal.py: the agree collective runs too
  (b) milliseconds of one synchronous ``check_replicas()`` and one ``sync_replicas()`` on the same agents (one rank: the
      broadcast itself is not exercised);
  (c) microseconds of one bd_fingerprint launch over the agent's ten flat buffers between two HIP events on an idle device
      (launch overhead included; not a profiler's kernel time), and the bytes it reads.

Every agent is warmed up first; BLOCKS blocks of BLOCK steps per setting; median and [min, max] over the blocks.
``outside_interval0_range`` says whether a setting's median lies outside interval 0's own [min, max] in that cell -- only then
does a difference count.  Not measured here: more than one rank on RCCL, configs[4].
Writes <out_dir>/<tag>_replica_time.json (default out_dir: profiles/).

    python tools/replica_time.py [tag] [out_dir]"""
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

tag = sys.argv[1] if len(sys.argv) > 1 else "replica"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
BLOCKS, BLOCK, BURST, ROWS = 7, 200, 5, 4000
INTERVALS = (0, 1, 100)
SIZES = {"configs[1]": synth.CONFIG2, "configs[2]": synth.CONFIG3}


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


def make_agent(d):
    class _Env:
        action_size, observation_size = d.A, (3 if d.pixel else d.O)

    params = load_config([f"experience_size={ROWS}", f"pixel_observation={'true' if d.pixel else 'false'}"])
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


def timed_ms(fn, n=7):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def fingerprint_launch_us(eng, n=21):
    names = eng.replica._fp_table()[0]
    out = torch.empty(len(names), 2, dtype=torch.int64, device=eng.dev)
    eng.flush_optimizers()
    eng.join()
    ts = []
    for _ in range(n + 3):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.replica._fingerprint_into(out)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    nbytes = 4 * sum(getattr(eng.groups[g], b).numel() for g, b in names)
    res = stats(ts[3:])
    res["bytes_read"] = nbytes
    res["GB_per_s_at_median"] = nbytes / res["median"] * 1e-3
    return res


def measure(agent):
    eng = agent.engine
    for k in INTERVALS:                                  # warm-up of every setting
        eng.resolve_replica_checks()
        eng.set_replica_check(k)
        burst_block(agent)
    times = {k: [] for k in INTERVALS}
    for _ in range(BLOCKS):
        for k in INTERVALS:
            eng.resolve_replica_checks()
            eng.set_replica_check(k)
            times[k].append(burst_block(agent))
    eng.resolve_replica_checks()
    eng.set_replica_check(0)
    res = {f"interval_{k}": stats(v) for k, v in times.items()}
    base = res["interval_0"]
    for k in INTERVALS[1:]:
        c = res[f"interval_{k}"]
        c["outside_interval0_range"] = not base["min"] <= c["median"] <= base["max"]
        c["median_minus_interval0_ms"] = c["median"] - base["median"]
    return {"train_step_burst_ms_per_step": res, "check_replicas_ms": timed_ms(agent.check_replicas),
            "sync_replicas_ms": timed_ms(agent.sync_replicas), "fingerprint_launch_us": fingerprint_launch_us(eng)}


out = {"what": __doc__.split("\n\n")[0] + " See tools/replica_time.py for what each cell is.",
       "blocks": BLOCKS, "steps_per_block": BLOCK, "burst": BURST, "intervals": list(INTERVALS),
       "device": torch.cuda.get_device_name(0),
       "kernel_time_by_profiler": "not measured (no rocprofv3 --kernel-trace --stats run of this tool was made)",
       "not_measured": ["more than one rank on RCCL", "configs[4]"]}
torch.cuda.set_device(0)
torch.cuda.set_stream(torch.cuda.Stream())               # off the legacy null stream, as src/main.py
np.random.seed(0)
for mode in ("plain", "rehearsal"):
    if mode == "rehearsal":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29535")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        os.environ["BD_FORCE_DP"] = "1"
    out[mode] = {}
    for name, d in SIZES.items():
        agent = make_agent(d)
        assert agent.engine.dp.force == (mode == "rehearsal")
        out[mode][name] = measure(agent)
        print(mode, name, json.dumps(out[mode][name]), flush=True)
        del agent
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
if "BD_FORCE_DP" in os.environ:
    del os.environ["BD_FORCE_DP"]
    torch.distributed.destroy_process_group()
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_replica_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
