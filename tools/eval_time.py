"""Wall time of one default evaluation (Dreamer.evaluate: test_episodes = 10 synthetic environments, max_episode_length //
action_repeat = 500 decisions, the reference's test loop src/main.py:191-283) on the GPU box, config sizes of BASELINE.json:
configs[1] on state observations, configs[2] (64x64 pixels, A = 17) with the video off and on.  Per case one warm-up
evaluation, then REPEATS timed ones; the figures are the median and the range over the repeats, host wall clock around
evaluate() (which ends with the video's D2H copy, so nothing is left in flight).  The wall time includes the synthetic
environments' own stepping on the host.  Writes <out_dir>/<tag>_eval_time.json (default out_dir: profiles/).

    python tools/eval_time.py [tag] [out_dir]"""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402
from big_dreamer_amd.env import Env  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "eval"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
REPEATS = 3
CASES = {
    "configs[1] state": (["experience_size=100"], False),
    "configs[2] pixel, video off": (["experience_size=100", "pixel_observation=true", "synthetic_env_action_size=17"], False),
    "configs[2] pixel, video on": (["experience_size=100", "pixel_observation=true", "synthetic_env_action_size=17"], True),
}
out = {"what": "Dreamer.evaluate(), host wall time of one evaluation: 10 episodes side by side, 500 decisions; seconds and us "
               "per decision, median and [min, max] over the repeats", "repeats": REPEATS}
for name, (overrides, video) in CASES.items():
    params = load_config(overrides)
    torch.manual_seed(0)
    agent = Dreamer(params, Env(params))
    res = agent.evaluate(video=video)                     # warm-up
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = agent.evaluate(video=video)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    out[name] = {"episodes": int(res["returns"].shape[0]), "decisions": res["steps"], "act_fused": bool(agent.act_fused),
                 "seconds_median": statistics.median(times), "seconds_min": min(times), "seconds_max": max(times),
                 "us_per_decision_median": statistics.median(times) / res["steps"] * 1e6,
                 "video_shape": None if res["video"] is None else list(res["video"].shape)}
    print(name, json.dumps(out[name]), flush=True)
    del agent
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_eval_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
