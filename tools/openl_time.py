"""Wall time of one open-loop prediction (Dreamer.open_loop: 6 replay sequences of seq_len = 50, context 5 -- the replay
sample, the encoder on the context, the two transition-model scans, one decoder pass over 49 x 6 rows, the error curve and, for
pixels, the video with its D2H copy) on the GPU box, config sizes of BASELINE.json: configs[1] on state observations,
configs[2] (64x64 pixels, A = 17) with the video off and on.  Per case one warm-up call, then REPEATS timed ones; the figures
are the median and the range over the repeats, host wall clock around open_loop() between device synchronisations.  Writes
<out_dir>/<tag>_openl_time.json (default out_dir: profiles/).

    python tools/openl_time.py [tag] [out_dir]"""
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

tag = sys.argv[1] if len(sys.argv) > 1 else "openl"
out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
REPEATS = 3
FILL = ["experience_size=2000", "seed_steps=1000"]            # one random episode of 500 records to sample from
CASES = {
    "configs[1] state": (FILL, None),
    "configs[2] pixel, video off": (FILL + ["pixel_observation=true", "synthetic_env_action_size=17"], False),
    "configs[2] pixel, video on": (FILL + ["pixel_observation=true", "synthetic_env_action_size=17"], True),
}
out = {"what": "Dreamer.open_loop(), host wall time of one call: 6 sequences of seq_len 50, context 5; milliseconds, median and "
               "[min, max] over the repeats", "repeats": REPEATS}
for name, (overrides, video) in CASES.items():
    params = load_config(overrides)
    torch.manual_seed(0)
    agent = Dreamer(params, Env(params))
    agent.randomly_initialize_replay_buffer()
    call = lambda: agent.open_loop(sequences=params["openl_sequences"], context=params["openl_context"], video=video)
    res = call()                                          # warm-up
    times = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    out[name] = {"sequences": int(res["beliefs"].shape[1]), "steps": int(res["openl_obs_mse"].shape[0]), "context": res["context"],
                 "ms_median": statistics.median(times), "ms_min": min(times), "ms_max": max(times),
                 "openl_mse_context": res["openl_mse_context"], "openl_mse_open": res["openl_mse_open"],
                 "video_shape": None if res["video"] is None else list(res["video"].shape)}
    print(name, json.dumps(out[name]), flush=True)
    del agent
os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, f"{tag}_openl_time.json"), "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out))
