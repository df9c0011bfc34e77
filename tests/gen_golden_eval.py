"""Golden record of the reference's EnvBatcher (src/env.py:343-394) on the scripted environments of tests/eval_ref.py:
n = 4, observations (1, 3), 6 steps, environments finishing at steps 2, 4, never, 2.  TEST INFRASTRUCTURE; runs where the
reference is installed (see oracle/gen_golden.py, whose import stubs it uses), never on the GPU box.

    python tests/gen_golden_eval.py            # writes tests/golden/env_batcher.npz

Recorded: the reset() output and, per step, observations, rewards and dones as the reference returns them, plus their
dtypes as strings and its sticky `dones` list.  Data only.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests.eval_ref import SCRIPT_N, SCRIPT_STEPS, ScriptedEnv, script_actions, script_params  # noqa: E402


def main() -> None:
    from oracle import gen_golden
    gen_golden._import_reference()          # stub gym / cv2 / torchtyping / typeguard, the reference's src on sys.path
    import env as ref_env
    params = script_params()
    batch = ref_env.EnvBatcher(ScriptedEnv, params, SCRIPT_N)
    out = {"n": np.int64(batch.n), "initial_dones": np.array(batch.dones)}
    first = batch.reset()
    out["reset"], out["reset.dtype"] = first.numpy(), np.array(str(first.dtype))
    obs, rew, don, sticky = [], [], [], []
    for t in range(1, SCRIPT_STEPS + 1):
        o, r, d = batch.step(script_actions(t))
        obs.append(o.numpy().copy()), rew.append(r.numpy().copy()), don.append(d.numpy().copy())
        sticky.append(np.array(batch.dones, dtype=bool))
        dtypes = (str(o.dtype), str(r.dtype), str(d.dtype))
    out.update(observations=np.stack(obs), rewards=np.stack(rew), dones=np.stack(don), sticky=np.stack(sticky))
    out.update({"observations.dtype": np.array(dtypes[0]), "rewards.dtype": np.array(dtypes[1]),
                "dones.dtype": np.array(dtypes[2])})
    # every environment saw every action, finished ones included
    out["actions_seen"] = np.stack([np.stack(e.actions) for e in batch.envs])
    batch.close()
    out["closed"] = np.int64(params["closed"])
    path = os.path.join(ROOT, "tests", "golden", "env_batcher.npz")
    np.savez(path, **out)
    print("wrote", path, {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
