"""Worker of tests/test_checkpoint_gpu.py::test_two_ranks_checkpoint_and_resume: one rank of a 2-process data-parallel run
on ONE GPU (gloo transport, as tests/dp_gpu_worker.py).

CK_PHASE=first:  two train steps, then every rank saves models_2_rank<r>.pth and experience_2_rank<r>.npz into CK_DIR (save is
                 collective: it issues the held-back actor / critic updates), one more train step, and the rank's parameter
                 groups go to after_rank<r>.pt.
CK_PHASE=second: a fresh pair builds the agents from the per-rank files (models=, buffer.load, load_run_state), trains that
                 one step and compares its parameter groups with after_rank<r>.pt, exactly."""
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import checkpoint as ck  # noqa: E402
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402

D = synth.SMALL
ROWS = 200


class Env:
    action_size, observation_size = D.A, D.O


def groups(agent):
    torch.cuda.synchronize()
    out = {}
    for g in ("model", "actor", "critic"):
        grp = agent.engine.groups[g]
        out[g] = {"flat": grp.flat.cpu(), "m": grp.m.cpu(), "v": grp.v.cpu(), "step": int(grp.step)}
    out["critic_target"] = {"flat": agent.engine.groups["critic_target"].flat.cpu()}
    return out


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    phase, directory = os.environ["CK_PHASE"], os.environ["CK_DIR"]
    models, replay = ck.models_path(directory, 2, rank, world), ck.experience_path(directory, 2, rank, world)
    ov = [f"belief_size={D.Be}", f"state_size={D.S}", f"hidden_size={D.Hd}", f"embedding_size={D.E}", f"batch_size={D.B}",
          f"seq_len={D.L}", f"planning_horizon={D.H}", "experience_size=300"]
    first = phase == "first"
    torch.manual_seed(5 if first else 99)                # the same initial weights on both ranks, as the CLI seeds them
    np.random.seed((100 if first else 700) + rank)       # rank-local index draws
    random.seed((100 if first else 700) + rank)
    agent = Dreamer(load_config(ov + ([] if first else [f"models={models}"])), Env(), world_size=world)
    eng = agent.engine
    assert eng.defer_opt and eng.pipeline                # one communicator: actor / critic updates are held back a step
    if first:
        rep = synth.make_replay(D, rows=ROWS, seed=20 + rank)          # every rank has collected its own experience
        for k, v in rep.items():
            getattr(agent.buffer, k)[:ROWS] = v
        agent.buffer.idx, agent.buffer.steps = ROWS, ROWS
        agent.buffer.mark_dirty()
        for _ in range(2):
            agent.train_step()
        assert len(eng._pending_opt) == 2                # actor and critic of step 2 are still to be issued
        agent.save(models, extra={"step": 2, "collect_envs": 1})
        assert len(eng._pending_opt) == 0
        agent.buffer.save(replay)
        saved = torch.load(models, map_location="cpu", weights_only=True)
        assert float(saved["actor_optimizer"]["state"][0]["step"]) == 2 and saved["run_state"]["noise"]["step"]["bh"] == 2
        agent.train_step()
        noise = eng.noise_state()                        # collective: issues the held-back updates of the third step
        torch.save({"groups": groups(agent), "noise": noise}, os.path.join(directory, f"after_rank{rank}.pt"))
    else:
        agent.buffer.load(replay)
        assert agent.load_run_state(models) == {"step": 2, "collect_envs": 1}
        agent.train_step()
        noise = eng.noise_state()
        want = torch.load(os.path.join(directory, f"after_rank{rank}.pt"), map_location="cpu", weights_only=True)
        got = groups(agent)
        for g, fields in want["groups"].items():
            for k, v in fields.items():
                same = torch.equal(got[g][k], v) if isinstance(v, torch.Tensor) else got[g][k] == v
                assert same, f"rank {rank}: {g}.{k} differs after the resumed step"
        assert noise == want["noise"]
    dist.barrier()
    print(f"CKPT_DP_OK phase={phase} rank={rank}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
