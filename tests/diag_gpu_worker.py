"""Worker of tests/test_diag_two_ranks_gpu.py: one rank of a 2-process data-parallel run of the HIP engine on ONE GPU (gloo
transport) with diagnostics on every step.  Rank 0 alone reads a step's lazy log dict (no collective may hide in that read:
it must not hang), then both ranks read the next one: grad_norm/* (the reduced gradient) agree bit for bit, the ranks' shard
statistics need not."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.engine import DreamerEngine  # noqa: E402
from big_dreamer_amd.parallel import DataParallel  # noqa: E402

D = synth.Dims(B=4, L=5, H=4, Be=24, S=6, Hd=20, E=40, A=2, O=5)


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dp = DataParallel(world, rank)
    cu = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}

    def shard(i):
        batch, noise = cu(synth.make_batch(D, 6 + i)), cu(synth.make_noise(D, 6 + i))
        ln = {"obs_prior": dp.shard_batch({"x": noise["obs_prior"]})["x"],
              "obs_post": dp.shard_batch({"x": noise["obs_post"]})["x"],
              "action": dp.shard_rows(noise["action"], D.T, D.B), "entropy": dp.shard_rows(noise["entropy"], D.T, D.B),
              "img_prior": dp.shard_rows(noise["img_prior"], D.T, D.B)}
        return dp.shard_batch(batch), ln

    eng = DreamerEngine(D, None, "cuda:0", params=synth.make_params(D, 6), world_size=world, diagnostics_interval=1)
    first = eng.train_step(*shard(0), sync_logs="lazy")
    second = eng.train_step(*shard(1), sync_logs="lazy")
    eng.flush_optimizers()                       # the held-back updates of the second step: a collective, on every rank
    if rank == 0:                                # one rank alone reads: no collective, no hang
        assert "kl_raw" in first and "grad_norm/actor" in first
    got = {k: v for k, v in second.items() if k.startswith(("grad_norm/", "kl_raw"))}
    both = [None] * world
    dist.all_gather_object(both, got)
    norms = [{k: v for k, v in g.items() if k.startswith("grad_norm/")} for g in both]
    assert len(norms[0]) == 6 and norms[0] == norms[1], norms
    assert all(v > 0 for v in norms[0].values())
    assert both[0]["kl_raw"] != both[1]["kl_raw"]                # each rank describes its own shard
    eng.join()
    torch.cuda.synchronize()
    print(f"DIAG_GPU_OK rank={rank}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
