"""Worker of tests/test_retnorm_two_ranks_gpu.py: one rank of a 2-process data-parallel run of the HIP engine on ONE GPU
(gloo transport) with ActorCritic.return_normalization=percentile.  Three train steps on this rank's batch shard: each
rank normalises by its own shard's range (no new collective), the all-reduced gradients keep the weights identical
(check_replicas), the ranks' ranges differ, and sync_replicas(0) makes them rank 0's."""
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.engine import DreamerEngine  # noqa: E402
from big_dreamer_amd.parallel import DataParallel  # noqa: E402


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    d = synth.Dims(B=8, L=7, H=5, Be=40, S=10, Hd=36, E=72, A=2, O=4)
    hp = dict(return_normalization="percentile", return_norm_decay=0.5, return_norm_floor=0.01, entropy_weight=0.1)
    P = synth.make_params(d, 6)
    cu = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}
    dp = DataParallel(world, rank)
    eng = DreamerEngine(d, hp, "cuda:0", params=P, world_size=world)
    for step in range(3):
        batch = cu(synth.make_batch(d, 6 + step))
        noise = cu(synth.make_noise(d, 6 + step))
        lb = dp.shard_batch(batch)
        ln = {"obs_prior": dp.shard_batch({"x": noise["obs_prior"]})["x"],
              "obs_post": dp.shard_batch({"x": noise["obs_post"]})["x"],
              "action": dp.shard_rows(noise["action"], d.T, d.B), "entropy": dp.shard_rows(noise["entropy"], d.T, d.B),
              "img_prior": dp.shard_rows(noise["img_prior"], d.T, d.B)}
        logs = eng.train_step(lb, ln)
    torch.cuda.synchronize()
    assert logs["return_scale"] > 0.01, logs            # a range, not the floor
    verdict = eng.check_replicas()
    assert verdict["agree"] and not verdict["nonfinite"], verdict
    mine = eng.return_norm_state()
    assert mine["count"] == 3.0 and mine["skipped"] == 0.0, mine
    both = [None, None]
    dist.all_gather_object(both, mine)
    assert both[0] != both[1] and both[0]["lo"] != both[1]["lo"], both      # each rank's own shard
    eng.sync_replicas(0)
    after = eng.return_norm_state()
    assert after == both[0], (after, both)
    logs = eng.train_step(lb, ln)                       # and the next step divides by rank 0's range on both
    torch.cuda.synchronize()
    scales = [None, None]
    dist.all_gather_object(scales, logs["return_scale"])
    assert scales[0] == scales[1], scales
    assert eng.check_replicas()["agree"]
    if rank == 0:
        print(f"RETNORM_DP_OK world={world} lo=({both[0]['lo']:.4f}, {both[1]['lo']:.4f}) scale={scales[0]:.4f}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
