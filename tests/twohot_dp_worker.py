"""Worker of tests/test_twohot_two_ranks_gpu.py: one rank of a 2-process data-parallel run of the HIP engine on ONE GPU
(gloo transport) with ActorCritic.critic_head=twohot.  Two train steps on this rank's batch shard: no new collective --
the critic's flat buffers are just longer -- and the all-reduced gradients keep the weights identical (check_replicas,
and the ranks' fingerprints compared word by word)."""
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
    K = 31
    d = synth.Dims(B=8, L=7, H=5, Be=40, S=10, Hd=36, E=72, A=2, O=4, critic_head="twohot", critic_bins=K, critic_bin_range=10.0)
    hp = dict(entropy_weight=0.1, gradient_mixing=0.5)
    P = synth.make_params(d, 6)
    cu = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}
    dp = DataParallel(world, rank)
    eng = DreamerEngine(d, hp, "cuda:0", params=P, world_size=world)
    assert eng.W("critic", "model.8.weight").shape == (K, d.Hd)
    start = eng.W("critic", "model.8.weight").clone()
    for step in range(2):
        batch = cu(synth.make_batch(d, 6 + step))
        noise = cu(synth.make_noise(d, 6 + step))
        lb = dp.shard_batch(batch)
        ln = {"obs_prior": dp.shard_batch({"x": noise["obs_prior"]})["x"],
              "obs_post": dp.shard_batch({"x": noise["obs_post"]})["x"],
              "action": dp.shard_rows(noise["action"], d.T, d.B), "entropy": dp.shard_rows(noise["entropy"], d.T, d.B),
              "img_prior": dp.shard_rows(noise["img_prior"], d.T, d.B)}
        logs = eng.train_step(lb, ln)
        if step == 0:
            eng.update_critic()
    torch.cuda.synchronize()
    assert all(v == v for v in logs.values()), logs
    assert not torch.equal(start, eng.W("critic", "model.8.weight"))          # the K-wide layer trained
    verdict = eng.check_replicas()
    assert verdict["agree"] and not verdict["nonfinite"], verdict
    words, _ = eng.fingerprint()
    both = [None, None]
    dist.all_gather_object(both, words.cpu().tolist())
    assert both[0] == both[1], "the ranks' weights differ"
    losses = [None, None]
    dist.all_gather_object(losses, logs["value_loss"])
    assert losses[0] != losses[1], losses                                      # each rank logs its own shard's loss
    if rank == 0:
        print(f"TWOHOT_DP_OK world={world} K={K} value_loss=({losses[0]:.4f}, {losses[1]:.4f})")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
