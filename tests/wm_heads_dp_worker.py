"""Worker of tests/test_wm_heads_two_ranks_gpu.py: one rank of a 2-process data-parallel run of the HIP engine on ONE GPU
(gloo transport) with reward_head=twohot and symlog_observations=true (and the two-hot critic, at another K and Z).  Two
train steps on this rank's batch shard, rewards x 300 and observations x 50: no new collective -- the model optimiser's
flat buffers are just longer, and each rank transforms its own shard -- and the all-reduced gradients keep the weights
identical (check_replicas, and the ranks' fingerprints compared word by word).  Rank 0 then runs the same two steps in a
single-process engine on the whole batch and compares gradient norms, clipped gradients and post-Adam weights."""
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
    d = synth.Dims(B=8, L=7, H=5, Be=40, S=10, Hd=36, E=72, A=2, O=4, critic_head="twohot", critic_bins=255,
                   critic_bin_range=20.0, reward_head="twohot", reward_bins=K, reward_bin_range=10.0, symlog_obs=True)
    hp = dict(entropy_weight=0.1, gradient_mixing=0.5)
    P = synth.make_params(d, 6)
    cu = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}
    dp = DataParallel(world, rank)
    eng = DreamerEngine(d, hp, "cuda:0", params=P, world_size=world)
    assert eng.W("reward_model", "model.8.weight").shape == (K, d.Hd) and not eng.heads_fused
    start = eng.W("reward_model", "model.8.weight").clone()
    for step in range(2):
        batch = synth.make_batch(d, 6 + step)
        batch = cu(dict(batch, rewards=batch["rewards"] * 300, observations=batch["observations"] * 50))
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
    assert not torch.equal(start, eng.W("reward_model", "model.8.weight"))    # the K-wide layer trained
    verdict = eng.check_replicas()
    assert verdict["agree"] and not verdict["nonfinite"], verdict
    words, _ = eng.fingerprint()
    both = [None, None]
    dist.all_gather_object(both, words.cpu().tolist())
    assert both[0] == both[1], "the ranks' weights differ"
    losses = [None, None]
    dist.all_gather_object(losses, logs["reward_loss"])
    assert losses[0] != losses[1], losses                                      # each rank logs its own shard's loss
    worst = 0.0
    if rank == 0:
        # the same two steps in a single-process engine on the whole batch: the shards' symlog rows, the 1 / (global rows)
        # of the K-wide reward gradient and the all-reduce must add up to it.  Gradient norms as tests/dp_gpu_worker.py; the
        # clipped gradients and post-Adam weights at the tolerances of test_wm_heads_gpu.test_train_steps_vs_restatement.
        ref = DreamerEngine(d, hp, "cuda:0", params=P, world_size=1)
        for step in range(2):
            batch = synth.make_batch(d, 6 + step)
            batch = cu(dict(batch, rewards=batch["rewards"] * 300, observations=batch["observations"] * 50))
            rlogs = ref.train_step(batch, cu(synth.make_noise(d, 6 + step)))
            if step == 0:
                ref.update_critic()
        torch.cuda.synchronize()
        for k in ("grad_norm_model", "grad_norm_actor", "grad_norm_critic", "kl_loss"):
            assert abs(logs[k] - rlogs[k]) <= 1e-5 + 1e-4 * abs(rlogs[k]), (k, logs[k], rlogs[k])
        for g in ("model", "actor", "critic"):
            for (mod, name, _) in eng.groups[g].specs:
                a, b = eng.G(mod, name).double(), ref.G(mod, name).double()
                scale = float(b.abs().max()) + 1e-12
                assert bool(((a - b).abs() <= 2e-3 * scale + 1e-9 + 2e-3 * b.abs()).all()), ("grad", mod, name)
                a, b = eng.W(mod, name).double(), ref.W(mod, name).double()
                assert bool(((a - b).abs() <= 2e-5 + 1e-5 * b.abs()).all()), ("weight", mod, name)
                worst = max(worst, float((a - b).abs().max()))
        a, b = eng.groups["critic_target"].flat, ref.groups["critic_target"].flat
        assert bool(((a - b).abs() <= 2e-5 + 1e-5 * b.abs()).all()), "critic_target"
        print(f"WM_HEADS_DP_OK world={world} K={K} reward_loss=({losses[0]:.4f}, {losses[1]:.4f}) "
              f"max_weight_diff_to_one_rank={worst:.3e}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
