"""Worker of tests/test_replica_gpu.py: one rank of a 2-process data-parallel run of the HIP engine on ONE GPU (gloo
transport).  Four legs in one launch:
  a) after two data-parallel steps check_replicas agrees on both ranks (and the watch changed nothing);
  b) rank 1 moves one critic weight by one ulp: under "raise" both ranks raise ReplicaMismatch naming critic.flat, at the
     same step;
  c) the same under "resync": both ranks then agree, rank 1's buffers equal rank 0's bitwise, and one further step leaves the
     fingerprints of a pair of ranks that was never perturbed (the packed weights were refreshed);
  d) rank 0 alone loads a checkpoint written by Dreamer.save, both call sync_replicas(0): buffers and Adam step counts agree
     and the next step is the step the saved agents take."""
import os
import sys
import warnings

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.engine import DreamerEngine, ReplicaMismatch  # noqa: E402
from big_dreamer_amd.parallel import DataParallel  # noqa: E402

D = synth.Dims(B=4, L=5, H=4, Be=24, S=6, Hd=20, E=40, A=2, O=5)
BUFFERS = [(g, b) for g in ("model", "actor", "critic") for b in ("flat", "m", "v")] + [("critic_target", "flat")]


class Env:
    action_size, observation_size = D.A, D.O


def gathered(x):
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, x)
    return out


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    dp = DataParallel(world, rank)
    P = synth.make_params(D, 6)
    cu = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}

    def shard(i):
        batch, noise = cu(synth.make_batch(D, 6 + i)), cu(synth.make_noise(D, 6 + i))
        ln = {"obs_prior": dp.shard_batch({"x": noise["obs_prior"]})["x"],
              "obs_post": dp.shard_batch({"x": noise["obs_post"]})["x"],
              "action": dp.shard_rows(noise["action"], D.T, D.B), "entropy": dp.shard_rows(noise["entropy"], D.T, D.B),
              "img_prior": dp.shard_rows(noise["img_prior"], D.T, D.B)}
        return dp.shard_batch(batch), ln

    data = [shard(i) for i in range(6)]

    def step(eng, i):
        eng.train_step(*data[i % len(data)], sync_logs=False)

    def words(eng):
        fp, names = eng.fingerprint()
        assert names == BUFFERS
        w = fp.cpu().numpy().view(np.uint64)
        return {f"{g}.{b}": (int(w[i, 0]), int(w[i, 1])) for i, (g, b) in enumerate(names)}

    def same_everywhere(x):
        g = gathered(x)
        return all(y == g[0] for y in g)

    def one_ulp(eng):
        """Rank 1 moves one critic weight by one ulp, in the flat buffer only (as a stray write would)."""
        if rank == 1:
            eng.groups["critic"].flat.view(torch.int32)[5] += 1
        torch.cuda.synchronize()

    def engine(**kw):
        return DreamerEngine(D, None, "cuda:0", params=P, world_size=world, **kw)

    # the pair that is never perturbed, and never watched
    ref = engine()
    for i in range(2):
        step(ref, i)
    ref2 = words(ref)
    for i in range(2, 4):
        step(ref, i)
    ref4 = words(ref)
    assert same_everywhere(ref2) and same_everywhere(ref4) and ref2 != ref4

    # ---- a) ----
    e1 = engine(replica_check_interval=1, replica_on_mismatch="raise")
    for i in range(2):
        step(e1, i)
    v = e1.check_replicas()
    assert v == {"agree": True, "mismatch": [], "nonfinite": {}}, v
    assert same_everywhere(v) and words(e1) == ref2
    print(f"REPLICA_GPU_OK leg=a rank={rank}", flush=True)

    # ---- b) ----
    one_ulp(e1)
    raised = None
    for i in range(2, 8):
        try:
            step(e1, i)
        except ReplicaMismatch as exc:
            raised = (i, str(exc))
            break
    torch.cuda.synchronize()
    assert raised is not None, "no ReplicaMismatch within six steps of the perturbation"
    assert same_everywhere(raised), gathered(raised)
    # the check of train step 3, the first after the perturbation, read where train_step waits host_ahead steps later
    assert raised[0] == 2 + e1.host_ahead and "train step 3:" in raised[1], raised
    assert "differ in critic.flat (" in raised[1], raised
    print(f"REPLICA_GPU_OK leg=b rank={rank} call={raised[0]}", flush=True)

    # ---- c) ----
    e2 = engine(replica_check_interval=1, replica_on_mismatch="resync")
    for i in range(2):
        step(e2, i)
    assert e2.check_replicas()["agree"]                      # (also issues the held-back updates: nothing is pending now)
    one_ulp(e2)
    step(e2, 2)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        e2.resolve_replica_checks()
        e2.resolve_replica_checks()
    texts = [str(w.message) for w in caught if "replica check" in str(w.message)]
    assert len(texts) == 1 and "critic.flat" in texts[0] and "train step 3" in texts[0] and "resync" in texts[0], texts
    v = e2.check_replicas()
    assert v == {"agree": True, "mismatch": [], "nonfinite": {}} and same_everywhere(v), v
    for g, b in BUFFERS:
        mine = getattr(e2.groups[g], b)
        theirs = dp.broadcast_(mine.clone(), 0)
        assert torch.equal(mine.view(torch.int32), theirs.view(torch.int32)), (g, b)
    assert same_everywhere([e2.groups[g].step for g in ("model", "actor", "critic")])
    step(e2, 3)
    got = words(e2)
    assert same_everywhere(got) and got == ref4, [k for k in got if got[k] != ref4[k]]
    print(f"REPLICA_GPU_OK leg=c rank={rank}", flush=True)

    # ---- d) ----
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    ov = [f"belief_size={D.Be}", f"state_size={D.S}", f"hidden_size={D.Hd}", f"embedding_size={D.E}", f"batch_size={D.B}",
          f"seq_len={D.L}", f"planning_horizon={D.H}", "experience_size=100"]
    torch.manual_seed(0)
    a = Dreamer(load_config(ov), Env(), world_size=world)
    for i in range(3):
        step(a.engine, i)
    path = os.path.join(os.environ["REPLICA_TMP"], f"models_rank{rank}.pth")
    a.save(path)
    saved = a.fingerprint()
    saved_steps = [a.engine.groups[g].step for g in ("model", "actor", "critic")]
    assert saved_steps == [3, 3, 3] and same_everywhere(saved)
    torch.manual_seed(100 + rank)                              # a caller that seeds per rank: the replicas start apart
    b = Dreamer(load_config(ov), Env(), world_size=world)
    v = b.check_replicas()
    assert not v["agree"] and "model.flat" in v["mismatch"] and "model.step" not in v["mismatch"] and same_everywhere(v), v
    if rank == 0:
        b.load({"models": path})
    v = b.check_replicas()
    assert set(v["mismatch"]) >= {"model.flat", "model.m", "actor.v", "critic.step", "model.step"}, v
    b.sync_replicas(0)
    v = b.check_replicas()
    assert v == {"agree": True, "mismatch": [], "nonfinite": {}} and same_everywhere(v), v
    assert b.fingerprint() == saved
    assert [b.engine.groups[g].step for g in ("model", "actor", "critic")] == saved_steps
    assert same_everywhere(sorted((g, tuple(sorted(o.items()))) for g, o in b.engine._opt_over.items()))
    step(a.engine, 3)
    step(b.engine, 3)
    fa, fb = a.fingerprint(), b.fingerprint()
    assert fb == fa and same_everywhere(fb) and fa != saved, [k for k in fa if fa[k] != fb[k]]
    print(f"REPLICA_GPU_OK leg=d rank={rank}", flush=True)

    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
