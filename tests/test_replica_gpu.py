"""GPU: the engine's replica fingerprint, the periodic check (one rank: the NaN watch) and, in one two-rank run on one
GPU over gloo, agreement, ReplicaMismatch, resync and sync_replicas after a load on rank 0 only.  Bit-exact throughout."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import replica_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = synth.TINY
NAMES = [(g, b) for g in ("model", "actor", "critic") for b in ("flat", "m", "v")] + [("critic_target", "flat")]


def cu(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


@pytest.fixture(scope="module")
def case():
    return dict(P=synth.make_params(D, 3), batch=[cu(synth.make_batch(D, 3 + i)) for i in range(3)],
                noise=[cu(synth.make_noise(D, 3 + i)) for i in range(3)])


def engine(case, **kw):
    from big_dreamer_amd.engine import DreamerEngine
    return DreamerEngine(D, None, "cuda:0", params=case["P"], **kw)


def steps(eng, case, n):
    for i in range(n):
        eng.train_step(case["batch"][i], case["noise"][i], sync_logs=False)


def words(eng):
    fp, names = eng.fingerprint()
    assert fp.dtype == torch.int64 and tuple(fp.shape) == (len(NAMES), 2) and fp.is_cuda and names == NAMES
    w = fp.cpu().numpy().view(np.uint64)
    return {n: (int(w[i, 0]), int(w[i, 1])) for i, n in enumerate(names)}


def test_fingerprint_is_the_reference_of_every_flat_buffer(case):
    eng = engine(case)
    steps(eng, case, 1)
    got = words(eng)
    torch.cuda.synchronize()
    for g, b in NAMES:
        buf = getattr(eng.groups[g], b)
        assert buf.numel() == eng.groups[g].numel                       # the whole buffer, padding floats included
        assert got[(g, b)] == R.fingerprint(buf.cpu().numpy()), (g, b)
        assert got[(g, b)][1] == 0


def test_equal_engines_have_equal_fingerprints_before_and_after_training(case):
    a, b = engine(case), engine(case)
    fa = words(a)
    assert fa == words(b)
    steps(a, case, 2)
    steps(b, case, 2)
    fa2 = words(a)
    assert fa2 == words(b)
    assert all(fa2[n] != fa[n] for n in NAMES if n != ("critic_target", "flat"))      # training moved every buffer
    # one ulp in one actor weight: exactly actor.flat differs
    b.join()
    b.groups["actor"].flat.view(torch.int32)[11] += 1
    fb = words(b)
    assert [n for n in NAMES if fb[n] != fa2[n]] == [("actor", "flat")]


def test_the_watch_perturbs_nothing(case):
    plain, watched = engine(case), engine(case, replica_check_interval=1)
    assert plain.replica.interval == 0 and plain.replica.on_mismatch == "raise"
    steps(plain, case, 3)
    steps(watched, case, 3)
    assert len(watched.replica._checks_out) <= max(watched.host_ahead, 1) and not plain.replica._checks_out
    watched.resolve_replica_checks()
    assert not watched.replica._checks_out
    assert words(plain) == words(watched)
    every_other = engine(case, replica_check_interval=2)
    steps(every_other, case, 3)
    assert [r.step for r in every_other.replica._checks_out] == [2]
    assert words(every_other) == words(plain)


def test_nan_in_a_world_model_weight_raises_at_the_next_check(case):
    eng = engine(case, replica_check_interval=1)
    steps(eng, case, 1)
    eng.join()
    eng.groups["model"].flat[7] = float("nan")
    with pytest.raises(FloatingPointError, match=r"model\.flat \(\d+\)") as exc:
        eng.train_step(case["batch"][1], case["noise"][1], sync_logs=False)
        eng.resolve_replica_checks()            # at the latest here; never later
    assert "train step 2" in str(exc.value)
    assert not any(r.step == 2 for r in eng.replica._checks_out)
    torch.cuda.synchronize()


@pytest.mark.parametrize("switch", ["BD_HOST_AHEAD", "BD_PIPELINE"])
def test_without_the_host_throttle_the_next_check_reads_the_verdict(case, monkeypatch, switch):
    """train_step reads a verdict where it waits for the step of BD_HOST_AHEAD steps ago; with the throttle off, or the serial
    schedule, the next check does -- and the watch still perturbs nothing."""
    monkeypatch.setenv(switch, "0")
    plain, eng = engine(case), engine(case, replica_check_interval=1)
    assert (eng.host_ahead == 0) if switch == "BD_HOST_AHEAD" else (not eng.pipeline)
    steps(plain, case, 2)
    steps(eng, case, 2)
    assert [r.step for r in eng.replica._checks_out] == [2]
    assert words(plain) == words(eng)
    eng.groups["model"].flat[7] = float("nan")
    eng.train_step(case["batch"][2], case["noise"][2], sync_logs=False)          # check 3 sees it; check 2 is read, clean
    assert [r.step for r in eng.replica._checks_out] == [3]
    with pytest.raises(FloatingPointError, match=r"train step 3: .*model\.flat"):
        eng.train_step(case["batch"][0], case["noise"][0], sync_logs=False)      # the next check reads verdict 3
    torch.cuda.synchronize()


def test_interval_zero_raises_nothing_and_check_replicas_counts(case):
    eng = engine(case)
    steps(eng, case, 1)
    assert eng.check_replicas() == {"agree": True, "mismatch": [], "nonfinite": {}}
    eng.groups["model"].flat[7] = float("nan")
    eng.groups["critic"].v[2] = float("-inf")
    v = eng.check_replicas()
    assert v == {"agree": True, "mismatch": [], "nonfinite": {"model.flat": 1, "critic.v": 1}}
    eng.train_step(case["batch"][1], case["noise"][1], sync_logs=False)
    eng.resolve_replica_checks()
    assert not eng.replica._checks_out
    v = eng.check_replicas()
    assert v["agree"] and v["nonfinite"]["model.flat"] >= 1
    torch.cuda.synchronize()


def test_bad_options_are_refused(case):
    for kw in (dict(replica_check_interval=-1), dict(replica_check_interval=1.5), dict(replica_on_mismatch="ignore")):
        with pytest.raises(ValueError):
            engine(case, **kw)


def test_agent_fingerprint_and_sync_with_one_rank():
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer

    class Env:
        action_size, observation_size = D.A, D.O

    ov = [f"belief_size={D.Be}", f"state_size={D.S}", f"hidden_size={D.Hd}", f"embedding_size={D.E}", f"batch_size={D.B}",
          f"seq_len={D.L}", f"planning_horizon={D.H}", "experience_size=100", "replica_check_interval=5"]
    torch.manual_seed(0)
    agent = Dreamer(load_config(ov), Env())
    assert agent.engine.replica.interval == 5
    fp = agent.fingerprint()
    assert list(fp) == [f"{g}.{b}" for g, b in NAMES]
    for (g, b) in NAMES:
        h, nf = fp[f"{g}.{b}"]
        assert isinstance(h, int) and isinstance(nf, int) and 0 <= h < 1 << 64 and nf == 0
        assert (h, nf) == R.fingerprint(getattr(agent.engine.groups[g], b).cpu().numpy())
    assert fp["critic.flat"] == fp["critic_target.flat"]                 # the target starts as a copy
    assert fp["model.m"] == fp["model.v"] == R.fingerprint(np.zeros(agent.engine.groups["model"].numel, np.float32))
    assert agent.check_replicas() == {"agree": True, "mismatch": [], "nonfinite": {}}
    agent.sync_replicas(0)                                                # one rank: re-packs, changes nothing
    assert agent.fingerprint() == fp


def test_two_ranks_agree_mismatch_resync_and_sync_after_a_one_sided_load(tmp_path):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29655", os.path.join(ROOT, "tests", "replica_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0", REPLICA_TMP=str(tmp_path))
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2500:] + out.stderr[-3000:]
    for leg in "abcd":
        assert f"REPLICA_GPU_OK leg={leg}" in out.stdout, out.stdout[-2500:]
    print("\n".join(l for l in out.stdout.splitlines() if l.startswith("REPLICA_GPU_OK")))
