"""CPU: the host side of checkpoint and resume ("Checkpoint and resume") -- ExperienceReplay.save / load on a
CPU-device buffer (append, append_batch and the index draws need no GPU), and big_dreamer_amd/checkpoint.py: atomic write,
file names, prune, capture / restore of the torch CPU, numpy and Python generators.  Every comparison is exact."""
import os
import random

import numpy as np
import pytest
import torch

from big_dreamer_amd import checkpoint as ck
from big_dreamer_amd.config import load_config
from big_dreamer_amd.memory import ExperienceReplay

A, O = 2, 5
ARRAYS = ("observations", "actions", "rewards", "nonterminals")


def _buffer(size, lanes, pixel, bit_depth=5):
    return ExperienceReplay(size, A, bit_depth, pixel, O, "cpu", lanes=lanes)


def _transitions(rng, lanes, pixel, count):
    """`count` transitions (one per lane each) from `rng`: observations in [-0.5, 0.5] for pixels, N(0, 1) otherwise."""
    out = []
    for _ in range(count):
        shape = (lanes, 3, 64, 64) if pixel else (lanes, O)
        obs = (rng.random(shape, dtype=np.float32) - 0.5) if pixel else rng.standard_normal(shape, dtype=np.float32)
        out.append((obs, rng.uniform(-1, 1, (lanes, A)).astype(np.float32), rng.standard_normal(lanes).astype(np.float32),
                    rng.random(lanes) < 0.2))
    return out


def _append(buf, transitions):
    for obs, act, rew, done in transitions:
        if buf.lanes == 1:
            buf.append(torch.from_numpy(obs[0]), torch.from_numpy(act[0]), float(rew[0]), bool(done[0]))
        else:
            buf.append_batch(obs, act, rew, done)


def _filled_rows(buf):
    """Indices of the rows that hold data, from the definition (not from the code under test)."""
    if buf.lanes == 1:
        return np.arange(buf.size if buf.full else buf.idx)
    k = buf.lane_size if buf.full else buf.idx
    return np.concatenate([e * buf.lane_size + np.arange(k) for e in range(buf.lanes)])


def _assert_same(a, b):
    assert (a.idx, a.full, a.steps, a.episodes) == (b.idx, b.full, b.steps, b.episodes)
    assert (a._pix_step, a._pix_seed) == (b._pix_step, b._pix_seed)
    rows = _filled_rows(a)
    for k in ARRAYS:
        x, y = getattr(a, k)[rows], getattr(b, k)[rows]
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


# (lanes, appended transitions per lane): sizes below make the second of each pair wrap with idx > 0
CASES = {"single_partial": (1, 10), "single_wrapped": (1, 30), "lanes_partial": (4, 5), "lanes_wrapped": (4, 8)}


@pytest.mark.parametrize("pixel", [False, True], ids=["state", "pixel"])
@pytest.mark.parametrize("case", list(CASES))
def test_replay_round_trip(case, pixel, tmp_path):
    lanes, count = CASES[case]
    size = 24 if lanes == 1 else 26                     # 4 lanes of 6 rows; rows 24, 25 belong to no lane
    rng = np.random.Generator(np.random.PCG64(11))
    a = _buffer(size, lanes, pixel)
    _append(a, _transitions(rng, lanes, pixel, count))
    wrapped = case.endswith("wrapped")
    assert a.full == wrapped and a.idx > 0 and a.steps == count * lanes
    if pixel:                                           # as after seven pixel samples under a 64-bit key
        a._pix_step, a._pix_seed = 7, 0xFEDCBA9876543210
    assert a.observations.dtype == (np.uint8 if pixel else np.float32)
    path = str(tmp_path / "experience_1.npz")
    a.save(path)
    with np.load(path, allow_pickle=False) as z:        # plain arrays only, filled rows only, pixels as uint8
        k = (a.lane_size if lanes > 1 else size) if wrapped else a.idx
        assert z["observations"].dtype == a.observations.dtype
        assert z["observations"].shape[:2 if lanes > 1 else 1] == ((lanes, k) if lanes > 1 else (k,))
        assert all(z[n].dtype != object for n in z.files)
    b = _buffer(size, lanes, pixel)
    for k in ARRAYS:                                    # whatever the fresh buffer holds must be overwritten
        getattr(b, k)[...] = 3
    b._dirty = False
    b.load(path)
    assert b._dirty                                     # the next sample uploads the mirror again
    _assert_same(a, b)
    draws = []
    for buf in (a, b):
        np.random.seed(4)
        draws.append([buf._sample_idx(3) for _ in range(20)])
    assert all(np.array_equal(x, y) for x, y in zip(*draws))
    more = _transitions(rng, lanes, pixel, 16)          # crosses the end of the ring in every case
    _append(a, more)
    _append(b, more)
    assert a.full
    _assert_same(a, b)


def test_pixel_seed_not_drawn_yet_round_trips(tmp_path):
    a = _buffer(24, 1, True)
    _append(a, _transitions(np.random.Generator(np.random.PCG64(1)), 1, True, 4))
    path = str(tmp_path / "e.npz")
    a.save(path)
    b = _buffer(24, 1, True)
    b._pix_seed, b._pix_step = 5, 9
    b.load(path)
    assert b._pix_seed is None and b._pix_step == 0     # keyed by the first pixel sample, as on the original


def test_file_grows_with_the_rows_collected(tmp_path):
    sizes = []
    for count in (10, 500):
        buf = _buffer(1000, 1, False)
        _append(buf, _transitions(np.random.Generator(np.random.PCG64(2)), 1, False, count))
        path = str(tmp_path / f"e{count}.npz")
        buf.save(path)
        sizes.append(os.path.getsize(path))
    row = 4 * (O + A + 2)
    assert sizes[0] < sizes[1] and sizes[1] - sizes[0] == 490 * row      # uncompressed: exactly the rows
    assert sizes[0] < 1000 * row                                          # not the whole allocation


@pytest.mark.parametrize("other", [dict(size=25), dict(lanes=2), dict(bit_depth=4), dict(pixel=True)],
                         ids=["size", "lanes", "bit_depth", "observation_kind"])
def test_load_into_another_shape_raises(other, tmp_path):
    a = _buffer(24, 1, False)
    _append(a, _transitions(np.random.Generator(np.random.PCG64(3)), 1, False, 6))
    path = str(tmp_path / "e.npz")
    a.save(path)
    kw = dict(size=24, lanes=1, pixel=False, bit_depth=5)
    kw.update(other)
    b = _buffer(**kw)
    key = {"size": "size", "lanes": "lanes", "bit_depth": "bit_depth", "pixel": "pixel_observation"}[next(iter(other))]
    with pytest.raises(ValueError, match=key):
        b.load(path)
    assert b.steps == 0 and b.idx == 0


def test_atomic_write_keeps_the_earlier_file(tmp_path, monkeypatch):
    a = _buffer(24, 1, False)
    _append(a, _transitions(np.random.Generator(np.random.PCG64(5)), 1, False, 6))
    path, fresh = str(tmp_path / "experience_5.npz"), str(tmp_path / "experience_10.npz")
    a.save(path)
    before = open(path, "rb").read()
    _append(a, _transitions(np.random.Generator(np.random.PCG64(6)), 1, False, 6))
    real = np.savez

    def half_way(fh, **arrays):                         # writes a part of the file, then fails
        real(fh, **{k: arrays[k] for k in list(arrays)[:3]})
        raise OSError("disk full")

    monkeypatch.setattr(np, "savez", half_way)
    for target in (path, fresh):
        with pytest.raises(OSError, match="disk full"):
            a.save(target)
    assert open(path, "rb").read() == before
    assert sorted(os.listdir(tmp_path)) == ["experience_5.npz"]          # no experience_10.npz, no temporary left
    monkeypatch.setattr(np, "savez", real)
    a.save(path)
    b = _buffer(24, 1, False)
    b.load(path)
    _assert_same(a, b)

    def boom(fh):
        fh.write(b"half")
        raise RuntimeError("interrupted")

    with pytest.raises(RuntimeError, match="interrupted"):
        ck.atomic_write(str(tmp_path / "models_5.pth"), boom)
    assert sorted(os.listdir(tmp_path)) == ["experience_5.npz"]


def test_file_names():
    assert ck.models_path("d", 40) == os.path.join("d", "models_40.pth")
    assert ck.experience_path("d", 40) == os.path.join("d", "experience_40.npz")
    assert ck.models_path("d", 40, rank=1, world_size=2) == os.path.join("d", "models_40_rank1.pth")
    assert ck.experience_path("d", 40, rank=0, world_size=2) == os.path.join("d", "experience_40_rank0.npz")
    assert ck.for_rank(os.path.join("d", "models_40_rank0.pth"), 3, 4) == os.path.join("d", "models_40_rank3.pth")
    assert ck.for_rank(os.path.join("d", "models_40_rank0.pth"), 3, 1) == os.path.join("d", "models_40_rank0.pth")
    assert ck.for_rank(os.path.join("d", "models_40.pth"), 1, 2) == os.path.join("d", "models_40.pth")
    assert ck.for_rank("", 1, 2) == ""


def test_prune(tmp_path):
    names = [f"{kind}_{step}{ext}" for step in (5, 10, 100, 20) for kind, ext in (("models", ".pth"), ("experience", ".npz"))]
    names += ["models_30.pth"]                          # a step without a replay file
    foreign = ["models_best.pth", "notes.txt", "models_10.pth.bak", "experience_10.npy", "Eval_rollout_10.npy",
               "models_7.npz", "xmodels_5.pth"]
    for n in names + foreign:
        (tmp_path / n).write_bytes(b"x")
    (tmp_path / "models_200.pth").mkdir()               # not a file: not ours
    assert ck.prune(str(tmp_path), 0) == [] and ck.prune(str(tmp_path), -1) == []
    assert len(os.listdir(tmp_path)) == len(names) + len(foreign) + 1
    removed = ck.prune(str(tmp_path), 2)                # numeric order: 100 and 30 are the newest
    assert sorted(os.path.basename(p) for p in removed) == sorted(
        f"{kind}_{step}{ext}" for step in (5, 10, 20) for kind, ext in (("models", ".pth"), ("experience", ".npz")))
    assert sorted(os.listdir(tmp_path)) == sorted(foreign + ["models_200.pth", "models_30.pth", "models_100.pth",
                                                             "experience_100.npz"])
    assert ck.prune(str(tmp_path), 2) == []


def test_prune_by_rank(tmp_path):
    for step in (5, 10, 15):
        for r in (0, 1):
            (tmp_path / f"models_{step}_rank{r}.pth").write_bytes(b"x")
    (tmp_path / "models_20_rank0.pth").write_bytes(b"x")                  # rank 1 has not written step 20 yet
    ck.prune(str(tmp_path), 2, rank=1)
    assert sorted(os.listdir(tmp_path)) == ["models_10_rank0.pth", "models_10_rank1.pth", "models_15_rank0.pth",
                                            "models_15_rank1.pth", "models_20_rank0.pth", "models_5_rank0.pth"]
    ck.prune(str(tmp_path), 2, rank=0)
    assert "models_5_rank0.pth" not in os.listdir(tmp_path) and "models_10_rank0.pth" not in os.listdir(tmp_path)
    assert "models_10_rank1.pth" in os.listdir(tmp_path)


def _draw():
    return (torch.rand(5).tolist(), torch.randn(3).tolist(), np.random.randint(0, 1 << 30, 6).tolist(),
            np.random.standard_normal(3).tolist(), [random.random() for _ in range(4)], random.gauss(0, 1))


def test_generators_capture_and_restore(tmp_path):
    torch.manual_seed(12)
    np.random.seed(13)
    random.seed(14)
    _draw()
    np.random.standard_normal(1)                        # leaves a cached Gaussian in numpy's legacy generator
    random.gauss(0, 1)                                  # and one in Python's
    state = ck.capture_generators()
    assert "torch_device" not in state
    want = [_draw() for _ in range(3)]
    ck.restore_generators(state)
    assert [_draw() for _ in range(3)] == want
    # the captured object survives the loader that executes nothing from the file
    path = str(tmp_path / "g.pth")
    torch.save({"run_state": {"generators": state, "extra": ck.check_extra({"step": 7, "lr": 0.5, "tag": "a"})}}, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)["run_state"]
    assert loaded["extra"] == {"step": 7, "lr": 0.5, "tag": "a"}
    _draw()
    ck.restore_generators(loaded["generators"])
    assert [_draw() for _ in range(3)] == want


def test_extra_is_flat_and_plain():
    assert ck.check_extra(None) == {}
    for bad in ({"a": [1]}, {"a": {"b": 1}}, {1: 2}, {"a": None}, {"a": torch.zeros(1)}):
        with pytest.raises(ValueError, match="extra"):
            ck.check_extra(bad)


def test_read_run_state_refuses_files_without_one(tmp_path):
    path = str(tmp_path / "old.pth")
    torch.save({"transition_model": {}, "model_optimizer": {}}, path)
    with pytest.raises(ValueError, match="run_state"):
        ck.read_run_state(path)


def test_config_keys_default_to_off():
    p = load_config([])
    assert (p["checkpoint_dir"], p["checkpoint_keep"], p["resume"]) == ("", 0, False)
    p = load_config(["checkpoint_dir=/tmp/x", "checkpoint_keep=3", "resume=true"])
    assert (p["checkpoint_dir"], p["checkpoint_keep"], p["resume"]) == ("/tmp/x", 3, True)
