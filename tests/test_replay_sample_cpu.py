"""CPU tests of device-side replay sampling ("Device-side sampling"): ``ExperienceReplay.device_draw`` -- the host
restatement of what bd_replay_sample_gather draws -- against the reference's rejection rule by brute force, its uniformity,
its reproducibility, the Python-integer Philox against the published known answers, the config key, save / load, the host
checks and the argument block's layout against the header.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from big_dreamer_amd.memory import ExperienceReplay, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 0x0123456789ABCDEF


def _buffer(size, lanes=1, idx=0, full=False, **kw):
    b = ExperienceReplay(size, 2, 5, False, 3, "cpu", lanes=lanes, **kw)
    b.idx, b.full = idx, full
    return b


def _accepts(start, L, R, h):
    """The reference's predicate (src/memory.py:51-68): the chunk is kept unless the head is among its rows 1 .. L-1."""
    local = np.arange(start, start + L) % R
    return h not in local[1:]


def _reference_starts(R, L, h, full):
    """The starts the reference's loop can return: drawn from [0, R) (full) or [0, h - L) (not full), then filtered."""
    return {s for s in range(R if full else h - L) if _accepts(s, L, R, h)}


def _states(R, L):
    """Every (head, full) a ring of R rows can be sampled in with chunks of L."""
    return [(h, True) for h in range(R)] + [(h, False) for h in range(L + 1, R)]


# ---------------------------------------------------------------------------------------------- the draw rule
@pytest.mark.parametrize("lanes", [1, 3])
def test_sweeping_u_reaches_exactly_the_reference_starts(lanes):
    cases = 0
    for R in range(2, 13):
        size = R if lanes == 1 else lanes * R + 1          # the lane split leaves one row over
        for L in range(2, R + 1):
            for h, full in _states(R, L):
                b = _buffer(size, lanes, h, full, device_sampler=True)
                assert (b.lane_size if lanes > 1 else b.size) == R
                _, n_valid = b._draw_geometry(1, L)
                want = _reference_starts(R, L, h, full)
                assert n_valid == len(want), (R, L, h, full)
                for lane in range(lanes):
                    got = set()
                    for u in range(n_valid):
                        rows = np.asarray(b._chunk_rows(lane, u, L))
                        local = rows - lane * R
                        assert local.min() >= 0 and local.max() < R                       # inside its lane
                        assert (local < (R if full else h)).all()                        # inside the filled rows
                        assert h not in local[1:]                                         # the reference's own predicate
                        assert (local == (local[0] + np.arange(L)) % R).all()             # consecutive, wrapping at R
                        got.add(int(local[0]))
                    assert got == want, (R, L, h, full, lane)
                cases += 1
    assert cases > 500


def test_edges_of_the_rule():
    b = _buffer(7, idx=4, full=True, device_sampler=True)             # R == L, full: only start == head
    rows = b.device_draw(64, 7, step=0, seed=KEY).reshape(7, 64)
    assert (rows[0] == 4).all() and (rows == (4 + np.arange(7)[:, None]) % 7).all()
    b = _buffer(12, idx=6, full=False, device_sampler=True)           # not full, idx == L + 1: only start == 0
    rows = b.device_draw(64, 5, step=0, seed=KEY).reshape(5, 64)
    assert (rows == np.arange(5)[:, None]).all()


@pytest.mark.parametrize("idx,full", [(0, True), (11, True), (20, True), (8, False)])
def test_three_lanes_of_64_rows_never_touch_row_63(idx, full):
    b = _buffer(64, 3, idx, full, device_sampler=True)
    assert b.lane_size == 21
    seen_lanes = set()
    for step in (0, 7, 2 ** 32 - 1):
        rows = b.device_draw(200, 5, step=step, seed=KEY).reshape(5, 200)
        assert rows.min() >= 0 and rows.max() < 63
        lane = rows // 21
        assert (lane == lane[0]).all()
        local = rows - lane * 21
        assert (local == (local[0] + np.arange(5)[:, None]) % 21).all()
        assert not (local[1:] == idx).any()
        assert (local < (21 if full else idx)).all()
        seen_lanes |= set(lane[0].tolist())
    assert seen_lanes == {0, 1, 2}


# ---------------------------------------------------------------------------------------------- uniformity
def _chi_square_p(counts):
    counts = np.asarray(counts, dtype=np.float64)
    expected = counts.sum() / counts.size
    stat = float(((counts - expected) ** 2 / expected).sum())
    return float(torch.special.gammaincc(torch.tensor((counts.size - 1) / 2.0, dtype=torch.float64),
                                         torch.tensor(stat / 2.0, dtype=torch.float64)))


def _draw_20000(b, L):
    """20 000 sequences under the fixed key: five calls of 4000 (a call draws at most 4096)."""
    return np.concatenate([b.device_draw(4000, L, step=s, seed=KEY).reshape(L, 4000)[0] for s in range(5)])


@pytest.mark.parametrize("n_valid", [2, 3, 7, 16, 46])
def test_starts_are_uniform(n_valid):
    L, h = 5, 3
    R = n_valid + L - 1
    first = _draw_20000(_buffer(R, idx=h, full=True, device_sampler=True), L)
    counts = np.bincount((first - h) % R, minlength=n_valid)
    assert counts.size == n_valid and counts.sum() == 20000
    p = _chi_square_p(counts)
    print(f"n_valid={n_valid}: chi-square p = {p:.4f}")
    assert p > 1e-3, (n_valid, counts, p)


@pytest.mark.parametrize("lanes", [3, 16])
def test_lanes_are_uniform(lanes):
    b = _buffer(64, lanes, idx=1, full=True, device_sampler=True)
    counts = np.bincount(_draw_20000(b, 2) // b.lane_size, minlength=lanes)
    assert counts.size == lanes
    p = _chi_square_p(counts)
    print(f"lanes={lanes}: chi-square p = {p:.4f}")
    assert p > 1e-3, (lanes, counts, p)


# ---------------------------------------------------------------------------------------------- reproducibility
def test_python_philox_matches_the_published_known_answers():
    # Random123 kat_vectors: philox4x32, 10 rounds
    assert philox4x32_10([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_same_seed_and_step_same_vector_other_step_other_vector():
    b = _buffer(64, idx=30, full=True, device_sampler=True)
    v = {s: b.device_draw(50, 5, step=s, seed=KEY) for s in (3, 4, 2 ** 32 - 1)}
    for s, x in v.items():
        assert x.dtype == np.int64 and x.shape == (250,)
        assert (x == b.device_draw(50, 5, step=s, seed=KEY)).all()
    assert not (v[3] == v[4]).all() and not (v[3] == v[2 ** 32 - 1]).all() and not (v[4] == v[2 ** 32 - 1]).all()
    assert (b.device_draw(50, 5, step=3 + 2 ** 32, seed=KEY) == v[3]).all()          # the low 32 bits of the counter
    assert not (b.device_draw(50, 5, step=3, seed=KEY + 1) == v[3]).all()
    # step=None: the buffer's counter, which device_draw does not advance; seed=None: the buffer's key
    b._smp_seed, b._smp_step = KEY, 4
    assert (b.device_draw(50, 5) == v[4]).all() and b._smp_step == 4
    torch.manual_seed(77)
    b._smp_seed = None
    assert (b.device_draw(50, 5, step=3) == b.device_draw(50, 5, step=3, seed=77)).all() and b._smp_seed is None


# ---------------------------------------------------------------------------------------------- config
def test_sample_on_device_config_key():
    from big_dreamer_amd.config import load_config
    assert load_config()["sample_on_device"] is False
    assert load_config(["sample_on_device=true"])["sample_on_device"] is True
    for bad in ("1", "yes_please", "0.5", "[true]"):
        with pytest.raises(ValueError, match="sample_on_device"):
            load_config([f"sample_on_device={bad}"])


# ---------------------------------------------------------------------------------------------- save / load
def _filled(device_sampler=None, rows=20):
    kw = {} if device_sampler is None else {"device_sampler": device_sampler}       # None: today's constructor call
    b = ExperienceReplay(40, 2, 5, False, 3, "cpu", **kw)
    rng = np.random.Generator(np.random.PCG64(1))
    b.observations[:rows] = rng.standard_normal((rows, 3), dtype=np.float32)
    b.actions[:rows] = rng.standard_normal((rows, 2), dtype=np.float32)
    b.rewards[:rows], b.nonterminals[:rows] = 1.5, 1.0
    b.idx, b.steps = rows, rows
    return b


def test_save_and_load_carry_the_sampler_state(tmp_path):
    a = _filled(True)
    undrawn, drawn = str(tmp_path / "undrawn.npz"), str(tmp_path / "drawn.npz")
    a.save(undrawn)
    a._smp_seed, a._smp_step = 2 ** 64 - 3, 2 ** 33 + 5
    a.save(drawn)
    b = _filled(True, rows=0)
    b.load(drawn)
    assert (b._smp_seed, b._smp_step) == (2 ** 64 - 3, 2 ** 33 + 5)
    assert (b.device_draw(6, 4) == a.device_draw(6, 4)).all()
    b.load(undrawn)
    assert (b._smp_seed, b._smp_step) == (None, 0)
    with np.load(drawn, allow_pickle=False) as z:
        assert {"smp_step", "smp_seed", "smp_seed_drawn"} <= set(z.files)


def test_a_buffer_without_the_sampler_writes_todays_keys(tmp_path):
    paths = {}
    for name, flag in (("today", None), ("off", False), ("on", True)):
        paths[name] = str(tmp_path / f"{name}.npz")
        _filled(flag).save(paths[name])
    keys = {}
    for name, path in paths.items():
        with np.load(path, allow_pickle=False) as z:
            keys[name] = set(z.files)
            for k in z.files:
                z[k]                                      # every array loads without pickle
    assert keys["off"] == keys["today"] and not any(k.startswith("smp_") for k in keys["today"])
    assert keys["on"] == keys["today"] | {"smp_step", "smp_seed", "smp_seed_drawn"}
    b = _filled(True, rows=0)                              # a file without the keys starts the sampler at (undrawn, 0)
    b._smp_seed, b._smp_step = 9, 9
    b.load(paths["today"])
    assert (b._smp_seed, b._smp_step) == (None, 0) and b.idx == 20


# ---------------------------------------------------------------------------------------------- host checks
def test_sample_on_a_cpu_buffer_raises_the_host_routes_error():
    with pytest.raises(RuntimeError, match="the HIP path needs a GPU device"):
        _filled(True).sample(2, 4)
    with pytest.raises(RuntimeError, match="the HIP path needs a GPU device"):
        _filled(False).sample(2, 4)


def test_host_checks_raise_value_errors():
    b = _buffer(10, idx=3, full=True, device_sampler=True)
    for call in (b.device_draw, b._draw_geometry):
        with pytest.raises(ValueError, match="does not fit a ring of 10 rows"):
            call(2, 11)
    b = _buffer(10, idx=5, full=False, device_sampler=True)
    with pytest.raises(ValueError, match="holds 5 transitions, a chunk of 5 needs more"):
        b.device_draw(2, 5)
    assert b.device_draw(2, 4).shape == (8,)
    b = _buffer(64, 3, idx=5, full=False, device_sampler=True)        # laned: the message of the host route
    with pytest.raises(ValueError, match="each of the 3 lanes holds 5 transitions, a chunk of 6 needs more"):
        b.device_draw(2, 6)
    with pytest.raises(ValueError, match="does not fit a ring of 21 rows"):
        b.device_draw(2, 22)
    for n in (0, 4097):
        with pytest.raises(ValueError, match="1 to 4096 sequences"):
            b.device_draw(n, 2)
    with pytest.raises(ValueError, match="at least one row"):
        b.device_draw(2, 0)
    with pytest.raises(ValueError, match="_idx_out"):
        _filled(False).sample(2, 4, _idx_out=torch.zeros(8, dtype=torch.int64))


# ---------------------------------------------------------------------------------------------- the argument block
_CTYPES = {"int": C.c_int, "unsigned long long": C.c_ulonglong}


def _header_fields():
    """(name, ctypes type) of every member of bd_replay_sample_args as include/bigdreamer_hip.h declares it, in order."""
    text = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} bd_replay_sample_args;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(.*?)(\*?)\s*(\w+)", decl)
        ctype, star, name = m.group(1).strip(), m.group(2), m.group(3)
        out.append((name, C.c_void_p if star else _CTYPES[ctype]))
    return out


def test_argument_block_matches_the_header():
    from big_dreamer_amd import _cabi as cabi
    fields = _header_fields()
    assert [n for n, _ in fields] == [n for n, _ in cabi.ReplaySampleArgs._fields_]
    twin = type("Twin", (C.Structure,), {"_fields_": fields})        # the C compiler's layout of the header's members
    assert C.sizeof(cabi.ReplaySampleArgs) == C.sizeof(twin) == 144
    for name, typ in fields:
        mine, theirs = getattr(cabi.ReplaySampleArgs, name), getattr(twin, name)
        assert (mine.offset, mine.size) == (theirs.offset, theirs.size), name
    assert cabi.ReplaySampleArgs.seed.offset == 72 and cabi.ReplaySampleArgs.idx_out.offset == 136
    assert "bd_replay_sample_gather" in cabi.EXPORTED


GOOD = dict(obs=4096, act=4096, reward=4096, nonterminal=4096, obs_width=12, A=2, size=64, lanes=1, lane_size=64, idx=30,
            full=1, n=7, L=5, bit_depth=0, seed=KEY, step=0, pix_seed=0, pix_step=0, dst_obs=4096, dst_act=4096,
            dst_reward=4096, dst_nonterminal=4096, idx_out=None)     # (addresses are never dereferenced by a refusal)
REFUSALS = [({k: None}, "null pointer") for k in ("obs", "act", "reward", "nonterminal", "dst_obs", "dst_act", "dst_reward",
                                                    "dst_nonterminal")]
REFUSALS += [({"n": 0}, "n must be in [1, 4096] (got 0)"), ({"n": 4097}, "n must be in [1, 4096] (got 4097)"),
             ({"L": 0}, "L must be at least 1 (got 0)"), ({"L": 65}, "L = 65 does not fit a ring of 64 rows"),
             ({"lanes": 3, "lane_size": 21, "idx": 3, "L": 22}, "L = 22 does not fit a ring of 21 rows"),
             ({"full": 0, "idx": 5}, "not full and holds idx = 5 rows, a chunk of L = 5"),
             ({"full": 0, "idx": 4}, "not full and holds idx = 4 rows"),
             ({"idx": -1}, "idx must be in [0, 64) (got -1)"), ({"idx": 64}, "idx must be in [0, 64) (got 64)"),
             ({"lanes": 3, "lane_size": 21, "idx": 21}, "idx must be in [0, 21) (got 21)"),
             ({"lanes": 3, "lane_size": 22, "idx": 3}, "lanes * lane_size = 3 * 22 exceeds size 64"),
             ({"bit_depth": -1}, "bit_depth must be in [0, 8] (got -1)"), ({"bit_depth": 9}, "bit_depth must be in [0, 8] (got 9)"),
             ({"bit_depth": 5, "obs_width": 10}, "whole 4-byte words (obs_width 10)"),
             ({"bit_depth": 5, "obs": 4096 + 2}, "pixel obs must be 4-byte aligned"),
             ({"bit_depth": 5, "dst_obs": 4096 + 8}, "pixel dst_obs must be 16-byte aligned")]


def test_entry_point_refuses_bad_blocks_without_a_launch():
    from big_dreamer_amd import _cabi as cabi
    for change, text in REFUSALS:
        args = cabi.ReplaySampleArgs(**dict(GOOD, **change))
        assert cabi.lib.bd_replay_sample_gather(args, None) != 0, change
        err = cabi.lib.bd_last_error().decode()
        assert err.startswith("bd_replay_sample_gather:") and text in err, (change, err)
    assert cabi.lib.bd_replay_sample_gather(None, None) != 0
    assert cabi.lib.bd_last_error().decode() == "bd_replay_sample_gather: null argument struct"
