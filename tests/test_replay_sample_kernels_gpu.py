"""GPU: bd_replay_sample_gather (csrc/replay.hip) alone.  The rows it draws against ``ExperienceReplay.device_draw`` (exact), the
batch it writes against bd_replay_gather / bd_replay_gather_pixels_rng on those rows (torch.equal: pure copies, and the same
fp32 arithmetic on the same Philox words), that it writes every destination element and nothing behind them, and that every
refusal leaves the outputs alone.  No tolerance anywhere in this file."""
import functools

import numpy as np
import pytest
import torch

from big_dreamer_amd.memory import ExperienceReplay

pytestmark = pytest.mark.gpu
KEY = 0x0123456789ABCDEF
STEPS = (0, 7, 2 ** 32 - 1)
O, A = 5, 2                                 # an odd observation width
GUARD, SENTINEL = 64, -777.0

# (size, lanes, L, n, idx, full)
GEOMETRIES = [(64, 1, 5, 7, idx, full) for idx, full in ((0, True), (30, True), (63, True), (9, False), (6, False))]
GEOMETRIES += [(5, 1, 5, 3, 2, True)]
GEOMETRIES += [(64, 3, 5, 7, idx, full) for idx, full in ((0, True), (11, True), (20, True), (8, False))]
GEOMETRIES += [(64, 1, 5, n, 30, True) for n in (1, 257, 4096)]


def _host_twin(size, lanes, idx, full, pixels=False):
    """A buffer of the same geometry without a device: ``device_draw`` is the statement of what the kernel draws."""
    b = ExperienceReplay(size, A, 5, pixels, O, "cpu", lanes=lanes, device_sampler=True)
    b.idx, b.full = idx, full
    return b


def _mirror(size, pixels):
    rng = np.random.Generator(np.random.PCG64(size + 11))
    if pixels:
        obs = torch.from_numpy(rng.integers(0, 256, size=(size, 3 * 64 * 64), dtype=np.uint8)).cuda()
    else:
        obs = torch.from_numpy(rng.standard_normal((size, O), dtype=np.float32)).cuda()
    return {"obs": obs, "act": torch.from_numpy(rng.standard_normal((size, A), dtype=np.float32)).cuda(),
            "reward": torch.from_numpy(rng.standard_normal(size, dtype=np.float32)).cuda(),
            "nonterminal": torch.from_numpy((rng.random(size) < 0.8).astype(np.float32)).cuda()}


def _destinations(rows, width):
    """NaN where the kernel writes, a sentinel in the guard behind."""
    out = {}
    for key, w in (("obs", width), ("act", A), ("reward", 1), ("nonterminal", 1)):
        t = torch.full((rows * w + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        t[:rows * w] = float("nan")
        out[key] = t
    out["idx"] = torch.full((rows + GUARD,), -1, dtype=torch.int64, device="cuda")
    return out


def _block(m, d, size, lanes, L, n, idx, full, step, bit_depth=0, pix=(0, 0), over=None):
    from big_dreamer_amd import _cabi as cabi
    a = cabi.ReplaySampleArgs()
    a.obs, a.act, a.reward, a.nonterminal = (m[k].data_ptr() for k in ("obs", "act", "reward", "nonterminal"))
    a.obs_width, a.A, a.size, a.lanes, a.lane_size = m["obs"].shape[1], A, size, lanes, size // lanes
    a.idx, a.full, a.n, a.L, a.bit_depth = idx, int(full), n, L, bit_depth
    a.seed, a.step, a.pix_seed, a.pix_step = KEY, step, pix[0], pix[1]
    a.dst_obs, a.dst_act, a.dst_reward, a.dst_nonterminal = (d[k].data_ptr() for k in ("obs", "act", "reward", "nonterminal"))
    a.idx_out = d["idx"].data_ptr()
    for k, v in (over or {}).items():
        setattr(a, k, v)
    return a


def _gathered(m, rows_drawn, pixels, bit_depth, pix):
    """What the existing gather kernels write from the rows `rows_drawn`."""
    from big_dreamer_amd import _cabi as cabi
    vidx = torch.from_numpy(rows_drawn).cuda()
    k = vidx.numel()
    out = {}
    for key in ("obs", "act", "reward", "nonterminal"):
        src = m[key]
        width = src.numel() // src.shape[0]
        dst = torch.full((k * width,), float("nan"), dtype=torch.float32, device="cuda")
        if key == "obs" and pixels:
            cabi.check(cabi.lib.bd_replay_gather_pixels_rng(src.data_ptr(), vidx.data_ptr(), k, width, bit_depth, pix[0], pix[1],
                                                            dst.data_ptr(), cabi.stream()))
        else:
            cabi.check(cabi.lib.bd_replay_gather(src.data_ptr(), vidx.data_ptr(), k, width, dst.data_ptr(), cabi.stream()))
        out[key] = dst
    return out


@functools.lru_cache(maxsize=None)
def _run(geometry, step, pixels=False):
    """One launch; returns the destinations (with their guards), the host restatement's rows and the reference gather."""
    from big_dreamer_amd import _cabi as cabi
    size, lanes, L, n, idx, full = geometry
    bit_depth, pix = (5, (77, 3)) if pixels else (0, (0, 0))
    m = _mirror(size, pixels)
    d = _destinations(L * n, m["obs"].shape[1])
    a = _block(m, d, size, lanes, L, n, idx, full, step, bit_depth, pix)
    cabi.check(cabi.lib.bd_replay_sample_gather(a, cabi.stream()))
    torch.cuda.synchronize()
    want_rows = _host_twin(size, lanes, idx, full, pixels).device_draw(n, L, step=step, seed=KEY)
    want = _gathered(m, want_rows, pixels, bit_depth, pix)
    torch.cuda.synchronize()
    return d, want_rows, want


CASES = [(g, s) for g in GEOMETRIES for s in STEPS]
IDS = [f"size{g[0]}-lanes{g[1]}-L{g[2]}-n{g[3]}-idx{g[4]}-{'full' if g[5] else 'part'}-step{s}" for g, s in CASES]


@pytest.mark.parametrize("geometry,step", CASES, ids=IDS)
def test_indices_are_the_host_restatement(geometry, step):
    size, lanes, L, n, idx, full = geometry
    d, want_rows, _ = _run(geometry, step)
    got = d["idx"][:L * n].cpu().numpy()
    assert (got == want_rows).all(), (got, want_rows)
    R = size // lanes if lanes > 1 else size
    rows = got.reshape(L, n)
    lane = rows // R
    assert rows.min() >= 0 and rows.max() < lanes * R and (lane == lane[0]).all()
    local = rows - lane * R
    assert (local == (local[0] + np.arange(L)[:, None]) % R).all()
    for b in range(n):                                       # the reference's predicate: idx not in local[1:]
        assert idx not in local[1:, b]
    assert (local < (R if full else idx)).all()


@pytest.mark.parametrize("geometry,step", CASES, ids=IDS)
def test_batch_is_what_the_gather_kernels_write(geometry, step):
    L, n = geometry[2], geometry[3]
    d, _, want = _run(geometry, step)
    for key, w in (("obs", O), ("act", A), ("reward", 1), ("nonterminal", 1)):
        assert torch.equal(d[key][:L * n * w], want[key]), key


@pytest.mark.parametrize("geometry,step", CASES, ids=IDS)
def test_every_element_is_written_and_nothing_behind(geometry, step):
    L, n = geometry[2], geometry[3]
    d, _, _ = _run(geometry, step)
    for key, w in (("obs", O), ("act", A), ("reward", 1), ("nonterminal", 1)):
        assert not torch.isnan(d[key]).any(), key
        assert (d[key][L * n * w:] == SENTINEL).all() and d[key].numel() == L * n * w + GUARD, key
    assert (d["idx"][L * n:] == -1).all() and (d["idx"][:L * n] >= 0).all()


PIXEL = (16, 1, 4, 3, 9, True)          # a 16-row uint8 buffer of 3x64x64 frames, bit_depth 5, n = 3, L = 4


@pytest.mark.parametrize("step", STEPS)
def test_pixel_batch_is_what_gather_pixels_rng_writes(step):
    size, lanes, L, n, idx, full = PIXEL
    d, want_rows, want = _run(PIXEL, step, True)
    assert (d["idx"][:L * n].cpu().numpy() == want_rows).all()
    width = 3 * 64 * 64
    for key, w in (("obs", width), ("act", A), ("reward", 1), ("nonterminal", 1)):
        assert not torch.isnan(d[key]).any(), key
        assert torch.equal(d[key][:L * n * w], want[key]), key
        assert (d[key][L * n * w:] == SENTINEL).all(), key
    frames = d["obs"][:L * n * width]
    assert float(frames.min()) >= -0.5 and float(frames.max()) < 0.5          # dequantised 5-bit frames plus U[0, 1) / 32
    assert (d["idx"][L * n:] == -1).all()


REFUSALS = [({k: None}, "null pointer") for k in ("obs", "act", "reward", "nonterminal", "dst_obs", "dst_act", "dst_reward",
                                                    "dst_nonterminal")]
REFUSALS += [({"n": 0}, "n must be in [1, 4096] (got 0)"), ({"n": 4097}, "n must be in [1, 4096] (got 4097)"),
             ({"L": 0}, "L must be at least 1 (got 0)"), ({"L": 65}, "L = 65 does not fit a ring of 64 rows"),
             ({"lanes": 3, "lane_size": 21, "idx": 3, "L": 22}, "L = 22 does not fit a ring of 21 rows"),
             ({"full": 0, "idx": 5}, "not full and holds idx = 5 rows, a chunk of L = 5"),
             ({"idx": -1}, "idx must be in [0, 64) (got -1)"), ({"idx": 64}, "idx must be in [0, 64) (got 64)"),
             ({"lanes": 3, "lane_size": 21, "idx": 21}, "idx must be in [0, 21) (got 21)"),
             ({"lanes": 3, "lane_size": 22, "idx": 3}, "lanes * lane_size = 3 * 22 exceeds size 64"),
             ({"bit_depth": -1}, "bit_depth must be in [0, 8] (got -1)"), ({"bit_depth": 9}, "bit_depth must be in [0, 8] (got 9)"),
             ({"bit_depth": 5, "obs_width": 10}, "whole 4-byte words (obs_width 10)"),
             ({"bit_depth": 5, "obs_width": 4, "obs": 2}, "pixel obs must be 4-byte aligned"),            # (offsets, see below)
             ({"bit_depth": 5, "obs_width": 4, "dst_obs": 8}, "pixel dst_obs must be 16-byte aligned")]


def test_refusals_launch_nothing():
    from big_dreamer_amd import _cabi as cabi
    size, lanes, L, n, idx, full = GEOMETRIES[1]
    m = _mirror(size, False)
    d = _destinations(L * n, O)
    before = {k: v.clone() for k, v in d.items()}
    for change, text in REFUSALS:
        over = dict(change)
        if over.get("bit_depth") == 5 and "obs" in over:          # a misaligned address inside the real allocation
            over["obs"] = m["obs"].data_ptr() + over["obs"]
        if over.get("bit_depth") == 5 and "dst_obs" in over:
            over["dst_obs"] = d["obs"].data_ptr() + over["dst_obs"]
        a = _block(m, d, size, lanes, L, n, idx, full, 0, over=over)
        assert cabi.lib.bd_replay_sample_gather(a, cabi.stream()) != 0, change
        err = cabi.lib.bd_last_error().decode()
        assert err.startswith("bd_replay_sample_gather:") and text in err, (change, err)
    assert cabi.lib.bd_replay_sample_gather(None, cabi.stream()) != 0
    assert "null argument struct" in cabi.lib.bd_last_error().decode()
    torch.cuda.synchronize()
    for k in d:                                                # the outputs keep their NaN / sentinel
        assert torch.equal(d[k].view(torch.int64 if k == "idx" else torch.int32), before[k].view(
            torch.int64 if k == "idx" else torch.int32)), k
