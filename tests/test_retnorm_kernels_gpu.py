"""GPU: bd_return_range and bd_return_seed (csrc/retnorm.hip) on their own -- the two selected order statistics against
np.sort, the update of the running range against tests/retnorm_ref.py, the scale, the refusal of non-finite returns, and
the seed fill.  The selection runs in one workgroup with its counts in LDS: there is no global workspace to find zeroed."""
import functools

import numpy as np
import pytest
import torch

from tests import retnorm_ref

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4097, 37500, 65537, 600000]
FLT_MAX = np.finfo(np.float32).max


def _bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def _fillings(M):
    """name -> M fp32 values; made once per size and shared (read-only) by the tests."""
    rng = np.random.default_rng(M)
    k = M // 2
    k95 = retnorm_ref.ranks(M)[1]
    normal = rng.standard_normal(M).astype(np.float32)
    out = {"equal": np.full(M, -3.25, np.float32), "normal": normal,
           "ascending": np.linspace(-7.0, 11.0, M, dtype=np.float32) if M > 1 else np.array([2.0], np.float32),
           "descending": np.linspace(9.0, -13.0, M, dtype=np.float32) if M > 1 else np.array([-2.0], np.float32)}
    for tag, b in (("below", k - 1), ("at", k), ("above", k + 1)):     # values below the boundary: b of them
        b = min(max(b, 0), M)
        x = np.where(np.arange(M) < b, np.float32(-0.5), np.float32(0.75)).astype(np.float32)
        out[f"two_values_{tag}"] = rng.permutation(x)
    tied = normal.copy()
    tied[rng.permutation(M)[:M // 2]] = np.sort(normal)[k95]
    out["half_tied_at_percentile"] = tied
    out["low_mantissa_bits"] = _bits(np.float32(1.5).view(np.uint32) | rng.integers(0, 256, M, dtype=np.uint32))
    sign = rng.integers(0, 2, M, dtype=np.uint32) << 31
    out["sign_and_exponent"] = _bits(sign | (rng.integers(1, 255, M, dtype=np.uint32) << 23) | np.uint32(0x2AAAAA))
    den = _bits((rng.integers(0, 2, M, dtype=np.uint32) << 31) | rng.integers(0, 1 << 23, M, dtype=np.uint32))
    den[::7] = 0.0
    den[3::11] = -0.0
    out["denormals_and_zeros"] = den
    out["flt_max"] = rng.choice(np.array([FLT_MAX, -FLT_MAX, 0.0, 1.0, -1.0], np.float32), M).astype(np.float32)
    for v in out.values():
        assert v.dtype == np.float32 and v.shape == (M,) and np.isfinite(v).all()
        v.setflags(write=False)
    return out


def _pairs(M):
    return [(0, M - 1), (M // 2, M // 2), retnorm_ref.ranks(M)]


def _launch(x, k_lo, k_hi, decay, floor, state, rng_out):
    from big_dreamer_amd import _cabi
    _cabi.check(_cabi.lib.bd_return_range(x.data_ptr(), x.numel(), k_lo, k_hi, decay, floor, state.data_ptr(),
                                          rng_out.data_ptr(), _cabi.stream()))


@pytest.mark.parametrize("M", SIZES)
def test_selection_equals_sort(M):
    """From the empty state the update stores p_lo and p_hi as they are: state[0:2] against np.sort(x)[k], equal as floats
    (-0.0 == +0.0), for every filling and index pair; the first scale against its definition."""
    fills, pairs = _fillings(M), _pairs(M)
    n = len(fills) * len(pairs)
    states = torch.zeros(n, 4, dtype=torch.float64, device="cuda")
    ranges = torch.zeros(n, 4, dtype=torch.float32, device="cuda")
    want, i = [], 0
    for name, x in fills.items():
        dx = torch.from_numpy(np.array(x)).cuda()
        srt = np.sort(x)
        for k_lo, k_hi in pairs:
            _launch(dx, k_lo, k_hi, 0.99, 1.0, states[i], ranges[i])
            want.append((name, k_lo, k_hi, srt[k_lo], srt[k_hi]))
            i += 1
        torch.cuda.synchronize()               # dx is freed next
    got, rg = states.cpu().numpy(), ranges.cpu().numpy()
    for (name, k_lo, k_hi, p_lo, p_hi), st, r in zip(want, got, rg):
        tag = f"M={M} {name} k=({k_lo},{k_hi})"
        assert st[0] == np.float64(p_lo) and st[1] == np.float64(p_hi), (tag, st, p_lo, p_hi)
        assert st[2] == 1.0 and st[3] == 0.0, tag
        with np.errstate(over="ignore"):       # FLT_MAX - (-FLT_MAX) rounds to +inf in fp32, in the kernel as here
            assert r[0] == np.float32(max(1.0, float(p_hi) - float(p_lo))), tag
        assert r[1] == p_lo and r[2] == p_hi, tag


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_selection_from_a_buffer_off_the_16_byte_grid(offset):
    M = 1000
    x = _fillings(M + 3)["normal"][offset:offset + M]
    dx = torch.from_numpy(np.array(_fillings(M + 3)["normal"])).cuda()[offset:offset + M]
    assert dx.data_ptr() % 16 == 4 * offset
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    rg = torch.zeros(4, device="cuda")
    k_lo, k_hi = retnorm_ref.ranks(M)
    _launch(dx, k_lo, k_hi, 0.5, 1.0, state, rg)
    srt = np.sort(x)
    assert state.cpu().tolist() == [float(srt[k_lo]), float(srt[k_hi]), 1.0, 0.0]


@pytest.mark.parametrize("M", [257, 37500])
def test_chained_updates_vs_restatement(M):
    """Ten updates from the empty state.  State within 1e-12 relative of the float64 restatement (three roundings per
    update, about 3e-16 each); the scale the kernel leaves equals np.float32(max(floor, hi - lo)) of ITS state, exactly."""
    rng = np.random.default_rng(5)
    k_lo, k_hi = retnorm_ref.ranks(M)
    decay, floor = 0.9, 0.75
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    rg = torch.zeros(4, device="cuda")
    ref = retnorm_ref.empty_state()
    for step in range(10):
        x = (rng.standard_normal(M) * (0.1 + step) + step).astype(np.float32)
        _launch(torch.from_numpy(x).cuda(), k_lo, k_hi, decay, floor, state, rg)
        ref = retnorm_ref.update(ref, x, k_lo, k_hi, decay)
        got, r = state.cpu().numpy(), rg.cpu().numpy()
        for j, key in enumerate(("lo", "hi")):
            assert abs(got[j] - ref[key]) <= 1e-12 * abs(ref[key]), (step, key, got[j], ref[key])
        assert got[2] == ref["count"] == step + 1 and got[3] == 0.0
        mine = dict(lo=got[0], hi=got[1])
        assert r[0] == retnorm_ref.scale(mine, floor) and r[1] == np.float32(got[0]) and r[2] == np.float32(got[1])
    assert r[0] > floor                        # the range, not the floor, by now


def test_floor_holds_the_scale():
    x = torch.linspace(0.0, 0.5, 1000, device="cuda")
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    rg = torch.zeros(4, device="cuda")
    _launch(x, 50, 949, 0.99, 2.5, state, rg)
    assert rg.cpu().tolist()[0] == 2.5


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("M,where", [(1, 0), (1000, 999), (4097, 1234)])
def test_non_finite_returns_are_skipped(bad, M, where):
    rng = np.random.default_rng(M)
    k_lo, k_hi = retnorm_ref.ranks(M)
    state = torch.zeros(4, dtype=torch.float64, device="cuda")
    rg = torch.zeros(4, device="cuda")
    x = rng.standard_normal(M).astype(np.float32)
    _launch(torch.from_numpy(x).cuda(), k_lo, k_hi, 0.5, 1.0, state, rg)
    before, rg_before = state.cpu().numpy().copy(), rg.cpu().numpy().copy()
    y = (2 * x + 1).astype(np.float32)
    y[where] = bad
    _launch(torch.from_numpy(y).cuda(), k_lo, k_hi, 0.5, 1.0, state, rg)
    after = state.cpu().numpy()
    assert np.array_equal(after[:3], before[:3]) and after[3] == before[3] + 1 == 1.0
    assert np.array_equal(rg.cpu().numpy(), rg_before)           # the scale of the unchanged state
    _launch(torch.from_numpy((2 * x + 1).astype(np.float32)).cuda(), k_lo, k_hi, 0.5, 1.0, state, rg)
    assert state.cpu().numpy()[2] == 2.0 and state.cpu().numpy()[3] == 1.0


@pytest.mark.parametrize("M", [4097, 600000])
def test_two_launches_are_bit_identical(M):
    x = torch.from_numpy(np.array(_fillings(M)["half_tied_at_percentile"])).cuda()
    k_lo, k_hi = retnorm_ref.ranks(M)
    outs = []
    for _ in range(2):
        state = torch.tensor([-0.3, 0.9, 4.0, 1.0], dtype=torch.float64, device="cuda")
        rg = torch.zeros(4, device="cuda")
        _launch(x, k_lo, k_hi, 0.99, 1.0, state, rg)
        outs.append((state.cpu().numpy().view(np.uint64).copy(), rg.cpu().numpy().view(np.uint32).copy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][0].view(np.float64)[2] == 5.0


@pytest.mark.parametrize("n", [1, 257, 37500, 300001])          # one thread .. past one grid of 1024 workgroups
@pytest.mark.parametrize("weighted", [False, True])
def test_seed_kernel(n, weighted):
    """dreturns = dconst / S (times the weights), element for element, in fp32 as the kernel forms it: the quotient
    rounded, then the product; and the scale and range copied to the board's three slots."""
    from big_dreamer_amd import _cabi
    rng = np.random.default_rng(n)
    rg_np = np.array([7.3, -1.25, 6.05, 99.0], np.float32)
    dconst = np.float32(-1.0 / 37500)
    w_np = rng.random(n).astype(np.float32)
    rg, w = torch.from_numpy(rg_np).cuda(), torch.from_numpy(w_np).cuda()
    out = torch.full((n + 1,), 5.0, device="cuda")
    board = torch.full((16,), -2.0, device="cuda")
    _cabi.check(_cabi.lib.bd_return_seed(rg.data_ptr(), float(dconst), w.data_ptr() if weighted else None, n, out.data_ptr(),
                                         board.data_ptr(), 12, _cabi.stream()))
    g = dconst / rg_np[0]
    assert g.dtype == np.float32
    want = g * w_np if weighted else np.full(n, g, np.float32)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want) and got[n] == 5.0
    b = board.cpu().numpy()
    assert np.array_equal(b[12:15], rg_np[:3]) and (b[:12] == -2.0).all() and b[15] == -2.0
    # board only
    board2 = torch.zeros(16, device="cuda")
    _cabi.check(_cabi.lib.bd_return_seed(rg.data_ptr(), float(dconst), None, 0, None, board2.data_ptr(), 3, _cabi.stream()))
    assert np.array_equal(board2.cpu().numpy()[3:6], rg_np[:3])
