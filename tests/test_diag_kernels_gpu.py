"""The training-diagnostics kernels (csrc/diag.hip) against their float64 restatements (tests/diag_ref.py), called through
the C ABI at the sizes where they could go wrong: empty and one-element buffers, sizes around a wave, several grid-stride
trips over several workgroups, pointers off every 16-byte phase, p and q on different phases, non-finite values at the
ends, one row / one column / one class, more factors than the grid has workgroups, segments that are empty, shorter than a
vector or spread over several workgroups' chunks.  Inputs lie in NaN-filled buffers, every output in a sentinel-filled one
that must stay untouched outside it, the workspace starts NaN-filled, and every call runs twice and must give the same
bits.  Each case prints its worst err / bound (DIAG_WORST lines, visible under -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import diag_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -31415.926
GUARD = 8


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


@pytest.fixture(scope="module")
def ws(cabi):
    return torch.full((int(cabi.lib.bd_diag_ws_floats()),), float("nan"), device="cuda")


def _report(entry, case, worst):
    print(f"DIAG_WORST {entry} {case} {worst:.3e}")


def _inp(x: np.ndarray, off: int = 1) -> torch.Tensor:
    """x flat in a NaN-filled device buffer, `off` floats past a 16-byte boundary (and NaN behind it)."""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    buf = torch.full((x.size + 16,), float("nan"), device="cuda")
    view = buf[4 + off:4 + off + x.size]
    view.copy_(torch.from_numpy(x))
    view._keep = buf
    return view


class Out:
    """n words of `dtype` between two guards, all prefilled with a sentinel."""

    def __init__(self, n, dtype=torch.float64):
        self.fill = SENTINEL if dtype.is_floating_point else -7
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device="cuda")
        self.n = n
        self.view = self.buf[GUARD:GUARD + n]

    def ptr(self):
        return self.view.data_ptr()

    def reset(self):
        self.buf.fill_(self.fill)

    def guards_ok(self):
        g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]])
        return bool((g == self.fill).all())

    def bits(self):
        return self.view.cpu().numpy().copy()


def _twice(outs, launch):
    """Run `launch` twice into freshly sentinel-filled outputs: same bits, guards intact; returns the outputs' values."""
    runs = []
    for _ in range(2):
        for o in outs:
            o.reset()
        launch()
        torch.cuda.synchronize()
        assert all(o.guards_ok() for o in outs), "wrote outside its output"
        runs.append([o.bits() for o in outs])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes(), "not deterministic"
    return runs[0]


def _check_sextuple(name, got, p, q=None):
    ref, S1, S2 = R.moments_ref(p, q)
    n = max(int(ref[0]), 1)
    assert got[0] == ref[0] and got[5] == ref[5], (name, got, ref)
    assert got[3] == ref[3] and got[4] == ref[4], (name, got, ref)
    worst = 0.0
    for k, S in ((1, S1), (2, S2)):
        err, bound = abs(got[k] - ref[k]), R.sum_bound(n, S)
        assert err <= bound, (name, k, got[k], ref[k], bound)
        worst = max(worst, err / bound if bound > 0 else 0.0)
    return worst


# ---- bd_moments ------------------------------------------------------------------------------------------------------------
BIG = 3 * 256 * 256 * 4 + 5            # three grid-stride trips of the largest grid (256 workgroups x 256 lanes x 4 floats)


def _moments(cabi, ws, entries):
    """entries: [(p view or None, q view or None, n)] -> the sextuples as an (n_buf, 6) array."""
    a = cabi.MomentsArgs()
    a.n_buf = len(entries)
    for i, (p, q, n) in enumerate(entries):
        a.buf[i].p = p.data_ptr() if p is not None else None
        a.buf[i].q = q.data_ptr() if q is not None else None
        a.buf[i].n = n
    out = Out(6 * len(entries))
    got, = _twice([out], lambda: cabi.check(cabi.lib.bd_moments(C.byref(a), out.ptr(), ws.data_ptr(), None)))
    return got.reshape(len(entries), 6)


def _data(n, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4099, BIG])
@pytest.mark.parametrize("with_q", [False, True])
def test_moments_sizes(cabi, ws, n, with_q):
    for off in ((0, 1) if n != BIG else (1,)):
        x, y = _data(n, n + 1), _data(n, n + 2) if with_q else None
        p, q = _inp(x, off), _inp(y, off) if with_q else None
        got = _moments(cabi, ws, [(p, q, n)])
        _report("bd_moments", f"n={n} q={with_q} off={off}", _check_sextuple("moments", got[0], x, y))
    if n == 0:
        got = _moments(cabi, ws, [(None, None, 0)])
        assert list(got[0]) == [0, 0, 0, np.inf, -np.inf, 0]


def test_moments_p_and_q_on_different_phases(cabi, ws):
    for n in (5, 4099):
        x, y = _data(n, 7), _data(n, 8)
        got = _moments(cabi, ws, [(_inp(x, 1), _inp(y, 3), n)])
        _report("bd_moments", f"phases n={n}", _check_sextuple("phases", got[0], x, y))


def test_moments_sixteen_entries(cabi, ws):
    sizes = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 1025, 4099, 70001, 2, 7, 300000]
    xs = [_data(n, 100 + i) for i, n in enumerate(sizes)]
    ys = [_data(n, 200 + i) if i % 3 == 0 else None for i, n in enumerate(sizes)]
    entries = [(_inp(x, i % 4), _inp(y, i % 4) if y is not None else None, x.size) for i, (x, y) in enumerate(zip(xs, ys))]
    got = _moments(cabi, ws, entries)
    worst = max(_check_sextuple(f"entry {i}", got[i], xs[i], ys[i]) for i in range(16))
    _report("bd_moments", "16 entries", worst)


def test_moments_special_values(cabi, ws):
    neg = -np.abs(_data(777, 3)) - 1.0                      # all negative: min and max must not start from 0
    zeros = np.array([-0.0, 0.0, -0.0], dtype=np.float32)
    ends = _data(4099, 4)
    ends[0], ends[-1], ends[17] = np.nan, np.inf, -np.inf
    allnan = np.full(66, np.nan, dtype=np.float32)
    infdiff = np.full(9, np.inf, dtype=np.float32)          # inf - inf = NaN: the DIFFERENCE is what is classified
    xs = [neg, zeros, ends, allnan, infdiff]
    qs = [None, None, None, None, infdiff.copy()]
    got = _moments(cabi, ws, [(_inp(x, 1), _inp(q, 1) if q is not None else None, x.size) for x, q in zip(xs, qs)])
    for i, (x, q) in enumerate(zip(xs, qs)):
        _check_sextuple(f"special {i}", got[i], x, q)
    assert got[0][4] < 0 and got[2][5] == 3 and list(got[3]) == [0, 0, 0, np.inf, -np.inf, 66] and got[4][5] == 9


# ---- bd_latent_stats -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 17, 300])
@pytest.mark.parametrize("S", [1, 30, 33])
def test_latent_stats_gaussian(cabi, ws, rows, S):
    rng = np.random.default_rng(rows * 100 + S)
    qm, pm = (rng.standard_normal((rows, S)).astype(np.float32) * 2 for _ in range(2))
    qs, ps = (np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (rows, S))).astype(np.float32) for _ in range(2))
    qs.flat[0], ps.flat[-1] = 1e-3, 1e2
    ins = [_inp(a, i % 4) for i, a in enumerate((qm, qs, pm, ps))]
    out, col = Out(R.LATENT_WORDS), Out(S)
    got, gcol = _twice([out, col], lambda: cabi.check(cabi.lib.bd_latent_stats(
        *[t.data_ptr() for t in ins], rows, S, out.ptr(), col.ptr(), ws.data_ptr(), None)))
    ref, rcol, mags, mcol = R.latent_stats_ref(qm, qs, pm, ps)
    worst = 0.0
    for k in range(3):
        err = abs(got[k] - ref[k])
        assert err <= R.C_TOL * mags[k], (k, got[k], ref[k], mags[k])
        worst = max(worst, err / (R.C_TOL * mags[k]))
    errc = np.abs(gcol - rcol)
    assert (errc <= R.C_TOL * mcol).all(), (gcol, rcol)
    worst = max(worst, float((errc / (R.C_TOL * mcol)).max()))
    _check_sextuple("qs", got[3:9], qs)
    _check_sextuple("ps", got[9:15], ps)
    _report("bd_latent_stats", f"rows={rows} S={S}", worst)


# ---- bd_latent_stats_categorical -------------------------------------------------------------------------------------------
# C spans what bd_kl_categorical_forward accepts (1 .. 128); D has no upper limit there: 1100 factors are more than the
# grid has workgroup rows, so a workgroup walks several factors
@pytest.mark.parametrize("D,C_", [(1, 1), (1, 128), (3, 5), (32, 32), (1100, 2)])
@pytest.mark.parametrize("rows", [1, 70])
def test_latent_stats_categorical(cabi, ws, D, C_, rows):
    if D == 1100:
        rows = min(rows, 9)
    rng = np.random.default_rng(D * 1000 + C_ + rows)
    ql = (rng.standard_normal((rows, D, C_)) * 3).astype(np.float32)
    pl = (rng.standard_normal((rows, D, C_)) * 3).astype(np.float32)
    if C_ > 1:
        # saturated posteriors: one class at +80, the others at -80 (q = 0 exactly in fp32 for them); the prior stays
        # within +-40 so that no prior probability underflows where the posterior has mass
        sat = rng.random((rows, D)) < 0.25
        hot = rng.integers(0, C_, (rows, D))
        satl = np.where(np.arange(C_) == hot[..., None], 80.0, -80.0).astype(np.float32)
        ql = np.where(sat[..., None], satl, ql)
        pl = np.clip(pl * 8, -40, 40).astype(np.float32)
        # exact ties: the two largest logits of some groups are equal; all-equal groups
        tie = (rng.random((rows, D)) < 0.25) & ~sat
        top = ql.max(-1)
        second = rng.integers(0, C_, (rows, D))
        ql = np.where(tie[..., None] & (np.arange(C_) == second[..., None]), top[..., None], ql)
        ql[0, 0, :] = 0.25
        pl[0, 0, :] = -1.5
    a, b = _inp(ql, 1), _inp(pl, 3)
    out, col, used = Out(R.LATENT_CAT_WORDS), Out(D), Out(D * C_, torch.int32)
    got, gcol, gused = _twice([out, col, used], lambda: cabi.check(cabi.lib.bd_latent_stats_categorical(
        a.data_ptr(), b.data_ptr(), rows, D, C_, out.ptr(), col.ptr(), used.ptr(), ws.data_ptr(), None)))
    ref, rcol, rused, mags, mcol = R.latent_stats_cat_ref(ql, pl)
    assert (gused.reshape(D, C_) == rused).all(), "used flags differ"
    worst = 0.0
    for k in range(5):
        err = abs(got[k] - ref[k])
        assert err <= R.C_TOL * mags[k], (k, got[k], ref[k], mags[k])
        worst = max(worst, err / (R.C_TOL * mags[k]))
    errc = np.abs(gcol - rcol)
    assert (errc <= R.C_TOL * mcol).all(), (gcol, rcol)
    _report("bd_latent_stats_categorical", f"D={D} C={C_} rows={rows}", max(worst, float((errc / (R.C_TOL * mcol)).max())))


# ---- bd_segment_sumsq ------------------------------------------------------------------------------------------------------
def _segments(cabi, ws, x, offsets, off):
    buf = _inp(x, off)
    offs = (C.c_size_t * len(offsets))(*offsets)
    out = Out(len(offsets) - 1)
    got, = _twice([out], lambda: cabi.check(cabi.lib.bd_segment_sumsq(buf.data_ptr(), len(offsets) - 1, offs, out.ptr(),
                                                                      ws.data_ptr(), None)))
    ref = R.segment_sumsq_ref(x, offsets)
    worst = 0.0
    for s, (g, r) in enumerate(zip(got, ref)):
        n = max(offsets[s + 1] - offsets[s], 1)
        assert abs(g - r) <= R.sum_bound(n, r), (s, g, r)
        worst = max(worst, abs(g - r) / R.sum_bound(n, r) if r > 0 else 0.0)
    return worst


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_segment_sumsq_layouts(cabi, ws, off):
    x = _data(60000, 11 + off)
    # empty, one element, shorter than a vector, spread over several workgroups' chunks (4096-float chunks here), offsets
    # off the 16-byte grid, an empty segment at the end; the first segment does not start at 0
    offsets = [3, 3, 4, 9, 20010, 20013, 41000, 41000, 59999, 59999]
    _report("bd_segment_sumsq", f"mixed off={off}", _segments(cabi, ws, x, offsets, off))
    _report("bd_segment_sumsq", f"one off={off}", _segments(cabi, ws, x, [0, 60000], off))
    _report("bd_segment_sumsq", f"one short off={off}", _segments(cabi, ws, x, [7, 10], off))


def test_segment_sumsq_thirty_two_segments(cabi, ws):
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.integers(0, 300000, 31))
    offsets = [0] + [int(c) for c in cuts] + [300000]
    offsets[5] = offsets[4]                                  # an empty one among them
    offsets = sorted(offsets)
    _report("bd_segment_sumsq", "32 segments", _segments(cabi, ws, _data(300000, 6), offsets, 1))


def test_zero_counts_launch_nothing_and_leave_outputs_alone(cabi, ws):
    out = Out(6)
    a = cabi.MomentsArgs()
    a.n_buf = 0
    cabi.check(cabi.lib.bd_moments(C.byref(a), out.ptr(), ws.data_ptr(), None))
    cabi.check(cabi.lib.bd_segment_sumsq(None, 0, None, out.ptr(), ws.data_ptr(), None))
    torch.cuda.synchronize()
    assert (out.buf == SENTINEL).all()
