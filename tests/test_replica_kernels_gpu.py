"""GPU: bd_fingerprint against tests/replica_ref.py, word for word (integers mod 2^64: no tolerance anywhere).

Geometry of the launch (csrc/fingerprint.hip): 256 lanes x at most 1024 workgroups, one 16-byte load per lane and trip, so
ONE pass of a full grid covers 1024 * 256 * 4 = 1 048 576 elements; LONG below is longer and takes a second, partial trip."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import replica_ref as R

pytestmark = pytest.mark.gpu

ONE_PASS = 1024 * 256 * 4
LONG = ONE_PASS + 4099
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099]


def run(tensors):
    """One launch over a table of device tensors (None: a null pointer with n = 0) -> [(hash, nonfinite)]."""
    from big_dreamer_amd import _cabi
    a = _cabi.FingerprintArgs()
    a.n_buf = len(tensors)
    for i, t in enumerate(tensors):
        a.buf[i].p, a.buf[i].n = (None, 0) if t is None else ((t.data_ptr() if t.numel() else None), t.numel())
    out = torch.full((max(1, len(tensors)), 2), -1, dtype=torch.int64, device="cuda")     # stale words: the call zeroes them
    _cabi.check(_cabi.lib.bd_fingerprint(C.byref(a), out.data_ptr(), _cabi.stream()))
    w = out.cpu().numpy().view(np.uint64)
    return [(int(w[i, 0]), int(w[i, 1])) for i in range(len(tensors))]


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def long_case():
    x = R.special_values(LONG + 4, 77)
    return x, dev(x)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_vector_width_and_the_workgroup(n):
    x = R.special_values(n, 100 + n)
    assert run([dev(x)]) == [R.fingerprint(x)]
    y = np.random.RandomState(n).standard_normal(n).astype(np.float32)          # finite only: nonfinite must be 0
    assert run([dev(y)]) == [R.fingerprint(y)] and R.fingerprint(y)[1] == 0


@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 257, 4099])
def test_starts_that_are_only_4_byte_aligned(off, n):
    x = R.special_values(n + off, 31 * n + off)
    t = dev(x)
    assert t.data_ptr() % 16 == 0 and t[off:].data_ptr() % 16 == 4 * off
    assert run([t[off:]]) == [R.fingerprint(x[off:])]


def test_longer_than_one_pass_of_the_grid(long_case):
    x, t = long_case
    assert x.size > ONE_PASS
    want = R.fingerprint(x)
    assert want[1] > 0
    assert run([t]) == [want]
    assert run([t]) == [want]                                    # a second launch: identical words
    for off in (1, 3):
        assert run([t[off:]]) == [R.fingerprint(x[off:])]


def test_sixteen_buffers_of_mixed_sizes_in_one_launch(long_case):
    x, t = long_case
    cuts = [0, 5, 5 + 1023, 1033, 1033 + 4099, 5200, 5200 + 65, 5300, 5300, 5301, 5301 + 256, 6000, 6000 + 300000, 310000,
            310003, 310003 + 257, 320000]
    views, want = [], []
    for i in range(16):
        lo, hi = cuts[i], cuts[i + 1]
        views.append(t[lo:hi] if hi > lo else None)             # buffer 7 is empty (a null pointer, n = 0)
        want.append(R.fingerprint(x[lo:hi]))
    assert views[7] is None and want[7] == (0, 0)
    assert any(v is not None and v.data_ptr() % 16 for v in views)
    got = run(views)
    assert got == want
    assert run(views) == got
    # an empty table and a table of empty buffers
    assert run([]) == []
    assert run([None, t[:0], None]) == [(0, 0)] * 3
    # the same buffer in several slots is read independently
    assert run([t[:1000], t[:1000], t[1:1000]]) == [R.fingerprint(x[:1000])] * 2 + [R.fingerprint(x[1:1000])]


def test_one_ulp_and_a_swap_are_detected():
    n = 4099
    x = np.random.RandomState(5).standard_normal(n).astype(np.float32)
    base = run([dev(x)])[0]
    assert base == R.fingerprint(x)
    y = x.copy()
    y[-1] = np.nextafter(y[-1], np.float32(np.inf))             # one ulp in the last element (a tail element: 4099 = 4 * 1024 + 3)
    got = run([dev(y)])[0]
    assert got == R.fingerprint(y) and got[0] != base[0] and got[1] == 0
    z = x.copy()
    assert z[17] != z[2500]
    z[[17, 2500]] = z[[2500, 17]]
    got = run([dev(z)])[0]
    assert got == R.fingerprint(z) and got[0] != base[0]
    s = x.copy()
    s[100] = -0.0
    p = x.copy()
    p[100] = 0.0
    assert run([dev(s)])[0][0] != run([dev(p)])[0][0]          # bit patterns, not values
