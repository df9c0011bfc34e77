"""CPU: the numpy restatement of the replica fingerprint (tests/replica_ref.py) against a plain-Python big-int loop, and
the properties the replica check relies on.  Everything is exact: integers mod 2^64."""
import numpy as np
import pytest

from tests import replica_ref as R


@pytest.mark.parametrize("n", [0, 1, 2, 5, 64, 333])
def test_numpy_form_equals_bigint_loop(n):
    x = R.special_values(n, 10 + n)
    assert R.fingerprint(x) == R.fingerprint_bigint(x)
    y = np.random.RandomState(n).standard_normal(n).astype(np.float32) * 1e3
    assert R.fingerprint(y) == R.fingerprint_bigint(y)


def test_known_small_cases():
    assert R.fingerprint(np.zeros(0, np.float32)) == (0, 0)
    # one element, pattern 0: x = mix(1 * GOLDEN) by hand
    v = R.GOLDEN
    v = ((v ^ (v >> 30)) * R.M1) & R.MASK
    v = ((v ^ (v >> 27)) * R.M2) & R.MASK
    v ^= v >> 31
    assert R.fingerprint(np.zeros(1, np.float32)) == (v, 0)


def test_any_single_bit_flip_changes_the_hash():
    """The mixer is a bijection of u for a fixed index: two patterns at one index never give the same term."""
    x = R.special_values(37, 3)
    h0, _ = R.fingerprint(x)
    for i in range(x.size):
        for b in range(32):
            y = x.copy()
            y.view(np.uint32)[i] ^= np.uint32(1 << b)
            assert R.fingerprint(y)[0] != h0, (i, b)


def test_swapping_unequal_elements_changes_the_hash():
    x = R.special_values(29, 4)
    u = x.view(np.uint32)
    h0, nf0 = R.fingerprint(x)
    for i in range(x.size):
        for j in range(i + 1, x.size):
            if u[i] == u[j]:
                continue
            y = x.copy()
            y.view(np.uint32)[[i, j]] = u[[j, i]]
            h, nf = R.fingerprint(y)
            assert h != h0, (i, j)
            assert nf == nf0
    # -0.0 and +0.0 are different patterns: the fingerprint is over bits, not values
    assert R.fingerprint(np.array([0.0, 1.0], np.float32))[0] != R.fingerprint(np.array([-0.0, 1.0], np.float32))[0]


def test_nonfinite_counts_inf_and_every_nan_payload_only():
    pats = {0x7F800000: 1, 0xFF800000: 1,                                  # +-Inf
            0x7FC00000: 1, 0x7F800001: 1, 0xFFFFFFFF: 1, 0x7FBFFFFF: 1,    # quiet / signalling NaNs, any payload and sign
            0x00000000: 0, 0x80000000: 0,                                  # +-0
            0x00000001: 0, 0x007FFFFF: 0, 0x807FFFFF: 0,                   # denormals
            0x7F7FFFFF: 0, 0xFF7FFFFF: 0, 0x00800000: 0, 0x3F800000: 0}    # largest / smallest normals, 1.0
    for p, want in pats.items():
        x = np.array([p], dtype=np.uint32).view(np.float32)
        assert R.fingerprint(x)[1] == want, hex(p)
        assert R.count_special(x) == want, hex(p)
    x = np.array(list(pats), dtype=np.uint32).view(np.float32)
    assert R.fingerprint(x)[1] == sum(pats.values()) == R.count_special(x)
    y = R.special_values(500, 8)
    assert R.fingerprint(y)[1] == R.count_special(y) > 0
