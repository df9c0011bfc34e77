"""CPU: the perf-mode generator's core (csrc/bd_rng.h) is Philox4x32-10: the published known-answer vectors of the Random123
distribution (kat_vectors, philox4x32 10 rounds) through the host build of the same source, and through the Python restatement
the GPU tests use to check the device output."""
import ctypes as C

from tests.rng_ref import KAT, philox as _philox_ref      # the shared restatement and the published vectors


def test_python_restatement_matches_known_answers():
    for ctr, key, want in KAT:
        assert _philox_ref(ctr, key) == want


def test_library_core_matches_known_answers():
    from big_dreamer_amd import _cabi as cabi
    for ctr, key, want in KAT:
        out = (C.c_uint * 4)()
        cabi.check(cabi.lib.bd_philox4x32_10((C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), out))
        assert list(out) == want
