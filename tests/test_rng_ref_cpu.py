"""CPU: the restatement of the perf-mode noise generator and its counter maps (tests/rng_ref.py).  It is pinned to the
published Philox vectors (also through the library's host build of the same source); the counters that hit the ends of
the 24-bit range are found again by search; every planted fault of rng_ref.VARIANTS is shown to fail the comparisons
tests/test_rng_values_gpu.py makes, on exactly its inputs; the entropy estimator's counter map is disjoint; and no two
consumers share a stream id."""
import ctypes as C

import numpy as np
import pytest

from tests import rng_ref as R


# ---- known answers ---------------------------------------------------------------------------------------------------------

def test_known_answers_through_the_library_and_the_restatement():
    from big_dreamer_amd import _cabi as cabi
    for ctr, key, want in R.KAT:
        out = (C.c_uint * 4)()
        cabi.check(cabi.lib.bd_philox4x32_10((C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), out))
        assert list(out) == want
        assert R.philox(ctr, key) == want
        assert R.philox_np(*ctr, *key).tolist() == want
    assert (cabi.BD_RNG_NORMAL, cabi.BD_RNG_EXPONENTIAL, cabi.BD_RNG_UNIFORM) == (R.NORMAL, R.EXPONENTIAL, R.UNIFORM)
    assert cabi.BD_RNG_MAX_TENSORS == R.MAX_TENSORS == len(R.FILL_COUNTS)


def test_vectorised_philox_is_the_integer_one():
    g = np.random.default_rng(0)
    ctr = g.integers(0, 2 ** 32, size=(64, 4), dtype=np.uint64)
    ctr[:8] = [[0xFFFFFFFF, 0, 0, 0], [0, 0xFFFFFFFF, 0, 0], [0, 0, 0xFFFFFFFF, 0], [0, 0, 0, 0xFFFFFFFF]] * 2
    for key in ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF), R.key_of(R.FILL_SEED)):
        got = R.philox_np(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key)
        assert got.dtype == np.uint32
        assert got.tolist() == [R.philox(c.tolist(), key) for c in ctr]
    w = R.words(R.FILL_SEED, 3, 7, 5, first=2 ** 32 - 2)           # the quad index carries into the counter's second word
    for i in range(5):
        q = 2 ** 32 - 2 + i
        assert w[i].tolist() == R.philox([q & R.M32, q >> 32, 3, 7], R.key_of(R.FILL_SEED))


# ---- u01 in float32 -----------------------------------------------------------------------------------------------------------

def test_u01_over_all_2_24_values():
    """Every k = word >> 8: strictly inside (0, 1); exact below 2^23, within 2^-25 of the real value from there on (the
    tie of k + 0.5 rounds to even); the clamp changes the one result k = 2^24 - 1 and no other."""
    k = np.arange(2 ** 24, dtype=np.uint32)
    w = k << np.uint32(8)
    u, raw = R.u01(w), R.u01(w, clamp=False)
    assert u.dtype == np.float32 and raw.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0 and float(u.max()) == float(R.U_MAX) == 1.0 - 2.0 ** -24
    assert np.flatnonzero(u != raw).tolist() == [2 ** 24 - 1] and float(raw[-1]) == 1.0
    real = (k.astype(np.float64) + 0.5) / 2.0 ** 24
    lo = k < 2 ** 23
    assert np.array_equal(u[lo].astype(np.float64), real[lo])
    d = np.abs(u[~lo].astype(np.float64) - real[~lo])
    assert float(d.max()) == 2.0 ** -25 and float(d.min()) == 2.0 ** -25         # every one of them is a tie
    assert (np.diff(u.astype(np.float64)) >= 0).all()
    # what the unclamped value does downstream
    assert float(-np.log(raw[-1])) == 0.0 and float(R.exponential(w[-1:])[0]) == pytest.approx(2.0 ** -24, rel=1e-6)
    assert R.uniform(w).dtype == np.float32 and float(R.uniform(w)[0]) == 0.0 and float(R.uniform(w)[-1]) == 1.0 - 2.0 ** -24


# ---- the edge counters ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def edge_hits():
    """Every word of (FILL_SEED, stream EDGE_STREAM, quads of an EDGE_COUNT tensor) whose top 24 bits are all ones or all
    zeros, steps in ascending order until both kinds have been seen in an even and in an odd word."""
    quads = R.EDGE_COUNT // 4
    q = np.arange(quads, dtype=np.uint64)[None, :]
    hits, seen, chunk = [], set(), 4096
    for s0 in range(0, 1 << 17, chunk):
        steps = np.arange(s0, s0 + chunk, dtype=np.uint64)[:, None]
        k = R.philox_np(q, 0, R.EDGE_STREAM, steps, *R.key_of(R.FILL_SEED)) >> np.uint32(8)
        for kind, mask in (("ones", k == 0xFFFFFF), ("zeros", k == 0)):
            for s, qq, wd in zip(*np.nonzero(mask)):
                hits.append((s0 + int(s), int(qq), int(wd), kind))
                seen.add((kind, int(wd) & 1))
        if len(seen) == 4:
            break
    return hits


def test_edge_search_finds_the_chosen_counters(edge_hits):
    assert {(k, w & 1) for _, _, w, k in edge_hits} == {("ones", 0), ("ones", 1), ("zeros", 0), ("zeros", 1)}
    assert set(R.EDGES) <= set(edge_hits), (R.EDGES, edge_hits)
    assert {(k, w & 1) for _, _, w, k in R.EDGES} == {("ones", 0), ("ones", 1), ("zeros", 0), ("zeros", 1)}
    # about one hit per 2^22 quads and kind: the search is no accident of a broken generator
    n_quads = (max(s for s, *_ in edge_hits) + 1) * (R.EDGE_COUNT // 4)
    assert 0.2 < len(edge_hits) / (2 * n_quads / 2.0 ** 22) < 5.0, (len(edge_hits), n_quads)
    for step, quad, word, kind in R.EDGES:
        x = R.philox([quad, 0, R.EDGE_STREAM, step], R.key_of(R.FILL_SEED))[word]
        assert x >> 8 == (0xFFFFFF if kind == "ones" else 0), hex(x)
        assert 4 * quad + word < R.EDGE_COUNT


def test_edge_values_of_the_restatement():
    """What the GPU edge tests expect: a finite positive Exp(1) variate and a radius of 3.45e-4 at the all-ones word
    (-0.0 and 0 without the clamp), exactly 0.0 as the uniform of the all-zeros word."""
    for step, quad, word, kind in R.EDGES:
        e = 4 * quad + word
        nrm, ex, uni = R.fill(R.FILL_SEED, step, R.EDGE_TENSORS)
        raw_n, raw_e, _ = R.fill(R.FILL_SEED, step, R.EDGE_TENSORS, variant="u01_unclamped")
        assert np.isfinite(nrm).all() and np.isfinite(ex).all() and (ex > 0).all()
        assert uni.dtype == np.float32 and (uni >= 0).all() and (uni < 1).all()
        if kind == "zeros":
            assert float(uni[e]) == 0.0 and float(ex[e]) == pytest.approx(25 * np.log(2.0), rel=1e-12)
            assert np.array_equal(raw_n, nrm) and np.array_equal(raw_e, ex)
            continue
        assert float(uni[e]) == 1.0 - 2.0 ** -24
        assert float(ex[e]) == pytest.approx(2.0 ** -24, rel=1e-6) and int(np.argmin(ex)) == e
        assert float(raw_e[e]) == 0.0 and not float(raw_e[e]) > 0.0
        if word % 2 == 0:                   # a Box-Muller radius word
            pair, raw_pair = nrm[e:e + 2], raw_n[e:e + 2]
            assert float(np.hypot(*pair)) == pytest.approx(np.sqrt(2.0 ** -23), rel=1e-6)      # 3.45e-4
            assert np.abs(raw_pair).max() == 0.0


# ---- the teeth of the GPU comparison ------------------------------------------------------------------------------------------

def _gpu_inputs():
    """(name, seed, step, tensors) of every launch of tests/test_rng_values_gpu.py."""
    for rot in R.FILL_ROTATIONS:
        yield f"rotation {rot}", R.FILL_SEED, R.FILL_STEP, R.fill_case(rot)
    for step, *_ in R.EDGES:
        yield f"edge step {step}", R.FILL_SEED, step, R.EDGE_TENSORS


def test_gpu_fill_inputs_cover_the_launch_geometry():
    assert R.FILL_COUNTS == (1, 3, 1023, 1024, 1025, 4099) and R.FILL_STEP & R.M32 != 0
    for rot in R.FILL_ROTATIONS:
        case = R.fill_case(rot)
        assert {k for _, k, _ in case} == {R.NORMAL, R.EXPONENTIAL, R.UNIFORM}
        assert case[4][1:] == case[5][1:], "the last two tensors share a stream id and a kind"
        assert len({s for _, _, s in case}) == 5
        assert all(s != 0 for _, _, s in case)
    assert [o % 4 for o in R.FILL_OFFSETS].count(0) == 5 and R.FILL_OFFSETS[3] % 4 != 0
    assert {tuple(k for _, k, _ in R.fill_case(r))[3] for r in R.FILL_ROTATIONS} == {0, 1, 2}      # each kind, scalar stores


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_every_variant_fails_the_gpu_comparison(variant):
    """In at least one element of the GPU tests' own inputs the planted fault is off by more than 10 x the tolerance the
    GPU test applies there (uniform: by any bit): a kernel with that fault cannot pass."""
    caught = []
    for name, seed, step, tensors in _gpu_inputs():
        ref, bad = R.fill(seed, step, tensors), R.fill(seed, step, tensors, variant=variant)
        for i, (count, kind, _) in enumerate(tensors):
            assert ref[i].shape == bad[i].shape == (count,)
            if R.worst_ratio(bad[i], ref[i], kind) > 10.0:
                caught.append((name, i, R.KIND_NAMES[kind]))
    assert caught, variant
    if variant == "u01_unclamped":
        # seen by tolerance where the all-ones word is a radius; the Exp(1) value there is off by 6e-8 only, which is why
        # the GPU test also requires it to be strictly positive and feeds it to a sampler
        assert caught == [("edge step 46795", 0, "normal")], caught
    else:
        # every launch of six tensors catches it on its own, in every kind
        for rot in R.FILL_ROTATIONS:
            kinds = {k for n, _, k in caught if n == f"rotation {rot}"}
            assert kinds == {"normal", "exponential", "uniform"} or variant == "pair_swapped" and kinds == {"normal"}, (rot, caught)


def test_shared_stream_prefix_of_the_restatement():
    for rot in R.FILL_ROTATIONS:
        out = R.fill(R.FILL_SEED, R.FILL_STEP, R.fill_case(rot))
        assert np.array_equal(out[4], out[5][:R.FILL_COUNTS[4]])
        assert not np.array_equal(out[3][:1], out[0])


# ---- the entropy estimator's counter map ----------------------------------------------------------------------------------------

def test_entropy_map_is_disjoint_for_every_width_and_sample_count():
    """For every A in 1 .. kMaxA and n_samples in 1 .. 200: the quads of (row, j, part) lie in that owner's own range
    [owner per, (owner + 1) per) -- ranges of different owners cannot meet --, draw m of a part is word m % 4 of quad
    m / 4 of the range, so no word is used twice, and the buffer length covers every index."""
    Hm, N = 2, 1
    for ns in range(1, 201):
        per, use = R.entropy_quads(1, ns)
        assert sum(len(v) for v in use.values()) == ns
        for part, lst in use.items():
            assert len(set(lst)) == len(lst) and all(0 <= q < per and 0 <= w < 4 for q, w in lst), (ns, part)
        k = np.arange(ns).reshape(1, ns, 1, 1)
        part, m = k % R.K_ENT_PARTS, k // R.K_ENT_PARTS
        for A in range(1, R.K_MAX_A + 1):
            idx, n = R.rng_gather_index(Hm, N, A, ns)
            assert idx.shape == (Hm, ns, N, A) and n == 4 * Hm * N * A * R.K_ENT_PARTS * per
            row = np.arange(Hm).reshape(Hm, 1, 1, 1) * N + np.arange(N).reshape(1, 1, N, 1)
            owner = (row * A + np.arange(A).reshape(1, 1, 1, A)) * R.K_ENT_PARTS + part
            off = idx // 4 - owner * per
            assert ((off >= 0) & (off < per)).all(), (A, ns)
            assert np.array_equal(4 * off + idx % 4, np.broadcast_to(m, idx.shape)), (A, ns)
            assert int(idx.max()) < n and int(idx.min()) >= 0
    # the dense check once, without the structure: all indices distinct
    for A, ns in ((1, 1), (3, 17), (17, 100), (64, 200)):
        idx, n = R.rng_gather_index(2, 3, A, ns)
        assert np.unique(idx).size == idx.size and int(idx.max()) < n


def test_entropy_ref_keeps_the_same_map():
    from tests import entropy_ref as E
    assert (E.K_ENT_PARTS, 64) == (R.K_ENT_PARTS, R.K_MAX_A)
    idx, n = E.rng_gather_index(2, 7, 3, 100)
    want, n2 = R.rng_gather_index(2, 7, 3, 100)
    assert n == n2 and np.array_equal(idx.numpy(), want)


# ---- streams and keys -----------------------------------------------------------------------------------------------------------

def test_stream_audit():
    from big_dreamer_amd import memory
    from big_dreamer_amd.engine import DreamerEngine
    assert DreamerEngine.RNG_STREAMS == R.RNG_STREAMS and set(R.STEP_COUNTER) == set(R.RNG_STREAMS)
    assert memory.SAMPLE_STREAM == R.REPLAY_STREAM == 12 and R.PIXEL_STREAM == 6
    ids = list(R.RNG_STREAMS.values()) + [R.PIXEL_STREAM, R.REPLAY_STREAM]
    assert len(set(ids)) == len(ids) and all(0 < i < 2 ** 32 for i in ids)
    # streams that share a step counter and can be live in the same step differ in their id: that is all that keeps
    # their counters apart (same key, same step, quad indices from 0)
    for seed in (0, 1234, 2 ** 64 - 1):
        keys = [R.engine_key(seed, r) for r in range(8)]
        assert len(set(keys)) == 8 and all(0 <= k < 2 ** 64 for k in keys)
        assert keys[0] == (seed + 0x9E3779B97F4A7C15) % 2 ** 64
    # the same counter under the keys of two ranks gives unrelated words
    a, b = (R.words(R.engine_key(5, r), 1, 0, 64) for r in (0, 1))
    assert not (a == b).any()


def test_replay_draw_is_the_memory_module_restatement():
    from big_dreamer_amd.memory import philox4x32_10
    for b in (0, 1, 49):
        x = philox4x32_10((b, 0, 12, 9), R.key_of(R.FILL_SEED))
        assert R.replay_draw(R.FILL_SEED, 9, b, 4, 1000) == ((x[0] * 4) >> 32, ((x[2] | x[3] << 32) * 1000) >> 64)
        lane, u = R.replay_draw(R.FILL_SEED, 9, b, 4, 1000)
        assert 0 <= lane < 4 and 0 <= u < 1000


def test_pixel_uniforms_use_stream_6_row_major():
    u = R.pixel_uniforms(R.PIXEL_SEED, 2 ** 32 - 1, 5, 12)
    assert u.shape == (5, 12) and u.dtype == np.float32
    for r, q in ((0, 0), (3, 2), (4, 1)):
        w = R.philox([r * 3 + q, 0, 6, 2 ** 32 - 1], R.key_of(R.PIXEL_SEED))
        assert u[r, 4 * q:4 * q + 4].tolist() == [(x >> 8) / 2.0 ** 24 for x in w]
    assert 342 * 12288 // 4 > 4096 * 256 and (342, 12288) in R.PIXEL_SHAPES
