"""GPU: the perf-mode noise kernels value for value against tests/rng_ref.py (whose teeth on exactly these inputs
tests/test_rng_ref_cpu.py shows): bd_rng_fill in one launch of six tensors -- every count at which it takes another
path, every kind, an unaligned base, a shared stream id, guards around every tensor --, the counters whose words hit
the two ends of the 24-bit range (the all-ones word used to give u = 1.0: an Exp(1) variate of -0.0 that no Categorical
sampler could pick, and a Box-Muller pair of zeros), and bd_replay_gather_pixels_rng against the explicit-noise kernel
fed the host's uniforms.

Tolerances (rng_ref.TOL) are the ones test_act_step_cat_gpu.test_rng_fill_uniform_kind derives: uniform bit-exact,
exponential 1e-6 + 1e-6 |v|, normal 4e-6 + 1e-6 |v|.  The reference starts from the float32 u, so they cover logf, sqrtf,
sincosf and the float32 product 2 pi u alone.  Each case prints its worst |err| / tolerance per kind (RNG_WORST lines,
visible under -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import rng_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64          # sentinel floats before, between and after the tensors


def _launch(seed, step, tensors, offsets=None):
    """One bd_rng_fill launch into ONE sentinel-filled buffer: tensor i starts `offsets[i]` floats past a 16-byte
    boundary, with at least GUARD sentinels on either side.  Returns the tensors (CPU float32) after asserting that
    nothing else was written."""
    from big_dreamer_amd import _cabi as cabi
    offsets = offsets or [0] * len(tensors)
    starts, pos = [], GUARD
    for (count, _, _), off in zip(tensors, offsets):
        pos = (pos + 3) // 4 * 4 + off
        starts.append(pos)
        pos += count + GUARD
    buf = torch.full((pos,), R.SENTINEL, device="cuda")
    assert buf.data_ptr() % 16 == 0
    a = cabi.RngFillArgs()
    a.n, a.seed, a.step = len(tensors), seed, step
    for i, ((count, kind, stream), s) in enumerate(zip(tensors, starts)):
        assert (buf.data_ptr() + 4 * s) % 16 == 4 * offsets[i]
        a.t[i] = cabi.RngTensor(buf.data_ptr() + 4 * s, count, kind, stream)
    cabi.check(cabi.lib.bd_rng_fill(C.byref(a), cabi.stream()))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    inside = np.zeros(pos, dtype=bool)
    for (count, _, _), s in zip(tensors, starts):
        inside[s:s + count] = True
    assert (host[~inside] == np.float32(R.SENTINEL)).all(), "bd_rng_fill wrote outside its tensors"
    return [host[s:s + count].copy() for (count, _, _), s in zip(tensors, starts)]


def _compare(tag, got, want, tensors):
    """Every element of every tensor; prints and returns the worst ratio per kind."""
    worst = {}
    for i, (count, kind, _) in enumerate(tensors):
        assert got[i].shape == want[i].shape == (count,)
        assert np.isfinite(got[i]).all(), f"{tag} tensor {i}: non-finite values"
        if kind == R.UNIFORM:
            assert got[i].dtype == want[i].dtype == np.float32
            assert np.array_equal(got[i], want[i]), f"{tag} tensor {i}: uniform draws differ from the restatement's bits"
        worst[kind] = max(worst.get(kind, 0.0), R.worst_ratio(got[i], want[i], kind))
    print(f"RNG_WORST {tag} " + " ".join(f"{R.KIND_NAMES[k]}={v:.3e}" for k, v in sorted(worst.items())))
    for i, (count, kind, _) in enumerate(tensors):
        r = R.worst_ratio(got[i], want[i], kind)
        assert r <= 1.0, f"{tag} tensor {i} ({R.KIND_NAMES[kind]}, {count} elements): worst |err| / tolerance {r:.3e}"
    return worst


@pytest.mark.parametrize("rotation", R.FILL_ROTATIONS)
def test_six_tensor_launch_value_for_value(rotation):
    """Counts 1, 3, 1023, 1024, 1025, 4099 (below a quad, below, at and past one block, several blocks, ragged); tensor 3
    starts 4 bytes past a 16-byte boundary, so all its quads take the scalar stores; tensors 4 and 5 share a stream id
    and a kind: the quad index restarts in every tensor, so the shorter is a bit-identical prefix of the longer.  The
    three rotations give every tensor every kind."""
    tensors = R.fill_case(rotation)
    got = _launch(R.FILL_SEED, R.FILL_STEP, tensors, R.FILL_OFFSETS)
    for g in got:
        assert (g != np.float32(R.SENTINEL)).all(), "an element was left unwritten"
    _compare(f"six_tensors rotation={rotation}", got, R.fill(R.FILL_SEED, R.FILL_STEP, tensors), tensors)
    assert np.array_equal(got[4], got[5][:R.FILL_COUNTS[4]]), "the quad index must restart at 0 in every tensor"
    for g, (_, kind, _) in zip(got, tensors):
        if kind == R.EXPONENTIAL:
            assert (g > 0).all()
        if kind == R.UNIFORM:
            assert (g >= 0).all() and (g < 1).all()


def _cat_sample(q):
    """bd_categorical_head_forward on equal logits: 32 groups of 32 classes; the class with the smallest draw wins."""
    from big_dreamer_amd import _cabi as cabi
    rows, D, Cc = 32, 1, 32
    assert q.numel() == rows * D * Cc
    logits = torch.full((rows, D * Cc), 0.25, device="cuda")
    state, probs = torch.zeros_like(logits), torch.zeros_like(logits)
    cabi.check(cabi.lib.bd_categorical_head_forward(cabi.ptr(logits), cabi.ptr(q), rows, D, Cc, cabi.ptr(state), cabi.ptr(probs),
                                                    cabi.stream()))
    torch.cuda.synchronize()
    return state.cpu().numpy().reshape(rows, Cc)


@pytest.mark.parametrize("step, quad, word, kind", R.EDGES, ids=[f"{k}_step{s}_word{w}" for s, _, w, k in R.EDGES])
def test_edge_counters(step, quad, word, kind):
    """A word whose top 24 bits are all ones (u01's k + 0.5 rounds up to 2^24: clamped below 1) or all zeros, in an even
    (Box-Muller radius) and an odd word, in 1024-element tensors of every kind filled by one launch.
    Exponential: finite, strictly positive, within tolerance.  Normal: finite, within tolerance (at the all-ones radius
    word the pair is 3.45e-4 (cos, sin), not zeros).  Uniform: in [0, 1), the restatement's bits, exactly 0.0 at the
    all-zeros word.  Consumer: the Exponential tensor as q_noise of the Categorical head on equal logits -- the class
    with the smallest draw, the edge element at an all-ones word, is the one sampled."""
    e = 4 * quad + word
    got = _launch(R.FILL_SEED, step, R.EDGE_TENSORS)
    want = R.fill(R.FILL_SEED, step, R.EDGE_TENSORS)
    nrm, ex, uni = got
    print(f"RNG_EDGE step={step} element={e} {kind}: exponential {ex[e]!r} (want {want[1][e]:.9e}), normal pair "
          f"{nrm[e & ~1]!r}, {nrm[(e & ~1) + 1]!r} (want {want[0][e & ~1]:.9e}, {want[0][(e & ~1) + 1]:.9e}), uniform {uni[e]!r}")
    bad = []            # every finding of the case is reported, not the first alone
    if not (np.isfinite(ex).all() and (ex > 0).all()):
        bad.append(f"Exp(1) draws must be finite and strictly positive; element {e} is {ex[e]!r}")
    if not ((uni >= 0).all() and (uni < 1).all()):
        bad.append("uniform draws outside [0, 1)")
    try:
        _compare(f"edge step={step} {kind} word={word}", got, want, R.EDGE_TENSORS)
    except AssertionError as err:
        bad.append(str(err))
    if kind == "zeros":
        if float(uni[e]) != 0.0:
            bad.append(f"the uniform of the all-zeros word is {uni[e]!r}, not 0.0")
    else:
        if float(uni[e]) != 1.0 - 2.0 ** -24:
            bad.append(f"the uniform of the all-ones word is {uni[e]!r}, not 1 - 2^-24")
        if word % 2 == 0 and not np.hypot(nrm[e], nrm[e + 1]) > 3e-4:
            bad.append(f"the radius at u = 1 - 2^-24 is 3.45e-4, got the pair {nrm[e]!r}, {nrm[e + 1]!r}")
    # the consumer's view
    state = _cat_sample(torch.from_numpy(ex).cuda())
    if not ((state.sum(1) == 1).all() and ((state == 0) | (state == 1)).all()):
        bad.append("the sampled state is not one-hot")
    picked = state.argmax(1)
    lost = np.flatnonzero(picked != want[1].reshape(32, 32).argmin(1))
    if lost.size:
        bad.append(f"groups {lost.tolist()}: the class with the smallest draw was not sampled "
                   f"(picked {picked[lost].tolist()}, smallest {want[1].reshape(32, 32).argmin(1)[lost].tolist()})")
    if kind == "ones":
        assert int(np.argmin(want[1])) == e
        if picked[e // 32] != e % 32:
            bad.append(f"the edge class {e % 32} of group {e // 32} was not sampled (picked {picked[e // 32]})")
    assert not bad, "\n".join(bad)


# ---- bd_replay_gather_pixels_rng ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", R.PIXEL_STEPS)
@pytest.mark.parametrize("n_idx, pixels", R.PIXEL_SHAPES)
def test_pixel_gather_rng_value_for_value(n_idx, pixels, step):
    """bd_replay_gather_pixels_rng == bd_replay_gather_pixels fed the host's stream-6 uniforms (torch.equal: one kernel
    body, and the uniforms k 2^-24 are exact in float32), for bit depths 1, 5 and 8; and both within 4 * 2^-24 of
    floor(u8 / 2^(8 - bits)) / 2^bits - 0.5 + u / 2^bits in float64.
    The bound: the kernel forms three float32 results on the way -- q 2^-bits - 0.5, u 2^-bits and their sum (or the
    first and one fused multiply-add) -- each of magnitude at most 1, so each rounds by at most 2^-24 even in a
    whole-ulp model: 3 * 2^-24 <= 4 * 2^-24.  (With powers of two as factors only the last can round at all.)
    (342, 12288): 342 * 3072 quads exceed the 4096 * 256 threads of the grid, so the grid-stride loop runs twice; step
    2^32 - 1 is the largest value of the counter's step word."""
    from big_dreamer_amd import _cabi as cabi
    rows = 7
    g = torch.Generator().manual_seed(n_idx + step % 1000)
    u8 = torch.randint(0, 256, (rows, pixels), dtype=torch.uint8, generator=g)
    u8[0, :4] = torch.tensor([0, 255, 128, 127], dtype=torch.uint8)
    idx = torch.randint(0, rows, (n_idx,), dtype=torch.int64, generator=g)
    idx[0] = 0
    host_u = R.pixel_uniforms(R.PIXEL_SEED, step, n_idx, pixels)
    assert host_u.dtype == np.float32 and float(host_u.min()) >= 0.0 and float(host_u.max()) < 1.0
    u8d, idxd, noise = u8.cuda(), idx.cuda(), torch.from_numpy(host_u).cuda()
    gathered = u8[idx].numpy()
    for bits in R.PIXEL_BITS:
        a = torch.full((n_idx * pixels + 2 * GUARD,), R.SENTINEL, device="cuda")
        b = torch.full((n_idx * pixels + 2 * GUARD,), R.SENTINEL, device="cuda")
        da, db = a[GUARD:GUARD + n_idx * pixels], b[GUARD:GUARD + n_idx * pixels]
        assert da.data_ptr() % 16 == 0
        cabi.check(cabi.lib.bd_replay_gather_pixels_rng(u8d.data_ptr(), idxd.data_ptr(), n_idx, pixels, bits, R.PIXEL_SEED, step,
                                                        da.data_ptr(), cabi.stream()))
        cabi.check(cabi.lib.bd_replay_gather_pixels(u8d.data_ptr(), idxd.data_ptr(), n_idx, pixels, bits, noise.data_ptr(),
                                                    db.data_ptr(), cabi.stream()))
        torch.cuda.synchronize()
        for t in (a, b):
            assert bool((t[:GUARD] == R.SENTINEL).all()) and bool((t[-GUARD:] == R.SENTINEL).all()), "written outside dst"
        assert torch.equal(da, db), f"bits={bits}: in-kernel uniforms differ from stream 6 of the restatement"
        want = R.dequantise64(gathered, host_u, bits).reshape(-1)
        err = float(np.abs(da.cpu().numpy().astype(np.float64) - want).max())
        print(f"RNG_WORST pixels n_idx={n_idx},pixels={pixels},bits={bits},step={step} {err / R.PIXEL_TOL:.3e}")
        assert err <= R.PIXEL_TOL, (bits, err)
