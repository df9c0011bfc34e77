"""One restatement of the perf-mode noise generator (csrc/bd_rng.h) and of every counter map that consumes it: plain
Python / numpy, no device, no project code.  The GPU tests (test_rng_values_gpu.py, test_perf_step_gpu.py) compare the
kernels with it; test_rng_ref_cpu.py pins it to the published Philox vectors and shows that each planted fault of
VARIANTS would fail those GPU tests.

The generator.  Philox4x32-10 (Salmon et al., SC'11): words = philox(counter, key) with
    key     = (seed lo, seed hi)                        seed: Engine.rng_seed, see engine_key
    counter = (quad lo, quad hi, stream id, step)       quad: which group of four values; step: 32 bits
One counter gives four 32-bit words x[0..3], and each value kind uses the top 24 bits k = x >> 8 of a word:
    uniform      v = k * 2^-24                          in [0, 1), exact in float32
    u01          u = min(fl(fl(k) + 0.5) * 2^-24, 1 - 2^-24)     float32: convert (exact), add (rounds), scale (exact)
    exponential  v = -log(u)
    normal       (v[2h], v[2h + 1]) = sqrt(-2 log u(x[2h])) * (cos, sin)(2 pi u(x[2h + 1])),  h = 0, 1
u01 IS a float32 computation: for k >= 2^23 the sum k + 0.5 is not a float32 and the tie rounds to even, so u differs
from the real (k + 0.5) / 2^24 by up to 2^-25 there, and k = 2^24 - 1 would round up to u = 1.0 (-log u = -0.0, a
Categorical sampler's p / q = -inf, a Box-Muller radius of 0) without the clamp to the largest float32 below 1.  The
radius sqrt(-2 log u) magnifies a change of u without bound as u -> 1 (d r / d u = -1 / (r u)), so a reference that
started from the real-valued u would be off by far more than the kernels' libm error there.  The restatement therefore
takes u in float32, exactly as numpy computes it, and everything after it (log, sqrt, cos, sin) in float64: what is left
between it and the kernel is logf, sqrtf, sincosf and the float32 product 2 pi u.

The counter maps (who uses which quad, word, stream and step) are the functions below the value kinds.
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85

NORMAL, EXPONENTIAL, UNIFORM = 0, 1, 2          # BD_RNG_NORMAL, BD_RNG_EXPONENTIAL, BD_RNG_UNIFORM (bigdreamer_hip.h)
MAX_TENSORS = 6                                 # BD_RNG_MAX_TENSORS
U_MAX = np.float32(1.0) - np.float32(2.0 ** -24)       # 0x1.fffffep-1f, the largest float32 below 1

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, words)
KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------

def philox(ctr, key):
    """Philox4x32-10 in Python integers: four counter words, two key words -> four words."""
    c, k = [int(v) for v in ctr], [int(v) for v in key]
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + _W0) & M32, (k[1] + _W1) & M32]
    return c


def philox_np(c0, c1, c2, c3, k0, k1):
    """The same on numpy arrays (broadcast against each other): uint32 [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) & np.uint64(M32) for v in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & M32, int(k1) & M32
    m32, s32 = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2              # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + _W0) & M32, (k1 + _W1) & M32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def key_of(seed):
    seed = int(seed) & M64
    return seed & M32, seed >> 32


def words(seed, stream, step, quads, first=0):
    """Words of the quads first .. first + quads - 1 of (seed, stream, step): uint32 [quads, 4]."""
    q = np.arange(first, first + quads, dtype=np.uint64)
    return philox_np(q & np.uint64(M32), q >> np.uint64(32), int(stream) & M32, int(step) & M32, *key_of(seed))


# ---- the three value kinds -------------------------------------------------------------------------------------------------

def u01(w, clamp=True):
    """bd::u01 in IEEE float32, operation by operation (numpy rounds each as the hardware does)."""
    k = (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)      # < 2^24: exact
    u = (k + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return np.minimum(u, U_MAX) if clamp else u


def uniform(w):
    """rng_uniform4: float32, exact."""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def exponential(w, clamp=True):
    """rng_exp4 in float64 from the float32 u."""
    return -np.log(u01(w, clamp).astype(np.float64))


def normal(w, clamp=True, variant=None):
    """rng_normal4 in float64 from the float32 u: w [quads, 4] -> [quads, 4]."""
    w = np.asarray(w, dtype=np.uint32).reshape(-1, 2, 2)
    ur, ua = (u01(w[..., j], clamp).astype(np.float64) for j in (0, 1))          # even word: radius, odd word: angle
    r, a = np.sqrt(-2.0 * np.log(ur)), 2.0 * np.pi * ua
    pair = (np.sin(a), np.cos(a)) if variant == "pair_swapped" else (np.cos(a), np.sin(a))
    return np.stack([r * pair[0], r * pair[1]], -1).reshape(-1, 4)


def values(kind, w, clamp=True, variant=None):
    """The four values of every quad of w [quads, 4]: float32 for UNIFORM (exact), float64 otherwise."""
    if kind == UNIFORM:
        return uniform(w)
    return exponential(w, clamp) if kind == EXPONENTIAL else normal(w, clamp, variant)


# ---- bd_rng_fill -------------------------------------------------------------------------------------------------------------
# One launch fills up to MAX_TENSORS tensors; element i of a tensor is word i & 3 of quad i >> 2 of (seed, the tensor's
# stream id, the launch's step), the quad index restarting at 0 in every tensor.

VARIANTS = ("u01_unclamped", "pair_swapped", "stream_ignored", "step_ignored", "quad_carried_across_tensors",
            "tail_quad_dropped")
SENTINEL = -7.0                 # what the GPU tests pre-fill their buffers with; "tail_quad_dropped" leaves it standing


def fill(seed, step, tensors, variant=None):
    """bd_rng_fill restated: tensors = [(count, kind, stream id), ...] -> one array per tensor.  `variant`: one planted
    fault of VARIANTS (the teeth of test_rng_ref_cpu.py)."""
    assert variant is None or variant in VARIANTS, variant
    out, carried = [], 0
    for count, kind, stream in tensors:
        quads = (count + 3) // 4
        first = carried if variant == "quad_carried_across_tensors" else 0
        w = words(seed, 0 if variant == "stream_ignored" else stream, 0 if variant == "step_ignored" else step, quads, first)
        v = values(kind, w, clamp=variant != "u01_unclamped", variant=variant).reshape(-1)[:count].copy()
        if variant == "tail_quad_dropped" and count % 4:
            v[count - count % 4:] = SENTINEL
        out.append(v)
        carried += quads
    return out


# ---- the other counter maps -------------------------------------------------------------------------------------------------

K_ENT_PARTS = 16                # imagine.hip kEntParts
K_MAX_A = 64                    # imagine.hip kMaxA


def entropy_quads(A, ns):
    """bd_actor_entropy_rng (actor_entropy_kernel<true>): sample part `part` of (row, j) owns the `per` quads from
    base = ((row A + j) 16 + part) per, per = (ns / 16 + 4) / 4, and draw k = part + 16 m is word m % 4 of quad
    base + m / 4.  Returns (per, {part: [(quad offset, word) of m = 0, 1, ...]})."""
    per = (ns // K_ENT_PARTS + 4) // 4
    use = {}
    for part in range(K_ENT_PARTS):
        mine = (ns - part + K_ENT_PARTS - 1) // K_ENT_PARTS if part < ns else 0
        use[part] = [(m // 4, m % 4) for m in range(mine)]
    return per, use


def rng_gather_index(Hm, N, A, ns):
    """Element of a fill(NORMAL, stream 4) buffer that bd_actor_entropy_rng uses as draw k of (row, j) (entropy_quads;
    the fill writes quad q at elements 4 q .. 4 q + 3).  Returns (index [Hm, ns, N, A] int64 array, buffer length)."""
    per = (ns // K_ENT_PARTS + 4) // 4
    k = np.arange(ns, dtype=np.int64).reshape(1, ns, 1, 1)
    row = np.arange(Hm, dtype=np.int64).reshape(Hm, 1, 1, 1) * N + np.arange(N, dtype=np.int64).reshape(1, 1, N, 1)
    j = np.arange(A, dtype=np.int64).reshape(1, 1, 1, A)
    part, m = k % K_ENT_PARTS, k // K_ENT_PARTS
    base = ((row * A + j) * K_ENT_PARTS + part) * per
    return 4 * (base + m // 4) + m % 4, 4 * Hm * N * A * K_ENT_PARTS * per


PIXEL_STREAM = 6                # bd_replay_gather_pixels_rng, bd_replay_sample_gather: the dequantisation noise
REPLAY_STREAM = 12              # bd_replay_sample_gather: the draw of the chunks


def pixel_uniforms(seed, step, n_idx, pixels):
    """The dequantisation uniforms of gather_pixels_kernel<true>: the four pixels 4 q .. 4 q + 3 of gathered row r are
    the words of quad e = r (pixels / 4) + q of (seed, stream 6, step): float32 [n_idx, pixels], exact."""
    assert pixels % 4 == 0
    return uniform(words(seed, PIXEL_STREAM, step, n_idx * (pixels // 4))).reshape(n_idx, pixels)


def dequantise64(u8, noise, bit_depth):
    """floor(u8 / 2^(8 - bits)) / 2^bits - 0.5 + noise / 2^bits in float64 (preprocess_observation_)."""
    return (np.floor(u8.astype(np.float64) / 2.0 ** (8 - bit_depth)) / 2.0 ** bit_depth - 0.5 +
            noise.astype(np.float64) / 2.0 ** bit_depth)


def replay_draw(seed, step, b, lanes, n_valid):
    """Sequence b of one device sample call (replay.hip): counter (b, 0, 12, step) -> (lane, u), lane = x[0] lanes >> 32,
    u = (x[2] | x[3] << 32) n_valid >> 64."""
    x = philox([b, 0, REPLAY_STREAM, step & M32], key_of(seed))
    return (x[0] * lanes) >> 32, ((x[2] | x[3] << 32) * n_valid) >> 64


GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def engine_key(seed, rank=0):
    """Engine.set_noise_seed: ranks get distinct keys."""
    return (int(seed) + GOLDEN_GAMMA * (rank + 1)) & M64


# Engine.RNG_STREAMS, restated (the CPU test asserts the two are the same table)
RNG_STREAMS = {"obs_post": 1, "action": 2, "img_prior": 3, "entropy": 4, "obs_prior": 5, "plan_prior": 7, "act_post": 8,
               "act_action": 9, "act_explore": 10, "act_mode": 11}
# which counter is the `step` word of each stream.  "wm" / "bh": Engine._rng_step, one per train step and phase, both
# reset by set_noise_seed; "entropy": Engine._rng_entropy_step, the "bh" value of the same step; "act" / "plan": one per
# decision / plan; the replay buffer keeps its own two counters (one per pixel sample, one per device draw).
STEP_COUNTER = {"obs_post": "wm", "action": "bh", "img_prior": "bh", "entropy": "entropy", "obs_prior": None,
                "plan_prior": "plan", "act_post": "act", "act_action": "act", "act_explore": "act", "act_mode": "act"}


def train_step_fills(d, B):
    """The bd_rng_fill tensors of one perf-mode train step (Engine.make_noise): name -> (shape, kind, stream id).  The
    sampler of a Categorical latent or actor consumes Exp(1) variates, one per class; obs_prior is never drawn and the
    entropy draws are generated inside bd_actor_entropy_rng (rng_gather_index)."""
    lat = EXPONENTIAL if d.categorical else NORMAL
    act = EXPONENTIAL if d.discrete_actions else NORMAL
    N = d.T * B
    return {"obs_post": ((d.T, B, d.S), lat, RNG_STREAMS["obs_post"]),
            "action": ((d.Hm, N, d.A), act, RNG_STREAMS["action"]),
            "img_prior": ((d.Hm, N, d.S), lat, RNG_STREAMS["img_prior"])}


# ---- the inputs of tests/test_rng_values_gpu.py (the CPU test checks their teeth on exactly these) ---------------------------

FILL_SEED, FILL_STEP = 0x0123456789ABCDEF, 0x80000007          # (the step's top bit set: it is an unsigned word)
FILL_COUNTS = (1, 3, 1023, 1024, 1025, 4099)
FILL_STREAMS = (1, 2, 10, 3, 9, 9)          # the last two share a stream id (and a kind): one is a prefix of the other
FILL_OFFSETS = (0, 0, 0, 1, 0, 0)           # floats past a 16-byte boundary: tensor 3 takes the scalar stores throughout
_FILL_KINDS = (NORMAL, EXPONENTIAL, UNIFORM, NORMAL, EXPONENTIAL, EXPONENTIAL)
FILL_ROTATIONS = (0, 1, 2)                  # every tensor is filled with every kind


def fill_case(rotation):
    """[(count, kind, stream id), ...] of the six-tensor launch with the kinds rotated by `rotation`."""
    return [(c, (k + rotation) % 3, s) for c, k, s in zip(FILL_COUNTS, _FILL_KINDS, FILL_STREAMS)]


TOL = {UNIFORM: (0.0, 0.0), EXPONENTIAL: (1e-6, 1e-6), NORMAL: (4e-6, 1e-6)}      # (atol, rtol); uniform: bit-exact
KIND_NAMES = {NORMAL: "normal", EXPONENTIAL: "exponential", UNIFORM: "uniform"}

# Counters whose words hit the two ends of the 24-bit range: (step, quad, word, "ones" | "zeros"), all for seed
# FILL_SEED, stream EDGE_STREAM, inside a tensor of EDGE_COUNT elements.  test_rng_ref_cpu.py finds them again by search.
EDGE_STREAM, EDGE_COUNT = 3, 1024
EDGES = ((4378, 102, 1, "ones"), (46795, 135, 2, "ones"), (1515, 87, 3, "zeros"), (3993, 34, 0, "zeros"))


EDGE_TENSORS = [(EDGE_COUNT, k, EDGE_STREAM) for k in (NORMAL, EXPONENTIAL, UNIFORM)]     # one launch: every kind, same words


def worst_ratio(got, want, kind):
    """max |got - want| / (atol + rtol |want|) (uniform: 0 where the bits agree, inf elsewhere; NaN counts as inf)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    atol, rtol = TOL[kind]
    err = np.abs(got - want)
    if kind == UNIFORM:
        return float(np.where(err == 0.0, 0.0, np.inf).max())
    return float(np.nan_to_num(err / (atol + rtol * np.abs(want)), nan=np.inf).max())


# bd_replay_gather_pixels_rng cases: (n_idx, pixels) x bit_depth x step.  342 * 12288 / 4 quads exceed the 4096 * 256
# threads of the grid: the grid-stride loop takes a second pass (and the output is 16.8 MB).
PIXEL_SHAPES = ((1, 4), (5, 12), (342, 12288))
PIXEL_BITS = (1, 5, 8)
PIXEL_STEPS = (0, 2 ** 32 - 1)
PIXEL_SEED = 77
PIXEL_TOL = 4.0 * 2.0 ** -24
