"""The replica fingerprint of include/bigdreamer_hip.h (bd_fingerprint), restated in numpy uint64 and, for checking that
restatement, as a plain-Python big-int loop.  For element i (0-based) with 32-bit pattern u, arithmetic mod 2^64:

    x = u64(u) ^ ((i + 1) * 0x9E3779B97F4A7C15)
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9
    x = (x ^ (x >> 27)) * 0x94D049BB133111EB
    x =  x ^ (x >> 31)
    hash      = sum of x
    nonfinite = number of i with (u & 0x7F800000) == 0x7F800000
"""
import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
M1 = 0xBF58476D1CE4E5B9
M2 = 0x94D049BB133111EB
MASK = (1 << 64) - 1
EXP = 0x7F800000


def bits(x) -> np.ndarray:
    """The 32-bit patterns of a float32 array (any shape), flattened."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).reshape(-1).view(np.uint32)


def fingerprint(x) -> tuple:
    """(hash, nonfinite) of a float32 array as Python ints; uint64 arithmetic wraps mod 2^64 as the definition asks."""
    u = bits(x)
    if u.size == 0:
        return 0, 0
    with np.errstate(over="ignore"):
        k = (np.arange(1, u.size + 1, dtype=np.uint64)) * np.uint64(GOLDEN)
        v = u.astype(np.uint64) ^ k
        v = (v ^ (v >> np.uint64(30))) * np.uint64(M1)
        v = (v ^ (v >> np.uint64(27))) * np.uint64(M2)
        v = v ^ (v >> np.uint64(31))
        h = int(np.add.reduce(v, dtype=np.uint64))
    return h, int(np.count_nonzero((u & np.uint32(EXP)) == np.uint32(EXP)))


def fingerprint_bigint(x) -> tuple:
    """The same by a loop over Python integers (no wrap-around semantics to trust but `& MASK`)."""
    h = nf = 0
    for i, u in enumerate(int(w) for w in bits(x)):
        v = u ^ (((i + 1) * GOLDEN) & MASK)
        v = ((v ^ (v >> 30)) * M1) & MASK
        v = ((v ^ (v >> 27)) * M2) & MASK
        v = v ^ (v >> 31)
        h = (h + v) & MASK
        nf += (u & EXP) == EXP
    return h, nf


def special_values(n: int, seed: int) -> np.ndarray:
    """n floats: normals mixed with NaNs of several payloads (quiet, signalling, negative), +-Inf, +-0 and denormals."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(n).astype(np.float32)
    pats = np.array([0x7FC00000, 0x7FC00001, 0x7F800001, 0xFFC12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
                     0x00000001, 0x807FFFFF, 0x00400000], dtype=np.uint32)
    if n:
        where = rng.choice(n, size=min(n, max(1, n // 3)), replace=False)
        x.view(np.uint32)[where] = pats[rng.randint(0, len(pats), size=where.size)]
    return x


def count_special(x) -> int:
    """Non-finite elements counted the floating-point way (not by the bit mask)."""
    return int(np.count_nonzero(~np.isfinite(np.asarray(x, dtype=np.float32))))
