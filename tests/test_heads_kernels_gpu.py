"""bd_img_heads_fwd_bwd (csrc/heads.hip) end to end against a float64 reference (tests/heads_ref.py) through the C ABI,
at the shapes that select each path: every (per, left) column-block class of tall_sweep at the row-tile count heads_rt
picks, row counts around the 16- / 32-row tiles, both tile loaders, F < Hd, the > 64 KiB LDS launch up to the 160 KiB
boundary, one head at a time, the engine's binding and the -DBD_EXACT_MATH twin; and bd_pack_weights (csrc/cabi.hip) bit
for bit against the documented fragment layout.  Inputs are NaN-padded, every output sits in a sentinel-filled buffer
that must stay untouched outside it.  Each case prints its worst err / S (HEADS_WORST lines, visible under -s)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import heads_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- shape tables (tests/test_heads_ref_cpu.py checks that they reach every dispatch class) -------------------------------
WIDTH_M, WIDTH_F = 33, 52
# Nb = 1..15 column blocks, i.e. all fifteen (per, left) classes (144 is the only width here with nine blocks: per 2, left 1)
WIDTHS = [1, 3, 16, 17, 20, 30, 32, 33, 36, 48, 64, 80, 90, 112, 128, 144, 150, 176, 192, 200, 224, 225, 240]
ROW_SHAPES = [(230, 200), (58, 36)]                       # RT = 2, RT = 1
ROW_MS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000]
ROWS_BIG = (34307, 230, 200)                              # more workgroups than one round of the chip, ragged last tile
INPUT_M, INPUT_HDS = 33, [200, 36]
INPUT_FS = [1, 2, 7, 15, 16, 17, 39, 230, 231]
F_LT_HD = [(20, 64), (17, 240), (39, 200)]
BIG_LDS = [(600, 200), (1072, 200), (1100, 176), (2320, 240)]      # RT = 2 (the second: exactly 160 KiB), RT = 1 (ditto)
OVER_LDS = [(1073, 200), (2321, 240)]
ONE_HEAD = [(230, 200), (58, 36)]
EXACT_SHAPES = [(33, 230, 200), (33, 52, 30)]


def input_cases():
    """(F, Hd, off): every input width at both hidden widths, every even one also 4- but not 8-byte aligned, F < Hd."""
    cases = [(F, Hd, 0) for Hd in INPUT_HDS for F in INPUT_FS]
    cases += [(F, Hd, 1) for Hd in INPUT_HDS for F in INPUT_FS if F % 2 == 0]
    return cases + [(F, Hd, 0) for F, Hd in F_LT_HD]


def all_shapes():
    """(M, F, Hd, off) of every launch of the parametrised families below."""
    s = [(WIDTH_M, WIDTH_F, Hd, 0) for Hd in WIDTHS]
    s += [(M, F, Hd, 0) for F, Hd in ROW_SHAPES for M in ROW_MS] + [ROWS_BIG + (0,)]
    s += [(INPUT_M, F, Hd, off) for F, Hd, off in input_cases()]
    s += [(33, F, Hd, 0) for F, Hd in BIG_LDS + ONE_HEAD]
    return s


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def run_case(cabi, M, F, Hd, window=None, off=0, twice=False, family=""):
    """One launch into sentinel buffers, checked against float64; `twice`: a second launch into fresh buffers, same bits."""
    cls = R.heads_class(F, Hd, off)
    name = f"{family}:M={M},F={F},Hd={Hd},win={window},off={off},rt{cls[0]},per{cls[1]},left{cls[2]},{cls[3]}" \
           + (",F<Hd" if cls[4] else "") + (",biglds" if cls[5] else "")
    case = R.HeadsCase(M, F, Hd, seed=1000 * Hd + F + M, window=window, off=off)
    cabi.check(case.launch(cabi))
    worst = case.check(name)
    print(f"HEADS_WORST {name} {worst:.3e}")
    if window == "rows":
        assert not case.dx.view[:M - 1].any(), name
    if twice:
        first = case.outputs()
        case.fresh_outputs()
        cabi.check(case.launch(cabi))
        assert case.out_r.outside_unchanged() and case.out_v.outside_unchanged() and case.dx.outside_unchanged(), name
        for a, b in zip(first, case.outputs()):
            assert torch.equal(a, b), f"{name}: a second launch gave other bits"
    return worst


# ---- the fused kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [None, "hidden"])
@pytest.mark.parametrize("Hd", WIDTHS)
def test_widths(cabi, Hd, window):
    """Every (per, left) class of the Hd-wide sweeps, widths that are no multiple of 4 / of 16, one column."""
    run_case(cabi, WIDTH_M, WIDTH_F, Hd, window, twice=(Hd == WIDTHS[0] and window is None), family="widths")


@pytest.mark.parametrize("window", [None, "rows"])
@pytest.mark.parametrize("M", ROW_MS)
@pytest.mark.parametrize("F,Hd", ROW_SHAPES)
def test_rows(cabi, F, Hd, M, window):
    """Row counts around one and two tiles of either tile height, from a single row."""
    run_case(cabi, M, F, Hd, window, twice=((F, Hd) == ROW_SHAPES[0] and M == ROW_MS[0] and window is None), family="rows")


def test_rows_more_workgroups_than_one_round(cabi):
    run_case(cabi, *ROWS_BIG, family="rows")


@pytest.mark.parametrize("window", [None, "cols"])
@pytest.mark.parametrize("F,Hd,off", input_cases())
def test_input_widths_and_placement(cabi, F, Hd, off, window):
    """Input widths from one column, odd ones and a misaligned base (the scalar tile loader), F < Hd (img behind an
    Nb-block xim)."""
    run_case(cabi, INPUT_M, F, Hd, window, off, twice=((F, Hd, off) == input_cases()[0] and window is None), family="input")


@pytest.mark.parametrize("window", [None, "cols"])
@pytest.mark.parametrize("F,Hd", BIG_LDS)
def test_large_lds(cabi, F, Hd, window):
    """Dynamic LDS above 64 KiB for both instantiations, up to exactly 160 KiB."""
    assert R.heads_class(F, Hd)[5]
    run_case(cabi, 33, F, Hd, window, twice=((F, Hd) == BIG_LDS[0] and window is None), family="biglds")


@pytest.mark.parametrize("F,Hd", OVER_LDS)
def test_over_the_lds_limit_is_refused_without_a_launch(cabi, F, Hd):
    assert R.heads_lds(R.heads_rt(Hd), F, Hd) == R.MAX_LDS + R.heads_rt(Hd) * 1024
    case = R.HeadsCase(33, F, Hd, seed=F)
    assert case.launch(cabi) == -1 and b"LDS" in cabi.lib.bd_last_error()
    assert cabi.lib.bd_img_heads_supported(F, Hd) == 0
    for p in (case.out_r, case.out_v, case.dx):
        assert bool((p.buf == R.SENTINEL).all())


@pytest.mark.parametrize("window", ["head_r", "head_v"])
@pytest.mark.parametrize("F,Hd", ONE_HEAD)
def test_one_head_at_a_time(cabi, F, Hd, window):
    run_case(cabi, 33, F, Hd, window, twice=((F, Hd) == ONE_HEAD[0] and window == "head_r"), family="onehead")


# ---- the engine's binding ------------------------------------------------------------------------------------------------

def _engine_dims():
    from big_dreamer_amd import synth
    odd = synth.Dims(B=3, L=5, H=4, Be=24, S=7, Hd=20, E=40, A=2, O=5, n_entropy=100)      # Gaussian latents, F = 31
    return [("small", synth.SMALL), ("tiny", synth.TINY), ("cat_tiny", synth.CAT_TINY), ("tiny_odd_f", odd)]


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["small", "tiny", "cat_tiny", "tiny_odd_f"])
def test_engine_binding(cabi, which):
    """DreamerEngine.img_heads_fused on a row slice that starts at an odd row (with an odd F: a base that is not 8-byte
    aligned) against heads_ref built from the weights the engine holds.  The engine fuses the heads with Gaussian
    latents only; with Categorical ones (CAT_TINY, F = 39) the binding and its packed weights exist all the same."""
    from big_dreamer_amd import synth
    from big_dreamer_amd.engine import DreamerEngine
    name, d = _engine_dims()[which]
    eng = DreamerEngine(d, None, "cuda", params=synth.make_params(d, 7))
    F, Hd = d.Be + d.S, d.Hd
    assert bool(cabi.lib.bd_img_heads_supported(F, Hd))
    assert eng.heads_fused == (not d.categorical)
    M = d.Hm * d.N + 5
    g = torch.Generator(device="cuda").manual_seed(11)
    x = R.placed_input(torch.randn(M, F, device="cuda", generator=g), F, off=F)            # starts at row 1
    d_r = R.placed_input(torch.randn(M, 1, device="cuda", generator=g), 1, off=1)
    d_v = R.placed_input(torch.randn(M, 1, device="cuda", generator=g), 1, off=1)
    r_out, v_out, dx = R.Placed(M, 1, 1, off=1), R.Placed(M, 1, 1, off=1), R.Placed(M, F, F, off=F)
    eng.img_heads_fused(M, x.view, d_r.view[:, 0], d_v.view[:, 0], r_out.view[:, 0], v_out.view[:, 0], dx.view)
    torch.cuda.synchronize()
    heads = []
    for mod, dout in (("reward_model", d_r), ("critic_target", d_v)):
        heads.append(dict(W=[eng.W(mod, f"model.{2 * l}.weight") for l in range(R.HIDDEN)],
                          b=[eng.W(mod, f"model.{2 * l}.bias") for l in range(R.HIDDEN)],
                          w_out=eng.W(mod, f"model.{2 * R.HIDDEN}.weight"), b_out=eng.W(mod, f"model.{2 * R.HIDDEN}.bias"),
                          dout=dout.view[:, 0]))
    assert heads[0]["W"][0].shape == (Hd, F) and heads[0]["w_out"].shape == (1, Hd)
    for tag, p in (("r_out", r_out), ("v_out", v_out), ("dx", dx)):
        assert p.outside_unchanged(), f"{name}: wrote outside {tag}"
    (r, S_r), (v, S_v), (rdx, S_dx) = R.heads_ref(x.view, heads, M)
    worst = max(R.check_close(f"{name} r_out", r_out.view[:, 0], r, S_r, c=R.HEADS_C_TOL),
                R.check_close(f"{name} v_out", v_out.view[:, 0], v, S_v, c=R.HEADS_C_TOL),
                R.check_close(f"{name} dx", dx.view, rdx, S_dx, c=R.HEADS_C_TOL))
    print(f"HEADS_WORST engine:{name},M={M},F={F},Hd={Hd},{R.heads_class(F, Hd, F)[3]} {worst:.3e}")


# ---- the -DBD_EXACT_MATH twin, in a fresh process ------------------------------------------------------------------------

def test_exact_math_twin_against_float64():
    lib = os.path.join(ROOT, "big_dreamer_amd", "libbigdreamer_hip_exact.so")
    assert os.path.exists(lib), "build() makes the exact-math twin"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "heads_exact_worker.py")], cwd=ROOT,
                         env=dict(os.environ, BD_LIB=lib), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("HEADS_EXACT_RESULT ")]
    assert line, res.stdout[-2000:]
    rep = json.loads(line[-1][len("HEADS_EXACT_RESULT "):])
    assert len(rep) == len(EXACT_SHAPES), rep
    for name, worst in rep.items():
        print(f"HEADS_WORST exact:{name} {worst:.3e}")
        assert worst <= R.HEADS_C_TOL, rep


# ---- bd_pack_weights, bit for bit ----------------------------------------------------------------------------------------

PACK_SHAPES = [(1, 1), (15, 17), (16, 16), (17, 15), (200, 230), (230, 200), (1, 300)]


class PackCase:
    """A row-major (N, K) source with leading dimension ld inside a NaN-filled buffer, and a destination whose
    bd_packed_floats(N, K) floats are NaN (every one of them must be written) with SENTINEL behind them."""

    def __init__(self, cabi, N, K, ld_pad, transpose, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.W = torch.randn(N, K, device="cuda", generator=g)
        self.src = R.placed_input(self.W, K + ld_pad)
        self.n = int(cabi.lib.bd_packed_floats(N, K))
        assert self.n == R.cdiv(N, 16) * R.cdiv(K, 16) * 256
        self.dst = torch.full((self.n + 256,), R.SENTINEL, device="cuda")
        self.dst[:self.n] = float("nan")
        self.transpose = transpose
        self.desc = cabi.PackDesc(self.src.ptr, self.dst.data_ptr(), K + ld_pad, N, K, int(transpose))

    def check(self, name):
        assert torch.equal(self.dst[:self.n], R.pack_ref(self.W, self.transpose)), f"{name}: packed image differs"
        assert bool((self.dst[self.n:] == R.SENTINEL).all()), f"{name}: wrote past the packed image"


def _run_pack(cabi, cases):
    descs = (cabi.PackDesc * len(cases))(*[c.desc for c in cases])
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to("cuda")
    cabi.check(cabi.lib.bd_pack_weights(table.data_ptr(), len(cases), cabi.stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("ld_pad", [0, 3])
@pytest.mark.parametrize("N,K", PACK_SHAPES)
def test_pack_weights_bit_for_bit(cabi, N, K, ld_pad, transpose):
    """Ragged n and k, a padded leading dimension, both forms; 200 x 230 has more float4s than the grid has threads."""
    if (N, K) == (200, 230):
        assert R.cdiv(N, 16) * R.cdiv(K, 16) * 64 > 16 * 256
    c = PackCase(cabi, N, K, ld_pad, transpose, seed=N * 1000 + K)
    _run_pack(cabi, [c])
    c.check(f"pack N={N},K={K},ld={K + ld_pad},transpose={transpose}")


def test_pack_weights_three_descriptors_in_one_launch(cabi):
    cases = [PackCase(cabi, 200, 230, 3, True, 1), PackCase(cabi, 17, 15, 0, False, 2), PackCase(cabi, 1, 300, 1, True, 3)]
    _run_pack(cabi, cases)
    for i, c in enumerate(cases):
        c.check(f"pack descriptor {i}")
