"""Dense weight-gradient passes that run several rounds of short row units (csrc/wgrad.hip: bd_wgrad_plan's rule for
passes with no gathered operand, the dense body's prologue and float4 flush, the padded slab pitch and the float4 reduce)
against float64 (tests/dense_ref.py: C_TOL, NaN-filled slab workspace, sentinel-filled outputs, NaN input padding).

The pass is a set of actor / critic layers at the smallest row count at which the rule (restated in
tests/test_wgrad_units_cpu.py) takes a second round, moved off the multiples of 16 so that the last unit is ragged."""
import pytest
import torch

from tests import dense_ref as R
from tests import test_wgrad_units_cpu as U

pytestmark = pytest.mark.gpu

# N = 200 / 208 (8 / 0 pad columns of dpre), K = 200 / 230 (one tile / the two-tile K split: 7|6 x 4|3|2|1 shares), and
# the actor's 2-wide output layer: seven tiles
SET = [(200, 230), (208, 200), (200, 200), (208, 230), (2, 200)]
SHAPES = [(N, K, True) for N, K in SET]
M_16 = next(M for M in range(16, 1 << 20, 16) if U.rule(SHAPES, M)[0] > 1)
M_MIN = next(M for M in range(M_16 - 15, M_16 + 1) if U.rule(SHAPES, M)[0] > 1)     # first row count with a second round
M_PASS = M_MIN + (7 if (M_MIN + 7) % 16 else 8)
ROWS = U.rule(SHAPES, M_PASS)[1]


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def make(bias, M1s=None, seed0=0):
    M1s = M1s or {}
    return [R.WgradCase(M_PASS, N, K, M1=M1s.get(i), bias=bias, lda2_pad=8 if i % 2 else 4, seed=seed0 + i)
            for i, (N, K) in enumerate(SET)]


def run(cabi, cases):
    table, descs, ws = R.run_grouped(cabi, cases)
    return table, descs, ws


def test_the_pass_runs_several_rounds_of_ragged_units(cabi):
    assert M_PASS % 16 != 0 and M_PASS % ROWS != 0 and U.rule(SHAPES, M_PASS)[0] > 1
    cases = make(True)
    descs = (cabi.WgradDesc * len(cases))(*[c.desc(cabi) for c in cases])
    rc, tb, tr, wsf = R.wgrad_plan(cabi, descs)
    assert rc == 0 and tb > 256 and all(d.rows_per == ROWS for d in descs), (tb, [d.rows_per for d in descs], ROWS)


@pytest.mark.parametrize("bias", [True, False])
def test_units_against_float64(cabi, bias):
    """Bias on: K + 1 = 201 / 231 is no multiple of 4 (pad columns in every slab row); off: 200 is, 230 is not."""
    cases = make(bias)
    keep = run(cabi, cases)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        print(f"DENSE_WORST wgrad_units M={M_PASS},rows={ROWS},N={c.N},K={c.K},bias={bias} "
              f"{c.check(f'units bias={bias} entry {i}'):.3e}")
    first = [c.flat.clone() for c in cases]
    for c in cases:
        c.flat.fill_(R.SENTINEL)
    keep2 = run(cabi, cases)
    torch.cuda.synchronize()
    assert all(torch.equal(a, c.flat) for a, c in zip(first, cases)), "the same launch twice differs"
    del keep, keep2


def test_two_sources_split_inside_on_and_after_unit_boundaries(cabi):
    """M1 inside a unit and no multiple of 16, exactly on a unit boundary, and in the last unit."""
    last = (M_PASS - 1) // ROWS * ROWS
    M1s = {0: ROWS + 37, 1: 2 * ROWS, 2: last + 3, 3: M_PASS - 1}
    assert (ROWS + 37) % 16 != 0 and last < last + 3 < M_PASS
    cases = make(True, M1s, seed0=20)
    keep = run(cabi, cases)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        print(f"DENSE_WORST wgrad_units two sources M1={c.M1},N={c.N},K={c.K} {c.check(f'two sources entry {i}'):.3e}")
    del keep


def test_units_do_not_depend_on_where_or_when_they_run(cabi):
    """The same pass on a high-priority and on a normal-priority stream at once: each equals its solo run bit for bit."""
    a, b = make(True, seed0=40), make(True, seed0=40)
    solo = []
    for cases in (a, b):
        keep = run(cabi, cases)
        torch.cuda.synchronize()
        solo.append([c.flat.clone() for c in cases])
        for c in cases:
            c.flat.fill_(R.SENTINEL)
        del keep
    assert all(torch.equal(x, y) for x, y in zip(*solo))
    hi, lo = torch.cuda.Stream(priority=-1), torch.cuda.Stream(priority=0)
    torch.cuda.synchronize()
    with torch.cuda.stream(lo):
        keep_b = run(cabi, b)
    with torch.cuda.stream(hi):
        keep_a = run(cabi, a)
    torch.cuda.synchronize()
    for cases, want, name in ((a, solo[0], "high priority"), (b, solo[1], "normal priority")):
        assert all(torch.equal(w, c.flat) for w, c in zip(want, cases)), f"{name}: differs from its solo run"
    del keep_a, keep_b
