"""GPU: bd_symlog and bd_symexp (csrc/symlog.hip) on their own against the float64 restatement tests/symlog_ref.py within
the budgets measured there: every size at which the kernel splits the array differently (a dword head, a float4 body, a
dword tail), x and out at every offset of 0-3 floats from a 16-byte boundary (equal offsets: the vector path; unequal:
the dword path), guard elements on both sides of out, the special values, launch determinism and the refused arguments."""
import numpy as np
import pytest
import torch

from tests import symlog_ref as R

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 4099)
GUARD = 8
SENT = -7777.0
KERNELS = {"symlog": ("bd_symlog", R.symlog, R.SYMLOG_BUDGET), "symexp": ("bd_symexp", R.symexp, R.SYMEXP_BUDGET)}


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def _values(which, n):
    """n fp32 inputs: the value set of tests/symlog_ref.kernel_inputs, cycled, starting at another place per size."""
    v = R.kernel_inputs(which)
    return np.resize(np.roll(v, -(n % v.size)), n)


def _placed(host, off):
    """`host` on the device at `off` floats from a 256-byte-aligned base (torch's allocations are)."""
    base = torch.zeros(host.size + 4, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[off:off + host.size]
    view.copy_(torch.from_numpy(host))
    return base, view


def _out(n, off):
    base = torch.full((GUARD + 4 + n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    assert base.data_ptr() % 16 == 0
    lo = GUARD + off                      # GUARD = 8 floats keeps the 16-byte phase: out sits `off` floats past a boundary
    return base, base[lo:lo + n], lo


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_against_float64_at_every_size_and_alignment(cabi, which):
    name, ref, budget = KERNELS[which]
    fn, st = getattr(cabi.lib, name), cabi.stream()
    worst = 0.0
    for n in SIZES:
        host = _values(which, n)
        want = ref(host)
        for xo in range(4):
            for oo in range(4):
                _, x = _placed(host, xo)
                base, out, lo = _out(n, oo)
                assert x.data_ptr() % 16 == 4 * xo and out.data_ptr() % 16 == 4 * oo
                cabi.check(fn(x.data_ptr(), n, out.data_ptr(), st))
                got = base.cpu().numpy()
                assert (got[:lo] == SENT).all() and (got[lo + n:] == SENT).all(), (n, xo, oo, "guards")
                assert np.array_equal(x.cpu().numpy().view(np.uint32), host.view(np.uint32)), "the input was modified"
                err = R.rel_error(got[lo:lo + n], want)
                worst = max(worst, err)
                assert err <= budget, (which, n, xo, oo, err, budget)
    print(f"{name}: largest relative error {worst:.3e} (budget {budget:.3e})")


@pytest.mark.parametrize("which", sorted(KERNELS))
@pytest.mark.parametrize("xo,oo", [(1, 1), (0, 3)], ids=["vector_path", "dword_path"])
def test_grid_stride_beyond_the_block_cap(cabi, which, xo, oo):
    """n above 2048 workgroups x 256 threads x 4 elements: the grid is capped and both loops take their stride, more than
    once on the dword path.  Random inputs (symexp: within +-80), the same budget, guards on both sides."""
    name, ref, budget = KERNELS[which]
    n = 2 * 2048 * 256 * 4 + 4099
    rng = np.random.Generator(np.random.PCG64(n + xo))
    host = (rng.uniform(-80, 80, n) if which == "symexp" else rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    _, x = _placed(host, xo)
    base, out, lo = _out(n, oo)
    cabi.check(getattr(cabi.lib, name)(x.data_ptr(), n, out.data_ptr(), cabi.stream()))
    got = base.cpu().numpy()
    assert (got[:lo] == SENT).all() and (got[lo + n:] == SENT).all(), "guards"
    err = R.rel_error(got[lo:lo + n], ref(host))
    print(f"{name} n={n}: largest relative error {err:.3e} (budget {budget:.3e})")
    assert err <= budget, (which, err, budget)


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_special_values_and_oddness(cabi, which):
    name, _, _ = KERNELS[which]
    fn, st = getattr(cabi.lib, name), cabi.stream()
    v = R.kernel_inputs(which)
    x = torch.from_numpy(np.concatenate([v, -v])).cuda()
    out = torch.empty_like(x)
    cabi.check(fn(x.data_ptr(), x.numel(), out.data_ptr(), st))
    got = out.cpu().numpy()
    a, b = got[:v.size], got[v.size:]
    nan = np.isnan(v)
    assert np.isnan(a[nan]).all() and np.isnan(b[nan]).all()
    assert np.array_equal(a[~nan].view(np.uint32) ^ np.uint32(0x80000000), b[~nan].view(np.uint32)), "not odd bit for bit"
    zero = v == 0
    assert (a[zero] == 0).all() and np.array_equal(np.signbit(a[zero]), np.signbit(v[zero]))
    assert np.array_equal(a[np.isinf(v)], v[np.isinf(v)])
    if which == "symexp":       # overflow exactly where the float32 restatement overflows
        fin = np.isfinite(v)
        assert np.array_equal(np.isinf(a[fin]), np.isinf(R.symexp32(v[fin])))
        assert np.isinf(a[fin]).any()


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_two_launches_are_bit_identical(cabi, which):
    name, _, _ = KERNELS[which]
    fn, st = getattr(cabi.lib, name), cabi.stream()
    n = 4099
    _, x = _placed(_values(which, n), 1)
    outs = []
    for _ in range(2):
        _, out, _ = _out(n, 1)
        cabi.check(fn(x.data_ptr(), n, out.data_ptr(), st))
        outs.append(out.cpu().numpy().view(np.uint32))
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("which", sorted(KERNELS))
def test_refused_arguments(cabi, which):
    name, _, _ = KERNELS[which]
    fn, st = getattr(cabi.lib, name), cabi.stream()
    x = torch.ones(16, device="cuda")
    out = torch.full((16,), SENT, device="cuda")
    for args in ((None, 16, out.data_ptr()), (x.data_ptr(), 16, None), (x.data_ptr(), 0, out.data_ptr()),
                 (x.data_ptr(), 16, x.data_ptr())):
        assert fn(*args, st) != 0, args
        with pytest.raises(RuntimeError):
            cabi.check(fn(*args, st))
    torch.cuda.synchronize()
    assert (out == SENT).all() and (x == 1).all()           # nothing was enqueued
