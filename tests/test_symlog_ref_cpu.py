"""CPU: the symlog / symexp specification (tests/symlog_ref.py) -- oddness, monotonicity, the round trip, special values --
and the measurement its kernel budgets rest on: the float32 restatement against float64 over the kernel test's own
inputs, recorded beside the budget constants."""
import numpy as np
import pytest

from tests import symlog_ref as R


def _grid():
    rng = np.random.Generator(np.random.PCG64(7))
    mag = 10.0 ** rng.uniform(-30, 30, size=4000)
    return np.sort(np.concatenate([mag, -mag, [0.0]]))


def test_odd_bit_for_bit():
    x = _grid()
    for f in (R.symlog, R.symexp):
        xs = x if f is R.symlog else np.clip(x, -700, 700)
        assert np.array_equal(f(-xs), -f(xs))
    x32 = R.kernel_inputs("symlog")
    fin = ~np.isnan(x32)
    assert np.array_equal(R.symlog32(-x32[fin]).view(np.uint32), (-R.symlog32(x32[fin])).view(np.uint32))
    xe = R.kernel_inputs("symexp")
    fin = ~np.isnan(xe)
    assert np.array_equal(R.symexp32(-xe[fin]).view(np.uint32), (-R.symexp32(xe[fin])).view(np.uint32))


def test_monotone():
    x = _grid()
    assert (np.diff(R.symlog(x)) > 0).all()
    xe = np.linspace(-700, 700, 5001)
    assert (np.diff(R.symexp(xe)) > 0).all()


def test_round_trip_float64():
    x = _grid()
    back = R.symexp(R.symlog(x))
    nz = x != 0
    # log1p then expm1: each within an ulp or two of float64, the second amplifying the first's error by |symlog x| <= 70
    assert (np.abs(back[nz] - x[nz]) <= 1e-13 * np.abs(x[nz])).all()
    assert back[~nz][0] == 0.0
    y = np.linspace(-80, 80, 3201)
    assert np.abs(R.symlog(R.symexp(y)) - y).max() <= 1e-13


def test_special_values():
    for f in (R.symlog, R.symexp, R.symlog32, R.symexp32):
        out = f(np.asarray([0.0, -0.0, np.nan, np.inf, -np.inf]))
        assert out[0] == 0 and not np.signbit(out[0])
        assert out[1] == 0 and np.signbit(out[1])
        assert np.isnan(out[2]) and out[3] == np.inf and out[4] == -np.inf
    assert R.symlog(1.0) == pytest.approx(np.log(2.0), rel=1e-15)
    assert R.symexp(np.log(2.0)) == pytest.approx(1.0, rel=1e-15)
    tiny = np.float32(1e-42)          # a denormal: symlog and symexp are the identity to fp32 precision
    assert R.symlog32(tiny) == tiny and R.symexp32(-tiny) == -tiny
    # overflow in fp32: 88.72 is finite, 88.73 is not
    assert np.isfinite(R.symexp32(np.float32(88.72))) and R.symexp32(np.float32(88.73)) == np.inf
    assert R.symexp32(np.float32(-89.0)) == -np.inf
    assert R.to_float32(R.symexp(np.float32(88.73))) == np.inf and np.isfinite(R.to_float32(R.symexp(np.float32(88.72))))


def test_kernel_inputs_hold_what_the_kernel_test_promises():
    for which in ("symlog", "symexp"):
        x = R.kernel_inputs(which)
        assert x.dtype == np.float32 and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
        assert (x == 0).sum() == 2 and np.signbit(x[x == 0]).sum() == 1
        fin = x[np.isfinite(x) & (x != 0)]
        assert (np.abs(fin) < 1.1754944e-38).any()                         # denormals
        assert np.float32(1e-30) in fin and -np.float32(1e-30) in fin
        one = np.float32(1)
        for nb in (np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2))):
            assert nb in fin and -nb in fin
    assert np.float32(3e38) in R.kernel_inputs("symlog")
    xe = R.kernel_inputs("symexp")
    assert np.abs(xe[np.isfinite(xe)]).max() == 89.0 and np.isinf(R.symexp32(xe[np.isfinite(xe)])).any()


def test_measured_float32_error_is_what_the_budgets_record():
    """The float32 restatement against float64 over the kernel test's inputs.  The constants in tests/symlog_ref.py
    record this measurement and the kernel budgets are four times it.  numpy's float32 log1p / expm1 come from the
    host's math library, whose last bit may differ between builds: the measurement must agree with the record to a
    factor of two and stay inside the budget it sets."""
    m = R.measure()
    print(f"symlog32 vs float64: {m['symlog']:.3e}   symexp32 vs float64: {m['symexp']:.3e}")
    assert np.isfinite(m["symlog"]) and np.isfinite(m["symexp"])           # zeros, NaN, inf, overflow: exact
    for got, rec, budget in ((m["symlog"], R.SYMLOG_MEASURED, R.SYMLOG_BUDGET), (m["symexp"], R.SYMEXP_MEASURED, R.SYMEXP_BUDGET)):
        assert rec / 2 <= got <= 2 * rec and got <= budget, (got, rec)
        assert budget == 4 * rec
