"""TEST INFRASTRUCTURE: symlog / symexp (csrc/symlog.hip; DESIGN.md, "World-model heads on any scale") restated in
float64 -- the specification -- and again in float32 with numpy, the form whose error against float64 sets the kernels'
budget.

    symlog(x) = sign(x) log1p(|x|)        symexp(x) = sign(x) expm1(|x|)

with the sign taken by copysign: +-0 -> +-0, NaN -> NaN, +-inf -> +-inf.

``kernel_inputs(which)`` is the value set the kernel test runs (tests/test_symlog_kernels_gpu.py) and the set the
budgets are measured on (tests/test_symlog_ref_cpu.py): +-0, denormals, +-1e-30 .. +-3e38 in decades, the fp32
neighbours of +-1, NaN, +-inf; for symexp the magnitudes are capped so that the inputs span +-89 and overflow is in the
set (88.72 is the last listed finite result, 88.73 and 89 overflow).

Error budgets (the constants at the end): the largest relative error of the float32 restatement against the float64
one over ``kernel_inputs``, times 4 -- the project's rule (tests/twohot_ref.py).  ``python -m tests.symlog_ref`` prints the
measured values.
"""
from __future__ import annotations

import numpy as np


def symlog(x):
    x = np.asarray(x, dtype=np.float64)
    return np.copysign(np.log1p(np.abs(x)), x)


def symexp(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore"):
        return np.copysign(np.expm1(np.abs(x)), x)


def symlog32(x):
    x = np.asarray(x, dtype=np.float32)
    return np.copysign(np.log1p(np.abs(x)), x).astype(np.float32)


def symexp32(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore"):
        return np.copysign(np.expm1(np.abs(x)), x).astype(np.float32)


def to_float32(y64):
    """The float64 result as the float32 the kernel should write: beyond the fp32 range it is +-inf."""
    with np.errstate(over="ignore"):
        return np.asarray(y64, dtype=np.float64).astype(np.float32)


def kernel_inputs(which: str) -> np.ndarray:
    """The fp32 value set of the kernel tests, `which` = "symlog" | "symexp"; both signs of everything."""
    one = np.float32(1.0)
    pos = [0.0, 1.4e-45, 1e-42, 1e-39, 1.1754942e-38]                          # zero, denormals, the largest denormal
    pos += [float(np.nextafter(one, np.float32(0))), 1.0, float(np.nextafter(one, np.float32(2)))]
    if which == "symlog":
        pos += [10.0 ** e for e in range(-30, 39)] + [3e38, 3.4028235e38]
    else:
        pos += [10.0 ** e for e in range(-30, 2)] + [0.5, 2.0, 20.0, 50.0, 80.0, 88.0, 88.72, 88.73, 89.0]
    v = np.asarray(pos, dtype=np.float32)
    return np.concatenate([v, -v, np.asarray([np.nan, np.inf, -np.inf], dtype=np.float32)])


def rel_error(got, want64) -> float:
    """Largest |got - want| / |want| over the elements where want is finite and non-zero; elsewhere (zeros, NaN, inf,
    results beyond the fp32 range) `got` must equal the float32 of `want` exactly, else the error is inf."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    want32 = to_float32(want64).astype(np.float64)
    exact = ~np.isfinite(want32) | (want64 == 0)
    same = (got == want32) | (np.isnan(got) & np.isnan(want32))
    same &= np.signbit(got) == np.signbit(want32)
    if not same[exact].all():
        return float("inf")
    m = ~exact
    if not m.any():
        return 0.0
    return float((np.abs(got[m] - want64[m]) / np.abs(want64[m])).max())


def measure() -> dict:
    """The float32 restatement against float64 over the kernel test's own inputs."""
    xl, xe = kernel_inputs("symlog"), kernel_inputs("symexp")
    return {"symlog": rel_error(symlog32(xl), symlog(xl)), "symexp": rel_error(symexp32(xe), symexp(xe))}


# measured on the CPU (python -m tests.symlog_ref), times 4
SYMLOG_MEASURED = 4.937e-08          # under one fp32 rounding (2^-24 = 5.96e-08)
SYMEXP_MEASURED = 1.444e-07          # numpy's float32 expm1 at the large arguments: just over one ulp
SYMLOG_BUDGET = 4 * SYMLOG_MEASURED
SYMEXP_BUDGET = 4 * SYMEXP_MEASURED


if __name__ == "__main__":
    for k, v in measure().items():
        print(f"{k}: {v:.3e}")
