"""Worker of test_exact_math_twin_against_float64: runs in a fresh process whose BD_LIB points at the -DBD_EXACT_MATH build
(libm expm1f / log1pf / tanhf / expf in the activation epilogues) -- one observe shape on every form, one imagination
shape and the Categorical actor's cases scan_ref.DISCRETE_EXACT against the float64 step references with the libm-grade
allowances (scan_ref.EXACT), printing the worst err / bound ratio per tensor."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import _cabi  # noqa: E402
from tests import scan_ref as R  # noqa: E402
from tests import test_scan_kernels_gpu as T  # noqa: E402

assert "exact" in _cabi.LIB_PATH, _cabi.LIB_PATH
rep = dict(observe=T.run_observe_shape("ragged42", AL=R.EXACT, repeats=False),
           imagine=T.run_imagine_shape("ragged42", AL=R.EXACT, extras=False), discrete={}, ambiguous=0, draws=0)
for name, variant in R.DISCRETE_EXACT:
    rep["discrete"][f"{name}:{variant}"], (amb, n, _) = T.run_discrete_case(name, variant, AL=R.EXACT, extras=False)
    rep["ambiguous"] += amb
    rep["draws"] += n
print("SCAN_EXACT_RESULT " + json.dumps(rep))
