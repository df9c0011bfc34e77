"""Worker of test_scan_cat_kernels_gpu.test_exact_math_twin_against_float64: runs in a fresh process whose BD_LIB points at
the -DBD_EXACT_MATH build -- the observe shapes c32_d12 and c16_d20 on every form and the imagination shapes of the same
names, and the Categorical actor's cases scan_ref.DISCRETE_EXACT, against the float64 step references with the libm-grade
allowances (scan_ref.EXACT) and the libm sampler margin (C == 32 takes the exact branch of cat_sample_reg there), printing
the worst err / bound ratio per tensor; the actor's draws are counted with the factors."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import _cabi  # noqa: E402
from tests import scan_ref as R  # noqa: E402
from tests import test_scan_cat_kernels_gpu as T  # noqa: E402

assert "exact" in _cabi.LIB_PATH, _cabi.LIB_PATH
rep = dict(observe={}, imagine={}, discrete={}, ambiguous=0, factors=0)
for name in ("c32_d12", "c16_d20"):
    rep["observe"][name], (amb, n, _) = T.run_observe_shape(name, AL=R.EXACT, exact=True, repeats=False)
    rep["imagine"][name], (amb2, n2, _) = T.run_imagine_shape(name, AL=R.EXACT, exact=True)
    rep["ambiguous"] += amb + amb2
    rep["factors"] += n + n2
for name, variant in R.DISCRETE_EXACT:
    rep["discrete"][f"{name}:{variant}"], (amb, n), _ = T.run_discrete_case(name, variant, AL=R.EXACT, exact=True, extras=False)
    rep["ambiguous"] += amb
    rep["factors"] += n
print("SCAN_CAT_EXACT_RESULT " + json.dumps(rep))
