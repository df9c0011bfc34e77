"""Worker of test_heads_kernels_gpu.test_exact_math_twin_against_float64: runs in a fresh process whose BD_LIB points at
the -DBD_EXACT_MATH build (libm expm1f in the ELU epilogues) -- two shapes of bd_img_heads_fwd_bwd against the float64
reference under the same bound, printing the worst err / S per shape."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import _cabi  # noqa: E402
from tests import heads_ref as R  # noqa: E402
from tests import test_heads_kernels_gpu as T  # noqa: E402

assert "exact" in _cabi.LIB_PATH, _cabi.LIB_PATH
rep = {}
for M, F, Hd in T.EXACT_SHAPES:
    rep[f"M={M},F={F},Hd={Hd}"] = T.run_case(_cabi, M, F, Hd, family="exact")
print("HEADS_EXACT_RESULT " + json.dumps(rep))
