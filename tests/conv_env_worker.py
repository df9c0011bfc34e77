"""Child process of tests/test_conv_kernels_gpu.py: BD_CONV_PATCH (csrc/conv.hip) and BD_WGRAD_THIN (csrc/wgrad.hip) are
read once per process, so the forms they switch off run here, in a fresh process with the variable set by the parent.
  patch <file>   every PATCH case of tests/conv_ref.py on the gather form (BD_CONV_PATCH=0): each within the float64 bound,
                 and compared bit for bit with the patch-form outputs the parent saved to <file>
  wgrad          the 3-channel weight gradients on the staged-row bodies (BD_WGRAD_THIN=0)
Stops at the first failure (nonzero exit); prints CONV_ENV_RESULT {...} on success."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import _cabi as cabi  # noqa: E402
from tests import conv_ref as R  # noqa: E402

mode = sys.argv[1]
res = {"mode": mode, "env": {k: os.environ.get(k) for k in ("BD_CONV_PATCH", "BD_WGRAD_THIN")}, "worst": 0.0, "cases": 0}
if mode == "patch":
    assert os.environ.get("BD_CONV_PATCH") == "0"
    parent = torch.load(sys.argv[2])
    res["bit_equal"] = {}
    for name in R.PATCH:
        got, worst = R.gpu_patch_case(cabi, name)
        res["worst"] = max(res["worst"], worst)
        res["bit_equal"][name] = bool(torch.equal(got, parent[name]))
        res["cases"] += 1
else:
    assert mode == "wgrad" and os.environ.get("BD_WGRAD_THIN") == "0"
    res["bodies"] = {}
    for name, c in R.WGRAD.items():
        if not c.thin_env:
            worst, body = R.gpu_wgrad_case(cabi, name, False)
            assert body[0] == "staged", (name, body)
            res["worst"] = max(res["worst"], worst)
            res["bodies"][name] = sorted(body[1])
            res["cases"] += 1
print("CONV_ENV_RESULT " + json.dumps(res))
