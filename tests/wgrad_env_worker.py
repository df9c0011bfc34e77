"""Worker of test_dense_kernels_gpu.test_wgrad_env_paths: BD_WGRAD_WIDE / BD_WGRAD_ROWS are read once per process
(csrc/wgrad.hip, wgrad_wide / wgrad_rows), so the weight-gradient paths they select -- the 64 x 64-tile grouped kernel,
16-row splits, 48-row splits with a ragged last split -- run here, in a fresh process with the variable set.  Stops at
the first failure (nonzero exit); prints WGRAD_ENV_RESULT {"worst": ..., "cases": ...} on success."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import _cabi as cabi  # noqa: E402
from tests import dense_ref as R  # noqa: E402

worst, n = 0.0, 0
singles = [(M, N, K, kw) for M in (1, 17, 33, 2450 + 7) for N, K, kw in (
    (64, 1024, {}), (32, 1024, {"lda_pad": 1}), (128, 48, {"ldp_pad": 3}), (208, 255, {}), (209, 200, {}),
    (17, 230, {"act_off": 1}), (200, 17, {"w_off": 3, "ldw_pad": 1}))]
for M, N, K, kw in singles:
    for bias in (True, False):
        c = R.WgradCase(M, N, K, bias=bias, seed=M + N, **kw)
        keep = R.run_grouped(cabi, [c])
        torch.cuda.synchronize()
        worst = max(worst, c.check(f"M={M} N={N} K={K} bias={bias} {kw}"))
        n += 1
for M in (17, 2450):
    for M1 in (0, 1, M - 1):
        c = R.WgradCase(M, 200, 200, M1=M1, lda2_pad=8, seed=M1)
        keep = R.run_grouped(cabi, [c])
        torch.cuda.synchronize()
        worst = max(worst, c.check(f"two sources M={M} M1={M1}"))
        n += 1
for window in ("last16", "tail", "m1"):
    c = R.WgradCase(2450 + 7, 208, 200, M1=2450 if window == "m1" else None, seed=5, window=window)
    keep = R.run_grouped(cabi, [c])
    torch.cuda.synchronize()
    worst = max(worst, c.check(f"window {window}"))
    n += 1
cases = [R.WgradCase(2450, N, K, seed=i) for i, (N, K) in enumerate([(200, 230), (200, 200), (200, 200), (1, 200)])]
cases.append(R.WgradCase(2450, 48, 33, M1=800, lda2_pad=5, w_off=1, seed=9))
keep = R.run_grouped(cabi, cases)
torch.cuda.synchronize()
for i, c in enumerate(cases):
    worst = max(worst, c.check(f"mixed table entry {i}"))
    n += 1
first = [c.flat.clone() for c in cases]
for c in cases:
    c.flat.fill_(R.SENTINEL)
keep = R.run_grouped(cabi, cases, phase=1)
torch.cuda.synchronize()
assert all(torch.equal(a, c.flat) for a, c in zip(first, cases)), "phase 1 + phase 2 differs from phase 0"
print("WGRAD_ENV_RESULT " + json.dumps({"worst": worst, "cases": n,
                                        "env": {k: os.environ.get(k) for k in ("BD_WGRAD_WIDE", "BD_WGRAD_ROWS")}}))
