"""GPU: the two-hot reward head and symlog observations in a data-parallel run -- two ranks on one GPU
(tests/wm_heads_dp_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_hold_identical_weights_after_two_steps():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29684", os.path.join(ROOT, "tests", "wm_heads_dp_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert "WM_HEADS_DP_OK world=2" in out.stdout
    print(out.stdout.strip().splitlines()[-1])
