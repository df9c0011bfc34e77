"""GPU: training diagnostics in a two-rank data-parallel run on one GPU over gloo (tests/diag_gpu_worker.py)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_one_reader_and_equal_module_norms():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", "29671", os.path.join(ROOT, "tests", "diag_gpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2500:] + out.stderr[-3000:]
    assert "DIAG_GPU_OK rank=0" in out.stdout and "DIAG_GPU_OK rank=1" in out.stdout, out.stdout[-2500:]
