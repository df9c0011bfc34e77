"""CPU: the replica check's host side -- bd_fingerprint's declaration and its refusals (made before anything is
enqueued, so they need no GPU), the three config keys, and DataParallel.agree / broadcast_ over gloo."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fingerprint_is_declared_and_exported():
    from big_dreamer_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    assert re.search(r"^int\s+bd_fingerprint\s*\(const bd_fingerprint_args\* a, unsigned long long\* out, void\* stream\);",
                     hdr, flags=re.M)
    assert "bd_fingerprint" in _cabi.EXPORTED and hasattr(_cabi.lib, "bd_fingerprint")
    m = re.search(r"#define BD_FP_MAX_BUFFERS (\d+)", hdr)
    assert m and int(m.group(1)) == _cabi.BD_FP_MAX_BUFFERS == 16
    # the struct as the header lays it out: int, then 16 x (pointer, size_t)
    assert C.sizeof(_cabi.FingerprintArgs) == 8 + 16 * 16
    assert _cabi.FingerprintArgs.buf.offset == 8 and C.sizeof(_cabi.FingerprintBuf) == 16
    assert "fingerprint.hip" in open(os.path.join(ROOT, "big_dreamer_amd", "csrc", "Makefile")).read()


def test_fingerprint_refuses_bad_arguments_before_any_launch():
    """Each refusal returns non-zero with its own message in bd_last_error: the message of a refusal, not of a failed
    memset or launch, so nothing was handed to the device (this test runs where there is none)."""
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    host = (C.c_float * 8)()                     # never read: every call below is refused first
    out = (C.c_ulonglong * 64)()
    p, o = C.addressof(host), C.addressof(out)

    def call(a, outp):
        rc = lib.bd_fingerprint(C.byref(a) if a is not None else None, outp, None)
        return rc, lib.bd_last_error().decode()

    a = _cabi.FingerprintArgs()
    a.n_buf = 17
    rc, msg = call(a, o)
    assert rc != 0 and "17 buffers" in msg and "max 16" in msg, msg
    a = _cabi.FingerprintArgs()
    a.n_buf = -1
    rc, msg = call(a, o)
    assert rc != 0 and "negative" in msg, msg
    a = _cabi.FingerprintArgs()
    a.n_buf = 3
    a.buf[0].p, a.buf[0].n = p, 8
    a.buf[1].p, a.buf[1].n = None, 0               # legal: empty
    a.buf[2].p, a.buf[2].n = None, 5               # not legal
    rc, msg = call(a, o)
    assert rc != 0 and "buffer 2 is null" in msg and "n = 5" in msg, msg
    a = _cabi.FingerprintArgs()
    a.n_buf = 1
    a.buf[0].p, a.buf[0].n = p, 8
    rc, msg = call(a, None)
    assert rc != 0 and "null output" in msg, msg
    rc, msg = call(None, o)
    assert rc != 0 and "null argument block" in msg, msg
    a.buf[0].p = p + 2
    rc, msg = call(a, o)
    assert rc != 0 and "4-byte aligned" in msg, msg
    for m in ("memset", "launch failed"):
        assert m not in msg.lower()
    assert all(v == 0 for v in out)


def test_replica_config_keys():
    from big_dreamer_amd.config import load_config
    cfg = load_config()
    assert cfg["replica_check_interval"] == 0 and isinstance(cfg["replica_check_interval"], int)
    assert cfg["replica_on_mismatch"] == "raise"
    assert cfg["replica_sync_at_start"] is False
    cfg = load_config(["replica_check_interval=100", "replica_on_mismatch=resync", "replica_sync_at_start=true"])
    assert (cfg["replica_check_interval"], cfg["replica_on_mismatch"], cfg["replica_sync_at_start"]) == (100, "resync", True)
    for bad in ("replica_check_interval=-1", "replica_check_interval=1.5", "replica_check_interval=often",
                "replica_check_interval=true", "replica_on_mismatch=ignore", "replica_on_mismatch=1",
                "replica_sync_at_start=1", "replica_sync_at_start=maybe"):
        with pytest.raises(ValueError):
            load_config([bad])


def test_engine_validates_the_same_options():
    from big_dreamer_amd.config import REPLICA_POLICIES, check_replica_options
    assert REPLICA_POLICIES == ("raise", "resync")
    assert check_replica_options(0, "raise") == (0, "raise") and check_replica_options(7, "resync") == (7, "resync")
    for bad in ((-1, "raise"), (1.5, "raise"), (True, "raise"), ("3", "raise"), (1, "repair"), (1, None)):
        with pytest.raises(ValueError):
            check_replica_options(*bad)


@pytest.mark.parametrize("world,port", [(2, 29651), (3, 29652)])
def test_agree_and_broadcast_over_gloo(world, port):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "tests", "replica_cpu_worker.py")]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert f"REPLICA_CPU_OK world={world}" in out.stdout


def test_agree_with_one_rank_needs_no_process_group():
    import torch
    from big_dreamer_amd.parallel import DataParallel
    dp = DataParallel()
    w = torch.tensor([-(1 << 63), -1, 5], dtype=torch.int64)
    assert dp.agree(w).tolist() == [True, True, True]
    assert dp.broadcast_(w) is w
