"""Is the dense-kernel test itself sharp?  (no GPU)

tests/dense_ref.py accepts a kernel value when |got - ref| <= C_TOL * sum|a*b| + allow.  Here a CPU emulation of the
kernels' arithmetic (fp32 fused multiply-adds in a fixed order per row split, then an fp32 sum of the split slabs; the
chain forward as a k-ordered fp32 fma chain plus bias and one-hot gather terms) must pass that check, and every planted
fault that drops, doubles or misplaces work in the same emulation must fail it.  The host-side argument checks of the
three entry points are exercised with argument sets they reject, so nothing is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_ref as R

F32, F64 = np.float32, np.float64


def _fma_rows(acc, a_col, b_row):
    """acc (f32) + outer(a, b) with one rounding per element: the fp32 MFMA / fma step."""
    return (acc.astype(F64) + np.outer(a_col.astype(F64), b_row.astype(F64))).astype(F32)


def emulate_wgrad(dpre, act1, act2, M1, rows_per, fault=None):
    """dW | db of wgrad_*_kernel: per row split an fp32 fma chain over the rows (act column K = the ones column of the
    bias), then the fixed-order fp32 sum of the slabs (wgrad_grouped_reduce_kernel)."""
    M, N = dpre.shape
    K = act1.shape[1]
    m1 = M1 + 1 if fault == "shift_m1" else M1
    act = np.concatenate([act1[:m1], act2[:M - m1]], 0) if m1 < M else act1[:M]
    act = np.concatenate([act, np.ones((M, 1), F32)], 1)
    if fault == "drop_last_col":
        act[:, K - 1] = 0.0
    last = M - 1 if fault == "drop_last_row" else M
    slabs = []
    for m0 in range(0, M, rows_per):
        acc = np.zeros((N, K + 1), F32)
        for m in range(m0, min(M, m0 + rows_per, last)):
            acc = _fma_rows(acc, dpre[m], act[m])
        slabs.append(acc)
    if fault == "double_split":
        slabs.append(slabs[len(slabs) // 2])
    s = np.zeros((N, K + 1), F32)
    for sl in slabs:
        s = (s + sl).astype(F32)
    return s[:, :K], s[:, K]


def emulate_forward(x, W, b, gWT, gidx, gC, act, fault=None):
    """One chain layer: a k-ordered fp32 fma chain, + bias, + the one-hot gather sum, then ELU (mlp_fwd_kernel)."""
    M, K = x.shape
    acc = np.zeros((M, W.shape[0]), F32)
    for k in range(K):
        acc = (acc.astype(F64) + np.outer(x[:, k], W[:, k]).astype(F64)).astype(F32)
    if fault != "omit_bias":
        acc = (acc + b[None, :]).astype(F32)
    gD = gidx.shape[1] - (1 if fault == "omit_gather_last" else 0)
    g = np.zeros_like(acc)
    for f in range(gD):
        g = (g + gWT[f * gC + gidx[:, f].astype(np.int64)]).astype(F32)
    acc = (acc + g).astype(F32)
    return np.where(acc > 0, acc, np.expm1(acc.astype(F64)).astype(F32)) if act else acc


def _wgrad_case(seed=0):
    rng = np.random.default_rng(seed)
    M, N, K, M1 = 2450, 9, 17, 1201
    dpre = rng.standard_normal((M, N)).astype(F32)
    act1 = rng.standard_normal((M, K)).astype(F32)
    act2 = rng.standard_normal((M - M1, K)).astype(F32)
    return dpre, act1, act2, M1


def _check_wgrad(dpre, act1, act2, M1, dW, db):
    act = torch.from_numpy(np.concatenate([act1[:M1], act2], 0))
    rW, sW, rb, sb = R.wgrad_ref(torch.from_numpy(dpre), act)
    R.check_close("dW", torch.from_numpy(dW), rW, sW)
    R.check_close("db", torch.from_numpy(db), rb, sb)


def test_wgrad_emulation_passes_the_tolerance():
    dpre, act1, act2, M1 = _wgrad_case()
    for rows_per in (64, 320, 2450):
        _check_wgrad(dpre, act1, act2, M1, *emulate_wgrad(dpre, act1, act2, M1, rows_per))


@pytest.mark.parametrize("fault", ["drop_last_row", "drop_last_col", "double_split", "shift_m1"])
def test_wgrad_planted_fault_fails_the_tolerance(fault):
    dpre, act1, act2, M1 = _wgrad_case(1)
    dW, db = emulate_wgrad(dpre, act1, act2, M1, 320, fault)
    with pytest.raises(AssertionError, match="out of tolerance"):
        _check_wgrad(dpre, act1, act2, M1, dW, db)


def _forward_case(seed=0):
    rng = np.random.default_rng(seed)
    M, K, N, gD, gC = 97, 230, 40, 9, 32
    x = rng.standard_normal((M, K)).astype(F32)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(F32)
    b = (0.5 * rng.standard_normal(N)).astype(F32)
    gWT = (0.3 * rng.standard_normal((gD * gC, N))).astype(F32)
    gidx = rng.integers(0, gC, (M, gD)).astype(np.uint8)
    return x, W, b, gWT, gidx, gC


def _check_forward(x, W, b, gWT, gidx, gC, got):
    t = torch.from_numpy
    ref, S, allow = R.linear_ref(t(x), t(W), t(b), True, R.gather_ref(t(gWT), t(gidx), gC))
    R.check_close("forward", t(got), ref, S, allow)


def test_forward_emulation_passes_the_tolerance():
    case = _forward_case()
    _check_forward(*case, emulate_forward(*case, act=True))


@pytest.mark.parametrize("fault", ["omit_bias", "omit_gather_last"])
def test_forward_planted_fault_fails_the_tolerance(fault):
    case = _forward_case(1)
    with pytest.raises(AssertionError, match="out of tolerance"):
        _check_forward(*case, emulate_forward(*case, act=True, fault=fault))


def test_check_close_rejects_nan():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    got = torch.zeros(3, 4)
    got[2, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"\(2, 1\)"):
        R.check_close("nan", got, ref, torch.ones_like(ref))


def test_dispatch_restatement_reaches_every_path():
    """The restated host dispatch (dense_ref.fwd_path / bwd_path / wgrad_body) on shapes the GPU tests use."""
    assert R.fwd_path(16400, [64, 64, 64, 1], 0) == "rt2"
    assert R.fwd_path(16400, [230, 200, 200, 200, 200, 1], 0) == "rt1"
    assert R.fwd_path(8197, [230, 200, 200, 200, 200, 1], -1) == "tall"
    assert R.fwd_path(1000, [230, 200, 200, 200, 200, 1], -1) == "rt1"
    assert R.fwd_path(17, [230, 1024, 200, 1], 0) == "rt1:biglds"
    assert R.fwd_path(8197, [200, 256, 256, 1], -1) == "rt1"         # 16 blocks: not a tall shape
    assert R.bwd_path(16400, [64, 64, 64, 1], 0) == "rt2"
    assert R.bwd_path(8197, [230, 200, 200, 200, 200, 1], -1) == "tall"
    assert R.wgrad_body(64, 1024, True, True, True) == {"deep"}
    assert R.wgrad_body(64, 1024, True, False, False) == {"narrow"}
    assert R.wgrad_body(128, 200, True, True, True) == {"mid"}
    assert R.wgrad_body(208, 200, True, True, True) == {"dense"}
    assert R.wgrad_body(200, 17, True, True, True) == {"general"}
    assert R.wgrad_body(209, 200, False, True, True) == {"mid"}


# ---- host checks: rejected without a launch --------------------------------------------------------------------------

_FAKE = 0x1000      # never dereferenced: every argument set below fails a host check before any launch


def _fwd_args(cabi, dims, M=1, gD=0, gC=0):
    a = cabi.MlpFwdArgs()
    a.M, a.in0, a.ld0, a.w0, a.in1, a.ld1, a.w1 = M, _FAKE, dims[0], dims[0], None, 0, 0
    a.n_layers = len(dims) - 1
    for l in range(a.n_layers):
        a.layer[l] = cabi.Layer(_FAKE, None, dims[l + 1], dims[l], cabi.ACT_ELU, None)
    a.out, a.ldo = _FAKE, dims[-1]
    a.gidx, a.gWT, a.gD, a.gC = (_FAKE if gD else None), (_FAKE if gD else None), gD, gC
    return a


def _rejected(cabi, rc, needle):
    err = cabi.lib.bd_last_error().decode()
    assert rc != 0 and needle in err, (rc, err)


def test_forward_host_checks_reject():
    from big_dreamer_amd import _cabi as cabi
    cabi.lib.bd_mlp_set_tall(0)
    try:
        # hidden width 1100: (69 + 69) x 16 x 16 floats of chain images + the split-K scratch > 160 KiB of LDS
        _rejected(cabi, cabi.lib.bd_mlp_forward(C.byref(_fwd_args(cabi, [16, 1100, 1100, 1])), None), "LDS")
        a = _fwd_args(cabi, [17, 32, 8])
        a.layer[1].K = 31
        _rejected(cabi, cabi.lib.bd_mlp_forward(C.byref(a), None), "layer 1 has K=31, expected 32")
        _rejected(cabi, cabi.lib.bd_mlp_forward(C.byref(_fwd_args(cabi, [17, 32, 8], gD=3, gC=257)), None), "gC <= 256")
        _rejected(cabi, cabi.lib.bd_mlp_forward(C.byref(_fwd_args(cabi, [17, 30, 8], gD=3, gC=5)), None), "N0 % 4")
    finally:
        cabi.lib.bd_mlp_set_tall(-1)


def test_backward_host_checks_reject():
    from big_dreamer_amd import _cabi as cabi
    cabi.lib.bd_mlp_set_tall(0)
    try:
        a = cabi.MlpBwdArgs()
        a.M, a.dout, a.lddo, a.dout_scale, a.n_layers = 1, _FAKE, 8, 1.0, 2
        a.layer[0] = cabi.LayerBwd(_FAKE, _FAKE, 32, 17, cabi.ACT_ELU, None)
        a.layer[1] = cabi.LayerBwd(_FAKE, None, 8, 31, cabi.ACT_NONE, None)
        _rejected(cabi, cabi.lib.bd_mlp_backward(C.byref(a), None), "layer 1 K mismatch")
        a.layer[1].K = 32
        a.din0, a.ld0, a.w0, a.din1, a.ld1, a.w1 = _FAKE, 17, 16, None, 0, 0
        _rejected(cabi, cabi.lib.bd_mlp_backward(C.byref(a), None), "din widths")
        a.din0 = None
        a.layer[0] = cabi.LayerBwd(_FAKE, None, 32, 17, cabi.ACT_ELU, None)
        _rejected(cabi, cabi.lib.bd_mlp_backward(C.byref(a), None), "needs its saved output")
        for l in range(3):      # 16 -> 1100 -> 1100 -> 1: the d(out) images of 1100-wide layers exceed 160 KiB
            a.layer[l] = cabi.LayerBwd(_FAKE, _FAKE, [1100, 1100, 1][l], [16, 1100, 1100][l], cabi.ACT_ELU, None)
        a.n_layers, a.lddo = 3, 1
        _rejected(cabi, cabi.lib.bd_mlp_backward(C.byref(a), None), "LDS")
    finally:
        cabi.lib.bd_mlp_set_tall(-1)


def test_wgrad_plan_host_checks_reject():
    from big_dreamer_amd import _cabi as cabi

    def desc(M, M1, act2):
        return cabi.WgradDesc(_FAKE, 8, _FAKE, 17, M1, act2, 17 if act2 else 0, M, 8, 17, _FAKE, 17, None)

    for d, needle in ((desc(40, 41, _FAKE), "malformed"), (desc(40, 39, None), "second activation source"),
                      (desc(40, -1, _FAKE), "malformed")):
        descs = (cabi.WgradDesc * 1)(d)
        rc = R.wgrad_plan(cabi, descs)[0]
        _rejected(cabi, rc, needle)
    d = desc(40, 40, None)
    d.ldw = 16
    _rejected(cabi, R.wgrad_plan(cabi, (cabi.WgradDesc * 1)(d))[0], "leading dimension")
    _rejected(cabi, cabi.lib.bd_wgrad(_FAKE, 8, _FAKE, 16, 40, 8, 17, _FAKE, 17, None, 0, _FAKE, 1 << 20, None),
              "leading dimension")
    _rejected(cabi, cabi.lib.bd_wgrad(_FAKE, 8, _FAKE, 17, 40, 8, 17, _FAKE, 17, None, 0, _FAKE, 1, None), "workspace")
