"""GPU tests of cnn_activation_function = ReLU / Tanh: the forward epilogues of every conv kernel form, the fused and the
standalone derivative passes, the dense chains, and two whole train steps against the reference's own golden files.
Float64 references are computed on the CPU with plain torch.nn.functional calls."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as Fnn

from tests.cnn_act_ref import act64, act_grad_from_out64
from tests.dense_ref import ACT_ALLOW, C_TOL, check_close
from tests.test_conv_gpu import DEC, ENC, _close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ["ReLU", "Tanh"]


def _codes(act):
    from big_dreamer_amd import _cabi as cabi
    return cabi.CNN_ACTS[act]


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _saved(act, *shape, gen):
    """Saved outputs of `act` with both signs (ReLU: exact zeros where the pre-activation was negative)."""
    return act64(act, torch.randn(*shape, device="cuda", generator=gen).double()).float()


# ---- (a) forward epilogues per kernel form --------------------------------------------------------------------------

@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("imgs", [1, 5])
def test_thin_forward_epilogue(act, imgs):
    """conv_thin_f_kernel: Conv2d(3 -> 32, k4) on the 64 x 64 image."""
    from big_dreamer_amd import conv
    g = torch.Generator().manual_seed(100 + imgs)
    k = 4
    x = torch.randn(imgs, 3, 64, 64, generator=g)
    w = torch.randn(32, 3, k, k, generator=g) * 0.2
    b = torch.randn(32, generator=g)
    ref = act64(act, Fnn.conv2d(x.double(), w.double(), b.double(), stride=2))
    OH = conv.conv_out(64, k)
    ws = w.permute(0, 2, 3, 1).reshape(32, -1).contiguous().cuda()
    out = _nan(imgs, OH, OH, 32)
    conv.thin_f(conv.to_nhwc(x.cuda()), out, ws, b.cuda(), imgs, 64, 64, 3, k, _codes(act)[0])
    torch.cuda.synchronize()
    _close(out.permute(0, 3, 1, 2), ref)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin,Cout,k,size", ENC[1:])
def test_pattern_f_forward_epilogue(act, Cin, Cout, k, size):
    """Conv2d forward on the F pattern: the patch kernel (32 -> 64 on a 14-wide grid, C % 16 == 0) and the gather kernel
    (the two deeper layers, grids narrower than 12)."""
    from big_dreamer_amd import _cabi as cabi, conv
    g = torch.Generator().manual_seed(7)
    imgs = 5
    x = torch.randn(imgs, Cin, size, size, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    ref = act64(act, Fnn.conv2d(x.double(), w.double(), b.double(), stride=2))
    K = k * k * Cin
    wp = torch.zeros(cabi.packed_floats(Cout, K), device="cuda")
    conv.pack_matrix(w.permute(0, 2, 3, 1).contiguous().cuda().view(Cout, K), wp, Cout, K)
    OH = conv.conv_out(size, k)
    out = _nan(imgs, OH, OH, Cout)
    conv.pattern_f(conv.to_nhwc(x.cuda()), out, wp, b.cuda(), imgs, size, size, Cin, k, Cout, _codes(act)[0])
    torch.cuda.synchronize()
    _close(conv.to_nchw(out), ref)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin,Cout,k,size", DEC)
def test_fused_class_t_forward_epilogue(act, Cin, Cout, k, size):
    """ConvTranspose2d forward, four parity classes in one launch: gather kernel (5 x 5 and 30 x 30 inputs; the last has
    3 output channels) and patch kernel (64 -> 32 on the 15-wide class grid)."""
    from big_dreamer_amd import conv
    g = torch.Generator().manual_seed(8)
    imgs = 5
    x = torch.randn(imgs, Cin, size, size, generator=g)
    w = torch.randn(Cin, Cout, k, k, generator=g) * 0.1
    b = torch.randn(Cout, generator=g)
    ref = act64(act, Fnn.conv_transpose2d(x.double(), w.double(), b.double(), stride=2))
    fused = torch.zeros(conv.fused_pack_floats(Cin, Cout, k), device="cuda")
    conv.pack_fused(w.permute(0, 2, 3, 1).contiguous().cuda(), fused, Cin, Cout, k)
    OH = conv.convT_out(size, k)
    out = _nan(imgs, OH, OH, Cout)
    conv.pattern_t_fused(conv.to_nhwc(x.cuda()), out, fused, b.cuda(), imgs, size, size, Cin, k, Cout, OH, OH, _codes(act)[0])
    torch.cuda.synchronize()
    _close(conv.to_nchw(out), ref)


def test_conv_entry_points_reject_unknown_codes_and_missing_aux():
    from big_dreamer_amd import _cabi as cabi, conv
    x = torch.zeros(1, 64, 64, 3, device="cuda")
    ws = torch.zeros(32, 48, device="cuda")
    out = _nan(1, 31, 31, 32)
    for bad in (7, -1, 100):
        with pytest.raises(RuntimeError, match="unknown activation code"):
            conv.thin_f(x, out, ws, None, 1, 64, 64, 3, 4, bad)
        assert cabi.lib.bd_act_backward(cabi.ptr(out), cabi.ptr(out), out.numel(), bad, cabi.stream()) != 0
    for grad in cabi.GRAD_ACTS:
        rc = cabi.lib.bd_conv_thin_forward(cabi.ptr(x), 1, 64, 64, 3, 4, ws.data_ptr(), 48, None, grad, None, cabi.ptr(out),
                                           cabi.stream())
        assert rc != 0 and b"needs the saved outputs" in cabi.lib.bd_last_error()
    assert cabi.lib.bd_act_backward(cabi.ptr(out), cabi.ptr(out), out.numel(), cabi.ACT_NONE, cabi.stream()) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a rejected call wrote its output"


# ---- (b) fused against standalone backward --------------------------------------------------------------------------

@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("Cin,Cout,k,size", ENC[1:])
def test_fused_grad_epilogues_equal_dgrad_then_act_backward(act, Cin, Cout, k, size):
    """The _GRAD epilogue of the T pattern (fused classes) and of the F pattern = the plain dgrad followed by
    bd_act_backward, bit for bit (as tests/test_conv_gpu.py::test_dgrad_with_fused_elu_backward for ELU)."""
    from big_dreamer_amd import _cabi as cabi, conv
    fwd, grad = _codes(act)
    g = torch.Generator(device="cuda").manual_seed(11)
    imgs = 5
    w = torch.randn(Cout, Cin, k, k, device="cuda", generator=g) * 0.1
    stored = w.permute(0, 2, 3, 1).contiguous()
    OH = conv.conv_out(size, k)
    gys = torch.randn(imgs, OH, OH, Cout, device="cuda", generator=g)
    saved = _saved(act, imgs, size, size, Cin, gen=g)
    fused = torch.zeros(conv.fused_pack_floats(Cout, Cin, k), device="cuda")
    conv.pack_fused(stored, fused, Cout, Cin, k)
    plain = _nan(imgs, size, size, Cin)
    conv.pattern_t_fused(gys, plain, fused, None, imgs, OH, OH, Cout, k, Cin, size, size, cabi.ACT_NONE)
    cabi.check(cabi.lib.bd_act_backward(cabi.ptr(plain), cabi.ptr(saved), plain.numel(), fwd, cabi.stream()))
    got = _nan(imgs, size, size, Cin)
    conv.pattern_t_fused(gys, got, fused, None, imgs, OH, OH, Cout, k, Cin, size, size, grad, saved)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(plain).any()) and torch.equal(got, plain)
    HT = conv.convT_out(OH, k)
    Kt = k * k * Cin
    wp = torch.zeros(cabi.packed_floats(Cout, Kt), device="cuda")
    conv.pack_matrix(stored.view(Cout, Kt), wp, Cout, Kt)
    gyt = torch.randn(imgs, HT, HT, Cin, device="cuda", generator=g)
    saved2 = _saved(act, imgs, OH, OH, Cout, gen=g)
    plain2 = _nan(imgs, OH, OH, Cout)
    conv.pattern_f(gyt, plain2, wp, None, imgs, HT, HT, Cin, k, Cout, cabi.ACT_NONE)
    cabi.check(cabi.lib.bd_act_backward(cabi.ptr(plain2), cabi.ptr(saved2), plain2.numel(), grad, cabi.stream()))   # either code
    got2 = _nan(imgs, OH, OH, Cout)
    conv.pattern_f(gyt, got2, wp, None, imgs, HT, HT, Cin, k, Cout, grad, saved2)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(plain2).any()) and torch.equal(got2, plain2)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("imgs", [1, 5])
def test_thin_fused_grad_epilogue_equals_dgrad_then_act_backward(act, imgs):
    """The same for the thin kernel (dgrad of ConvTranspose2d(32 -> 3, k6): 64 x 64 x 3 gradient -> 30 x 30 x 32)."""
    from big_dreamer_amd import _cabi as cabi, conv
    fwd, grad = _codes(act)
    g = torch.Generator(device="cuda").manual_seed(imgs)
    k = 6
    x = torch.randn(imgs, 64, 64, 3, device="cuda", generator=g)
    ws = torch.randn(32, k * k * 3, device="cuda", generator=g) * 0.2
    OH = conv.conv_out(64, k)
    saved = _saved(act, imgs, OH, OH, 32, gen=g)
    plain = _nan(imgs, OH, OH, 32)
    conv.thin_f(x, plain, ws, None, imgs, 64, 64, 3, k, cabi.ACT_NONE)
    cabi.check(cabi.lib.bd_act_backward(cabi.ptr(plain), cabi.ptr(saved), plain.numel(), fwd, cabi.stream()))
    got = _nan(imgs, OH, OH, 32)
    conv.thin_f(x, got, ws, None, imgs, 64, 64, 3, k, grad, saved)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(plain).any()) and torch.equal(got, plain)


@pytest.mark.parametrize("act", ["ELU", "ReLU", "Tanh"])
def test_act_backward_against_float64(act):
    """g *= f'(y) from saved outputs of both signs (ReLU: exact zeros, which give exactly 0).  One fp32 product of g with
    a factor that is exact (ELU's 1, ReLU) or one or two roundings away (ELU's y + 1, Tanh's 1 - y^2): 4 ulp relative."""
    from big_dreamer_amd import _cabi as cabi
    gen = torch.Generator(device="cuda").manual_seed(5)
    n = 4 * 25013                                      # more than one block, a ragged last one
    y = _saved(act, n, gen=gen)
    g0 = torch.randn(n, device="cuda", generator=gen)
    assert bool((y > 0).any()) and bool((y <= 0).any())
    ref = g0.double() * act_grad_from_out64(act, y)
    g1 = g0.clone()
    cabi.check(cabi.lib.bd_act_backward(cabi.ptr(g1), cabi.ptr(y), n, _codes(act)[0], cabi.stream()))
    torch.cuda.synchronize()
    err = (g1.double() - ref).abs()
    assert bool((err <= 4 * 2.0 ** -24 * ref.abs() + 1e-37).all()), float(err.max())
    if act == "ReLU":
        assert int((y == 0).sum()) > n // 4 and bool((g1[y == 0] == 0).all()) and torch.equal(g1[y > 0], g0[y > 0])
    if act == "ELU":        # the exported ELU entry point is that case of the one kernel
        g2 = g0.clone()
        cabi.check(cabi.lib.bd_elu_backward(cabi.ptr(g2), cabi.ptr(y), n, cabi.stream()))
        torch.cuda.synchronize()
        assert torch.equal(g1, g2)


# ---- (c) dense chains -----------------------------------------------------------------------------------------------

def _chain_inputs(act, M, widths, seed):
    """Fixed-seed inputs; ReLU: drawn so that the float64 reference leaves at most 0.1 % of the pre-activations within the
    fp32 bound of 0 (checked on the float64 reference alone, before any kernel runs)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, widths[0], generator=g)
    Ws = [torch.randn(n, k, generator=g) / k ** 0.5 for k, n in zip(widths[:-1], widths[1:])]
    bs = [0.3 * torch.randn(n, generator=g) for n in widths[1:]]
    dout = torch.randn(M, widths[-1], generator=g)
    if act == "ReLU":
        h, near, total = x.double(), 0, 0
        for W, b in zip(Ws, bs):
            pre = h @ W.double().t() + b.double()
            S = h.abs() @ W.double().abs().t() + b.double().abs()
            near += int((pre.abs() <= C_TOL * S).sum())
            total += pre.numel()
            h = act64(act, pre)
        assert near <= 1e-3 * total, (near, total)
    return x, Ws, bs, dout


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("M,tall", [(50, False), (100, True)])
@pytest.mark.parametrize("widths", [(40, 68), (40, 68, 64, 12)])
def test_dense_chain_with_cnn_activation(act, M, tall, widths):
    """bd_mlp_forward / bd_mlp_backward with the new codes on every layer (the decoder's 1x1 -> 5x5 layer is a one-layer
    chain with an activation): M = 50 is the 16-row form with a ragged tile, M = 100 under bd_mlp_set_tall(2) the tall
    form.  Outputs, saved activations, dpre of every layer and din against float64, layer by layer from the kernel's own
    saved inputs, |err| <= C_TOL * sum|a*b| (+ ACT_ALLOW for the epilogue math), as tests/dense_ref.py states it.
    ReLU dpre: f' is taken from the float64 PRE-activation; elements whose pre-activation lies within the fp32 bound of 0
    are left out, at most 0.1 % of them."""
    from big_dreamer_amd import _cabi as cabi
    from big_dreamer_amd.categorical import _pack
    fwd = _codes(act)[0]
    x, Ws, bs, dout = _chain_inputs(act, M, widths, seed=len(widths) * 1000 + M)
    L = len(Ws)
    xd, Wd, bd_, doutd = x.cuda(), [W.cuda() for W in Ws], [b.cuda() for b in bs], dout.cuda()
    saves = [_nan(M, n) for n in widths[1:]]
    dpres = [_nan(M, n) for n in widths[1:]]
    out, din = _nan(M, widths[-1]), _nan(M, widths[0])
    pk = [_pack(W, False) for W in Wd]
    pkt = [_pack(W, True) for W in Wd]
    cabi.check(cabi.lib.bd_mlp_set_tall(2 if tall else 0))
    try:
        a = cabi.MlpFwdArgs()
        a.M, a.in0, a.ld0, a.w0 = M, cabi.ptr(xd), widths[0], widths[0]
        a.in1, a.ld1, a.w1 = None, 0, 0
        a.n_layers = L
        for l in range(L):
            a.layer[l] = cabi.Layer(cabi.ptr(pk[l]), cabi.ptr(bd_[l]), widths[l + 1], widths[l], fwd, cabi.ptr(saves[l]))
        a.out, a.ldo = cabi.ptr(out), widths[-1]
        cabi.check(cabi.lib.bd_mlp_forward(C.byref(a), cabi.stream()))
        b = cabi.MlpBwdArgs()
        b.M, b.dout, b.lddo, b.dout_scale = M, cabi.ptr(doutd), widths[-1], 1.0
        b.n_layers = L
        for l in range(L):
            b.layer[l] = cabi.LayerBwd(cabi.ptr(pkt[l]), cabi.ptr(saves[l]), widths[l + 1], widths[l], fwd, cabi.ptr(dpres[l]))
        b.din0, b.ld0, b.w0 = cabi.ptr(din), widths[0], widths[0]
        b.din1, b.ld1, b.w1 = None, 0, 0
        b.accumulate = 0
        cabi.check(cabi.lib.bd_mlp_backward(C.byref(b), cabi.stream()))
        torch.cuda.synchronize()
        # an unknown code is an error return, not ELU
        a.layer[0].act = 2
        assert cabi.lib.bd_mlp_forward(C.byref(a), cabi.stream()) != 0
        assert b"unknown activation code" in cabi.lib.bd_last_error()
        b.layer[L - 1].act = 9
        assert cabi.lib.bd_mlp_backward(C.byref(b), cabi.stream()) != 0
        assert b"unknown activation code" in cabi.lib.bd_last_error()
    finally:
        cabi.check(cabi.lib.bd_mlp_set_tall(-1))
    saves_c, dpres_c = [s.cpu() for s in saves], [p.cpu() for p in dpres]
    h, pres, bounds = x.double(), [], []
    for l in range(L):
        W64, b64 = Ws[l].double(), bs[l].double()
        pre = h @ W64.t() + b64
        S = h.abs() @ W64.abs().t() + b64.abs()
        check_close(f"save{l}", saves_c[l], act64(act, pre), S, ACT_ALLOW)
        pres.append(pre)
        bounds.append(C_TOL * S)
        h = saves_c[l].double()                      # the next layer's reference starts from what the kernel saved
    assert torch.equal(out.cpu(), saves_c[-1])
    left_out = total = 0
    dnext = dout.double()
    for l in range(L - 1, -1, -1):
        acc = dnext if l == L - 1 else dnext @ Ws[l + 1].double()
        S = torch.zeros_like(acc) if l == L - 1 else dnext.abs() @ Ws[l + 1].double().abs()
        if act == "ReLU":
            f = (pres[l] > 0).double()
            keep = pres[l].abs() > bounds[l]
        else:
            f = act_grad_from_out64(act, saves_c[l])
            keep = torch.ones_like(acc, dtype=torch.bool)
        left_out += int((~keep).sum())
        total += keep.numel()
        ref, got = acc * f, dpres_c[l].double()
        assert not bool(torch.isnan(got).any())
        bound = C_TOL * S * f.abs() + ACT_ALLOW * acc.abs() + 2.0 ** -23 * ref.abs()
        assert bool(((got - ref).abs() <= bound)[keep].all()), (l, float(((got - ref).abs() - bound)[keep].max()))
        dnext = got
    assert left_out <= 1e-3 * total, (left_out, total)
    check_close("din", din.cpu(), dnext @ Ws[0].double(), dnext.abs() @ Ws[0].double().abs())


# ---- (d) two whole train steps --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", ["0", "1"])
@pytest.mark.parametrize("act", ["ELU", "ReLU", "Tanh"])
def test_two_train_steps_vs_reference_golden(act, fuse):
    """Dreamer(cnn_activation_function=act) on TINY_PIXEL: logs, clipped gradients of every parameter tensor and post-Adam
    weights of two steps against the reference's golden file for that activation (ELU: the existing tiny_pixel.npz, through
    the same body), with the activation backward standalone and fused (BD_CONV_FUSE_ELU is read at import: a fresh child
    process per setting; tests/cnn_act_worker.py)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cnn_act_worker.py"), act], capture_output=True,
                         text=True, timeout=300, cwd=ROOT, env=dict(os.environ, BD_CONV_FUSE_ELU=fuse))
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "CNN_ACT_RESULT ok" in out.stdout and f"FUSE_ELU={fuse == '1'}" in out.stdout
