"""bd_mlp_forward / bd_mlp_backward (csrc/mlp.hip) and bd_wgrad_grouped / bd_wgrad (csrc/wgrad.hip) against float64
references (tests/dense_ref.py), layer by layer, at the shapes and placements that select each dispatch path: 16- and
32-row chain kernels, the tall form, the >64 KiB LDS launch, split-K, scalar / vector stores, the one-hot gather; the
dense, narrow, deep, mid and general bodies of the wide weight-gradient kernel, 16-byte / dword LDS-DMA, the bias column,
two activation sources and ragged row splits.  Every output sits in a sentinel-filled buffer that must stay untouched
outside it; input padding is NaN.  Each case prints its worst err / sum|a*b| (DENSE_WORST lines, visible under -s).
The environment-selected weight-gradient paths run in tests/wgrad_env_worker.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import dense_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def _report(entry, case, worst):
    print(f"DENSE_WORST {entry} {case} {worst:.3e}")


# ---- forward -----------------------------------------------------------------------------------------------------------

def run_forward(cabi, M, dims, w0=None, acts=None, bias=True, gD=0, gC=0, ldo_pad=0, save_off=0, in_off=0, tall=-1,
                seed=0, window=None, last_save=False, pads=(3, 5)):
    """One bd_mlp_forward launch; returns (worst ratio, outputs) after checking every layer against a float64 reference
    built from the kernel's own saved input of that layer."""
    L, K0 = len(dims) - 1, dims[0]
    w0 = K0 if w0 is None else w0
    w1 = K0 - w0
    acts = acts if acts is not None else [True] * (L - 1) + [False]
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(M, K0, device="cuda", generator=g)
    if window == "rows":
        x[:M - (M % 16 or 1)] = 0.0
    elif window == "cols":
        x[:, :K0 - (K0 % 16 or 1)] = 0.0
    in0 = R.placed_input(x[:, :w0], w0 + pads[0], in_off)
    in1 = R.placed_input(x[:, w0:], w1 + pads[1], in_off) if w1 else None
    Ws = [torch.randn(dims[l + 1], dims[l], device="cuda", generator=g) / dims[l] ** 0.5 for l in range(L)]
    bs = [0.5 * torch.randn(dims[l + 1], device="cuda", generator=g) if bias else None for l in range(L)]
    packed = [R.pack(W, False) for W in Ws]
    gWT = gidx = None
    if gD:
        gWT = 0.3 * torch.randn(gD * gC, dims[1], device="cuda", generator=g)
        gidx = torch.randint(0, gC, (M, gD), device="cuda", generator=g).to(torch.uint8)
        if window == "gather":      # only the last factor's row is nonzero: a dropped tail factor is an O(1) error
            gWT[:(gD - 1) * gC] = 0.0
    saves = [R.Placed(M, dims[l + 1], dims[l + 1], save_off) for l in range(L - 1)]
    saves.append(R.Placed(M, dims[-1], dims[-1], save_off) if last_save else None)
    out = R.Placed(M, dims[-1], dims[-1] + ldo_pad)
    a = cabi.MlpFwdArgs()
    a.M, a.in0, a.ld0, a.w0 = M, in0.ptr, in0.ld, w0
    a.in1, a.ld1, a.w1 = (in1.ptr, in1.ld, w1) if in1 else (None, 0, 0)
    a.n_layers = L
    for l in range(L):
        a.layer[l] = cabi.Layer(packed[l].data_ptr(), bs[l].data_ptr() if bias else None, dims[l + 1], dims[l],
                                cabi.ACT_ELU if acts[l] else cabi.ACT_NONE, saves[l].ptr if saves[l] else None)
    a.out, a.ldo = out.ptr, out.ld
    a.gidx, a.gWT, a.gD, a.gC = (gidx.data_ptr(), gWT.data_ptr(), gD, gC) if gD else (None, None, 0, 0)
    cabi.lib.bd_mlp_set_tall(tall)
    try:
        cabi.check(cabi.lib.bd_mlp_forward(C.byref(a), cabi.stream()))
    finally:
        cabi.lib.bd_mlp_set_tall(-1)
    torch.cuda.synchronize()
    for i, p in enumerate(saves + [out]):
        assert p is None or p.outside_unchanged(), f"forward wrote outside buffer {i}"
    worst = 0.0
    for l in range(L):
        xin = x if l == 0 else saves[l - 1].view
        extra = R.gather_ref(gWT, gidx, gC) if (l == 0 and gD) else None
        ref, S, allow = R.linear_ref(xin, Ws[l], bs[l], acts[l], extra)
        got = out.view if l == L - 1 else saves[l].view
        worst = max(worst, R.check_close(f"forward layer {l} (M={M}, dims={dims})", got, ref, S, allow))
    if last_save:
        assert torch.equal(saves[-1].view, out.view)
    return worst, out.view.clone()


ENGINE = [230, 200, 200, 200, 200, 1]          # DenseModel: 4 x (Linear + ELU) + Linear


@pytest.mark.parametrize("tall", [-1, 0, 2])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 47, 48, 49, 1000, 8192 + 5, 16400])
def test_forward_rows(cabi, M, tall):
    """Row counts around the 16- / 48-row tiles and the tall / RT = 2 thresholds; the engine chain on [in0 | in1]."""
    w = run_forward(cabi, M, ENGINE, w0=200, tall=tall, seed=M)[0]
    _report("fwd", f"M={M},tall={tall},{R.fwd_path(M, ENGINE, tall)}", w)
    if M == 16400 and tall == 0:      # narrow chain: the only shapes that reach mlp_fwd_kernel<2>
        dims = [64, 64, 64, 16]
        assert R.fwd_path(M, dims, 0) == "rt2"
        _report("fwd", "M=16400,rt2", run_forward(cabi, M, dims, w0=30, tall=0, seed=3)[0])


@pytest.mark.parametrize("N", [1, 2, 16, 17, 32, 33, 64, 200, 240, 256])
@pytest.mark.parametrize("M", [49, 8192 + 5])
def test_forward_widths(cabi, M, N):
    """Every width as a hidden and as the output layer; N <= 32 runs split-K, 4 | N tall-eligible shapes take the tall
    form at 8197 rows, 240 / 256 fall back to the 16-row form."""
    dims = [33, N, N, 5] if N % 4 else [36, N, N]
    w = run_forward(cabi, M, dims, w0=16, seed=N, ldo_pad=1)[0]
    _report("fwd", f"M={M},N={N},{R.fwd_path(M, dims, -1)}", w)


@pytest.mark.parametrize("K", [1, 3, 17, 230, 1024])
def test_forward_input_widths(cabi, K):
    """Input widths from 1 to 1024; a 1024-wide hidden layer needs more than 64 KiB of LDS."""
    w = run_forward(cabi, 17, [K, 40, 3], seed=K)[0]
    _report("fwd", f"K={K}", w)
    if K == 1024:
        for M, tall in ((17, -1), (8192 + 5, -1), (16400, 0)):
            dims = [230, 1024, 200, 1]
            assert R.fwd_path(M, dims, tall).endswith(":biglds") or R.fwd_path(M, dims, tall) == "tall"
            _report("fwd", f"K=1024,M={M},{R.fwd_path(M, dims, tall)}",
                    run_forward(cabi, M, dims, w0=200, tall=tall, seed=M)[0])


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("bias", [True, False])
def test_forward_depths(cabi, L, bias):
    dims = [30] + [48] * (L - 1) + [12]
    for M, tall in ((33, -1), (200, 2)):
        w = run_forward(cabi, M, dims, w0=7, bias=bias, tall=tall, seed=L, last_save=True, acts=[True] * L)[0]
        _report("fwd", f"L={L},bias={bias},M={M},{R.fwd_path(M, dims, tall)}", w)


@pytest.mark.parametrize("w0", [1, 7, 16, 30])
@pytest.mark.parametrize("tall", [-1, 0])
def test_forward_split_input(cabi, w0, tall):
    """[in0 | in1] with ld > w (odd and even leading dimensions: the pair and the scalar tile loaders), and in0 alone."""
    for pads in ((3, 5), (2, 4)):
        w = run_forward(cabi, 8192 + 5, [30, 64, 48, 8], w0=w0, tall=tall, seed=w0, pads=pads)[0]
        _report("fwd", f"w0={w0},tall={tall},pads={pads}", w)
    _report("fwd", f"in0only,tall={tall}", run_forward(cabi, 8192 + 5, [w0, 64, 8], tall=tall, seed=9)[0])


@pytest.mark.parametrize("gD", [1, 3, 8, 9, 32])
@pytest.mark.parametrize("gC", [5, 32, 256])
def test_forward_one_hot(cabi, gD, gC):
    """The one-hot segment of layer 0 (gD % 8 != 0: the tail loop), with and without [in0 | in1], one layer (which the
    tall form refuses) and the tall form."""
    for M, dims, w0, L1 in ((49, [40, 64, 32, 4], 17, False), (8192 + 5, [40, 64, 32, 4], None, False),
                            (33, [12, 20], None, True), (8192 + 5, [12, 20], None, True)):
        w = run_forward(cabi, M, dims, w0=w0, gD=gD, gC=gC, seed=gD * gC + M)[0]
        _report("fwd", f"gD={gD},gC={gC},M={M},L={len(dims) - 1},{R.fwd_path(M, dims, -1, gD)}", w)


@pytest.mark.parametrize("ldo_pad", [0, 1, 3])
@pytest.mark.parametrize("save_off", [0, 1, 3])
def test_forward_store_paths(cabi, ldo_pad, save_off):
    """ldo in {N, N+1, N+3} and saves at float offsets 1 / 3: the scalar store path (and no tall form)."""
    for M in (47, 8192 + 5):
        w = run_forward(cabi, M, [24, 32, 64, 16], ldo_pad=ldo_pad, save_off=save_off, seed=ldo_pad, last_save=True)[0]
        _report("fwd", f"ldo+{ldo_pad},save_off={save_off},M={M}", w)


@pytest.mark.parametrize("window", ["rows", "cols", "gather"])
@pytest.mark.parametrize("M,tall", [(47, 0), (8192 + 5, -1), (16400, 0)])
def test_forward_windows(cabi, window, M, tall):
    """Inputs zero outside one window (last M % 16 rows, last K % 16 columns, the last gather factor)."""
    dims, gD = ([44, 64, 8], 9) if window == "gather" else ([230, 200, 40, 3], 0)
    w = run_forward(cabi, M, dims, w0=None if gD else 200, bias=False, gD=gD, gC=5 if gD else 0, tall=tall, seed=7,
                    window=window)[0]
    _report("fwd", f"window={window},M={M},tall={tall}", w)


def test_forward_run_to_run(cabi):
    for M, tall in ((1000, -1), (8192 + 5, -1), (16400, 0)):
        a = run_forward(cabi, M, ENGINE, w0=200, tall=tall, seed=5)[1]
        b = run_forward(cabi, M, ENGINE, w0=200, tall=tall, seed=5)[1]
        assert torch.equal(a, b), M


# ---- backward ----------------------------------------------------------------------------------------------------------

def run_backward(cabi, M, dims, w0=None, acts=None, scale=1.0, accumulate=0, din1_null=False, off=0, din_off=0, tall=-1,
                 seed=0, want_din=True, dout_pad=3, window=None):
    L, K0 = len(dims) - 1, dims[0]
    w0 = K0 if w0 is None else w0
    w1 = K0 - w0
    acts = acts if acts is not None else [True] * (L - 1) + [False]
    g = torch.Generator(device="cuda").manual_seed(seed)
    Ws = [torch.randn(dims[l + 1], dims[l], device="cuda", generator=g) / dims[l + 1] ** 0.5 for l in range(L)]
    wts = [R.pack(Ws[l], True) if (l > 0 or want_din) else None for l in range(L)]
    saved = [R.placed_input(torch.nn.functional.elu(torch.randn(M, dims[l + 1], device="cuda", generator=g)), dims[l + 1],
                            off) if acts[l] else None for l in range(L)]
    dout = torch.randn(M, dims[-1], device="cuda", generator=g)
    if window == "rows":
        dout[:M - (M % 16 or 1)] = 0.0
    dout_p = R.placed_input(dout, dims[-1] + dout_pad)
    dpre = [R.Placed(M, dims[l + 1], dims[l + 1], off) for l in range(L)]
    din = R.Placed(M, K0, K0 + 2, din_off)
    prior = torch.randn(M, K0, device="cuda", generator=g)
    if accumulate or din1_null:
        din.view.copy_(prior)
    a = cabi.MlpBwdArgs()
    a.M, a.dout, a.lddo, a.dout_scale, a.n_layers = M, dout_p.ptr, dout_p.ld, scale, L
    for l in range(L):
        a.layer[l] = cabi.LayerBwd(wts[l].data_ptr() if wts[l] is not None else None, saved[l].ptr if saved[l] else None,
                                   dims[l + 1], dims[l], cabi.ACT_ELU if acts[l] else cabi.ACT_NONE, dpre[l].ptr)
    if want_din:
        a.din0, a.ld0, a.w0 = din.ptr, din.ld, w0
        a.din1, a.ld1, a.w1 = (None if din1_null else din.ptr + 4 * w0), din.ld, w1
    a.accumulate = accumulate
    cabi.lib.bd_mlp_set_tall(tall)
    try:
        cabi.check(cabi.lib.bd_mlp_backward(C.byref(a), cabi.stream()))
    finally:
        cabi.lib.bd_mlp_set_tall(-1)
    torch.cuda.synchronize()
    for i, p in enumerate(dpre + [din]):
        assert p.outside_unchanged(), f"backward wrote outside buffer {i}"
    tag = f"(M={M}, dims={dims})"
    s32 = torch.tensor(scale, dtype=torch.float32).double()
    d = dout.double() * s32
    if acts[-1]:
        f = R.elu_grad_from_out64(saved[-1].view)
        ref, S, allow = d * f, d.abs() * f, R.ACT_ALLOW * d.abs()
    else:
        ref, S, allow = d, d.abs(), 0.0
    worst = R.check_close(f"dpre layer {L - 1} {tag}", dpre[-1].view, ref, S, allow)
    for l in range(L - 1, 0, -1):
        ref, S, allow = R.dgrad_ref(dpre[l].view, Ws[l], saved[l - 1].view if acts[l - 1] else None, acts[l - 1])
        worst = max(worst, R.check_close(f"dpre layer {l - 1} {tag}", dpre[l - 1].view, ref, S, allow))
    if want_din:
        ref, S, _ = R.dgrad_ref(dpre[0].view, Ws[0])
        if accumulate:
            ref, S = ref + prior.double(), S + prior.double().abs()
        cols = w0 if din1_null else K0
        worst = max(worst, R.check_close(f"din {tag}", din.view[:, :cols], ref[:, :cols], S[:, :cols]))
        if din1_null:
            assert torch.equal(din.view[:, w0:], prior[:, w0:]), "din1 = NULL: its columns were written"
    else:
        assert torch.equal(din.buf, torch.full_like(din.buf, R.SENTINEL))
    return worst, [p.view.clone() for p in dpre] + [din.view.clone()]


@pytest.mark.parametrize("tall", [-1, 0, 2])
@pytest.mark.parametrize("M", [1, 17, 48, 49, 1000, 8192 + 5, 16400])
def test_backward_rows(cabi, M, tall):
    w = run_backward(cabi, M, ENGINE, w0=200, tall=tall, seed=M, scale=0.37)[0]
    _report("bwd", f"M={M},tall={tall},{R.bwd_path(M, ENGINE, tall)}", w)
    if M == 16400 and tall == 0:
        dims = [64, 64, 64, 16]
        assert R.bwd_path(M, dims, 0) == "rt2"
        _report("bwd", "M=16400,rt2", run_backward(cabi, M, dims, w0=30, tall=0, seed=3)[0])


@pytest.mark.parametrize("N", [1, 2, 16, 17, 32, 33, 64, 200, 240, 256, 1024])
def test_backward_widths(cabi, N):
    """Hidden widths (split-K at N <= 32, the >64 KiB launch at 1024), 16-row and tall forms."""
    dims = [33, N, N, 5] if N % 4 else [36, N, N, 8]
    for M in (49, 8192 + 5):
        w = run_backward(cabi, M, dims, w0=16, seed=N, dout_pad=1)[0]
        _report("bwd", f"M={M},N={N},{R.bwd_path(M, dims, -1)}", w)


@pytest.mark.parametrize("w0", [1, 7, 16, 30])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,tall", [(47, -1), (8192 + 5, -1), (16400, 0)])
def test_backward_din_split(cabi, w0, accumulate, M, tall):
    """din0 / din1 split at w0, plain and accumulating onto a random prior; din1 = NULL leaves its columns alone."""
    dims = [30, 64, 48, 8]
    for din1_null in ((False, True) if w0 < 30 else (False,)):
        w = run_backward(cabi, M, dims, w0=w0, accumulate=accumulate, din1_null=din1_null, tall=tall, seed=w0,
                         scale=0.37 if accumulate else 1.0)[0]
        _report("bwd", f"w0={w0},acc={accumulate},din1_null={din1_null},M={M},tall={tall}", w)


@pytest.mark.parametrize("L", [1, 2, 3, 6])
@pytest.mark.parametrize("off", [0, 1, 3])
def test_backward_depths_and_placements(cabi, L, off):
    """1 to 6 layers, an ELU on the last layer, saved / dpre at float offsets 1 / 3 (which refuse the tall form), no din."""
    dims = [20] + [48] * (L - 1) + [12]
    for M, tall in ((33, -1), (8192 + 5, 2)):
        for want_din in (True, False):
            w = run_backward(cabi, M, dims, acts=[True] * L, off=off, din_off=off, tall=tall, seed=L + off,
                             want_din=want_din)[0]
            _report("bwd", f"L={L},off={off},M={M},din={want_din},{R.bwd_path(M, dims, tall, al16=off == 0)}", w)


@pytest.mark.parametrize("M,tall", [(47, 0), (8192 + 5, -1), (16400, 0)])
def test_backward_window(cabi, M, tall):
    """d(out) zero except the last M % 16 rows."""
    w = run_backward(cabi, M, ENGINE, w0=200, tall=tall, seed=11, window="rows", accumulate=1)[0]
    _report("bwd", f"window=rows,M={M},tall={tall}", w)


def test_backward_run_to_run(cabi):
    for M, tall in ((1000, -1), (8192 + 5, -1), (16400, 0)):
        a = run_backward(cabi, M, ENGINE, w0=200, tall=tall, seed=5)[1]
        b = run_backward(cabi, M, ENGINE, w0=200, tall=tall, seed=5)[1]
        assert all(torch.equal(x, y) for x, y in zip(a, b)), M


# ---- weight gradients --------------------------------------------------------------------------------------------------

WG_MS = [1, 15, 16, 17, 33, 2450, 34300]
# (N, K, extra WgradCase arguments): one per body / DMA form of the wide kernel (dense_ref.wgrad_body)
WG_SHAPES = [
    (64, 1024, {}),                              # deep (16-byte act DMA)
    (32, 1024, {"lda_pad": 1}),                  # narrow, dword act DMA (odd lda)
    (65, 200, {}), (128, 48, {"ldp_pad": 3}),    # mid
    (208, 64, {}), (208, 255, {}),              # dense 13 x 13 (K % 16 = 15: the bias closes the last block)
    (209, 200, {}),                              # 14 blocks: a second column tile
    (1, 17, {}), (17, 230, {"act_off": 1}), (200, 17, {}), (230, 200, {"dpre_off": 3}),   # general / unaligned
]


@pytest.mark.parametrize("M", WG_MS)
def test_wgrad_grouped_shapes(cabi, M):
    for N, K, kw in WG_SHAPES:
        for bias in (True, False):
            c = R.WgradCase(M, N, K, bias=bias, seed=N + K, **kw)
            keep = R.run_grouped(cabi, [c])
            torch.cuda.synchronize()
            act16 = K % 4 == 0 and kw.get("lda_pad", 0) % 4 == 0 and kw.get("act_off", 0) % 4 == 0
            body = R.wgrad_body(N, K, bias, act16, act16 and kw.get("ldp_pad", 0) % 4 == 0 and not kw.get("dpre_off"))
            _report("wgrad_grouped", f"M={M},N={N},K={K},bias={bias},{'/'.join(sorted(body))}",
                    c.check(f"grouped M={M} N={N} K={K} bias={bias} {kw}"))
            del keep


@pytest.mark.parametrize("K", [32, 47, 208, 1023])
@pytest.mark.parametrize("w_off", [0, 1, 3])
def test_wgrad_grouped_bias_and_placement(cabi, K, w_off):
    """The bias column at K % 16 in {0, 15}; dW / db at float offsets 0 / 1 / 3 of a flat buffer with ldw >= K."""
    for N in (48, 208):
        for bias in (True, False):
            c = R.WgradCase(2450, N, K, bias=bias, w_off=w_off, ldw_pad=w_off, seed=K)
            keep = R.run_grouped(cabi, [c])
            torch.cuda.synchronize()
            _report("wgrad_grouped", f"K={K},N={N},w_off={w_off},bias={bias}", c.check(f"N={N} K={K} w_off={w_off}"))
            del keep


@pytest.mark.parametrize("M", [17, 2450, 34300])
def test_wgrad_grouped_two_sources(cabi, M):
    """Activations from two sources split at M1 in {0, 1, 17, M - 1, M}, lda2 != lda1."""
    for M1 in sorted({0, 1, min(17, M), M - 1, M}):
        for N, K in ((200, 200), (64, 1024), (33, 47)):
            c = R.WgradCase(M, N, K, M1=M1, lda_pad=4, lda2_pad=8 if K % 4 == 0 else 3, seed=M1)
            keep = R.run_grouped(cabi, [c])
            torch.cuda.synchronize()
            _report("wgrad_grouped", f"M={M},M1={M1},N={N},K={K}", c.check(f"M={M} M1={M1} N={N} K={K}"))
            del keep


def _mixed_table(M=2450):
    """A DenseModel's five layers plus a two-source layer in one table: block_begin, red_begin and ws_off all move."""
    cases = [R.WgradCase(M, N, K, seed=i) for i, (N, K) in enumerate([(200, 230), (200, 200), (200, 200), (200, 200),
                                                                       (1, 200)])]
    cases.append(R.WgradCase(M, 48, 33, M1=M // 3, lda2_pad=5, w_off=1, seed=9))
    return cases


def test_wgrad_grouped_mixed_table_and_phases(cabi):
    cases = _mixed_table()
    keep = R.run_grouped(cabi, cases)
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        _report("wgrad_grouped", f"mixed[{i}]", c.check(f"mixed table entry {i}"))
    first = [c.flat.clone() for c in cases]
    keep2 = R.run_grouped(cabi, cases)                     # run to run
    torch.cuda.synchronize()
    assert all(torch.equal(a, c.flat) for a, c in zip(first, cases)), "grouped run-to-run differs"
    for c in cases:
        c.flat.fill_(R.SENTINEL)
    keep3 = R.run_grouped(cabi, cases, phase=1)            # phase 1 then phase 2
    torch.cuda.synchronize()
    assert all(torch.equal(a, c.flat) for a, c in zip(first, cases)), "phase 1 + phase 2 differs from phase 0"
    del keep, keep2, keep3


@pytest.mark.parametrize("window", ["last16", "tail", "m1", "cols"])
def test_wgrad_grouped_windows(cabi, window):
    """Inputs zero outside one window: the expected values have a handful of terms each."""
    for M in (17, 2450, 34300):
        for N, K in ((208, 200), (64, 1024), (128, 47), (200, 17)):
            c = R.WgradCase(M, N, K, M1=M - 5 if window == "m1" else None, lda2_pad=4, seed=M + N, window=window)
            keep = R.run_grouped(cabi, [c])
            torch.cuda.synchronize()
            _report("wgrad_grouped", f"window={window},M={M},N={N},K={K}", c.check(f"window {window} M={M} N={N} K={K}"))
            del keep


@pytest.mark.parametrize("M", WG_MS)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_wgrad_plain(cabi, M, accumulate):
    """bd_wgrad (categorical.py, engine.wgrad): the same shapes, plain and accumulating onto a random prior."""
    for N, K, kw in WG_SHAPES[::2] + [(70, 130, {"w_off": 3, "ldw_pad": 2})]:
        kw = {k: v for k, v in kw.items() if k != "dpre_off"}
        c = R.WgradCase(M, N, K, bias=(N + M) % 2 == 0, seed=N, **kw)
        if accumulate:
            c.set_prior()
        ws = R.run_plain(cabi, c, accumulate)
        torch.cuda.synchronize()
        _report("wgrad_plain", f"M={M},N={N},K={K},acc={accumulate}", c.check(f"plain M={M} N={N} K={K}", bool(accumulate)))
        del ws


def test_wgrad_plain_windows_and_run_to_run(cabi):
    for window in ("last16", "tail", "cols"):
        c = R.WgradCase(2450 + 7, 70, 130, seed=3, window=window)
        R.run_plain(cabi, c)
        torch.cuda.synchronize()
        _report("wgrad_plain", f"window={window}", c.check(f"plain window {window}"))
    c = R.WgradCase(34300, 200, 200, seed=4)
    R.run_plain(cabi, c)
    torch.cuda.synchronize()
    first = c.flat.clone()
    R.run_plain(cabi, c)
    torch.cuda.synchronize()
    assert torch.equal(first, c.flat)


# ---- paths selected by the environment (read once per process): fresh child processes ---------------------------------

@pytest.mark.parametrize("env", [{"BD_WGRAD_WIDE": "0"}, {"BD_WGRAD_ROWS": "16"}, {"BD_WGRAD_ROWS": "48"}])
def test_wgrad_env_paths(env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wgrad_env_worker.py")], capture_output=True,
                         text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **env))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("WGRAD_ENV_RESULT ")][-1].split(" ", 1)[1])
    print("DENSE_WORST wgrad_env", json.dumps(env), f"{res['worst']:.3e}", res["cases"])
    assert res["cases"] > 0
