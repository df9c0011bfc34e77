"""CPU tests of tests/conv_ref.py: the index-formula references agree with F.conv2d / F.conv_transpose2d / autograd in
float64 on every geometry of the GPU case tables (both readings of each pattern); the pack formulas round-trip; an fp32
emulation of each contraction passes the tolerance at every case while each planted fault fails at the case named for it;
every form the dispatch mirror can name is hit by a GPU case; the ReLU cases stay under the ambiguity cap; and the mirror
equals the library where the library reports (LDS byte counts, bd_wgrad_plan's fields)."""
import ctypes as C
import re

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R
from tests.dense_ref import C_TOL, SENTINEL, check_close

D64 = torch.float64


def _nchw(x):
    return x.permute(0, 3, 1, 2).double()


def _grid(fr: R.FlatRef, imgs, OH, OW, ldo, N):
    assert bool(fr.written.reshape(imgs, OH, OW, ldo)[..., :N].all()) and int(fr.written.sum()) == imgs * OH * OW * N
    return fr.ref.reshape(imgs, OH, OW, ldo)[..., :N]


def _close(a, b):
    assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-10 * (1.0 + float(b.abs().max()))


# ---- reference agreement ---------------------------------------------------------------------------------------------

def _check_f(a, x, stored, bias):
    """Pattern F as Conv2d forward and as the dgrad of the ConvTranspose2d with the same stored tensor."""
    a = dict(a, act=0)
    N, k, C = stored.shape[0], stored.shape[1], stored.shape[3]
    got = _grid(R.conv_gemm_ref(a, x.reshape(-1), stored.reshape(N, -1), bias), a["imgs"], a["OH"], a["OW"], a["ldo"], N)
    xz = torch.nan_to_num(x)                          # (the NaN row / column is outside every window)
    w = stored.permute(0, 3, 1, 2).double()           # Conv2d (co, ci, ky, kx) = ConvTranspose2d (ci_T, co_T, ky, kx)
    _close(got, F.conv2d(_nchw(xz), w, None if bias is None else bias.double(), stride=2).permute(0, 2, 3, 1))
    if bias is None:
        xt = torch.zeros(a["imgs"], N, a["OH"], a["OW"], dtype=D64, requires_grad=True)
        y = F.conv_transpose2d(xt, w, None, stride=2)
        (gx,) = torch.autograd.grad(y, xt, _nchw(xz)[:, :, :y.shape[2], :y.shape[3]])
        _close(got, gx.permute(0, 2, 3, 1))


def _check_t(g, x, stored, bias, fr):
    """Pattern T as ConvTranspose2d forward (cropped / zero-extended to OH x OW) and as the dgrad of the Conv2d."""
    imgs, OH, OW, N, k = g["imgs"], g["OH"], g["OW"], g["N"], g["k"]
    got = _grid(fr, imgs, OH, OW, fr.ref.numel() // (imgs * OH * OW), N)
    w = stored.permute(0, 3, 1, 2).double()           # ConvTranspose2d (ci, co, ky, kx) = Conv2d (co_c, ci_c, ky, kx)
    full = F.conv_transpose2d(_nchw(x), w, None if bias is None else bias.double(), stride=2).permute(0, 2, 3, 1)
    want = torch.zeros(imgs, OH, OW, N, dtype=D64)
    h, wd = min(OH, full.shape[1]), min(OW, full.shape[2])
    want[:, :h, :wd] = full[:, :h, :wd]
    assert bias is None or (OH <= full.shape[1] and OW <= full.shape[2])
    _close(got, want)
    if OH > full.shape[1] or OW > full.shape[2]:
        assert bool((got[:, full.shape[1]:] == 0).all()) and bool((got[:, :, full.shape[2]:] == 0).all())
    if bias is None and R.conv_out(OH, k) == g["IH"] and R.conv_out(OW, k) == g["IW"]:
        xin = torch.zeros(imgs, N, OH, OW, dtype=D64, requires_grad=True)
        (gx,) = torch.autograd.grad(F.conv2d(xin, w, None, stride=2), xin, _nchw(x))
        _close(got, gx.permute(0, 2, 3, 1))


@pytest.mark.parametrize("name", list(R.GATHER_F))
def test_f_reference_matches_torch(name):
    a, x, w, b = R.build_gather_f(name)
    _check_f(a, x, w, b)
    _check_f(a, x, w, None)


@pytest.mark.parametrize("name", list(R.T_GATHER))
def test_t_reference_matches_torch(name):
    g, x, w, b = R.build_t(name)
    for bias in ([b, None] if b is not None else [None]):
        _check_t(g, x, w, bias, R.t_class_refs(g, x, w, bias, ldo=g["N"] + 2))
        a = R.args_t_fused(g["imgs"], g["IH"], g["IW"], g["C"], g["k"], g["N"], g["OH"], g["OW"], g["N"] + 1)
        _check_t(g, x, w, bias, R.conv_gemm_ref(a, x.reshape(-1), R.fused_matrix(w, g["k"]), bias))


@pytest.mark.parametrize("name", list(R.PATCH))
def test_patch_case_reference_matches_torch(name):
    a, x, w, b = R.build_patch(name, ldo_pad=1)
    if R.PATCH[name].kind == "F":
        _check_f(a, x, w, b)
        _check_f(a, x, w, None)
    else:
        k = R.PATCH[name].k
        g = dict(imgs=a["imgs"], IH=a["IH"], IW=a["IW"], C=a["C"], k=k, N=a["fuse_cq"], OH=a["OH"], OW=a["OW"])
        for bias in ([b, None] if b is not None else [None]):
            _check_t(g, x, w, bias, R.conv_gemm_ref(a, x.reshape(-1), R.fused_matrix(w, k), bias))


def _thin_inputs(name):
    imgs, IH, IW, Cc, k, bias, act, ldw_pad, w_off = R.THIN[name]
    x, w, b = R.make_inputs(R.seed_of(name), (imgs, IH, IW, Cc), (32, k * k * Cc), 32, 0.2)
    return (imgs, IH, IW, Cc, k), R.poison_unused(x, k), w, (b if bias else None), act


@pytest.mark.parametrize("name", list(R.THIN))
def test_thin_reference_matches_torch(name):
    (imgs, IH, IW, Cc, k), x, w, b, _ = _thin_inputs(name)
    fr = R.thin_ref(imgs, IH, IW, Cc, k, x.reshape(-1), w, b)
    want = F.conv2d(_nchw(torch.nan_to_num(x)), w.reshape(32, k, k, Cc).permute(0, 3, 1, 2).double(),
                    None if b is None else b.double(), stride=2).permute(0, 2, 3, 1)
    _close(fr.ref.reshape(want.shape), want)


_wgrad_inputs = R.wgrad_inputs


@pytest.mark.parametrize("name", list(R.WGRAD))
def test_gathered_wgrad_reference_matches_autograd(name):
    g, d, dpre, img = _wgrad_inputs(name)
    dW, _, db, _ = R.wgrad_gathered_ref(d, dpre, img.reshape(-1))
    w = torch.zeros(g["N"], g["C"], g["k"], g["k"], dtype=D64, requires_grad=True)
    bz = torch.zeros(g["N"], dtype=D64, requires_grad=True)
    y = F.conv2d(_nchw(torch.nan_to_num(img)), w, bz, stride=2)
    gy = dpre.double().reshape(g["imgs"], g["gh"], g["gw"], g["N"]).permute(0, 3, 1, 2)
    gw_, gb_ = torch.autograd.grad(y, (w, bz), gy)
    _close(dW.reshape(g["N"], g["k"], g["k"], g["C"]), gw_.permute(0, 2, 3, 1))
    _close(db, gb_)


# ---- round trips -----------------------------------------------------------------------------------------------------

def test_pack_formulas_round_trip():
    gen = torch.Generator().manual_seed(3)
    for N, K, ld in R.PACK_W:
        src = torch.randn(max(N, K) + 1, max(ld, N + 1), generator=gen)
        for tr in (False, True):
            n_, k_ = (K, N) if tr else (N, K)
            W = src[:N, :K].t() if tr else src[:N, :K]            # transposed: the packed matrix is W^T (out = K, in = N)
            p = R.pack_weights_ref(src, N, K, tr)
            assert p.numel() == R.cdiv(n_, 16) * R.cdiv(k_, 16) * 256
            assert torch.equal(R.unpack_ref(p, n_, k_), W)
            assert int((p != 0).sum()) == int((W != 0).sum())               # the padding is zero
    for Co, Ci in R.PACK_CH:
        for k in (3, 4, 5, 6):
            stored = torch.randn(Co, k, k, Ci, generator=gen)
            back, back_f = torch.zeros_like(stored), torch.zeros_like(stored)
            T = (k + 1) // 2
            Wf = R.unpack_ref(R.pack_ref(R.fused_matrix(stored, k)), 4 * Ci, T * T * Co)
            for py in range(2):
                for px in range(2):
                    Ta, Tb = R.taps(k, py), R.taps(k, px)
                    Wc = R.unpack_ref(R.pack_ref(R.class_matrix(stored, k, py, px)), Ci, Ta * Tb * Co)
                    cls = 2 * py + px
                    for a in range(T):
                        for b in range(T):
                            ky, kx = py + 2 * a, px + 2 * (T - 1 - b)
                            blk = Wf[cls * Ci:(cls + 1) * Ci, (a * T + b) * Co:(a * T + b + 1) * Co]
                            if ky < k and kx < k:
                                back_f[:, ky, kx, :] = blk.t()
                            else:
                                assert float(blk.abs().sum()) == 0.0
                    for a in range(Ta):
                        for b in range(Tb):
                            back[:, py + 2 * a, px + 2 * (Tb - 1 - b), :] = Wc[:, (a * Tb + b) * Co:(a * Tb + b + 1) * Co].t()
            assert torch.equal(back, stored) and torch.equal(back_f, stored)
    for imgs, Cc, HW in R.LAYOUT:
        src = torch.randn(imgs * Cc * HW, generator=gen)
        assert torch.equal(R.layout_ref(R.layout_ref(src, imgs, Cc, HW, True), imgs, Cc, HW, False), src)
        assert torch.equal(R.layout_ref(src, imgs, Cc, HW, True).reshape(imgs, HW, Cc)[0, 5 % HW, Cc - 1],
                           src.reshape(imgs, Cc, HW)[0, Cc - 1, 5 % HW])


# ---- sharpness: fp32 emulation passes, planted faults fail ---------------------------------------------------------------

def _conv_cases():
    """(name, args, flat image, [N x K] matrix, bias) of every bd_conv_gemm launch of the GPU tables, activation off."""
    out = []
    for name in R.GATHER_F:
        a, x, w, b = R.build_gather_f(name, act="none")
        out.append((name, a, x, w.reshape(w.shape[0], -1), b))
    for name in R.T_GATHER:
        g, x, w, b = R.build_t(name)
        for py in range(2):
            for px in range(2):
                a = R.args_t_class(g["imgs"], g["IH"], g["IW"], g["C"], g["k"], g["N"], g["OH"], g["OW"], py, px)
                out.append((f"{name}/c{py}{px}", a, x, R.class_matrix(w, g["k"], py, px), b))
        a = R.args_t_fused(g["imgs"], g["IH"], g["IW"], g["C"], g["k"], g["N"], g["OH"], g["OW"])
        out.append((f"{name}/fused", a, x, R.fused_matrix(w, g["k"]), b))
    for name in R.PATCH:
        a, x, w, b = R.build_patch(name)
        out.append((name, a, x, R.conv_weight_matrix(a, w, R.PATCH[name].k), b))
    return out


CONV_CASES = _conv_cases()


def _emu_flat(a, x, Wm, b, fr):
    """The fp32 emulation of one launch, placed like the reference places it."""
    A = R.im2col(a, x.reshape(-1))
    bias = None
    if b is not None:
        n = torch.arange(a["N"])
        bias = b[n % a["fuse_cq"]] if a["fuse_cq"] else b
    emu = R.emu_dot(A, Wm, bias)
    got = torch.full((fr.ref.numel(),), SENTINEL, dtype=D64)
    pos, valid = _positions(a)
    got[pos[valid]] = emu.double()[valid]
    return got


def _positions(a):
    """Output position and validity of (m, n), by the same formula as conv_gemm_ref (kept apart so that the emulation does
    not lean on the reference's values)."""
    gh, gw, N, OH, OW, ldo, cq = a["gh"], a["gw"], a["N"], a["OH"], a["OW"], a["ldo"], a["fuse_cq"]
    m = torch.arange(a["imgs"] * gh * gw)
    img, rem = m // (gh * gw), m % (gh * gw)
    y, x = rem // gw, rem % gw
    n = torch.arange(N)
    valid = torch.ones(m.numel(), N, dtype=torch.bool)
    coff = n
    if cq:
        cls, c = n // cq, n % cq
        py, px = cls >> 1, cls & 1
        coff = (py * OW + px) * ldo + c
        valid = ((py == 0)[None] | (2 * y + 1 < OH)[:, None]) & ((px == 0)[None] | (2 * x + 1 < OW)[:, None])
    pos = (((img * OH + y * a["osy"] + a["oy0"]) * OW + x * a["osx"] + a["ox0"]) * ldo)[:, None] + coff[None]
    return pos, valid


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_fp32_emulation_passes_conv(case):
    name, a, x, Wm, b = case
    fr = R.conv_gemm_ref(a, x.reshape(-1), Wm, b)
    got = _emu_flat(a, x, Wm, b, fr)
    assert fr.check(name, got) <= C_TOL


def test_fp32_emulation_passes_thin_gemm_wgrad():
    worst = {}
    for name in R.THIN:
        (imgs, IH, IW, Cc, k), x, w, b, _ = _thin_inputs(name)
        fr = R.thin_ref(imgs, IH, IW, Cc, k, x.reshape(-1), w, b)
        emu = R.emu_dot(R.thin_matrix(imgs, IH, IW, Cc, k, x.reshape(-1)), w, b, chains=1, strided=False)
        worst[name] = fr.check(name, emu.reshape(-1))
    for name, (M, N, K, lda_pad, b_off, acc) in R.GEMM.items():
        gen = torch.Generator().manual_seed(R.seed_of(name))
        A, B, P = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(M, N, generator=gen)
        ref, S = R.gemm_ref(A, B, P if acc else None)
        emu = R.emu_dot(A, B, chains=1)
        worst[name] = check_close(name, P + emu if acc else emu, ref, S)
    for name in R.WGRAD:
        g, d, dpre, img = _wgrad_inputs(name)
        plan = R.wgrad_plan_mirror([d], g["thin_env"])[0]
        dW, sW, db, sb = R.wgrad_gathered_ref(d, dpre, img.reshape(-1))
        eW, eb = R.emu_wgrad(dpre, R.wgrad_matrix(d, img.reshape(-1)), plan["rows_per"])
        worst[name] = max(check_close(name, eW, dW, sW), check_close(name, eb, db, sb))
    assert max(worst.values()) <= C_TOL, worst


def _conv_case(name):
    return next(c for c in CONV_CASES if c[0] == name)


def _faulted_conv(name, fault):
    _, a, x, Wm, b = _conv_case(name)
    fr = R.conv_gemm_ref(a, x.reshape(-1), Wm, b)
    if fault == "x_not_reversed":
        base = name.split("/")[0]
        _, _, stored, _ = R.build_t(base)
        Wm = R.conv_weight_matrix(a, stored, R.T_GATHER[base].k, fault)
    bad = R.conv_gemm_ref(a, x.reshape(-1), Wm, b, size=fr.ref.numel(), fault=fault)
    got = torch.full((fr.ref.numel(),), SENTINEL, dtype=D64)
    got[bad.written] = bad.ref[bad.written]
    return fr, got


# fault -> the case it must fail at
CONV_FAULTS = {
    "drop_tap": "f_k2048_rt1", "mask_top": "t_k4/fused", "mask_bottom": "t_k4/c00", "mask_left": "t_k5/fused",
    "mask_right": "t_k6/c11", "rowflag_le": "t_k3/fused", "classes_swapped": "t_k3/fused", "x_not_reversed": "t_k5/c01",
    "bias_by_column": "t_k5/fused", "ldo_as_N": "f_c6k3_m45", "rowstride_gw": "f_c4k3_unused",
}


@pytest.mark.parametrize("fault,name", list(CONV_FAULTS.items()))
def test_planted_conv_fault_fails(fault, name):
    fr, got = _faulted_conv(name, fault)
    with pytest.raises(AssertionError):
        fr.check(f"{name} with {fault}", got)
    fr2, clean = _faulted_conv(name, "probe")          # the same path without a fault passes
    fr2.check(name, clean)


def test_planted_gemm_thin_wgrad_faults_fail():
    for fault, name in (("drop_last_kblock", "g4_reg_k33"), ("ignore_accumulate", "g4_dma_k16")):
        M, N, K, _, _, acc = R.GEMM[name]
        gen = torch.Generator().manual_seed(R.seed_of(name))
        A, B, P = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen), torch.randn(M, N, generator=gen)
        ref, S = R.gemm_ref(A, B, P if acc else None)
        bad, _ = R.gemm_ref(A, B, P if acc else None, fault=fault)
        with pytest.raises(AssertionError):
            check_close(fault, bad, ref, S)
    (imgs, IH, IW, Cc, k), x, w, b, _ = _thin_inputs("th_c3k4_gw17")
    fr = R.thin_ref(imgs, IH, IW, Cc, k, x.reshape(-1), w, b)
    bad = R.thin_ref(imgs, IH, IW, Cc, k, torch.nan_to_num(x).reshape(-1), w, b, fault="thin_ky")
    with pytest.raises(AssertionError):
        fr.check("thin_ky", bad.ref)
    g, d, dpre, img = _wgrad_inputs("w_c4k3_n3")
    dW, sW, _, _ = R.wgrad_gathered_ref(d, dpre, img.reshape(-1))
    badW, _, _, _ = R.wgrad_gathered_ref(d, dpre, torch.nan_to_num(img).reshape(-1), fault="rowstride_gw")
    with pytest.raises(AssertionError):
        check_close("rowstride_gw", badW, dW, sW)


# ---- coverage ----------------------------------------------------------------------------------------------------------

def test_every_form_of_the_mirror_is_hit_by_a_gpu_case():
    forms = {"gather": set(), "patch": set()}
    runs, big, ragged2 = {"gather": set(), "patch": set()}, set(), False
    for name, a, *_ in CONV_CASES:
        f = R.conv_form(a)
        assert not f["rejected"], name
        forms[f["form"]].add(f["RT"])
        runs[f["form"]] |= f["runs"]
        if f["big"]:
            big.add(f["form"])
        ragged2 = ragged2 or (f["form"] == "patch" and f["tiles_x"] == 2 and f["ragged_x"])
        if name.startswith(("pf_", "pt_")):
            assert (f["form"] == "patch") != (name == "pf_gw11"), (name, f)
            assert R.conv_form(a, patch_env=False)["form"] == "gather"
    assert forms == {"gather": {1, 2, 4, 8}, "patch": {1, 2, 4, 8}}, forms
    assert runs["gather"] == {1, 2, 3, 4} and runs["patch"] == {1, 2}, runs
    assert "gather" in big and ragged2
    # the two named row counts: a ragged last tile (M = 45) and a second workgroup with one row (M = 16 RT + 1)
    f = R.conv_form(_conv_case("f_k1024_m33")[1])
    assert f["RT"] == 2 and f["blocks"] == 2 and _conv_case("f_k1024_m33")[1]["imgs"] * 11 == 16 * f["RT"] + 1
    thin = [R.thin_form(c.imgs, c.IH, c.IW, c.C, c.k, ldw=c.k * c.k * c.C + c.ldw_pad) for c in R.THIN.values()]
    assert all(t["reject"] is None for t in thin)
    assert {t["KS"] for t in thin} == {12, 27} and {t["nrt"] for t in thin} == {1, 2} and {t["ipw"] for t in thin} == {1, 2}
    assert any(t["KS"] == 27 and t["K"] < 108 for t in thin) and {t["gw"] for t in thin} >= {1, 5, 16, 17, 32}
    assert any(t["grid"] * t["ipw"] > 513 for t in thin), "no ragged last workgroup at ipw = 2"
    for n, (imgs, IH, IW, Cc, k, off) in R.THIN_REJECT.items():
        assert R.thin_form(imgs, IH, IW, Cc, k, in_al16=off % 4 == 0)["reject"] is not None, n
    gemm = {(f["RTM"], f["dma"]) for f in (R.gemm_form(M, N, K, K + lp, K, 0, bo) for M, N, K, lp, bo, _ in R.GEMM.values())}
    assert gemm == {(r, d) for r in (4, 6, 8, 10) for d in (False, True)}, gemm
    for n, (M, N, K, lp, bo, _) in R.GEMM.items():
        f = R.gemm_form(M, N, K, K + lp, K, 0, bo)
        assert n.startswith(f"g{f['RTM']}_{'dma' if f['dma'] else 'reg'}"), (n, f)
    bodies, staged = set(), set()
    for n in R.WGRAD:
        g, d, _, _ = _wgrad_inputs(n)
        p = R.wgrad_plan_mirror([d], g["thin_env"])[0]
        assert (p["body"][0] == "thin") == n.startswith("wt_"), (n, p)
        if p["body"][0] == "thin":
            bodies.add(p["body"][1:])
        else:
            staged |= p["body"][1]
    assert {b[0] for b in bodies} == {3, 7} and {b[1] for b in bodies} == {1, 2}, bodies
    assert staged >= {"narrow", "deep", "general"}, staged


# ---- ReLU cap ----------------------------------------------------------------------------------------------------------

def test_relu_cases_stay_under_the_ambiguity_cap():
    n = 0
    for name, c in R.GATHER_F.items():
        if c.act == "ReLU":
            a, x, w, b = R.build_gather_f(name)
            assert R.relu_ambiguous_share(R.conv_gemm_ref(a, x.reshape(-1), w.reshape(w.shape[0], -1), b)) <= R.RELU_CAP, name
            n += 1
    for name in R.THIN:
        (imgs, IH, IW, Cc, k), x, w, b, act = _thin_inputs(name)
        if act == "ReLU":
            assert R.relu_ambiguous_share(R.thin_ref(imgs, IH, IW, Cc, k, x.reshape(-1), w, b, act)) <= R.RELU_CAP, name
            n += 1
    for fam, name in R.GRAD_ON:
        if fam == "patch":
            a, x, w, b = R.build_patch(name)
            fr = R.conv_gemm_ref(a, x.reshape(-1), R.conv_weight_matrix(a, w, R.PATCH[name].k), b)
            assert R.relu_ambiguous_share(fr) <= R.RELU_CAP, name
            n += 1
    assert n >= 4


# ---- the mirror against the library ------------------------------------------------------------------------------------

def _conv_args_struct(cabi, a):
    """bd_conv_args over REAL zero-filled buffers of the full size of every operand (device memory where there is a device):
    the calls below must be rejected on the host, but should the library's limits ever drift from the mirror and one of
    them launch, every access of that launch stays inside these buffers."""
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    keep = [torch.zeros(a["imgs"] * a["IH"] * a["IW"] * a["C"] + 16, device=dev),
            torch.zeros(a["imgs"] * a["OH"] * a["OW"] * a["ldo"] + 16, device=dev),
            torch.zeros(R.cdiv(a["N"], 16) * R.cdiv(a["K"], 16) * 256, device=dev)]
    s = cabi.ConvArgs()
    for k_, v in a.items():
        setattr(s, k_, v)
    s.in_, s.out, s.w = (t.data_ptr() for t in keep)
    return s, keep


def test_lds_requests_of_the_mirror_equal_the_library_errors():
    """Shapes whose LDS request exceeds the CU's 160 KiB in EITHER form, so the call is rejected before any launch whatever
    BD_CONV_PATCH says; the byte count of the error text is the mirror's."""
    from big_dreamer_amd import _cabi as cabi
    import os
    patch_env = not os.environ.get("BD_CONV_PATCH", "").startswith("0")
    for a in (R.args_f(1, 26, 26, 4, 26, 8),                                           # gather: K = 2704 at 16 rows
              R.args_f(1, 9, 33, 128, 9, 16),                                          # patch (F): 9 x 39 x 132 floats
              R.args_t_fused(1, 13, 20, 128, 26, 4, 50, 40)):                          # patch (T, fused): T = 13
        f = R.conv_form(a, patch_env)
        assert f["rejected"] and R.conv_form(a, not patch_env)["rejected"]
        s, keep = _conv_args_struct(cabi, a)
        rc = cabi.lib.bd_conv_gemm(C.byref(s), None)
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        assert rc != 0, ("accepted", a)
        msg = cabi.lib.bd_last_error().decode()
        m = re.search(r"needs (\d+) B of LDS", msg)
        assert m and int(m.group(1)) == f["lds"], (msg, f)
        assert ("(patch)" in msg) == (f["form"] == "patch"), (msg, f)
        del keep


def test_wgrad_plan_of_the_mirror_equals_the_library():
    """bd_wgrad_plan runs on the host: placeholder (16-byte aligned) addresses, the fields it fills against the mirror."""
    from big_dreamer_amd import _cabi as cabi
    import os
    thin_env = not os.environ.get("BD_WGRAD_THIN", "").startswith("0")
    names = list(R.WGRAD)
    groups = [[n] for n in names] + [names[:4], names]
    for grp in groups:
        ds = [_wgrad_inputs(n)[1] for n in grp]
        arr = (cabi.WgradDesc * len(ds))()
        for s, d in zip(arr, ds):
            s.dpre, s.ldp, s.act1, s.lda1, s.M1, s.M, s.N, s.K = 0x1000, d["ldp"], 0x2000, 0, d["M"], d["M"], d["N"], d["K"]
            s.dW, s.ldw, s.db = 0x3000, d["K"], (0x4000 if d["bias"] else None)
            for f_ in ("g_nseg", "g_seglen", "g_gh", "g_gw", "g_IH", "g_IW", "g_C"):
                setattr(s, f_, d[f_])
        tb, tr, wsf = C.c_int(0), C.c_int(0), C.c_size_t(0)
        assert cabi.lib.bd_wgrad_plan(arr, len(ds), C.byref(tb), C.byref(tr), C.byref(wsf)) == 0, cabi.lib.bd_last_error()
        want = R.wgrad_plan_mirror(ds, thin_env)
        for n, s, p in zip(grp, arr, want):
            got = {f_: getattr(s, f_) for f_ in ("g_pad", "tiles_n", "tiles_k", "rows_per", "splits")}
            assert got == {f_: p[f_] for f_ in got}, (grp, n, got, p)
        assert tb.value == sum(p["tiles_n"] * p["tiles_k"] * p["splits"] for p in want)
