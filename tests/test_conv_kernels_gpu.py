"""GPU tests of the pixel kernels against the float64 index-formula references of tests/conv_ref.py, with the componentwise
bound |got - ref| <= C_TOL * sum|a*b| (+ the activation allowance) of tests/dense_ref.py: bd_conv_gemm in its gather and
patch forms (patterns F, T per class, T fused; the _GRAD epilogues), bd_conv_thin_forward and its rejections, bd_gemm_nt
at every rows-per-workgroup variant in both load forms, the gathered and thin-image weight gradients with the plan
bd_wgrad_plan wrote, and the pack / layout permutations bit for bit.  The shapes are the smallest that reach each path
(tests/test_conv_ref_cpu.py proves the coverage from the dispatch mirror).  Outputs lie in SENTINEL-filled buffers and
nothing outside the output region may change; inputs lie in NaN (see the runners in tests/conv_ref.py for what is
poisoned and why).  The forms that BD_CONV_PATCH=0 / BD_WGRAD_THIN=0 select run in tests/conv_env_worker.py.
Every test prints its worst err / bound (pytest -s)."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import conv_ref as R
from tests import dense_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTS = ["ELU", "ReLU", "Tanh"]


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def _report(family, name, worst, form=None):
    print(f"CONV_KERNELS {family} {name} worst err / sum|a*b| = {worst:.3e} (C_TOL {DR.C_TOL:g})" + (f" form={form}" if form else ""))
    assert worst <= DR.C_TOL


# ---- bd_conv_gemm ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.GATHER_F))
def test_gather_f(cabi, name):
    a, x, w, b = R.build_gather_f(name)
    f = R.conv_form(a)
    assert f["form"] == "gather"
    fr = R.conv_gemm_ref(a, x.reshape(-1), w.reshape(w.shape[0], -1), b, size=R.out_size(a))
    got = R.run_conv(cabi, a, x, R.dev_pack(cabi, a, w, R.GATHER_F[name].k), b)
    _report("gatherF", name, fr.check(name, got), f"RT{f['RT']} lds={f['lds']} runs={sorted(f['runs'])}")


@pytest.mark.parametrize("name", list(R.T_GATHER))
def test_t_per_class_and_fused(cabi, name):
    g, x, w, b = R.build_t(name)
    k, ldo = g["k"], g["N"] + 2
    size = g["imgs"] * g["OH"] * g["OW"] * ldo + R.TAIL
    fr = R.t_class_refs(g, x, w, b, ldo=ldo, size=size)
    out = torch.full((size,), DR.SENTINEL, device="cuda")
    for py in range(2):
        for px in range(2):
            a = R.args_t_class(g["imgs"], g["IH"], g["IW"], g["C"], k, g["N"], g["OH"], g["OW"], py, px, ldo)
            assert R.conv_form(a)["form"] == "gather"
            R.run_conv(cabi, a, x, R.dev_pack(cabi, a, w, k), b, out=out)
    _report("T", name, fr.check(name, out))
    a = R.args_t_fused(g["imgs"], g["IH"], g["IW"], g["C"], k, g["N"], g["OH"], g["OW"], ldo)
    fr2 = R.conv_gemm_ref(a, x.reshape(-1), R.fused_matrix(w, k), b, size=size)
    got = R.run_conv(cabi, a, x, R.dev_pack(cabi, a, w, k), b)
    _report("fused", name, fr2.check(name + " fused", got), f"RT{R.conv_form(a)['RT']}")
    # pixels that no window covers (OH / OW beyond the transposed convolution's extent) are exactly 0
    img = got[:size - R.TAIL].view(g["imgs"], g["OH"], g["OW"], ldo)[..., :g["N"]]
    hT, wT = R.convT_out(g["IH"], k), R.convT_out(g["IW"], k)
    assert bool((img[:, hT:] == 0).all()) and bool((img[:, :, wT:] == 0).all())


def test_patch_form_and_its_switch(cabi, tmp_path):
    """Every PATCH case here (patch form), then the same inputs in a child with BD_CONV_PATCH=0 (gather form): both within
    the bound; bit equality of the two forms is reported, not required (the K order differs: taps x 16-channel blocks)."""
    outs = {}
    for name in R.PATCH:
        a = R.patch_args(name, ldo_pad=1)[0]
        f = R.conv_form(a)
        got, worst = R.gpu_patch_case(cabi, name)
        outs[name] = got
        _report("patch" if f["form"] == "patch" else "gatherF", name, worst, f"{f['form']} RT{f['RT']} runs={sorted(f['runs'])}")
        if a["fuse_cq"]:
            img = got[:got.numel() - R.TAIL].view(a["imgs"], a["OH"], a["OW"], a["ldo"])[..., :a["fuse_cq"]]
            k = R.PATCH[name].k
            assert bool((img[:, R.convT_out(a["IH"], k):] == 0).all()) and bool((img[:, :, R.convT_out(a["IW"], k):] == 0).all())
    path = str(tmp_path / "patch_outputs.pt")
    torch.save(outs, path)
    res = _child("patch", {"BD_CONV_PATCH": "0"}, path)
    print("CONV_KERNELS patch-vs-gather bit equality:", res["bit_equal"])
    assert res["cases"] == len(R.PATCH) and res["worst"] <= DR.C_TOL
    assert res["bit_equal"]["pf_gw11"], "the gather-form neighbour must not depend on the switch"


def _child(mode, env, *args):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_env_worker.py"), mode, *args], capture_output=True,
                         text=True, env=e, timeout=240)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("CONV_ENV_RESULT ")][-1]
    print(line)
    return json.loads(line[len("CONV_ENV_RESULT "):])


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("fam,name", [c for c in R.GRAD_ON if c[0] != "thin"])
def test_conv_grad_epilogues(cabi, fam, name, act):
    """BD_ACT_*_GRAD on a ragged gather case, a fused-class gather case with a missing odd row, and two patch cases; aux is
    NaN wherever no output is stored (rows beyond M, the odd row / column a class does not have, the ldo padding)."""
    if fam == "gather_f":
        a, x, w, b = R.build_gather_f(name, act="none")
        k = R.GATHER_F[name].k
    elif fam == "t_fused":
        g, x, w, b = R.build_t(name)
        k = g["k"]
        a = R.args_t_fused(g["imgs"], g["IH"], g["IW"], g["C"], k, g["N"], g["OH"], g["OW"], g["N"] + 1)
    else:
        a, x, w, b = R.build_patch(name, ldo_pad=1)
        k = R.PATCH[name].k
    Wm = R.conv_weight_matrix(a, w, k)
    plain = R.conv_gemm_ref(a, x.reshape(-1), Wm, b, size=R.out_size(a))
    aux = R.saved_outputs(plain, act, R.seed_of(name + act))
    a = dict(a, act=R.ACT_CODE[act + "_GRAD"])
    fr = R.conv_gemm_ref(a, x.reshape(-1), Wm, b, aux=aux, size=R.out_size(a))
    got = R.run_conv(cabi, a, x, R.dev_pack(cabi, a, w, k), b, aux=aux)
    _report("grad", f"{name}/{act}", fr.check(f"{name} {act}_GRAD", got), R.conv_form(a)["form"])


# ---- bd_conv_thin_forward --------------------------------------------------------------------------------------------

def _thin_run(cabi, name, act=None, aux=None):
    imgs, IH, IW, Cc, k, bias, act0, ldw_pad, w_off = R.THIN[name]
    act = act or act0
    x, w, b = R.make_inputs(R.seed_of(name), (imgs, IH, IW, Cc), (32, k * k * Cc), 32, 0.2)
    x = R.poison_unused(x, k)
    b = b if bias else None
    K, ldw = k * k * Cc, k * k * Cc + ldw_pad
    wrows = torch.full((32, ldw), float("nan"))
    wrows[:, :K] = w
    keep_w = R.dev_input(wrows, w_off)
    keep_x = R.dev_input(x)
    n_out = imgs * R.conv_out(IH, k) * R.conv_out(IW, k) * 32
    out = torch.full((n_out + R.TAIL,), DR.SENTINEL, device="cuda")
    bd = None if b is None else b.cuda()
    ad = None if aux is None else aux.float().cuda()
    cabi.check(cabi.lib.bd_conv_thin_forward(keep_x[1].data_ptr(), imgs, IH, IW, Cc, k, keep_w[1].data_ptr(), ldw,
                                             None if bd is None else bd.data_ptr(), R.ACT_CODE[act],
                                             None if ad is None else ad.data_ptr(), out.data_ptr(), cabi.stream()))
    torch.cuda.synchronize()
    return (imgs, IH, IW, Cc, k), x, w, b, out, n_out


@pytest.mark.parametrize("name", list(R.THIN))
def test_thin_forward(cabi, name):
    geo, x, w, b, out, n_out = _thin_run(cabi, name)
    fr = R.thin_ref(*geo, x.reshape(-1), w, b, R.THIN[name].act)
    assert bool((out[n_out:] == DR.SENTINEL).all()), "wrote behind the output"
    f = R.thin_form(*geo)
    _report("thin", name, fr.check(name, out[:n_out]), f"KS{f['KS']} nrt={f['nrt']} npc={f['npc']} ipw={f['ipw']}")


@pytest.mark.parametrize("act", ACTS)
def test_thin_grad_epilogues(cabi, act):
    name = "th_c3k4_gw17"
    imgs, IH, IW, Cc, k = R.THIN[name][:5]
    g = torch.Generator().manual_seed(R.seed_of(name + act))
    n = imgs * R.conv_out(IH, k) * R.conv_out(IW, k) * 32
    aux = R.act64(act, torch.randn(n, generator=g, dtype=R.D64)).float().double()
    geo, x, w, b, out, n_out = _thin_run(cabi, name, act + "_GRAD", aux)
    fr = R.thin_ref(*geo, x.reshape(-1), w, b, act + "_GRAD", aux)
    assert bool((out[n_out:] == DR.SENTINEL).all())
    _report("thin", f"{name}/{act}_GRAD", fr.check(name, out[:n_out]))


def test_thin_forward_rejections(cabi):
    """gw = 33, K > 108, a row width that is no multiple of 4 floats, an image pointer 4 bytes off, C = 5: an error code,
    and the output untouched."""
    out = torch.full((1 << 16,), DR.SENTINEL, device="cuda")
    x = torch.zeros(1 << 14, device="cuda")
    w = torch.zeros(32 * 160, device="cuda")
    for name, (imgs, IH, IW, Cc, k, off) in R.THIN_REJECT.items():
        want = R.thin_form(imgs, IH, IW, Cc, k, in_al16=off % 4 == 0)["reject"]
        rc = cabi.lib.bd_conv_thin_forward(x.data_ptr() + 4 * off, imgs, IH, IW, Cc, k, w.data_ptr(), k * k * Cc, None, 0, None,
                                           out.data_ptr(), cabi.stream())
        assert rc != 0 and want is not None and want.encode() in cabi.lib.bd_last_error(), (name, cabi.lib.bd_last_error())
    torch.cuda.synchronize()
    assert bool((out == DR.SENTINEL).all()), "a rejected call wrote its output"


# ---- bd_gemm_nt --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.GEMM))
def test_gemm_nt(cabi, name):
    M, N, K, lda_pad, b_off, acc = R.GEMM[name]
    g = torch.Generator().manual_seed(R.seed_of(name))
    A, B, P = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(M, N, generator=g)
    Ad = DR.placed_input(A.cuda(), K + lda_pad)
    Bd = DR.placed_input(B.cuda(), K, b_off)
    Cd = DR.Placed(M, N, N + 3)
    if acc:
        Cd.view.copy_(P)
    f = R.gemm_form(M, N, K, K + lda_pad, K, (Ad.ptr % 16) // 4, (Bd.ptr % 16) // 4)
    assert name.startswith(f"g{f['RTM']}_{'dma' if f['dma'] else 'reg'}"), f
    cabi.check(cabi.lib.bd_gemm_nt(Ad.ptr, Ad.ld, Bd.ptr, Bd.ld, Cd.ptr, Cd.ld, M, N, K, acc, cabi.stream()))
    torch.cuda.synchronize()
    assert Cd.outside_unchanged(), "wrote outside C"
    ref, S = R.gemm_ref(A, B, P if acc else None)
    _report("gemm", name, DR.check_close(name, Cd.view.cpu(), ref, S), f"RTM{f['RTM']} vec={f['vec']} dma={f['dma']}")


# ---- gathered weight gradients -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n, c in R.WGRAD.items() if c.thin_env])
def test_gathered_wgrad(cabi, name):
    worst, body = R.gpu_wgrad_case(cabi, name, True)
    assert (body[0] == "thin") == name.startswith("wt_"), body
    _report("thin-wgrad" if body[0] == "thin" else "gathered-wgrad", name, worst, str(body))


def test_gathered_wgrad_thin_switched_off():
    res = _child("wgrad", {"BD_WGRAD_THIN": "0"})
    assert res["cases"] == sum(1 for c in R.WGRAD.values() if not c.thin_env) and res["worst"] <= DR.C_TOL


# ---- permutations, bit for bit -------------------------------------------------------------------------------------------

def test_pack_and_layout_permutations(cabi):
    from big_dreamer_amd import conv
    g = torch.Generator().manual_seed(17)
    for Co, Ci in R.PACK_CH:
        for k in (3, 4, 5, 6):
            stored = torch.randn(Co, k, k, Ci, generator=g)
            sd = stored.cuda()
            for py in range(2):
                for px in range(2):
                    want = R.pack_ref(R.class_matrix(stored, k, py, px))
                    dst = torch.full((want.numel() + 8,), DR.SENTINEL, device="cuda")
                    cabi.check(cabi.lib.bd_conv_pack_class(sd.data_ptr(), dst.data_ptr(), Co, Ci, k, py, px, R.taps(k, py),
                                                           R.taps(k, px), cabi.stream()))
                    assert torch.equal(dst.cpu(), torch.cat([want, torch.full((8,), DR.SENTINEL)])), (Co, Ci, k, py, px)
            want = R.pack_ref(R.fused_matrix(stored, k))
            dst = torch.full((want.numel() + 8,), DR.SENTINEL, device="cuda")
            conv.pack_fused(sd, dst, Co, Ci, k)
            assert torch.equal(dst.cpu(), torch.cat([want, torch.full((8,), DR.SENTINEL)])), (Co, Ci, k)
    for N, K, ld in R.PACK_W:
        src = torch.full((N, ld), float("nan"))
        src[:, :K] = torch.randn(N, K, generator=g)
        sd = src.cuda()
        for tr in (False, True):
            want = R.pack_weights_ref(src, N, K, tr)
            dst = torch.full((want.numel() + 8,), DR.SENTINEL, device="cuda")
            conv.pack_matrix(sd[:, :K], dst, N, K, tr)
            assert torch.equal(dst.cpu(), torch.cat([want, torch.full((8,), DR.SENTINEL)])), (N, K, ld, tr)
    for imgs, Cc, HW in R.LAYOUT:
        src = torch.randn(imgs * Cc * HW, generator=g)
        for to_nhwc in (1, 0):
            dst = torch.full((src.numel() + 8,), DR.SENTINEL, device="cuda")
            sd = src.cuda()
            cabi.check(cabi.lib.bd_image_layout(sd.data_ptr(), dst.data_ptr(), imgs, Cc, HW, to_nhwc, cabi.stream()))
            torch.cuda.synchronize()
            assert torch.equal(dst.cpu(), torch.cat([R.layout_ref(src, imgs, Cc, HW, bool(to_nhwc)), torch.full((8,), DR.SENTINEL)]))
