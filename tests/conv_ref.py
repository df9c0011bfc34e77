"""Float64 references, pack formulas, an fp32 emulation, a mirror of the host dispatch and the case tables for the tests of
the pixel kernels: csrc/conv.hip (bd_conv_gemm in its gather and patch forms, bd_conv_thin_forward, the two T-pattern
packs, bd_image_layout), csrc/gemm.hip (bd_gemm_nt) and the gathered / thin-image bodies of csrc/wgrad.hip.  Plain
helpers, not a conftest: tests/test_conv_ref_cpu.py uses them on CPU tensors, tests/test_conv_kernels_gpu.py and its child
tests/conv_env_worker.py on the device results copied to the host (every case is small).

References.  Each one is written from the index formula of include/bigdreamer_hip.h, not from torch's convolutions: the
im2col matrix A(m, k) with its mask, the output row of m, the fuse_cq column -> pixel map, the bias indexed by channel.
They return values over the FLAT output buffer (`FlatRef`: ref, S = |A| |W|^T + |b|, allow, written), so a wrong placement
(ldo, class parity, an odd row that does not exist) shows as a value where SENTINEL must stay.  The CPU test chains them
to F.conv2d / F.conv_transpose2d / autograd.

Tolerance: dense_ref.check_close with C_TOL and ACT_ALLOW unchanged: |got - ref| <= C_TOL * S (+ ACT_ALLOW for an ELU or
Tanh epilogue, ACT_ALLOW * |acc| for a _GRAD epilogue, as dense_ref.dgrad_ref states it).  ReLU: max(x, 0) is 1-Lipschitz,
so the bound holds for every element and none is left out of the comparison; the share of elements whose float64
pre-activation lies within C_TOL * S of 0 (where a kernel's ReLU' could legitimately differ from the reference's) is
still computed per ReLU case (`relu_ambiguous_share`) and held to RELU_CAP by the CPU test.  The _GRAD cases take f' from
a saved output that is itself act64 of a float64 pre-activation, so f' is exact there.

Dispatch mirror (`conv_form`, `thin_form`, `gemm_form`, `wgrad_plan_mirror`): plain Python restatements of the host code.
Held to the library: the LDS byte counts of `conv_form` (the "needs N B of LDS" errors of launch_conv_any /
launch_patch_any, CPU test) and the g_pad / splits / rows_per / tiles_n / tiles_k fields of `wgrad_plan_mirror`
(bd_wgrad_plan, CPU test with placeholder addresses, GPU test with the real ones); the rejections of `thin_form` are
checked against bd_conv_thin_forward's return codes on the GPU.  Restatement only (the library does not report them):
patch or gather and RT of bd_conv_gemm, the runs of row tiles per wave, KS / nrt / npc / ipw of the thin forward, RTM /
vec / DMA of bd_gemm_nt, KB of the thin weight-gradient body and the staged body names.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from tests.cnn_act_ref import act64, act_grad_from_out64
from tests.dense_ref import ACT_ALLOW, C_TOL, SENTINEL, cdiv, check_close, wgrad_body  # noqa: F401

D64 = torch.float64
ACT_CODE = {"none": 0, "ELU": 1, "ELU_GRAD": 2, "ReLU": 3, "ReLU_GRAD": 4, "Tanh": 5, "Tanh_GRAD": 6}
RELU_CAP = 1e-3          # largest share of a ReLU case whose float64 pre-activation is within C_TOL * S of 0
GUARD = 16               # NaN floats in front of and behind every input operand (keeps 16-byte alignment)


# ---- geometry (big_dreamer_amd/conv.py, restated so that the CPU test needs no library) -----------------------------

def conv_out(size: int, k: int) -> int:
    return (size - k) // 2 + 1


def convT_out(size: int, k: int) -> int:
    return (size - 1) * 2 + k


def taps(k: int, parity: int) -> int:
    return (k - parity + 1) // 2


def _log2(c: int) -> int:
    return c.bit_length() - 1 if c & (c - 1) == 0 else 0


def args_f(imgs, IH, IW, C, k, N, ldo=None, act="none"):
    """bd_conv_args of pattern F (conv.pattern_f), as a dict of the integer fields."""
    OH, OW = conv_out(IH, k), conv_out(IW, k)
    return dict(imgs=imgs, gh=OH, gw=OW, N=N, K=k * k * C, nseg=k, seglen=k * C, C=C, IH=IH, IW=IW, sy=2, y0=0, ss=1, sx=2,
                x0=0, mask=0, cshift=_log2(C), vec4=int(C % 4 == 0), OH=OH, OW=OW, osy=1, oy0=0, osx=1, ox0=0,
                ldo=ldo or N, act=ACT_CODE[act], fuse_cq=0)


def args_t_class(imgs, IH, IW, C, k, N, OH, OW, py, px, ldo=None, act="none"):
    """One parity class of pattern T (conv.pattern_t); None when the class has no pixel."""
    Ta, Tb = taps(k, py), taps(k, px)
    gh, gw = (OH - py + 1) // 2, (OW - px + 1) // 2
    if gh <= 0 or gw <= 0:
        return None
    return dict(imgs=imgs, gh=gh, gw=gw, N=N, K=Ta * Tb * C, nseg=Ta, seglen=Tb * C, C=C, IH=IH, IW=IW, sy=1, y0=0, ss=-1,
                sx=1, x0=-(Tb - 1), mask=1, cshift=_log2(C), vec4=1, OH=OH, OW=OW, osy=2, oy0=py, osx=2, ox0=px,
                ldo=ldo or N, act=ACT_CODE[act], fuse_cq=0)


def args_t_fused(imgs, IH, IW, C, k, Cq, OH, OW, ldo=None, act="none"):
    """The four classes in one launch (conv.pattern_t_fused): N = 4 * Cq columns."""
    T = (k + 1) // 2
    return dict(imgs=imgs, gh=(OH + 1) // 2, gw=(OW + 1) // 2, N=4 * Cq, K=T * T * C, nseg=T, seglen=T * C, C=C, IH=IH,
                IW=IW, sy=1, y0=0, ss=-1, sx=1, x0=-(T - 1), mask=1, cshift=_log2(C), vec4=1, OH=OH, OW=OW, osy=2, oy0=0,
                osx=2, ox0=0, ldo=ldo or Cq, act=ACT_CODE[act], fuse_cq=Cq)


# ---- pack / layout formulas ------------------------------------------------------------------------------------------

def pack_ref(W: torch.Tensor) -> torch.Tensor:
    """packed[nb][kb][lane][i] = W[nb*16 + (lane & 15)][kb*16 + 4*(lane >> 4) + i], zero padded (header, 'Weight layout')."""
    N, K = W.shape
    Nb, Kb = cdiv(N, 16), cdiv(K, 16)
    Wp = torch.zeros(Nb * 16, Kb * 16, dtype=W.dtype)
    Wp[:N, :K] = W
    lane, i = torch.arange(64), torch.arange(4)
    n = (torch.arange(Nb) * 16)[:, None, None, None] + (lane & 15)[None, None, :, None]
    k = (torch.arange(Kb) * 16)[None, :, None, None] + (4 * (lane >> 4))[None, None, :, None] + i[None, None, None, :]
    return Wp[n, k].reshape(-1)


def unpack_ref(packed: torch.Tensor, N: int, K: int) -> torch.Tensor:
    """Inverse of pack_ref (drops the padding)."""
    Nb, Kb = cdiv(N, 16), cdiv(K, 16)
    p = packed.reshape(Nb, Kb, 4, 16, 4)            # [nb][kb][lane >> 4][lane & 15][i]
    return p.permute(0, 3, 1, 2, 4).reshape(Nb * 16, Kb * 16)[:N, :K]


def pack_weights_ref(src: torch.Tensor, N: int, K: int, transpose: bool) -> torch.Tensor:
    """bd_pack_weights on the (N, K) sub-block of a row-major matrix view (ld = its row stride)."""
    W = src[:N, :K]
    return pack_ref(W.t() if transpose else W)


def class_matrix(stored: torch.Tensor, k: int, py: int, px: int, fault=None) -> torch.Tensor:
    """W[n = inner][(a, b', outer)] = stored[outer][py + 2a][px + 2(Tb - 1 - b')][inner] (bd_conv_pack_class)."""
    Co, _, _, Ci = stored.shape
    Ta, Tb = taps(k, py), taps(k, px)
    a, b, o = torch.arange(Ta), torch.arange(Tb), torch.arange(Co)
    ky = (py + 2 * a)[:, None, None].expand(Ta, Tb, Co)
    kx = (px + 2 * (b if fault == "x_not_reversed" else Tb - 1 - b))[None, :, None].expand(Ta, Tb, Co)
    oo = o[None, None, :].expand(Ta, Tb, Co)
    return stored[oo, ky, kx, :].reshape(Ta * Tb * Co, Ci).t().contiguous()


def fused_matrix(stored: torch.Tensor, k: int, fault=None) -> torch.Tensor:
    """W[n = cls*inner + c][(a, b', outer)] = stored[outer][py + 2a][px + 2(T - 1 - b')][c], 0 where ky or kx >= k."""
    Co, _, _, Ci = stored.shape
    T = (k + 1) // 2
    out = torch.zeros(4 * Ci, T * T * Co, dtype=stored.dtype)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        for a in range(T):
            for b in range(T):
                ky, kx = py + 2 * a, px + 2 * (b if fault == "x_not_reversed" else T - 1 - b)
                if ky < k and kx < k:
                    out[cls * Ci:(cls + 1) * Ci, (a * T + b) * Co:(a * T + b + 1) * Co] = stored[:, ky, kx, :].t()
    return out


def layout_ref(src: torch.Tensor, imgs: int, C: int, HW: int, to_nhwc: bool) -> torch.Tensor:
    """(imgs, C, HW) -> (imgs, HW, C) when to_nhwc, the reverse otherwise; flat."""
    if to_nhwc:
        return src.reshape(imgs, C, HW).permute(0, 2, 1).contiguous().reshape(-1)
    return src.reshape(imgs, HW, C).permute(0, 2, 1).contiguous().reshape(-1)


# ---- float64 references from the index formulas ----------------------------------------------------------------------

class FlatRef:
    """ref / S / allow over a flat output buffer of `size` floats; `written` marks the elements the kernel must store."""

    def __init__(self, size: int):
        self.ref = torch.zeros(size, dtype=D64)
        self.S = torch.zeros(size, dtype=D64)
        self.allow = torch.zeros(size, dtype=D64)
        self.pre = torch.zeros(size, dtype=D64)
        self.written = torch.zeros(size, dtype=torch.bool)

    def put(self, pos, ref, S, allow, pre):
        pos = pos.reshape(-1)
        assert int(pos.min()) >= 0 and int(pos.max()) < self.ref.numel(), "reference writes outside the output buffer"
        assert not bool(self.written[pos].any()) and pos.unique().numel() == pos.numel(), "an output element written twice"
        self.ref[pos], self.S[pos], self.allow[pos], self.pre[pos] = ref.reshape(-1), S.reshape(-1), allow.reshape(-1), pre.reshape(-1)
        self.written[pos] = True

    def check(self, name: str, got_flat: torch.Tensor, fill: float = SENTINEL) -> float:
        """`got_flat`: the whole output buffer after the launch.  Untouched elements must still hold `fill` (NaN: must
        still be NaN); the written ones pass check_close."""
        got = got_flat.detach().cpu()
        rest = got[~self.written]
        ok = torch.isnan(rest).all() if fill != fill else (rest == fill).all()
        assert bool(ok), f"{name}: wrote outside the output region"
        w = self.written
        return check_close(name, got[w], self.ref[w], self.S[w], self.allow[w])


def im2col(a: dict, inp: torch.Tensor, fault=None) -> torch.Tensor:
    """A(m, k) of the header: s = k / seglen, off = k % seglen; iy = y*sy + y0 + s*ss; ix0 = x*sx + x0;
    value = in[((img*IH + iy)*IW + ix0)*C + off], 0 outside the image when mask = 1.  inp: the flat image buffer."""
    gh, gw, C, IH, IW = a["gh"], a["gw"], a["C"], a["IH"], a["IW"]
    M = a["imgs"] * gh * gw
    m = torch.arange(M)
    img, rem = m // (gh * gw), m % (gh * gw)
    y, x = rem // gw, rem % gw
    k = torch.arange(a["K"])
    s, off = k // a["seglen"], k % a["seglen"]
    iy = (y * a["sy"] + a["y0"])[:, None] + (s * a["ss"])[None, :]
    ix0 = (x * a["sx"] + a["x0"])[:, None]
    ix = ix0 + (off // C)[None, :]
    stride = gw if fault == "rowstride_gw" else IW
    idx = ((img[:, None] * IH + iy) * stride + ix0) * C + off[None, :]
    ok = torch.ones(M, a["K"], dtype=torch.bool)
    if a["mask"]:
        lo_y, hi_y, lo_x, hi_x = 0, IH, 0, IW
        lo_y += fault == "mask_top"
        hi_y -= fault == "mask_bottom"
        lo_x += fault == "mask_left"
        hi_x -= fault == "mask_right"
        ok = (iy >= lo_y) & (iy < hi_y) & (ix >= lo_x) & (ix < hi_x)
    if fault is None:
        assert bool(((idx >= 0) & (idx < inp.numel()))[ok].all()), "an unmasked tap leaves the image buffer"
    A = torch.where(ok, inp.double()[idx.clamp(0, inp.numel() - 1)], torch.zeros((), dtype=D64))
    if fault == "drop_tap":             # the last tap of the last row: one border pixel, C of K terms
        A[M - 1, a["K"] - C:] = 0.0
    return A


def _act_name(code: int):
    name = {v: n for n, v in ACT_CODE.items()}[code]
    return (name[:-5], True) if name.endswith("_GRAD") else (name, False)


def conv_gemm_ref(a: dict, inp: torch.Tensor, Wm: torch.Tensor, bias, aux=None, size=None, fault=None, into=None) -> FlatRef:
    """bd_conv_gemm from the header's index formula.  Wm: the logical [N x K] weight matrix; aux: the flat saved-output
    buffer of a _GRAD code; size: floats of the output buffer (default imgs*OH*OW*ldo); into: a FlatRef to add to (the
    four class calls of pattern T share one output)."""
    N, OH, OW, ldo, cq = a["N"], a["OH"], a["OW"], a["ldo"], a["fuse_cq"]
    A = im2col(a, inp, fault)
    W64 = Wm.double()
    pre, S = A @ W64.t(), A.abs() @ W64.abs().t()
    M = A.shape[0]
    m = torch.arange(M)
    gh, gw = a["gh"], a["gw"]
    img, rem = m // (gh * gw), m % (gh * gw)
    y, x = rem // gw, rem % gw
    n = torch.arange(N)
    valid = torch.ones(M, N, dtype=torch.bool)
    if cq > 0:                          # column n = cls*cq + c -> pixel (2y + (cls >> 1), 2x + (cls & 1)), channel c
        cls, c = n // cq, n % cq
        py, px = (cls & 1, cls >> 1) if fault == "classes_swapped" else (cls >> 1, cls & 1)
        coff = (py * OW + px) * ldo + c
        bidx = n if fault == "bias_by_column" else c
        le = fault == "rowflag_le"
        fy = (2 * y + 1 <= OH) if le else (2 * y + 1 < OH)
        fx = (2 * x + 1 <= OW) if le else (2 * x + 1 < OW)
        valid = ((py == 0)[None, :] | fy[:, None]) & ((px == 0)[None, :] | fx[:, None])
    else:
        coff, bidx = n, n
    if bias is not None:
        b64 = bias.double()
        bidx = bidx.clamp(max=b64.numel() - 1)
        pre, S = pre + b64[bidx][None, :], S + b64[bidx].abs()[None, :]
    ld_row = N if fault == "ldo_as_N" else ldo
    rowoff = ((img * OH + y * a["osy"] + a["oy0"]) * OW + x * a["osx"] + a["ox0"]) * ld_row
    pos = rowoff[:, None] + coff[None, :]
    name, grad = _act_name(a["act"])
    if grad:
        f = act_grad_from_out64(name, aux.double()[pos.clamp(0, aux.numel() - 1)])
        f = torch.where(valid, f, torch.ones_like(f))
        ref, Sx, allow = pre * f, S * f.abs(), ACT_ALLOW * pre.abs()
    else:
        ref, Sx = act64(name, pre), S
        allow = torch.full_like(pre, ACT_ALLOW if name in ("ELU", "Tanh") else 0.0)
    out = into if into is not None else FlatRef(size if size is not None else a["imgs"] * OH * OW * ldo)
    if fault is not None:               # a faulted reference may collide or leave the buffer: keep what fits, collisions add
        sel = valid & (pos >= 0) & (pos < out.ref.numel())
        out.ref.index_put_((pos[sel],), ref[sel], accumulate=True)
        out.written[pos[sel]] = True
        return out
    out.put(pos[valid], ref[valid], Sx[valid], allow[valid], pre[valid])
    return out


def thin_matrix(imgs, IH, IW, C, k, inp: torch.Tensor, fault=None) -> torch.Tensor:
    """A(m, kidx) of bd_conv_thin_forward: ky = kidx / (k*C); value = in[(img*IH + 2y + ky)*IW*C + 2x*C + kidx - ky*k*C]."""
    gh, gw, K, roww = conv_out(IH, k), conv_out(IW, k), k * k * C, IW * C
    m = torch.arange(imgs * gh * gw)
    img, rem = m // (gh * gw), m % (gh * gw)
    y, x = rem // gw, rem % gw
    kidx = torch.arange(K)
    ky = kidx // k if fault == "thin_ky" else kidx // (k * C)
    aoff = ky * roww + (kidx - ky * k * C)
    idx = ((img * IH + 2 * y) * roww + 2 * x * C)[:, None] + aoff[None, :]
    if fault is None:
        assert int(idx.min()) >= 0 and int(idx.max()) < inp.numel()
    return inp.double()[idx.clamp(0, inp.numel() - 1)]


def thin_ref(imgs, IH, IW, C, k, inp, W, bias, act="none", aux=None, fault=None) -> FlatRef:
    """out (imgs, gh, gw, 32) = act(A W^T + bias); W: the plain [32 x K] matrix."""
    A = thin_matrix(imgs, IH, IW, C, k, inp, fault)
    W64 = W.double()
    pre, S = A @ W64.t(), A.abs() @ W64.abs().t()
    if bias is not None:
        pre, S = pre + bias.double()[None, :], S + bias.double().abs()[None, :]
    name, grad = _act_name(ACT_CODE[act])
    if grad:
        f = act_grad_from_out64(name, aux.double().reshape(-1, 32))
        ref, S, allow = pre * f, S * f.abs(), ACT_ALLOW * pre.abs()
    else:
        ref, allow = act64(name, pre), torch.full_like(pre, ACT_ALLOW if name in ("ELU", "Tanh") else 0.0)
    out = FlatRef(pre.numel())
    out.put(torch.arange(pre.numel()), ref, S, allow, pre)
    return out


def wgrad_matrix(d: dict, act_img: torch.Tensor, fault=None) -> torch.Tensor:
    """act(m, k) = act1[((img*g_IH + 2y + s)*g_IW + 2x)*g_C + off], s = k / g_seglen, off = k % g_seglen."""
    gh, gw = d["g_gh"], d["g_gw"]
    m = torch.arange(d["M"])
    img, rem = m // (gh * gw), m % (gh * gw)
    y, x = rem // gw, rem % gw
    k = torch.arange(d["K"])
    s, off = k // d["g_seglen"], k % d["g_seglen"]
    stride = gw if fault == "rowstride_gw" else d["g_IW"]
    idx = ((img[:, None] * d["g_IH"] + 2 * y[:, None] + s[None, :]) * stride + 2 * x[:, None]) * d["g_C"] + off[None, :]
    if fault is None:
        assert int(idx.min()) >= 0 and int(idx.max()) < act_img.numel()
    return act_img.double()[idx.clamp(0, act_img.numel() - 1)]


def wgrad_gathered_ref(d: dict, dpre: torch.Tensor, act_img: torch.Tensor, fault=None):
    """dW = dpre^T A, db = column sums of dpre, each with its sum|a*b| (float64)."""
    A, p = wgrad_matrix(d, act_img, fault), dpre.double()
    return p.t() @ A, p.abs().t() @ A.abs(), p.sum(0), p.abs().sum(0)


def gemm_ref(A, B, prior=None, fault=None):
    """C = A B^T (+ prior when accumulating); the prior value enters S."""
    A64, B64 = A.double(), B.double()
    if fault == "drop_last_kblock":
        K = A64.shape[1]
        keep = (cdiv(K, 32) - 1) * 32
        A64 = A64.clone()
        A64[:, keep:] = 0.0
    ref, S = A64 @ B64.t(), A.double().abs() @ B64.abs().t()
    if prior is not None:
        S = S + prior.double().abs()
        if fault != "ignore_accumulate":
            ref = ref + prior.double()
    return ref, S


# ---- fp32 emulation of the contractions (float32 operands, float32 sums in the kernels' K order) --------------------

def emu_dot(A: torch.Tensor, W: torch.Tensor, bias=None, chains: int = 2, strided: bool = True) -> torch.Tensor:
    """[M x N] float32.  K in blocks of 16; v_mfma_f32_16x16x4_f32 number i of a block takes k = 16 kb + 4 q + i over
    the four lane groups q (strided: the fragment order of conv.hip / gemm.hip) or k = 4 j .. 4 j + 3 (the thin kernels
    and the weight gradients, where the contraction index advances four rows or taps per instruction).  chains = 2: even
    i into one accumulator (which starts at the bias), odd i into a second, added at the end (conv_segment)."""
    A, W = A.float(), W.float()
    M, K = A.shape
    Kp = cdiv(K, 16) * 16
    Ap, Wp = torch.zeros(M, Kp), torch.zeros(W.shape[0], Kp)
    Ap[:, :K], Wp[:, :K] = A, W
    acc = torch.zeros(M, W.shape[0]) if bias is None else bias.float()[None, :].expand(M, -1).clone()
    acc2 = torch.zeros(M, W.shape[0])
    q = torch.arange(4)
    for kb in range(Kp // 16):
        for i in range(4):
            cols = kb * 16 + (4 * q + i if strided else 4 * i + q)
            p = Ap[:, cols] @ Wp[:, cols].t()
            if chains == 2 and (i & 1):
                acc2 = acc2 + p
            else:
                acc = acc + p
    return acc + acc2


def emu_wgrad(dpre: torch.Tensor, A: torch.Tensor, rows_per: int):
    """dW, db in float32: per row split a chain over its rows four at a time, then the splits in fixed order."""
    M = dpre.shape[0]
    dW = torch.zeros(dpre.shape[1], A.shape[1])
    db = torch.zeros(dpre.shape[1])
    ones = torch.ones(M, 1)
    for m0 in range(0, M, rows_per):
        sl = slice(m0, min(M, m0 + rows_per))
        dW = dW + emu_dot(dpre[sl].t(), A.float()[sl].t(), chains=1, strided=False)
        db = db + emu_dot(dpre[sl].t(), ones[sl].t(), chains=1, strided=False)[:, 0]
    return dW, db


def relu_ambiguous_share(fr: FlatRef) -> float:
    w = fr.written
    return float((fr.pre[w].abs() <= C_TOL * fr.S[w]).double().mean())


# ---- mirror of the host dispatch ---------------------------------------------------------------------------------------

K_MAX_LDS = 160 * 1024
K_CONV_WAVES = 8         # conv.hip is built with BD_WAVES = 8 (csrc/Makefile)


def _runs(nrt_list, Nb, cap):
    """Lengths of the runs of row tiles on one column block that the waves execute (conv_gemm_kernel / conv_patch_kernel)."""
    out = set()
    for nrt in nrt_list:
        U = nrt * Nb
        ub, urem = U // K_CONV_WAVES, U % K_CONV_WAVES
        for wave in range(K_CONV_WAVES):
            u = wave * ub + min(wave, urem)
            u1 = u + ub + (1 if wave < urem else 0)
            while u < u1:
                rt0 = u % nrt
                cnt = min(u1 - u, nrt - rt0, cap)
                out.add(cnt)
                u += cnt
    return out


def conv_form(a: dict, patch_env: bool = True) -> dict:
    """bd_conv_gemm (conv.hip): form 'patch' / 'gather', RT, the dynamic LDS request, whether it exceeds 64 KiB (the
    opt-in) or kMaxLds (rejected), and the run lengths of row tiles per wave."""
    M = a["imgs"] * a["gh"] * a["gw"]
    geom = (a["sy"] == 1 and a["sx"] == 1 and a["ss"] == -1) if a["mask"] else \
        (a["sy"] == 2 and a["sx"] == 2 and a["ss"] == 1 and a["x0"] == 0 and a["y0"] == 0)
    Nb = cdiv(a["N"], 16)
    if patch_env and a["C"] % 16 == 0 and a["gw"] >= 12 and a["N"] <= 128 and geom:
        span_y = a["nseg"] - 1 if a["ss"] < 0 else a["nseg"] - a["sy"]
        span_x = a["seglen"] // a["C"] - a["sx"]

        def patch_bytes(r):
            return (r * a["sy"] + span_y) * (16 * a["sx"] + span_x) * (a["C"] + 4) * 4
        rt = 8
        while rt > 1 and (rt // 2) * Nb >= 8:
            rt >>= 1
        while rt > 1 and patch_bytes(rt) > 56 * 1024:
            rt >>= 1
        if rt > a["gh"]:
            while rt > 1 and rt // 2 >= a["gh"]:
                rt >>= 1
        PH, PW = rt * a["sy"] + span_y, 16 * a["sx"] + span_x
        lds = (PH * PW * (a["C"] + 4) + (a["K"] >> 4) + rt + 32 * rt) * 4
        nrts = {min(rt, a["gh"] - y0) for y0 in range(0, a["gh"], rt)}
        return dict(form="patch", RT=rt, lds=lds, big=lds > 64 * 1024, rejected=lds > K_MAX_LDS, runs=_runs(nrts, Nb, 2),
                    tiles_x=cdiv(a["gw"], 16), ragged_x=a["gw"] % 16 != 0)
    Kb = cdiv(a["K"], 16)
    rt = 8
    while rt > 1 and (rt * Kb * 256 + 32 * rt) * 4 > 150 * 1024:
        rt >>= 1
    lds = (rt * Kb * 256 + 32 * rt) * 4
    nrts = {min(rt, cdiv(M - r0, 16)) for r0 in range(0, M, 16 * rt)}
    return dict(form="gather", RT=rt, lds=lds, big=lds > 64 * 1024, rejected=lds > K_MAX_LDS, runs=_runs(nrts, Nb, 4),
                blocks=cdiv(M, 16 * rt))


def thin_form(imgs, IH, IW, C, k, ldw=None, in_al16=True) -> dict:
    """bd_conv_thin_forward: the rejection it answers with, or KS (12 / 27), nrt, npc (1 KiB DMA pieces per band), ipw."""
    if not (imgs > 0 and 1 <= C <= 4 and k >= 2 and IH >= k and IW >= k):
        return dict(reject="bad arguments")
    K, gh, gw, roww = k * k * C, conv_out(IH, k), conv_out(IW, k), IW * C
    if K > 108 or (ldw is not None and ldw < K) or gw > 32:
        return dict(reject="K =")
    if roww % 4 or not in_al16:
        return dict(reject="16-byte aligned")
    band_al = (k * roww + 64 + 255) & ~255
    ipw = cdiv(imgs, 512)
    return dict(reject=None, KS=12 if K <= 48 else 27, K=K, gh=gh, gw=gw, nrt=cdiv(gw, 16), npc=cdiv(k * roww, 256), ipw=ipw,
                grid=cdiv(imgs, ipw), lds=8 * 2 * band_al * 4)


def gemm_form(M, N, K, lda, ldb, a_off=0, b_off=0, dma_env=True) -> dict:
    """bd_gemm_nt: RTM by the rounds-times-work cost, the vec bits, DMA or register-staged (a_off / b_off: float offsets
    of the operands from a 16-byte boundary)."""
    vec = (1 if K % 4 == 0 and lda % 4 == 0 and a_off % 4 == 0 else 0) | (2 if K % 4 == 0 and ldb % 4 == 0 and b_off % 4 == 0 else 0)
    ntn = cdiv(N, 64)
    best, best_cost = 10, 1e30
    for rtm in (10, 8, 6, 4):
        wgs = cdiv(M, 16 * rtm) * ntn
        cost = cdiv(wgs, 256) * rtm * (1.0 + 0.25 / rtm)
        if cost < best_cost:
            best, best_cost = rtm, cost
    return dict(RTM=best, vec=vec, dma=vec == 3 and K % 16 == 0 and dma_env, steps=cdiv(K, 32))


def gathered_desc(imgs, gh, gw, IH, IW, C, k, N, bias=True) -> dict:
    """The integer fields of a gathered bd_wgrad_desc (conv.wgrad_desc)."""
    return dict(M=imgs * gh * gw, N=N, K=k * k * C, bias=bias, ldp=N, g_nseg=k, g_seglen=k * C, g_gh=gh, g_gw=gw, g_IH=IH,
                g_IW=IW, g_C=C, lda1=0, act_al16=True, dpre_al16=True)


def _act16(d):
    if d["K"] % 4 or not d["act_al16"]:
        return False
    if d["g_nseg"] > 0:
        return d["g_C"] % 4 == 0 and d["g_seglen"] % 4 == 0
    return d["lda1"] % 4 == 0


def wgrad_thin_ok(d) -> bool:
    if d["g_nseg"] <= 0 or d["g_C"] > 4 or d["N"] != 32 or d["ldp"] != 32 or d["g_gw"] > 32:
        return False
    if cdiv(d["K"], 16) > 7 or d["g_seglen"] != d["g_nseg"] * d["g_C"]:
        return False
    roww = d["g_IW"] * d["g_C"]
    if roww % 4 or not d["act_al16"] or not d["dpre_al16"]:
        return False
    band = (d["g_nseg"] * roww + 64 + 255) & ~255
    return 8 * 2 * (band + 1024) * 4 <= 147456


def _tiles_k(NB, KB, deep_ok):
    if KB <= 13:
        return 1
    return cdiv(KB, 36) if NB <= 4 and deep_ok else cdiv(KB, 12)


def wgrad_plan_mirror(descs, thin_on: bool = True):
    """bd_wgrad_plan in its default (wide) form for single-source descriptors: per descriptor g_pad, splits, rows_per,
    tiles_n, tiles_k and the body: ('thin', KB, ipw) or ('staged', body names of dense_ref.wgrad_body)."""
    def geo(d):
        NB, KB = cdiv(d["N"], 16), cdiv(d["K"] + int(d["bias"]), 16)
        tn, tk = cdiv(NB, 13), _tiles_k(NB, KB, _act16(d))
        nb, kb = cdiv(NB, tn), cdiv(KB, tk)
        hn, kq, kr = (nb + 1) >> 1, kb >> 2, kb & 3
        c = hn * ((kq + (1 if kr > 0 else 0)) + (kq + (1 if kr > 2 else 0)))
        return tn, tk, (c if c > 0 else 1) + 12

    def thin(d):
        return thin_on and wgrad_thin_ok(d)

    def rows_for(d, T):
        r = (int(T / geo(d)[2]) // 16) * 16
        return min(max(r, 64), 1 << 22)

    def blocks_for(T):
        b = 0
        for d in descs:
            if thin(d):
                imgs = d["M"] // (d["g_gh"] * d["g_gw"])
                b += cdiv(imgs, cdiv(imgs, 256))
            else:
                tn, tk, _ = geo(d)
                b += tn * tk * cdiv(d["M"], rows_for(d, T))
        return b

    rows_wide = 128
    while sum(geo(d)[0] * geo(d)[1] * cdiv(d["M"], rows_wide) for d in descs) > 256 and rows_wide < (1 << 20):
        rows_wide += 16
    budget = 0.0
    if any(d["g_nseg"] > 0 for d in descs):
        Wk = sum(float(geo(d)[0] * geo(d)[1]) * d["M"] * geo(d)[2] for d in descs)
        R = min(max(Wk / (256.0 * 1024.0 * 61.0), 1.0), 24.0)
        rounds = int(R + 0.999)
        budget = Wk / (256.0 * rounds)
        target = 256 * rounds
        if blocks_for(budget * 8.0) > target:
            target += 256
        it = 0
        while it < 200 and blocks_for(budget) > target:
            budget *= 1.02
            it += 1
    out = []
    for d in descs:
        if thin(d):
            px = d["g_gh"] * d["g_gw"]
            imgs = d["M"] // px
            ipw = cdiv(imgs, 256)
            out.append(dict(g_pad=1, tiles_n=1, tiles_k=1, rows_per=ipw * px, splits=cdiv(imgs, ipw),
                            body=("thin", 3 if cdiv(d["K"], 16) <= 3 else 7, ipw)))
        else:
            tn, tk, _ = geo(d)
            rp = rows_for(d, budget) if budget > 0.0 else rows_wide
            out.append(dict(g_pad=0, tiles_n=tn, tiles_k=tk, rows_per=rp, splits=cdiv(d["M"], rp),
                            body=("staged", frozenset(wgrad_body(d["N"], d["K"], d["bias"], _act16(d), False)))))
    return out


class FCase(NamedTuple):
    imgs: int
    IH: int
    IW: int
    C: int
    k: int
    N: int
    bias: bool
    act: str
    ldo_pad: int


class TCase(NamedTuple):
    imgs: int
    IH: int
    IW: int
    C: int
    k: int
    N: int
    OH: int
    OW: int
    bias: bool


class PatchF(NamedTuple):
    kind: str
    imgs: int
    gh: int
    gw: int
    C: int
    k: int
    N: int
    extra: int


class PatchT(NamedTuple):
    kind: str
    imgs: int
    IH: int
    IW: int
    C: int
    k: int
    Cq: int
    OH: int
    OW: int


class ThinCase(NamedTuple):
    imgs: int
    IH: int
    IW: int
    C: int
    k: int
    bias: bool
    act: str
    ldw_pad: int
    w_off: int


class ThinReject(NamedTuple):
    imgs: int
    IH: int
    IW: int
    C: int
    k: int
    in_off: int


class GemmCase(NamedTuple):
    M: int
    N: int
    K: int
    lda_pad: int
    b_off: int
    accumulate: int


class WgradGeo(NamedTuple):
    imgs: int
    gh: int
    gw: int
    extra: int
    C: int
    k: int
    N: int
    bias: bool
    window: object
    thin_env: bool


# ---- case tables (the GPU test runs them, the CPU test proves the references and the coverage on them) ---------------
# Shapes are the smallest that reach each path; a few image widths exceed 20 where a row count (M = 16 RT + 1) or a grid
# width (gw = 17 / 31 of the patch form) needs it.

# name: (imgs, IH, IW, C, k, N, bias, act, ldo_pad)
GATHER_F = {
    "f_c3k4_scalar":   FCase(2, 10, 12, 3, 4, 3, True, "ELU", 0),         # scalar gather, N = 3
    "f_c6k3_m45":      FCase(5, 7, 7, 6, 3, 20, False, "none", 3),        # C not a power of two, K = 54 ragged, M = 45 ragged
    "f_c4k3_unused":   FCase(1, 20, 18, 4, 3, 33, True, "Tanh", 0),       # vec4 K = 36, (size - k) odd both ways, IH != IW
    "f_c12k3":         FCase(2, 9, 11, 12, 3, 3, True, "ReLU", 5),        # vec4 with cshift = 0
    "f_runs4":         FCase(2, 19, 19, 4, 3, 64, True, "none", 0),       # M = 162: a full 8-tile block (runs of 4) + 3 tiles
    "f_runs3":         FCase(1, 13, 17, 4, 3, 128, False, "ELU", 0),      # M = 48: 3 row tiles x 8 column blocks (runs of 3)
    "f_k512_rt4":      FCase(2, 8, 12, 32, 4, 256, True, "none", 0),      # K = 512, gw = 5
    "f_k1024_m33":     FCase(3, 4, 24, 64, 4, 20, True, "ReLU", 0),       # K = 1024, RT = 2, M = 33 = 16 RT + 1
    "f_k2048_rt1":     FCase(1, 6, 10, 128, 4, 33, False, "none", 0),     # K = 2048, RT = 1, 128 KiB of LDS
}

# name: (imgs, IH, IW, Cin, k, N, OH, OW, bias): per class and fused.  OH = convT_out + 1 is the dgrad of a conv whose
# last input row no window covers (the pixels must come out exactly 0, so no bias there); OH = convT_out - 1 crops.
T_GATHER = {
    "t_k3":  TCase(2, 3, 4, 4, 3, 3, 7, 8, True),          # convT_out 7 x 9: OW cropped, OH odd / OW even
    "t_k4":  TCase(1, 4, 3, 8, 4, 12, 11, 8, False),       # convT_out 10 x 8: an uncovered last row
    "t_k5":  TCase(3, 3, 5, 16, 5, 20, 9, 13, True),       # Cin = 16 on the gather form (class grid 7 wide)
    "t_k6":  TCase(2, 4, 4, 4, 6, 3, 12, 13, False),       # convT_out 12 x 12: an uncovered last column
}

# name: ("F", imgs, gh, gw, C, k, N, extra) with IH = 2(gh-1)+k+extra, IW likewise  |
#       ("T", imgs, IH, IW, Cin, k, Cq, OH, OW)
PATCH = {
    "pf_rt8":   PatchF("F", 2, 9, 17, 16, 4, 16, 0),        # gh = RT + 1, ragged second 16-column tile
    "pf_rt4":   PatchF("F", 1, 3, 12, 32, 4, 32, 1),
    "pf_rt2":   PatchF("F", 1, 3, 31, 16, 3, 64, 1),
    "pf_rt1":   PatchF("F", 2, 2, 16, 16, 4, 128, 0),
    "pf_gh1":   PatchF("F", 1, 1, 16, 16, 4, 16, 0),
    "pf_n48":   PatchF("F", 1, 4, 12, 16, 4, 48, 0),        # 4 row tiles x 3 column blocks: 12 units, runs of 2 (patch_segment<2>)
    "pf_gw11":  PatchF("F", 1, 3, 11, 16, 4, 16, 0),        # the gather-form neighbour
    "pt_rt8":   PatchT("T", 1, 8, 16, 16, 4, 4, 18, 34),    # class grid 9 x 17
    "pt_rt4":   PatchT("T", 1, 1, 10, 32, 5, 8, 5, 23),     # odd k: zero taps; odd OH / OW: no odd last row / column; grid 3 x 12
    "pt_rt2":   PatchT("T", 2, 1, 13, 16, 6, 16, 6, 31),    # an uncovered last column; grid 3 x 16
    "pt_rt1":   PatchT("T", 1, 2, 30, 16, 3, 32, 5, 61),    # grid 3 x 31
}

# _GRAD epilogues: (family, case name) x the three activations
GRAD_ON = [("gather_f", "f_c6k3_m45"), ("t_fused", "t_k3"), ("patch", "pt_rt4"), ("patch", "pf_rt2"), ("thin", "th_c3k4_gw17")]

# name: (imgs, IH, IW, C, k, bias, act, ldw_pad, w_off)
THIN = {
    "th_c1k3_gw1":   ThinCase(9, 7, 4, 1, 3, True, "none", 0, 0),
    "th_c2k4_gw5":   ThinCase(1, 10, 12, 2, 4, False, "ELU", 3, 1),          # ldw > K, weights at an odd float offset
    "th_c3k4_gw17":  ThinCase(2, 9, 36, 3, 4, True, "ReLU", 0, 3),
    "th_c4k4_gw16":  ThinCase(2, 6, 34, 4, 4, True, "Tanh", 1, 0),
    "th_c3k6_gw32":  ThinCase(1, 9, 68, 3, 6, False, "none", 0, 0),          # K = 108
    "th_c4k5_gw5":   ThinCase(9, 8, 13, 4, 5, True, "ELU", 0, 5),            # KS = 27 with K = 100
    "th_513":        ThinCase(513, 8, 8, 3, 4, True, "none", 0, 0),          # ipw = 2, the last workgroup has one image
}
# rejections: name -> (imgs, IH, IW, C, k, input offset in floats).  k*k*C = 112 has no solution for C <= 4, so the
# K > 108 case is C = 4, k = 6 (K = 144).
THIN_REJECT = {
    "gw33":    ThinReject(1, 6, 70, 2, 6, 0),
    "K144":    ThinReject(1, 8, 8, 4, 6, 0),
    "roww30":  ThinReject(1, 8, 10, 3, 4, 0),
    "in_off1": ThinReject(1, 8, 8, 3, 4, 1),
    "C5":      ThinReject(1, 8, 8, 5, 3, 0),
}

# name: (M, N, K, lda_pad, b_off, accumulate)
GEMM = {
    "g4_dma":       GemmCase(65, 63, 48, 0, 0, 0),
    "g4_dma_k16":   GemmCase(1, 1, 16, 4, 0, 1),
    "g4_reg_k1":    GemmCase(1, 65, 1, 0, 0, 0),
    "g4_reg_k33":   GemmCase(65, 65, 33, 0, 1, 1),
    "g6_dma":       GemmCase(8193, 65, 16, 0, 0, 1),
    "g6_reg_k20":   GemmCase(8193, 65, 20, 0, 0, 0),
    "g8_dma":       GemmCase(12289, 65, 32, 4, 0, 0),
    "g8_reg_lda":   GemmCase(12289, 65, 16, 1, 0, 1),
    "g10_dma":      GemmCase(16385, 65, 48, 0, 0, 1),
    "g10_reg_k33":  GemmCase(16385, 65, 33, 0, 1, 0),
}

# name: (imgs, gh, gw, extra, C, k, N, bias, window, thin_env): IH = 2(gh-1)+k+extra.  window: None, 'last' (dpre
# nonzero only in the last pixel of the last image), 'first' (only in the first pixel of image 1).
WGRAD = {
    "w_c4k3_n3":      WgradGeo(3, 3, 5, 1, 4, 3, 3, True, None, True),
    "w_c16k4_n64":    WgradGeo(2, 5, 3, 0, 16, 4, 64, False, None, True),
    "w_c32k6_deep":   WgradGeo(2, 3, 5, 0, 32, 6, 32, True, None, True),
    "w_c4k4_n208":    WgradGeo(2, 3, 7, 1, 4, 4, 208, True, None, True),
    "w_c16k4_last":   WgradGeo(3, 5, 3, 0, 16, 4, 64, True, "last", True),
    "w_c4k3_first":   WgradGeo(3, 3, 5, 1, 4, 3, 64, True, "first", True),
    "w_c3k4_staged":  WgradGeo(9, 3, 17, 0, 3, 4, 32, True, None, False),    # BD_WGRAD_THIN=0 (child process)
    "w_c3k4_staged_last": WgradGeo(9, 3, 17, 0, 3, 4, 32, False, "last", False),
    "wt_c3k4_gw17":   WgradGeo(9, 3, 17, 0, 3, 4, 32, True, None, True),
    "wt_c3k6_gw16":   WgradGeo(9, 1, 16, 0, 3, 6, 32, False, None, True),
    "wt_c4k4_257":    WgradGeo(257, 3, 5, 0, 4, 4, 32, True, None, True),    # ipw = 2 with a ragged last workgroup
    "wt_c1k6_gw32":   WgradGeo(1, 2, 32, 0, 1, 6, 32, True, None, True),
    "wt_c3k4_last":   WgradGeo(9, 3, 17, 0, 3, 4, 32, True, "last", True),
    "wt_c4k4_first":  WgradGeo(9, 3, 5, 0, 4, 4, 32, True, "first", True),
}

# (Couter, Cinner) of the pack cases, each with k = 3 .. 6
PACK_CH = [(5, 3), (20, 12)]
PACK_W = [(20, 37, 41), (33, 16, 16), (3, 70, 75)]          # (N, K, ld), both transposes
LAYOUT = [(1, 1, 63), (1, 3, 130), (2, 32, 63)]            # (imgs, C, HW)


def wgrad_geometry(name):
    imgs, gh, gw, extra, C, k, N, bias, window, thin_env = WGRAD[name]
    IH, IW = 2 * (gh - 1) + k + extra, 2 * (gw - 1) + k + extra
    if (IW * C) % 4 and thin_env and C <= 4:
        IW += 1
    return dict(imgs=imgs, gh=gh, gw=gw, IH=IH, IW=IW, C=C, k=k, N=N, bias=bias, window=window, thin_env=thin_env)


def patch_args(name, act="none", ldo_pad=0):
    """(args dict, input shape (imgs, IH, IW, C), stored-weight shape, N of the logical output) of a PATCH case."""
    c = PATCH[name]
    if c.kind == "F":
        _, imgs, gh, gw, C, k, N, extra = c
        IH, IW = 2 * (gh - 1) + k + extra, 2 * (gw - 1) + k + extra
        return args_f(imgs, IH, IW, C, k, N, N + ldo_pad, act), (imgs, IH, IW, C), (N, k, k, C)
    _, imgs, IH, IW, C, k, Cq, OH, OW = c
    return args_t_fused(imgs, IH, IW, C, k, Cq, OH, OW, Cq + ldo_pad, act), (imgs, IH, IW, C), (C, k, k, Cq)


def make_inputs(seed: int, in_shape, w_shape, n_bias, w_scale=0.3):
    """Deterministic CPU float32 operands of one conv case: image, stored weight, bias."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*in_shape, generator=g)
    w = torch.randn(*w_shape, generator=g) * w_scale
    b = torch.randn(n_bias, generator=g)
    return x, w, b


def poison_unused(x: torch.Tensor, k: int) -> torch.Tensor:
    """NaN in the last image row / column that no stride-2 window of size k covers (pattern F, thin, gathered wgrad)."""
    x = x.clone()
    _, IH, IW, _ = x.shape
    if (IH - k) % 2:
        x[:, IH - 1] = float("nan")
    if (IW - k) % 2:
        x[:, :, IW - 1] = float("nan")
    return x


def seed_of(name: str) -> int:
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


# ---- case builders ---------------------------------------------------------------------------------------------------

def build_gather_f(name, act=None):
    """(args, image with its unused last row / column NaN, stored weight (N, k, k, C), bias or None)."""
    imgs, IH, IW, C, k, N, bias, act0, pad = GATHER_F[name]
    a = args_f(imgs, IH, IW, C, k, N, N + pad, act or act0)
    x, w, b = make_inputs(seed_of(name), (imgs, IH, IW, C), (N, k, k, C), N)
    return a, poison_unused(x, k), w, (b if bias else None)


def build_t(name):
    """(geometry dict, image, stored weight (Cin, k, k, N), bias or None) of a T_GATHER case."""
    imgs, IH, IW, C, k, N, OH, OW, bias = T_GATHER[name]
    x, w, b = make_inputs(seed_of(name), (imgs, IH, IW, C), (C, k, k, N), N)
    return dict(imgs=imgs, IH=IH, IW=IW, C=C, k=k, N=N, OH=OH, OW=OW), x, w, (b if bias else None)


def build_patch(name, act="none", ldo_pad=0, patch_bias=True):
    a, in_shape, w_shape = patch_args(name, act, ldo_pad)
    nb = a["fuse_cq"] if a["fuse_cq"] else a["N"]
    x, w, b = make_inputs(seed_of(name), in_shape, w_shape, nb)
    if PATCH[name].kind == "F":
        x = poison_unused(x, PATCH[name].k)
    uncovered = PATCH[name].kind == "T" and (a["OH"] > convT_out(a["IH"], PATCH[name].k) or a["OW"] > convT_out(a["IW"], PATCH[name].k))
    return a, x, w, (b if patch_bias and not uncovered else None)


def conv_weight_matrix(a: dict, stored: torch.Tensor, k: int, fault=None) -> torch.Tensor:
    """The logical [N x K] matrix a bd_conv_args reads: the stored tensor itself (pattern F), one class or all four (T)."""
    if not a["mask"]:
        return stored.reshape(stored.shape[0], -1)
    if a["fuse_cq"]:
        return fused_matrix(stored, k, fault)
    return class_matrix(stored, k, a["oy0"], a["ox0"], fault)


def t_class_refs(g: dict, x, stored, bias, ldo=None, size=None, fault=None) -> FlatRef:
    """The four class calls of pattern T into one output."""
    out = FlatRef(size if size is not None else g["imgs"] * g["OH"] * g["OW"] * (ldo or g["N"]))
    for py in range(2):
        for px in range(2):
            a = args_t_class(g["imgs"], g["IH"], g["IW"], g["C"], g["k"], g["N"], g["OH"], g["OW"], py, px, ldo)
            if a is not None:
                conv_gemm_ref(a, x.reshape(-1), class_matrix(stored, g["k"], py, px, fault), bias, fault=fault, into=out)
    return out


# ---- GPU runners (shared by tests/test_conv_kernels_gpu.py and its child tests/conv_env_worker.py) -------------------
# Inputs sit inside NaN buffers (GUARD floats in front and behind; weight rows padded with NaN where ldw > K; the image
# row / column no window covers is NaN): every kernel here is specified to read the taps of valid output pixels only,
# or, where it reads more (the patch copy, the thin kernels' whole-band DMA, row tiles beyond M), to keep what it read
# out of every stored value -- a NaN that reaches an output fails the comparison.  Nothing is placed where a kernel may
# read beyond the operand's own buffer.  Outputs are SENTINEL-filled with TAIL floats behind the logical extent.

TAIL = 64


def dev_input(x: torch.Tensor, off: int = 0):
    """(buffer, view): the flat operand at float offset GUARD + off of a NaN-filled device buffer."""
    n = x.numel()
    buf = torch.full((GUARD + off + n + GUARD,), float("nan"), device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.copy_(x.reshape(-1))
    return buf, view


def dev_pack(cabi, a: dict, stored: torch.Tensor, k: int) -> torch.Tensor:
    """The packed weights of one launch, made by the library's own pack kernels from the stored tensor."""
    from big_dreamer_amd import conv
    sd = stored.contiguous().cuda()
    if not a["mask"]:
        dst = torch.zeros(cabi.packed_floats(a["N"], a["K"]), device="cuda")
        conv.pack_matrix(sd.view(a["N"], a["K"]), dst, a["N"], a["K"])
    elif a["fuse_cq"]:
        dst = torch.zeros(conv.fused_pack_floats(stored.shape[0], stored.shape[3], k), device="cuda")
        conv.pack_fused(sd, dst, stored.shape[0], stored.shape[3], k)
    else:
        py, px = a["oy0"], a["ox0"]
        dst = torch.zeros(cabi.packed_floats(a["N"], a["K"]), device="cuda")
        cabi.check(cabi.lib.bd_conv_pack_class(sd.data_ptr(), dst.data_ptr(), stored.shape[0], stored.shape[3], k, py, px,
                                               taps(k, py), taps(k, px), cabi.stream()))
    torch.cuda.synchronize()
    return dst


def out_size(a: dict) -> int:
    return a["imgs"] * a["OH"] * a["OW"] * a["ldo"] + TAIL


def run_conv(cabi, a: dict, x: torch.Tensor, packed: torch.Tensor, bias, aux=None, out=None) -> torch.Tensor:
    """One bd_conv_gemm launch; returns the whole output buffer (SENTINEL-prefilled unless `out` is given)."""
    import ctypes as C
    keep = dev_input(x)
    if out is None:
        out = torch.full((out_size(a),), SENTINEL, device="cuda")
    s = cabi.ConvArgs()
    for f, v in a.items():
        setattr(s, f, v)
    bd = None if bias is None else bias.cuda()
    ad = None if aux is None else aux.float().cuda()
    s.in_, s.out, s.w = keep[1].data_ptr(), out.data_ptr(), packed.data_ptr()
    s.bias = None if bd is None else bd.data_ptr()
    s.aux = None if ad is None else ad.data_ptr()
    cabi.check(cabi.lib.bd_conv_gemm(C.byref(s), cabi.stream()))
    torch.cuda.synchronize()
    return out


def saved_outputs(fr: FlatRef, name: str, seed: int) -> torch.Tensor:
    """A saved-output buffer for a _GRAD code: act(name) of float64 normal pre-activations (both signs; exact zeros for
    ReLU) where the launch stores, NaN everywhere else."""
    g = torch.Generator().manual_seed(seed)
    aux = torch.full((fr.ref.numel(),), float("nan"), dtype=D64)
    aux[fr.written] = act64(name, torch.randn(int(fr.written.sum()), generator=g, dtype=D64)).float().double()
    return aux


def gpu_patch_case(cabi, name: str):
    """One PATCH case end to end: (whole output buffer on the host, worst err / bound)."""
    a, x, w, b = build_patch(name, ldo_pad=1)
    k = PATCH[name].k
    fr = conv_gemm_ref(a, x.reshape(-1), conv_weight_matrix(a, w, k), b, size=out_size(a))
    got = run_conv(cabi, a, x, dev_pack(cabi, a, w, k), b).cpu()
    return got, fr.check(name, got)


def wgrad_inputs(name: str):
    """(geometry, descriptor fields, dpre [M x N], image) of a WGRAD case on the host."""
    g = wgrad_geometry(name)
    d = gathered_desc(g["imgs"], g["gh"], g["gw"], g["IH"], g["IW"], g["C"], g["k"], g["N"], g["bias"])
    gen = torch.Generator().manual_seed(seed_of(name))
    dpre = torch.randn(d["M"], g["N"], generator=gen)
    img = poison_unused(torch.randn(g["imgs"], g["IH"], g["IW"], g["C"], generator=gen), g["k"])
    if g["window"] is not None:
        mask = torch.zeros(d["M"], 1)
        mask[d["M"] - 1 if g["window"] == "last" else g["gh"] * g["gw"]] = 1.0
        dpre = dpre * mask
    return g, d, dpre, img


def gpu_wgrad_case(cabi, name: str, thin_on: bool):
    """One gathered weight gradient through bd_wgrad_plan + bd_wgrad_grouped (NaN slab workspace, dW / db inside a
    SENTINEL buffer with ldw > K); the plan's fields against the mirror.  Returns (worst err / bound, body)."""
    import ctypes as C
    g, d, dpre, img = wgrad_inputs(name)
    N, K = d["N"], d["K"]
    dp = dpre.cuda().contiguous()
    keep = dev_input(img)
    ldw, w_off = K + 3, 5
    flat = torch.full((w_off + N * ldw + N + 8,), SENTINEL, device="cuda")
    s = cabi.WgradDesc()
    s.dpre, s.ldp, s.act1, s.lda1, s.M1, s.M, s.N, s.K = dp.data_ptr(), N, keep[1].data_ptr(), 0, d["M"], d["M"], N, K
    s.dW, s.ldw = flat.data_ptr() + 4 * w_off, ldw
    s.db = flat.data_ptr() + 4 * (w_off + N * ldw) if d["bias"] else None
    for f in ("g_nseg", "g_seglen", "g_gh", "g_gw", "g_IH", "g_IW", "g_C"):
        setattr(s, f, d[f])
    arr = (cabi.WgradDesc * 1)(s)
    tb, tr, wsf = C.c_int(0), C.c_int(0), C.c_size_t(0)
    cabi.check(cabi.lib.bd_wgrad_plan(arr, 1, C.byref(tb), C.byref(tr), C.byref(wsf)))
    d["act_al16"], d["dpre_al16"] = keep[1].data_ptr() % 16 == 0, dp.data_ptr() % 16 == 0
    plan = wgrad_plan_mirror([d], thin_on)[0]
    got = {f: getattr(arr[0], f) for f in ("g_pad", "tiles_n", "tiles_k", "rows_per", "splits")}
    assert got == {f: plan[f] for f in got}, (name, got, plan)
    table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to("cuda")
    ws = torch.full((max(1, wsf.value),), float("nan"), device="cuda")
    cabi.check(cabi.lib.bd_wgrad_grouped(table.data_ptr(), 1, tb.value, tr.value, ws.data_ptr(), cabi.stream()))
    torch.cuda.synchronize()
    out = flat.cpu()
    dW = out[w_off:w_off + N * ldw].view(N, ldw)[:, :K]
    t = out.clone()
    t[w_off:w_off + N * ldw].view(N, ldw)[:, :K] = SENTINEL
    if d["bias"]:
        t[w_off + N * ldw:w_off + N * ldw + N] = SENTINEL
    assert bool((t == SENTINEL).all()), f"{name}: wrote outside dW / db"
    rW, sW, rb, sb = wgrad_gathered_ref(d, dpre, img.reshape(-1))
    worst = check_close(f"{name} dW", dW, rW, sW)
    if d["bias"]:
        worst = max(worst, check_close(f"{name} db", out[w_off + N * ldw:w_off + N * ldw + N], rb, sb))
    return worst, plan["body"]
