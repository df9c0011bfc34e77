"""Float64 reference, tolerance, case builder and restated host dispatch for the fused imagined-heads kernel
(csrc/heads.hip, bd_img_heads_fwd_bwd), and a restatement of the MFMA-fragment weight layout (csrc/cabi.hip,
bd_pack_weights).  Plain helpers in the style of tests/dense_ref.py, not a conftest: the CPU sharpness test builds the
cases on CPU tensors, the GPU tests on device tensors.

Tolerance: the hidden activations never leave the chip, so the kernel is held end to end: |got - ref| <= HEADS_C_TOL * S,
componentwise, with S the sum of absolute products of the LAST contraction only (|a_4| . |w_out| + |b_out| for a head's
output, |g_0^r| |W_0^r| + |g_0^v| |W_0^v| for dx).  A worst-case bound propagated through the chain is useless (the |W|
row sums multiply it by ~11 per layer at Hd = 200).  The bound is therefore empirical, not rigorous: what reaches dx
besides the last contraction's own rounding is the relative error of g_0, and that averages out over the columns of a
wide layer but not of a narrow one -- ELU' = a + 1 is taken from a saved output whose absolute error is an ulp of 1, and
a wide sum that feeds only a few columns keeps its cancellation.  A float32 restatement of the chain in torch (the CPU
test) stays below 5.1e-7 * S at Hd >= 16 without a window and reaches 0.6 - 1.6e-6 * S on dx at Hd <= 3 (3.5e-6 in one
of 92 narrowed cases of a seed sweep); its smallest planted fault stands at 2e-4 * S.  The 'hidden' window therefore narrows w_out together with W_1..W_3: with the hidden
layers alone narrowed, the Hd-term sums g_4 W_3 feed 1..15 columns and the same restatement reaches 9e-6 * S on dx
(on MI355X, 69 such cases: fused kernel 7.6e-6, the separate mlp.hip chains 2.0e-5 -- rounding in both, and above the
4e-6 ceiling of dense_ref.py).
Measured on MI355X over the cases of tests/test_heads_kernels_gpu.py: fused kernel 3.3e-7 (outputs) and 8.6e-7 (dx,
the widths family; every other family <= 6.4e-7), the separate mlp.hip chains on the same cases 2.4e-7 and 9.0e-7, so
HEADS_C_TOL stays at dense_ref.C_TOL.
"""
from __future__ import annotations

import ctypes as C

import torch

from tests.dense_ref import (C_TOL, K_TALL_MAX_PER, K_WAVES, SENTINEL, Placed, cdiv, check_close, elu64,  # noqa: F401
                             elu_grad_from_out64, pack, placed_input)

HEADS_C_TOL = C_TOL       # dense_ref.C_TOL, unchanged
HIDDEN = 4                # BD_HEAD_HIDDEN: Linear + ELU layers in front of the Hd -> 1 output layer
MAX_LDS = 160 * 1024      # bd_host.h: kMaxLds
FRAG_FLOATS = 256         # bd_device.h: kFragFloats
WINDOWS = (None, "cols", "rows", "hidden", "head_r", "head_v")


# ---- float64 reference -------------------------------------------------------------------------------------------------

def heads_ref(x: torch.Tensor, heads, M: int):
    """The whole operation in float64 from the float32 operands.  `heads` = two dicts with W (HIDDEN matrices, (N, K)),
    b (HIDDEN vectors), w_out (Hd), b_out (1), dout (>= M).  Returns (out_r, S_r), (out_v, S_v), (dx, S_dx)."""
    x64 = x[:M].double()
    outs = []
    dx = torch.zeros_like(x64)
    S_dx = torch.zeros_like(x64)
    for H in heads:
        a = [x64]
        for l in range(HIDDEN):
            a.append(elu64(a[-1] @ H["W"][l].double().t() + H["b"][l].double()))
        w_out = H["w_out"].double().reshape(-1)
        out = a[HIDDEN] @ w_out + H["b_out"].double().reshape(())
        S_out = a[HIDDEN].abs() @ w_out.abs() + H["b_out"].double().abs().reshape(())
        g = H["dout"][:M].double().reshape(M, 1) * w_out * elu_grad_from_out64(a[HIDDEN])
        for l in range(HIDDEN - 1, 0, -1):
            g = (g @ H["W"][l].double()) * elu_grad_from_out64(a[l])
        dx += g @ H["W"][0].double()
        S_dx += g.abs() @ H["W"][0].double().abs()
        outs.append((out, S_out))
    return outs[0], outs[1], (dx, S_dx)


# ---- restated host dispatch (heads.hip: heads_rt / heads_lds / bd_img_heads_supported) ------------------------------------

def _tall_shape_ok(N: int, rt: int) -> bool:
    Nb = cdiv(N, 16)
    per = Nb // K_WAVES
    return per <= K_TALL_MAX_PER and (Nb - per * K_WAVES) * rt <= K_WAVES


def heads_rt(Hd: int) -> int:
    return 2 if _tall_shape_ok(Hd, 2) else (1 if _tall_shape_ok(Hd, 1) else 0)


def heads_lds(rt: int, F: int, Hd: int) -> int:
    KbF, Nb = cdiv(F, 16), cdiv(Hd, 16)
    return rt * (max(KbF, Nb) + Nb) * FRAG_FLOATS * 4


def heads_supported(F: int, Hd: int) -> bool:
    if F <= 0 or Hd <= 0:
        return False
    rt = heads_rt(Hd)
    return rt > 0 and heads_lds(rt, F, Hd) <= MAX_LDS


def heads_class(F: int, Hd: int, off: int = 0):
    """(rt, per, left, 'pairs' | 'scalar', F < Hd, lds > 64 KiB) of a supported shape with x at float offset `off` of an
    allocation (the pair loader needs an even F and an 8-byte aligned base: bd_device.h, tile_pairs_ok)."""
    assert heads_supported(F, Hd), (F, Hd)
    rt, Nb = heads_rt(Hd), cdiv(Hd, 16)
    loader = "pairs" if F % 2 == 0 and off % 2 == 0 else "scalar"
    return rt, Nb // K_WAVES, Nb % K_WAVES, loader, F < Hd, heads_lds(rt, F, Hd) > 64 * 1024


# ---- bd_pack_weights, restated (cabi.hip:12-14) ---------------------------------------------------------------------------

def pack_ref(W: torch.Tensor, transpose: bool) -> torch.Tensor:
    """dst[((nb*Kb + kb)*64 + lane)*4 + i] = W[n][k0 + i], n = nb*16 + (lane & 15), k0 = kb*16 + 4*(lane >> 4); zero where
    n or k is out of range; the transposed form reads W[k][n]."""
    Wo = W.t() if transpose else W
    No, Ki = Wo.shape
    Nb, Kb = cdiv(No, 16), cdiv(Ki, 16)
    P = torch.zeros(Nb * 16, Kb * 16, dtype=W.dtype, device=W.device)
    P[:No, :Ki] = Wo
    # [nb, n & 15, kb, lane >> 4, i] -> [nb, kb, lane >> 4, n & 15, i]
    return P.view(Nb, 16, Kb, 4, 4).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


# ---- cases ---------------------------------------------------------------------------------------------------------------

class HeadsCase:
    """Operands of one bd_img_heads_fwd_bwd launch: x [M x F] NaN-padded at float offset `off` (ld = F), per head four
    hidden layers W_l ~ randn / sqrt(K), b_l ~ 0.5 randn, w_out ~ randn / sqrt(Hd), b_out, dout ~ randn (NaN-padded);
    out_r, out_v [M] and dx [M x F] in SENTINEL-filled buffers.  Windows (everything outside is zero, so that a dropped
    tail is an O(1) error): 'cols' x except its last F % 16 or 1 columns; 'rows' both dout except the last row (dx is
    then exactly 0 in every other row); 'hidden' the input columns of W_1..W_3 and the entries of w_out except the last
    Hd % 16 or 1 (every Hd-wide contraction, forward and backward, then has its only nonzero terms in the tail);
    'head_r' / 'head_v' zero that head's dout, so dx comes from the other head alone."""

    def __init__(self, M: int, F: int, Hd: int, seed: int, window=None, off: int = 0, device="cuda"):
        assert window in WINDOWS, window
        self.M, self.F, self.Hd, self.window, self.off, self.device = M, F, Hd, window, off, device
        g = torch.Generator(device=device).manual_seed(seed)

        def randn(*shape):
            return torch.randn(*shape, device=device, generator=g)

        self.heads = []
        for _ in range(2):
            dims = [F] + [Hd] * HIDDEN
            W = [randn(dims[l + 1], dims[l]) / dims[l] ** 0.5 for l in range(HIDDEN)]
            b = [0.5 * randn(Hd) for _ in range(HIDDEN)]
            w_out = randn(Hd) / Hd ** 0.5
            if window == "hidden":
                for l in range(1, HIDDEN):
                    W[l][:, :Hd - (Hd % 16 or 1)] = 0.0
                w_out[:Hd - (Hd % 16 or 1)] = 0.0
            self.heads.append(dict(W=W, b=b, w_out=w_out, b_out=randn(1)))
        x = randn(M, F)
        if window == "cols":
            x[:, :F - (F % 16 or 1)] = 0.0
        for h, H in enumerate(self.heads):
            d = randn(M)
            if window == "rows":
                d[:M - 1] = 0.0
            if window == ("head_r", "head_v")[h]:
                d.zero_()
            H["dout_p"] = placed_input(d.view(M, 1), 1)
            H["dout"] = H["dout_p"].view[:, 0]
        self.x = placed_input(x, F, off)
        self._packed = None
        self.fresh_outputs()

    def fresh_outputs(self):
        M, F = self.M, self.F
        self.out_r = Placed(M, 1, 1, device=self.device)
        self.out_v = Placed(M, 1, 1, device=self.device)
        self.dx = Placed(M, F, F, device=self.device)

    def outputs(self):
        return self.out_r.view[:, 0].clone(), self.out_v.view[:, 0].clone(), self.dx.view.clone()

    def launch(self, cabi) -> int:
        """Fill cabi.ImgHeadsArgs, call bd_img_heads_fwd_bwd and synchronise; returns the entry's return code."""
        if self._packed is None:
            self._packed = [([pack(W, False) for W in H["W"]], [pack(W, True) for W in H["W"]]) for H in self.heads]
        a = cabi.ImgHeadsArgs()
        a.M, a.F, a.Hd, a.x, a.dx = self.M, self.F, self.Hd, self.x.ptr, self.dx.ptr
        for h, (H, out) in enumerate(zip(self.heads, (self.out_r, self.out_v))):
            A = a.head[h]
            for l in range(HIDDEN):
                A.w[l], A.wt[l], A.b[l] = self._packed[h][0][l].data_ptr(), self._packed[h][1][l].data_ptr(), H["b"][l].data_ptr()
            A.w_out, A.b_out = H["w_out"].data_ptr(), H["b_out"].data_ptr()
            A.dout, A.out = H["dout_p"].ptr, out.ptr
        rc = cabi.lib.bd_img_heads_fwd_bwd(C.byref(a), cabi.stream())
        torch.cuda.synchronize()
        return rc

    def reference(self):
        return heads_ref(self.x.view, self.heads, self.M)

    def check(self, name: str, c: float = HEADS_C_TOL) -> float:
        """The outputs against the float64 reference; nothing written outside them.  Returns the worst err / S."""
        for tag, p in (("out_r", self.out_r), ("out_v", self.out_v), ("dx", self.dx)):
            assert p.outside_unchanged(), f"{name}: wrote outside {tag}"
        (r, S_r), (v, S_v), (dx, S_dx) = self.reference()
        self.worst = dict(out_r=check_close(f"{name} out_r", self.out_r.view[:, 0], r, S_r, c=c),
                          out_v=check_close(f"{name} out_v", self.out_v.view[:, 0], v, S_v, c=c),
                          dx=check_close(f"{name} dx", self.dx.view, dx, S_dx, c=c))
        return max(self.worst.values())
