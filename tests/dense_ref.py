"""Float64 references, a componentwise tolerance and buffer builders for the dense-chain (csrc/mlp.hip) and
weight-gradient (csrc/wgrad.hip) kernel tests.  Plain helpers, not a conftest: the CPU sharpness tests import them on
CPU tensors, the GPU tests on device tensors (the float64 references of the large cases stay on the device).

Tolerance: a kernel value passes when |got - ref| <= c * sum|a*b| + allow, with sum|a*b| the float64 contraction of the
absolute operands (bias and one-hot gather terms included) and `allow` an absolute allowance for the ELU epilogue.  fp32
MFMA accumulation was measured at 0.75-3.5e-7 * sum|a*b| for K <= 4096, so C_TOL = 1e-6 leaves headroom without hiding
a dropped or doubled term in the windowed cases (where a term is O(1) of sum|a*b|).
"""
from __future__ import annotations

import ctypes as C

import torch

C_TOL = 1e-6          # do not raise beyond 4e-6 without a written reason
ACT_ALLOW = 1e-6      # ELU outputs (__expf(x) - 1 in the default build) and ELU' factors
SENTINEL = -31415.926  # prefilled into every output region a kernel must not write


# ---- comparison ------------------------------------------------------------------------------------------------------

def check_close(name: str, got: torch.Tensor, ref: torch.Tensor, S: torch.Tensor, allow=0.0, c: float = C_TOL) -> float:
    """Componentwise |got - ref| <= c * S + allow (NaN fails).  Returns the worst (err - allow)+ / S for the report."""
    got = got.double()
    err = (got - ref).abs()
    bound = c * S + allow
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        n_bad = int(bad.sum())
        al = allow[idx] if torch.is_tensor(allow) else allow
        raise AssertionError(f"{name}: {n_bad} of {got.numel()} elements out of tolerance; first at {idx}: "
                             f"got {float(got[idx])!r}, ref {float(ref[idx])!r}, sum|a*b| {float(S[idx])!r}, "
                             f"allow {float(al)!r}, shape {tuple(got.shape)}")
    excess = (err - (allow if torch.is_tensor(allow) else torch.full_like(err, float(allow)))).clamp(min=0.0)
    pos = S > 0
    return float((excess[pos] / S[pos]).max()) if bool(pos.any()) else 0.0


def elu64(x: torch.Tensor) -> torch.Tensor:
    return torch.where(x > 0, x, torch.expm1(x))


def elu_grad_from_out64(y: torch.Tensor) -> torch.Tensor:
    """ELU' through the saved output y (bd_device.h: y > 0 ? 1 : y + 1), in float64."""
    y = y.double()
    return torch.where(y > 0, torch.ones_like(y), y + 1.0)


# ---- float64 references -----------------------------------------------------------------------------------------------

def gather_ref(gWT: torch.Tensor, gidx: torch.Tensor, gC: int, drop_last: bool = False):
    """sum_f gWT[f*gC + gidx[m, f]] over the gD factors (and the sum of absolute values): [M x N0] float64."""
    gD = gidx.shape[1] - (1 if drop_last else 0)
    rows = gidx[:, :gD].long() + gC * torch.arange(gD, device=gidx.device)
    w = gWT.double()[rows]                          # [M, gD, N0]
    return w.sum(1), w.abs().sum(1)


def linear_ref(x: torch.Tensor, W: torch.Tensor, b=None, act: bool = False, extra=None):
    """act(x W^T + b + extra) in float64; returns (ref, sum|a*b|, allow).  extra = (values, absolute values)."""
    x64, W64 = x.double(), W.double()
    pre = x64 @ W64.t()
    S = x64.abs() @ W64.abs().t()
    if b is not None:
        pre = pre + b.double()
        S = S + b.double().abs()
    if extra is not None:
        pre = pre + extra[0]
        S = S + extra[1]
    return (elu64(pre) if act else pre), S, (ACT_ALLOW if act else 0.0)


def dgrad_ref(dnext: torch.Tensor, W: torch.Tensor, saved=None, act: bool = False):
    """(dnext W) * ELU'(saved): the pre-activation gradient of the layer below, float64; (ref, sum|a*b|, allow)."""
    d64, W64 = dnext.double(), W.double()
    acc = d64 @ W64
    S = d64.abs() @ W64.abs()
    if not act:
        return acc, S, 0.0
    f = elu_grad_from_out64(saved)
    return acc * f, S * f, ACT_ALLOW * acc.abs()


def wgrad_ref(dpre: torch.Tensor, act: torch.Tensor):
    """dW = dpre^T act, db = colsum(dpre) in float64, each with its sum|a*b|."""
    p64, a64 = dpre.double(), act.double()
    return p64.t() @ a64, p64.abs().t() @ a64.abs(), p64.sum(0), p64.abs().sum(0)


# ---- buffers ---------------------------------------------------------------------------------------------------------

class Placed:
    """A [rows x cols] operand with leading dimension ld at a float offset `off` of a larger flat buffer filled with
    `fill` (NaN for inputs, SENTINEL for outputs); two rows past `rows` belong to the buffer too."""

    def __init__(self, rows: int, cols: int, ld: int, off: int = 0, fill: float = SENTINEL, device="cuda",
                 extra_rows: int = 2):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off, self.fill = rows, cols, ld, off, fill
        self.buf = torch.full((off + (rows + extra_rows) * ld + 4,), fill, dtype=torch.float32, device=device)
        self.full = self.buf[off:off + (rows + extra_rows) * ld].view(rows + extra_rows, ld)
        self.view = self.full[:rows, :cols]

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + 4 * self.off

    def outside_unchanged(self) -> bool:
        t = self.buf.clone()
        t[self.off:self.off + (self.rows + 2) * self.ld].view(self.rows + 2, self.ld)[:self.rows, :self.cols] = self.fill
        return bool(torch.equal(t, torch.full_like(t, self.fill)))


def placed_input(x: torch.Tensor, ld: int, off: int = 0) -> Placed:
    p = Placed(x.shape[0], x.shape[1], ld, off, float("nan"), x.device)
    p.view.copy_(x)
    return p


def pack(W: torch.Tensor, transpose: bool) -> torch.Tensor:
    """MFMA-fragment packing of a row-major (N, K) weight through bd_pack_weights (as categorical._pack does)."""
    from big_dreamer_amd.categorical import _pack
    return _pack(W.contiguous(), transpose)


def device_table(descs) -> torch.Tensor:
    """A ctypes descriptor array as a device byte tensor (keep the operands alive while it points at them)."""
    return torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to("cuda")


def wgrad_desc(cabi, dpre: Placed, act1: Placed, M1: int, act2, dW: torch.Tensor, dW_ptr: int, ldw: int, db_ptr):
    M, N = dpre.rows, dpre.cols
    K = act1.cols
    return cabi.WgradDesc(dpre.ptr, dpre.ld, act1.ptr, act1.ld, M1, act2.ptr if act2 is not None else None,
                          act2.ld if act2 is not None else 0, M, N, K, dW_ptr, ldw, db_ptr)


def wgrad_plan(cabi, descs):
    tb, tr, wsf = C.c_int(0), C.c_int(0), C.c_size_t(0)
    rc = cabi.lib.bd_wgrad_plan(descs, len(descs), C.byref(tb), C.byref(tr), C.byref(wsf))
    return rc, tb.value, tr.value, wsf.value


# ---- host dispatch, restated (for the coverage table and the CPU coverage test) ----------------------------------------

K_TALL_RT, K_TALL_MIN_TILES, K_WAVES, K_TALL_MAX_PER = 3, 512, 4, 3
K_SPLIT_SCRATCH_FLOATS = K_WAVES * 2 * 2 * 256 + 2 * 16 * 64


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def tall_shape_ok(N: int) -> bool:
    Nb = cdiv(N, 16)
    per = Nb // K_WAVES
    return per <= K_TALL_MAX_PER and (Nb - per * K_WAVES) * K_TALL_RT <= K_WAVES


def pick_rt(M: int, KbA: int, KbB: int, extra_per_rt: int = 0) -> int:
    rt = 2 if cdiv(M, 16) >= 1024 else 1
    while rt > 1 and (rt * ((KbA + KbB) * 256 + extra_per_rt) + K_SPLIT_SCRATCH_FLOATS) * 4 > 64 * 1024:
        rt >>= 1
    return rt


def fwd_path(M, dims, tall_mode, gD=0, saves_al16=True):
    """Which kernel bd_mlp_forward launches (mlp.hip:419-455): 'tall', 'rt1', 'rt2' (+ ':biglds' over 64 KiB)."""
    L = len(dims) - 1
    KbA = max(cdiv(dims[l], 16) for l in range(0, L, 2))
    KbB = max([cdiv(dims[l], 16) for l in range(1, L, 2)] or [0])
    on = tall_mode != 0
    if on and cdiv(M, 16) >= (1 if tall_mode == 2 else K_TALL_MIN_TILES):
        ok = not (gD > 0 and L == 1)
        for l in range(L):
            ok = ok and tall_shape_ok(dims[l + 1])
            if l + 1 < L:
                ok = ok and dims[l + 1] % 4 == 0 and saves_al16
        ok = ok and M * max(dims[1:]) < 2 ** 31
        if ok:
            return "tall"
    xs = 16 * dims[1] if gD > 0 else 0
    rt = pick_rt(M, KbA, KbB, xs)
    lds = (rt * (KbA + KbB) * 256 + K_SPLIT_SCRATCH_FLOATS + rt * xs) * 4
    return f"rt{rt}" + (":biglds" if lds > 64 * 1024 else "")


def bwd_path(M, dims, tall_mode, want_din=True, al16=True):
    """Which kernel bd_mlp_backward launches (mlp.hip:457-491)."""
    L = len(dims) - 1
    Ns = dims[1:]
    KbA = max(cdiv(Ns[l], 16) for l in range(L - 1, -1, -2))
    KbB = max([cdiv(Ns[l], 16) for l in range(L - 2, -1, -2)] or [0])
    if tall_mode != 0 and cdiv(M, 16) >= (1 if tall_mode == 2 else K_TALL_MIN_TILES):
        ok = all(tall_shape_ok(dims[l]) and dims[l] % 4 == 0 and al16 for l in range(1, L))
        if ok:
            return "tall"
    rt = pick_rt(M, KbA, KbB)
    lds = (rt * (KbA + KbB) * 256 + K_SPLIT_SCRATCH_FLOATS) * 4
    return f"rt{rt}" + (":biglds" if lds > 64 * 1024 else "")


def wgrad_body(N: int, K: int, bias: bool, act16: bool, dense_ok: bool, mid: bool = True):
    """The body(ies) of wgrad_wide_kernel that the tiles of one descriptor run (wgrad.hip:635-748, 804-921)."""
    NB, KB = cdiv(N, 16), cdiv(K + int(bias), 16)
    tn = cdiv(NB, 13)
    tk = 1 if KB <= 13 else (cdiv(KB, 36) if NB <= 4 and act16 else cdiv(KB, 12))
    nbw, kbw = cdiv(NB, tn), cdiv(KB, tk)
    out = set()
    for t_n in range(tn):
        for t_k in range(tk):
            nb, kb = min(nbw, NB - t_n * nbw), min(kbw, KB - t_k * kbw)
            hk = (kb + 3) >> 2
            if nb == 13 and kb >= 4 and dense_ok:
                out.add("dense")
            elif nb <= 4:
                out.add("deep" if kb > 15 else "narrow")
            elif nb <= 8 and mid:
                out.add("mid")
            else:
                out.add("general")
    return out


# ---- weight-gradient cases (GPU) ---------------------------------------------------------------------------------------

def _window_rows(M: int, kind):
    """Row indices that stay nonzero in a windowed case (None: all rows)."""
    if kind is None:
        return None
    if kind == "last16":
        r = M % 16 or 1
        return list(range(M - r, M))
    if kind == "tail":
        return list(range(max(0, M - 3), M))
    raise ValueError(kind)


class WgradCase:
    """One weight-gradient GEMM: dpre [M x N] (ldp = N + ldp_pad), activations split at M1 between act1 (lda1) and act2
    (lda2), dW / db at float offset w_off of one flat SENTINEL-filled buffer (ldw = K + ldw_pad, db right behind dW).
    Input padding is NaN.  window: None, 'last16' / 'tail' (rows), 'm1' (rows M1 - 1 and M1), 'cols' (last K % 16
    columns of act): everything outside is zero, so the result has a handful of terms."""

    def __init__(self, M, N, K, M1=None, bias=True, ldp_pad=0, lda_pad=0, lda2_pad=4, act_off=0, dpre_off=0, w_off=0,
                 ldw_pad=0, seed=0, window=None):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.M, self.N, self.K = M, N, K
        self.M1 = M if M1 is None else M1
        dpre = torch.randn(M, N, device="cuda", generator=g)
        act = torch.randn(M, K, device="cuda", generator=g)
        keep = _window_rows(M, window) if window in ("last16", "tail") else None
        if window == "m1":
            keep = [m for m in (self.M1 - 1, self.M1) if 0 <= m < M]
        if keep is not None:
            mask = torch.zeros(M, 1, device="cuda")
            mask[keep] = 1.0
            dpre *= mask
        if window == "cols":
            act[:, :K - (K % 16 or 1)] = 0.0
        self.dpre_t, self.act_t = dpre, act
        self.dpre = placed_input(dpre, N + ldp_pad, dpre_off)
        self.act1 = placed_input(act[:self.M1], K + lda_pad, act_off)
        self.act2 = placed_input(act[self.M1:], K + lda2_pad, act_off) if self.M1 < M else None
        self.ldw, self.w_off, self.bias = K + ldw_pad, w_off, bias
        self.flat = torch.full((w_off + N * self.ldw + N + 8,), SENTINEL, device="cuda")
        self.dW = self.flat[w_off:w_off + N * self.ldw].view(N, self.ldw)[:, :K]
        self.db = self.flat[w_off + N * self.ldw:w_off + N * self.ldw + N] if bias else None

    @property
    def dW_ptr(self):
        return self.flat.data_ptr() + 4 * self.w_off

    @property
    def db_ptr(self):
        return self.flat.data_ptr() + 4 * (self.w_off + self.N * self.ldw) if self.bias else None

    def desc(self, cabi):
        return wgrad_desc(cabi, self.dpre, self.act1, self.M1, self.act2, self.dW, self.dW_ptr, self.ldw, self.db_ptr)

    def set_prior(self, seed=1):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.prior_W = torch.randn(self.N, self.K, device="cuda", generator=g)
        self.dW.copy_(self.prior_W)
        if self.bias:
            self.prior_b = torch.randn(self.N, device="cuda", generator=g)
            self.db.copy_(self.prior_b)

    def check(self, name, accumulate=False) -> float:
        t = self.flat.clone()
        t[self.w_off:self.w_off + self.N * self.ldw].view(self.N, self.ldw)[:, :self.K] = SENTINEL
        if self.bias:
            t[self.w_off + self.N * self.ldw:self.w_off + self.N * self.ldw + self.N] = SENTINEL
        assert torch.equal(t, torch.full_like(t, SENTINEL)), f"{name}: wrote outside dW / db"
        rW, sW, rb, sb = wgrad_ref(self.dpre_t, self.act_t)
        if accumulate:
            rW, sW = rW + self.prior_W.double(), sW + self.prior_W.double().abs()
            if self.bias:
                rb, sb = rb + self.prior_b.double(), sb + self.prior_b.double().abs()
        worst = check_close(f"{name} dW", self.dW, rW, sW)
        if self.bias:
            worst = max(worst, check_close(f"{name} db", self.db, rb, sb))
        return worst


def run_grouped(cabi, cases, phase=0):
    """Plan, upload and run one grouped launch over `cases`; the slab workspace starts as NaN, so a slab element that no
    tile writes reaches the result.  Returns (table, plan, ws) -- keep them alive until the kernels are done."""
    descs = (cabi.WgradDesc * len(cases))(*[c.desc(cabi) for c in cases])
    rc, tb, tr, wsf = wgrad_plan(cabi, descs)
    cabi.check(rc)
    table = device_table(descs)
    ws = torch.full((max(1, wsf),), float("nan"), device="cuda")
    if phase == 0:
        cabi.check(cabi.lib.bd_wgrad_grouped(table.data_ptr(), len(cases), tb, tr, ws.data_ptr(), cabi.stream()))
    else:
        for ph in (1, 2):
            cabi.check(cabi.lib.bd_wgrad_grouped_phase(table.data_ptr(), len(cases), tb, tr, ws.data_ptr(), ph,
                                                       cabi.stream()))
    return table, descs, ws


def run_plain(cabi, c: WgradCase, accumulate=0):
    """bd_wgrad on a single-source case (NaN-filled workspace)."""
    assert c.M1 == c.M
    wsf = int(cabi.lib.bd_wgrad_ws_floats(c.M, c.N, c.K))
    ws = torch.full((max(1, wsf),), float("nan"), device="cuda")
    cabi.check(cabi.lib.bd_wgrad(c.dpre.ptr, c.dpre.ld, c.act1.ptr, c.act1.ld, c.M, c.N, c.K, c.dW_ptr, c.ldw,
                                 c.db_ptr, int(accumulate), ws.data_ptr(), wsf, cabi.stream()))
    return ws
