"""Is the reduce-kernel test itself sharp?  (no GPU)

tests/reduce_ref.py accepts a kernel output when it lies within its float64-derived bound.  Here an fp32 CPU emulation of
each kernel formula, written the way csrc/reduce.hip (and bd_colsum in csrc/conv.hip) writes it, must pass those checks,
and each planted fault in the same emulation must fail them.  The host-side argument checks of the entry points are
exercised with argument sets they reject, so nothing is launched."""
import numpy as np
import pytest
import torch

from tests import reduce_ref as R

F32 = torch.float32


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _fails(fn):
    with pytest.raises(AssertionError, match="out of tolerance|state"):
        fn()


# ---- normal_nll: leading dimensions --------------------------------------------------------------------------------------

def emulate_normal_nll(pbuf, ldp, tbuf, ldt, rows, D, gs, fault=None):
    if fault == "ignore_ld":
        ldp = ldt = D
    p = torch.stack([pbuf[r * ldp:r * ldp + D] for r in range(rows)])
    t = torch.stack([tbuf[r * ldt:r * ldt + D] for r in range(rows)])
    d = p - t
    term = torch.tensor(0.5, dtype=F32) * d * d + torch.tensor(R.O.HALF_LOG_2PI, dtype=F32)
    return float(torch.tensor(float(term.double().sum()), dtype=F32)), d * torch.tensor(gs, dtype=F32)


@pytest.mark.parametrize("fault", [None, "ignore_ld"])
def test_normal_nll(fault):
    rows, D, ldp, ldt = 40, 17, 20, 19
    g = _g(0)
    pred, target = 3 * torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    pbuf, tbuf = torch.randn(rows * ldp, generator=g), torch.randn(rows * ldt, generator=g)
    pbuf.view(rows, ldp)[:, :D] = pred
    tbuf.view(rows, ldt)[:, :D] = target
    gs = R.f32(1 / rows)
    got, dp = emulate_normal_nll(pbuf, ldp, tbuf, ldt, rows, D, gs, fault)
    ref, S, dref, Sd = R.normal_nll_ref(pred, target, gs)

    def check():
        R.check_scalar("nll", got, ref, S)
        R.check_close("dpred", dp, dref, Sd)
    (_fails if fault else (lambda f: f()))(check)


# ---- Gaussian KL: free nats tie, balance -------------------------------------------------------------------------------------

def _kl_elem(qm, qs, pm, ps):
    ratio = qs / ps
    vr = ratio * ratio
    t = (qm - pm) / ps
    return torch.tensor(0.5, dtype=F32) * (vr + t * t - 1 - torch.log(vr))


def emulate_kl(ins, fn, kl_balance, weight, inv_count, fault=None):
    """bd_kl_forward's balanced scalar, then kl_bwd_kernel's four gradients (fp32)."""
    qm, qs, pm, ps = ins
    scalar = float(torch.tensor(float(_kl_elem(*ins).double().sum()), dtype=F32))
    x = float(np.float32(scalar) * np.float32(inv_count))
    mg = 0.0 if x < fn else (1.0 if fault == "tie_factor_1" and x == fn else (0.5 if x == fn else 1.0))
    f = np.float32(np.float32(mg) * np.float32(weight) * np.float32(inv_count))
    fp, fq = np.float32(kl_balance) * f, np.float32(1 - kl_balance) * f
    if fault == "balance_swapped":
        fp, fq = fq, fp
    fq, fp = torch.tensor(fq, dtype=F32), torch.tensor(fp, dtype=F32)
    inv_d = 1 / ps
    inv_d2 = inv_d * inv_d
    diff = qm - pm
    return scalar, [fq * diff * inv_d2, fq * (qs * inv_d2 - 1 / qs), -fp * diff * inv_d2,
                    fp * (inv_d - (qs * qs + diff * diff) * inv_d2 * inv_d)]


@pytest.mark.parametrize("fault", [None, "tie_factor_1", "balance_swapped"])
def test_kl_balanced_tie(fault):
    rows, S, weight = 50, 30, 0.75
    g = _g(1)
    ins = [torch.randn(rows, S, generator=g), 0.2 + 2 * torch.rand(rows, S, generator=g),
           torch.randn(rows, S, generator=g), 0.2 + 2 * torch.rand(rows, S, generator=g)]
    inv = R.f32(1 / (rows * S))
    scalar0 = emulate_kl(ins, 0.0, 0.8, weight, inv)[0]
    fn_k = float(np.float32(scalar0) * np.float32(inv))           # the kernel's exact tie
    fn_r = R.kl_ref(*ins, 0.0, 0.8, 1.0)[2]                         # the float64 reference's exact tie
    scalar, grads = emulate_kl(ins, fn_k, 0.8, weight, inv, fault)
    ref, Ssc, _, rgrads, mags = R.kl_ref(*ins, fn_r, 0.8, weight)

    def check():
        R.check_scalar("kl", scalar, ref, Ssc)
        for a, b, m in zip(grads, rgrads, mags):
            R.check_close("kl grad", a, b, m)
    (_fails if fault else (lambda f: f()))(check)


# ---- lambda-return backward ----------------------------------------------------------------------------------------------

def emulate_lambda_bwd(dret, disc, lam, fault=None):
    Hm, N = dret.shape
    c, w = torch.tensor(disc * lam, dtype=F32), torch.tensor(disc * (1 - lam), dtype=F32)
    dr, dv = torch.empty(Hm, N), torch.zeros(Hm, N)
    G = torch.zeros(N)
    for t in range(Hm):
        G = dret[t] + c * G
        dr[t] = G
        if t < Hm - 1:
            dv[t + 1] = G * w
        else:
            dv[t] = (dv[t] if Hm > 1 else 0) + G * w + (0 if fault == "no_bootstrap_term" else c * G)
    return dr, dv


@pytest.mark.parametrize("fault", [None, "no_bootstrap_term"])
def test_lambda_backward(fault):
    Hm, N, disc, lam = 15, 300, R.f32(0.995), R.f32(0.95)
    g = _g(2)
    reward, value, dret = (torch.randn(Hm, N, generator=g) for _ in range(3))
    dr, dv = emulate_lambda_bwd(dret, disc, lam, fault)
    _, _, dr_ref, Sdr, dv_ref, Sdv = R.lambda_ref(reward, value, disc, lam, dret)

    def check():
        R.check_close("dreward", dr, dr_ref, Sdr)
        R.check_close("dvalue", dv, dv_ref, Sdv)
    (_fails if fault else (lambda f: f()))(check)


# ---- clip + Adam -----------------------------------------------------------------------------------------------------------

def emulate_adam(p, g, m, v, lr, b1, b2, eps, wd, step, max_norm, fault=None):
    b1, b2 = np.float32(b1), np.float32(b2)
    bstep = step - 1 if fault == "bias_step_minus_1" else step
    bc1, bc2 = 1.0 - float(b1) ** bstep, 1.0 - float(b2) ** bstep
    ss, isb2 = np.float32(lr / bc1), np.float32(1.0 / np.sqrt(bc2))
    total = np.sqrt(np.float32(float((g.double() ** 2).sum())))
    q = np.float32(max_norm) / (total + np.float32(1e-6))
    coef = torch.tensor(min(q, np.float32(1.0)), dtype=F32)
    gc = g * coef
    gw = gc + (0 if fault == "no_weight_decay" else torch.tensor(wd, dtype=F32) * p)
    m1 = m + torch.tensor(1 - b1, dtype=F32) * (gw - m)
    v1 = v * torch.tensor(b2) + torch.tensor(1 - b2, dtype=F32) * gw * gw
    denom = torch.sqrt(v1) * torch.tensor(isb2) + torch.tensor(eps, dtype=F32)
    p1 = p - torch.tensor(ss) * (m1 / denom)
    return p1, (g if fault == "clip_not_written" else gc), m1, v1


@pytest.mark.parametrize("fault,step", [(f, s) for f in (None, "bias_step_minus_1", "no_weight_decay", "clip_not_written")
                                         for s in (1, 2, 1000) if not (f == "bias_step_minus_1" and s == 1)])
def test_adam(fault, step):
    n, lr, betas, eps, wd = 1000, 1e-3, (0.9, 0.999), 1e-7, 1e-2
    g = _g(step)
    p, grad = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = 0.01 * torch.randn(n, generator=g) if step > 1 else torch.zeros(n)
    v = 1e-4 * torch.rand(n, generator=g) if step > 1 else torch.zeros(n)
    max_norm = 0.1 * float(grad.double().norm())                      # clipping active
    hp = [R.f32(x) for x in (lr, betas[0], betas[1], eps, wd)]
    out = emulate_adam(p, grad, m, v, *hp, step, R.f32(max_norm), fault)
    r = R.AdamRef(n, lr, betas, eps, wd, max_norm, step - 1).step(p, grad, m, v)

    def check():
        for nm, got in zip(("p", "g", "m", "v"), out):
            R.check_close(f"adam {nm}", got, *r[nm])
    (_fails if fault else (lambda f: f()))(check)


def test_adam_reference_nan_poisons_everything():
    """What the GPU test pins: torch's clip_grad_norm_ + Adam turn one NaN gradient into NaN parameters everywhere."""
    g = torch.randn(10, generator=_g(3))
    g[4] = float("nan")
    r = R.AdamRef(10, 1e-3, (0.9, 0.999), 1e-7, 0.0, 1.0, 0).step(torch.randn(10), g, torch.zeros(10), torch.zeros(10))
    assert bool(torch.isnan(r["p"][0]).all()) and bool(torch.isnan(r["g"][0]).all())


# ---- Gaussian head backward --------------------------------------------------------------------------------------------

def emulate_gauss_bwd(out, eps, dstate, dmean, dstd, fault=None):
    S = out.shape[1] // 2
    raw = out[:, S:]
    gm = dstate + dmean
    gs = dstate * eps + dstd
    arg = torch.nn.functional.softplus(raw, threshold=20) if fault == "sigmoid_of_softplus" else raw
    return torch.cat([gm, gs * torch.sigmoid(arg)], 1)


@pytest.mark.parametrize("fault", [None, "sigmoid_of_softplus"])
def test_gauss_head_backward(fault):
    M, S = 64, 9
    g = _g(4)
    raw = torch.tensor([-30.0, -17.0, -5.0, 0.0, 5.0, 19.99, 20.0, 20.01, 50.0]).repeat(M, 1)
    out = torch.cat([torch.randn(M, S, generator=g), raw], 1)
    eps, dstate, dmean, dstd = (torch.randn(M, S, generator=g) for _ in range(4))
    got = emulate_gauss_bwd(out, eps, dstate, dmean, dstd, fault)
    ref, S_, allow = R.gauss_head_bwd_ref(out, eps, dstate, dmean, dstd)
    (_fails if fault else (lambda f: f()))(lambda: R.check_close("gauss bwd", got, ref, S_, allow))


# ---- Categorical head argmax / Categorical KL tail ---------------------------------------------------------------------

def emulate_cat_state(probs, q, fault=None):
    """cat_head_fwd_kernel's argmax: per lane l the classes l, l+32, ... in order, then the xor-shuffle tie-break."""
    r = probs / q
    C = r.shape[-1]
    out = torch.zeros_like(r)
    for gi, row in enumerate(r.view(-1, C)):
        best, arg = [-np.inf] * 32, [1 << 31] * 32
        for l in range(32):
            for c in range(l, C, 32):
                if row[c] > best[l] or (fault == "last_max_wins" and row[c] == best[l]):
                    best[l], arg[l] = float(row[c]), c
        for o in (16, 8, 4, 2, 1):
            nb, na = best[:], arg[:]
            for l in range(32):
                ob, oa = best[l ^ o], arg[l ^ o]
                better = oa > arg[l] if fault == "last_max_wins" else oa < arg[l]
                if ob > best[l] or (ob == best[l] and better):
                    nb[l], na[l] = ob, oa
            best, arg = nb, na
        out.view(-1, C)[gi, arg[0]] = 1.0
    return out


@pytest.mark.parametrize("fault", [None, "last_max_wins"])
def test_categorical_argmax(fault):
    C = 33
    probs = torch.full((4, 1, C), 1.0 / C)
    q = torch.full((4, 1, C), 2.0)
    for i, (a, b) in enumerate(((1, 32), (0, 1), (5, 0 + 32))):
        q[i, 0, a] = q[i, 0, b] = 0.5
    q[3, 0, 32] = 0.25
    got = emulate_cat_state(probs, q, fault)

    def check():
        assert torch.equal(got, R.expected_state(probs, q)), "state differs"
    if fault:
        with pytest.raises(AssertionError, match="state"):
            check()
    else:
        check()


def emulate_cat_kl(ql, pl, fault=None):
    """group_kl per (row, factor) in fp32: log-softmax, then the class terms (float64 sum of fp32 terms here)."""
    C = ql.shape[-1]
    lq, lp = torch.log_softmax(ql, -1), torch.log_softmax(pl, -1)
    t = torch.exp(lq) * (lq - lp)
    if fault == "drop_tail_class":
        t = t[..., :C - C % 32]
    return float(torch.tensor(float(t.double().sum()), dtype=F32))


@pytest.mark.parametrize("fault", [None, "drop_tail_class"])
def test_categorical_kl_tail(fault):
    rows, D, C = 30, 4, 33
    g = _g(5)
    ql, pl = 3 * torch.randn(rows, D, C, generator=g), 3 * torch.randn(rows, D, C, generator=g)
    got = emulate_cat_kl(ql, pl, fault)
    scalar, Ssc = R.cat_kl_ref(ql, pl, 0.0, 0.8, 1.0)[:2]
    (_fails if fault else (lambda f: f()))(lambda: R.check_scalar("cat kl", got, scalar, Ssc, R.red_c(9)))


# ---- bd_colsum ---------------------------------------------------------------------------------------------------------------

def emulate_colsum(x, fault=None):
    """colsum_partial_kernel (per block, per thread a strided fp32 chain, then a fp32 sum over the row lanes) and
    colsum_final_kernel (fp32 strided sums, then a fixed tree), vectorised over columns."""
    M, N = x.shape
    Np = 1
    while Np < N:
        Np <<= 1
    rstep = 256 // Np
    nb = (M + 63) // 64 if M < R.K_COLSUM_BLOCKS * 64 else R.K_COLSUM_BLOCKS
    per = -(-M // nb)
    partial = torch.zeros(nb, N)
    last = (M - 1) // per                  # the last block with rows (M = 65537: block 1008; 1009..1023 are empty)
    for b in range(nb):
        if fault == "drop_last_block" and b == last:
            continue
        m0, m1 = b * per, min(M, b * per + per)
        acc = torch.zeros(rstep, N)
        for j, m in enumerate(range(m0, m1)):
            acc[j % rstep] += x[m]
        t = torch.zeros(N)
        for r in range(rstep):
            t += acc[r]
        partial[b] = t
    red = torch.zeros(256, N)
    for b in range(nb):
        red[b % 256] += partial[b]
    s = 128
    while s > 0:
        red[:s] += red[s:2 * s]
        s >>= 1
    return red[0]


@pytest.mark.parametrize("fault", [None, "drop_last_block"])
@pytest.mark.parametrize("M,N", [(65537, 3), (9000, 200)])
def test_colsum(fault, M, N):
    x = torch.randn(M, N, generator=_g(6)) + 1.0
    got = emulate_colsum(x, fault)
    ref, S = R.colsum_ref(x)
    c = (R.colsum_chain(M, N) + 8) * R.U
    (_fails if fault else (lambda f: f()))(lambda: R.check_close("colsum", got, ref, S, c=c))


# ---- host checks: rejected without a launch --------------------------------------------------------------------------

_FAKE = 0x1000      # never dereferenced: every argument set below fails a host check before any launch


def _rejected(cabi, rc, needle):
    err = cabi.lib.bd_last_error().decode()
    assert rc != 0 and needle in err, (rc, err)


def test_reduce_host_checks_reject():
    from big_dreamer_amd import _cabi as cabi
    L, F = cabi.lib, _FAKE
    for C in (0, 129):
        _rejected(cabi, L.bd_categorical_head_forward(F, F, 1, 1, C, F, F, None), "classes")
        _rejected(cabi, L.bd_categorical_head_backward(F, F, 1, 1, C, F, None), "classes")
        _rejected(cabi, L.bd_kl_categorical_forward(F, F, 1, 1, C, 0.0, 0, F, 0, F, None), "classes")
        _rejected(cabi, L.bd_kl_categorical_backward(F, F, 1, 1, C, 0.0, 0.8, 1.0, 1.0, F, 0, F, F, None), "classes")
    _rejected(cabi, L.bd_normal_nll(F, 4, F, 5, 3, 5, 1.0, F, 5, F, 0, F, None), "leading dimension")
    _rejected(cabi, L.bd_normal_nll(F, 5, F, 4, 3, 5, 1.0, F, 5, F, 0, F, None), "leading dimension")
    _rejected(cabi, L.bd_normal_nll(F, 5, F, 5, 3, 5, 1.0, F, 4, F, 0, F, None), "leading dimension")
    _rejected(cabi, L.bd_adam_step(F, F, F, F, 10, 1e-3, 0.9, 0.999, 1e-7, 0.0, 0, 1.0, F, 0, None), "bad arguments")
    for fn in (L.bd_sum, L.bd_sumsq):
        _rejected(cabi, fn(F, 0, F, 0, F, None), "bad arguments")
    _rejected(cabi, L.bd_bernoulli_nll(F, F, 0, 1.0, F, F, 0, F, None), "bad arguments")
    _rejected(cabi, L.bd_adam_step(F, F, F, F, 0, 1e-3, 0.9, 0.999, 1e-7, 0.0, 1, 1.0, F, 0, None), "bad arguments")
    _rejected(cabi, L.bd_polyak(F, F, 0, 0.5, None), "bad arguments")
    _rejected(cabi, L.bd_normal_nll(F, 5, F, 5, 0, 5, 1.0, F, 5, F, 0, F, None), "bad arguments")
    _rejected(cabi, L.bd_kl_forward(F, F, F, F, 0, 3, 0.0, 0, F, 0, F, None), "bad arguments")
    _rejected(cabi, L.bd_kl_backward(F, F, F, F, 0, 3, 0.0, 0.8, 1.0, 1.0, F, 0, F, F, F, F, None), "bad arguments")
    _rejected(cabi, L.bd_gauss_head_forward(F, F, 0, 3, 0.1, F, F, F, None), "bad arguments")
    _rejected(cabi, L.bd_lambda_return_forward(F, F, 3, 0, 0.99, 0.95, F, None), "bad arguments")
    _rejected(cabi, L.bd_lambda_return_backward(F, 1.0, 0, 3, 0.99, 0.95, F, F, None), "bad arguments")
    _rejected(cabi, L.bd_categorical_head_forward(F, F, 0, 1, 32, F, F, None), "bad arguments")
    _rejected(cabi, L.bd_kl_categorical_forward(F, F, 0, 1, 32, 0.0, 0, F, 0, F, None), "bad arguments")
    _rejected(cabi, L.bd_colsum(F, 10, 257, F, F, None), "N <= 256")
    _rejected(cabi, L.bd_colsum(F, 0, 3, F, F, None), "bad arguments")
    _rejected(cabi, L.bd_gauss_head_backward(F, None, F, F, F, 2, 3, F, None), "bad arguments")
    _rejected(cabi, L.bd_gauss_head_forward(F, None, 2, 3, 0.1, F, F, F, None), "bad arguments")
