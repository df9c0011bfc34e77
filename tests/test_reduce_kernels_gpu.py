"""The loss, KL, latent-head, lambda-return, clip+Adam and polyak kernels (csrc/reduce.hip) and bd_colsum (csrc/conv.hip)
against float64 references (tests/reduce_ref.py), called directly through the C ABI at the shapes and arguments where
they could go wrong: grid-stride loops with several trips, padded leading dimensions, NULL optional outputs, free-nats
branches and exact ties, clipping, resumed bias correction, non-finite gradients, 1..128 Categorical classes and argmax
ties.  Every output sits in a sentinel-filled buffer that must stay untouched outside it, input padding is NaN, every
other scalars slot stays at the sentinel, and each reduction runs twice and must give the same bits (the fixed-order sum
the header promises).  Each case prints its worst err / bound magnitude (REDUCE_WORST lines, visible under -s)."""
import math

import numpy as np
import pytest
import torch

from tests import reduce_ref as R

pytestmark = pytest.mark.gpu
SLOT = 5
NAN = float("nan")


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def _report(entry, case, worst):
    print(f"REDUCE_WORST {entry} {case} {worst:.3e}")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _inp(x, off=5):
    """x (any shape, CPU) flat in a NaN-filled device buffer at float offset `off`."""
    return R.placed_input(x.reshape(1, -1).cuda(), x.numel(), off)


def _out(n, off=3):
    return R.Placed(1, n, n, off)


class Red:
    """scalars (sentinel except after a write to SLOT) and a NaN-filled reduction workspace."""

    def __init__(self, cabi):
        self.sc = torch.full((8,), R.SENTINEL, device="cuda")
        self.ws = torch.full((int(cabi.lib.bd_reduce_ws_floats()),), NAN, device="cuda")

    def twice(self, cabi, launch) -> float:
        vals = []
        for _ in range(2):
            self.sc[SLOT] = R.SENTINEL
            cabi.check(launch(self.sc.data_ptr(), SLOT, self.ws.data_ptr()))
            torch.cuda.synchronize()
            vals.append(self.sc[SLOT].clone())
        assert torch.equal(vals[0].view(torch.int32), vals[1].view(torch.int32)), "reduction is not deterministic"
        others = torch.cat([self.sc[:SLOT], self.sc[SLOT + 1:]])
        assert torch.equal(others, torch.full_like(others, R.SENTINEL)), "wrote another scalars slot"
        return float(vals[0])


def _outside_ok(*placed):
    for p in placed:
        assert p.outside_unchanged(), "wrote outside its output"


# ---- bd_sum / bd_sumsq -----------------------------------------------------------------------------------------------------

def _wide(n, seed):
    g = _g(seed)
    return torch.randn(n, generator=g) * torch.exp(6 * torch.randn(n, generator=g).clamp(-3, 3))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262143, 262144, 262145, 5_000_003])
def test_sum_sumsq(cabi, n):
    x = _wide(n, n)
    xi = _inp(x)
    red = Red(cabi)
    for name, fn, sq in (("bd_sum", cabi.lib.bd_sum, False), ("bd_sumsq", cabi.lib.bd_sumsq, True)):
        got = red.twice(cabi, lambda sc, slot, ws: fn(xi.ptr, n, sc, slot, ws, cabi.stream()))
        ref, S = R.sum_ref(x, sq)
        _report(name, f"n={n}", R.check_scalar(f"{name} n={n}", got, ref, S))


# ---- bd_normal_nll / bd_bernoulli_nll ------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,D", [(1, 1), (2499, 1), (2500, 17), (50, 300)])
@pytest.mark.parametrize("with_grad", [True, False])
def test_normal_nll(cabi, rows, D, with_grad):
    g = _g(rows * D)
    pred, target = 3 * torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    pi, ti = R.placed_input(pred.cuda(), D + 3, 1), R.placed_input(target.cuda(), D + 1, 2)
    dp = R.Placed(rows, D, D + 2, 3)
    gs = R.f32(1.0 / rows)
    red = Red(cabi)
    got = red.twice(cabi, lambda sc, slot, ws: cabi.lib.bd_normal_nll(
        pi.ptr, pi.ld, ti.ptr, ti.ld, rows, D, gs, dp.ptr if with_grad else None, dp.ld, sc, slot, ws, cabi.stream()))
    ref, S, dref, Sd = R.normal_nll_ref(pred, target, gs)
    w = R.check_scalar("normal_nll", got, ref, S)
    if with_grad:
        _outside_ok(dp)
        w = max(w, R.check_close("normal_nll dpred", dp.view.cpu(), dref, Sd))
    else:
        assert torch.equal(dp.buf, torch.full_like(dp.buf, R.SENTINEL)), "dpred = NULL was written"
    _report("bd_normal_nll", f"rows={rows},D={D},grad={with_grad}", w)


def test_bernoulli_nll(cabi):
    special = torch.tensor([0.0, 1e-3, -1e-3, 20, -20, 88, -88, 100, -100, 1e4, -1e4])
    x = torch.cat([special.repeat_interleave(3), 5 * torch.randn(70_000, generator=_g(1))])
    t = torch.cat([torch.tensor([0.0, 1.0, 0.3]).repeat(len(special)), torch.rand(70_000, generator=_g(2))])
    t[len(special) * 3::3] = torch.randint(0, 2, t[len(special) * 3::3].shape, generator=_g(3)).float()
    n = x.numel()
    xi, ti, dl = _inp(x), _inp(t, 7), _out(n)
    gs = R.f32(1.0 / 4096)
    red = Red(cabi)
    for with_grad in (True, False):
        got = red.twice(cabi, lambda sc, slot, ws: cabi.lib.bd_bernoulli_nll(
            xi.ptr, ti.ptr, n, gs, dl.ptr if with_grad else None, sc, slot, ws, cabi.stream()))
        ref, S, dref, Sd = R.bernoulli_ref(x, t, gs)
        w = R.check_scalar("bernoulli_nll", got, ref, S)
        if with_grad:
            _outside_ok(dl)
            w = max(w, R.check_close("bernoulli dlogits", dl.view[0].cpu(), dref, Sd, R.TINY))   # x = -88: denormal
            dl.buf.fill_(R.SENTINEL)
        else:
            assert torch.equal(dl.buf, torch.full_like(dl.buf, R.SENTINEL))
        _report("bd_bernoulli_nll", f"n={n},grad={with_grad}", w)


# ---- Gaussian KL -----------------------------------------------------------------------------------------------------------

def _kl_inputs(rows, S, seed, exact=False):
    g = _g(seed)
    if exact:
        # qs = ps = 2^k and qm - pm in {0, ±1, ±2} * ps: every KL term is an exact dyadic 0.5 (qm - pm)^2 / ps^2, so
        # a row sum equals a chosen free_nats exactly in fp32 and in float64
        ps = torch.pow(2.0, torch.randint(-1, 2, (rows, S), generator=g).float())
        k = torch.randint(-2, 3, (rows, S), generator=g).float()
        pm = torch.round(64 * torch.randn(rows, S, generator=g)) / 64
        return pm + k * ps, ps.clone(), pm, ps
    qm, pm = torch.randn(rows, S, generator=g), torch.randn(rows, S, generator=g)
    qs = 0.2 + torch.rand(rows, S, generator=g) * 2
    ps = 0.2 + torch.rand(rows, S, generator=g) * 2
    return qm, qs, pm, ps


def _run_kl(cabi, ins, free_nats, kl_balance):
    qm, qs, pm, ps = ins
    rows, S = qm.shape
    sum_form = int(kl_balance == -1)
    di = [_inp(a, 1 + i) for i, a in enumerate(ins)]
    outs = [_out(rows * S, 2 + i) for i in range(4)]
    red = Red(cabi)
    got = red.twice(cabi, lambda sc, slot, ws: cabi.lib.bd_kl_forward(
        *[d.ptr for d in di], rows, S, free_nats, sum_form, sc, slot, ws, cabi.stream()))
    inv_count = 1.0 / (rows * S) if not sum_form else 1.0 / rows           # engine.py:1430-1431 with W = 1
    return got, red, di, outs, inv_count


@pytest.mark.parametrize("S", [1, 30, 33])
@pytest.mark.parametrize("rows", [1, 2499])
@pytest.mark.parametrize("kl_balance", [0.8, 0.0, 1.0, -1.0])
@pytest.mark.parametrize("branch", ["above", "below", "tie"])
def test_kl_forward_backward(cabi, S, rows, kl_balance, branch):
    sum_form = kl_balance == -1
    exact = sum_form and branch == "tie"
    ins = _kl_inputs(rows, S, rows * S + 7, exact)
    kl64 = R.kl_ref(*ins, 0.0, kl_balance if not sum_form else -1.0, 1.0)
    weight = 0.75
    if sum_form:
        rs = (R.O.kl_normal(*[a.double() for a in ins])).sum(-1)
        if branch == "above":      # 1e-3 below a row KL that may be ~0: far wider than its fp32 error
            fn = 0.5 * float(rs.min()) - 1e-3
        elif branch == "below":
            fn = 2.0 * float(rs.max()) + 1.0
        else:      # a value some rows hit exactly, others lie above or below
            fn = float(rs.median())
            assert fn == R.f32(fn)
        fn_k = fn_r = R.f32(fn)
    else:
        mean = kl64[2]
        fn_k = fn_r = R.f32({"above": 0.5 * mean, "below": 2 * mean + 1, "tie": mean}[branch])
    got, red, di, outs, inv_count = _run_kl(cabi, ins, fn_k, kl_balance)
    if branch == "tie" and not sum_form:
        # the kernel ties when fl(scalar * inv_count) == free_nats; the float64 reference ties at its own mean
        fn_k = float(np.float32(got) * np.float32(inv_count))
        fn_r = kl64[2]
    scalar, Ssc, mean, grads, mags = R.kl_ref(*ins, fn_r, kl_balance, weight)
    chain = S if sum_form else 0
    w = R.check_scalar("kl scalar", got, scalar, Ssc, R.red_c(chain))
    cabi.check(cabi.lib.bd_kl_backward(*[d.ptr for d in di], rows, S, fn_k, kl_balance, weight, R.f32(inv_count),
                                       red.sc.data_ptr(), SLOT, *[o.ptr for o in outs], cabi.stream()))
    torch.cuda.synchronize()
    _outside_ok(*outs)
    if sum_form and branch == "tie":
        rsum = R.O.kl_normal(*[a.double() for a in ins]).sum(-1)
        assert bool((rsum == fn_r).any()), "no exact tie row"
    for nm, o, ref, mag in zip(("dqm", "dqs", "dpm", "dps"), outs, grads, mags):
        w = max(w, R.check_close(f"kl {nm}", o.view[0].cpu().view(rows, S), ref, mag))
    _report("bd_kl", f"rows={rows},S={S},bal={kl_balance},{branch}", w)


def test_kl_backward_nan_mean_passes_gradient(cabi):
    """torch.maximum's backward gives a NaN KL mean the factor 1 (it is neither below free nats nor tied)."""
    rows, S = 3, 4
    ins = [a.contiguous() for a in _kl_inputs(rows, S, 5)]
    di = [_inp(a, 1 + i) for i, a in enumerate(ins)]
    outs = [_out(rows * S, 2) for _ in range(4)]
    sc = torch.full((8,), R.SENTINEL, device="cuda")
    sc[SLOT] = NAN
    cabi.check(cabi.lib.bd_kl_backward(*[d.ptr for d in di], rows, S, 3.0, 0.8, 1.0, 1.0 / (rows * S), sc.data_ptr(),
                                       SLOT, *[o.ptr for o in outs], cabi.stream()))
    torch.cuda.synchronize()
    _, _, _, grads, mags = R.kl_ref(*ins, -1.0, 0.8, 1.0)        # factor 1 everywhere
    for nm, o, ref, mag in zip(("dqm", "dqs", "dpm", "dps"), outs, grads, mags):
        R.check_close(f"kl nan {nm}", o.view[0].cpu().view(rows, S), ref, mag)


# ---- Gaussian head -----------------------------------------------------------------------------------------------------

RAW = [-30.0, -17.0, -5.0, 0.0, 5.0, 19.99, 20.0, 20.01, 50.0]


@pytest.mark.parametrize("M", [1, 2499])
def test_gauss_head(cabi, M):
    S = 9 if M == 1 else 33
    g = _g(M)
    mean = 2 * torch.randn(M, S, generator=g)
    raw = torch.tensor(RAW)[torch.randint(0, len(RAW), (M, S), generator=g)]
    raw[0, :len(RAW)] = torch.tensor(RAW)                       # every special value at least once
    out = torch.cat([mean, raw], 1)
    eps = torch.randn(M, S, generator=g)
    oi, ei = _inp(out), _inp(eps, 2)
    refs = R.gauss_head_ref(out, eps, 0.1)
    w = 0.0
    for mask in range(8):
        bufs = [_out(M * S, 1 + i) if mask >> i & 1 else None for i in range(3)]
        cabi.check(cabi.lib.bd_gauss_head_forward(oi.ptr, ei.ptr, M, S, R.f32(0.1),
                                                  *[b.ptr if b else None for b in bufs], cabi.stream()))
        torch.cuda.synchronize()
        for nm, b, (ref, mag, allow) in zip(("mean", "std", "state"), bufs, refs):
            if b is None:
                continue
            _outside_ok(b)
            w = max(w, R.check_close(f"gauss head {nm} mask={mask}", b.view[0].cpu().view(M, S), ref, mag, allow))
    _report("bd_gauss_head_forward", f"M={M},S={S}", w)

    dmean, dstd, dstate = (torch.randn(M, S, generator=g) for _ in range(3))
    w = 0.0
    for with_state in (False, True):     # the engine's call passes dstate = eps = NULL
        dmi, dsi = _inp(dmean, 3), _inp(dstd, 4)
        dsti = _inp(dstate, 6) if with_state else None
        dout = _out(M * 2 * S, 1)
        cabi.check(cabi.lib.bd_gauss_head_backward(oi.ptr, ei.ptr if with_state else None,
                                                   dsti.ptr if with_state else None, dmi.ptr, dsi.ptr, M, S, dout.ptr,
                                                   cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(dout)
        ref, mag, allow = R.gauss_head_bwd_ref(out, eps if with_state else None, dstate if with_state else None,
                                               dmean, dstd)
        w = max(w, R.check_close(f"gauss head bwd state={with_state}", dout.view[0].cpu().view(M, 2 * S), ref, mag,
                                 allow))
    _report("bd_gauss_head_backward", f"M={M},S={S}", w)


# ---- lambda-return -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Hm", [1, 2, 15, 16])
@pytest.mark.parametrize("N", [1, 255, 257, 300_001])
def test_lambda_return(cabi, Hm, N):
    g = _g(Hm * 1000 + N)
    reward, value = torch.randn(Hm, N, generator=g), 3 * torch.randn(Hm, N, generator=g)
    dret = torch.randn(Hm, N, generator=g)
    ri, vi, di = _inp(reward), _inp(value, 2), _inp(dret, 3)
    for disc, lam in ((0.995, 0.95), (1.0, 1.0), (0.99, 0.0)):
        d32, l32 = R.f32(disc), R.f32(lam)
        ret = _out(Hm * N)
        cabi.check(cabi.lib.bd_lambda_return_forward(ri.ptr, vi.ptr, Hm, N, d32, l32, ret.ptr, cabi.stream()))
        w = 0.0
        for use_dret in (True, False):
            dconst = R.f32(-0.37)
            dr, dv = _out(Hm * N, 1), _out(Hm * N, 2)     # dvalue prefilled with the sentinel: dvalue[0] must be written
            cabi.check(cabi.lib.bd_lambda_return_backward(di.ptr if use_dret else None, dconst, Hm, N, d32, l32, dr.ptr,
                                                          dv.ptr, cabi.stream()))
            torch.cuda.synchronize()
            _outside_ok(ret, dr, dv)
            r_ref, Sret, dr_ref, Sdr, dv_ref, Sdv = R.lambda_ref(reward, value, d32, l32, dret if use_dret else None,
                                                                 dconst)
            w = max(w, R.check_close("returns", ret.view[0].cpu().view(Hm, N), r_ref, Sret))
            w = max(w, R.check_close("dreward", dr.view[0].cpu().view(Hm, N), dr_ref, Sdr))
            w = max(w, R.check_close("dvalue", dv.view[0].cpu().view(Hm, N), dv_ref, Sdv))
        _report("bd_lambda_return", f"Hm={Hm},N={N},disc={disc},lam={lam}", w)


# ---- bd_sumsq + bd_adam_step ---------------------------------------------------------------------------------------------

def _adam_run(cabi, n, wd, clip, start_step=0, steps=4, seed=0, poison=None):
    g = _g(seed + n)
    p = torch.randn(n, generator=g)
    m = 0.01 * torch.randn(n, generator=g) if start_step else torch.zeros(n)
    v = 1e-4 * torch.rand(n, generator=g) if start_step else torch.zeros(n)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-7
    bufs = [R.Placed(1, n, n, 1 + i) for i in range(4)]
    for b, x in zip(bufs, (p, torch.zeros(n), m, v)):
        b.view[0].copy_(x.cuda())
    pb, gb, mb, vb = bufs
    red = Red(cabi)
    worst = 0.0
    for k in range(steps):
        grad = torch.randn(n, generator=g) * (1 + k)
        norm = float(grad.double().norm())
        if poison is not None and k == 1:
            grad[n // 2] = poison
        gb.view[0].copy_(grad.cuda())
        max_norm = 0.1 * norm if clip else 100.0 * (norm + 1)
        ref = R.AdamRef(n, lr, betas, eps, wd, max_norm, start_step + k)
        state = [b.view[0].cpu() for b in bufs]
        red.twice(cabi, lambda sc, slot, ws: cabi.lib.bd_sumsq(gb.ptr, n, sc, slot, ws, cabi.stream()))
        cabi.check(cabi.lib.bd_adam_step(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, R.f32(lr), R.f32(betas[0]), R.f32(betas[1]),
                                         R.f32(eps), R.f32(wd), start_step + k + 1, R.f32(max_norm), red.sc.data_ptr(),
                                         SLOT, cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(*bufs)
        r = ref.step(state[0], state[1], state[2], state[3])
        for nm, b in zip(("p", "g", "m", "v"), bufs):
            got, (rv, mag) = b.view[0].cpu(), r[nm]
            if poison is not None and k >= 1:
                fin = torch.isfinite(rv)
                assert torch.equal(torch.isnan(got), torch.isnan(rv)), f"adam {nm}: NaN pattern differs from torch"
                assert torch.equal(torch.isinf(got), torch.isinf(rv)), f"adam {nm}: inf pattern differs from torch"
                if bool(fin.any()):
                    worst = max(worst, R.check_close(f"adam {nm} step {k}", got[fin], rv[fin], mag[fin]))
            else:
                worst = max(worst, R.check_close(f"adam {nm} step {k}", got, rv, mag))
        if poison is not None and k >= 1:
            break
    return worst


@pytest.mark.parametrize("n", [1, 257, 3_000_001])
@pytest.mark.parametrize("wd", [0.0, 1e-6, 1e-2])
@pytest.mark.parametrize("clip", [False, True])
def test_adam(cabi, n, wd, clip):
    _report("bd_adam_step", f"n={n},wd={wd},clip={clip}", _adam_run(cabi, n, wd, clip))


@pytest.mark.parametrize("n", [257, 3_000_001])
def test_adam_resumed(cabi, n):
    """A run that resumes at step 1000 with nonzero moments (bias correction far from its first steps)."""
    _report("bd_adam_step", f"n={n},resume1000", _adam_run(cabi, n, 1e-2, True, start_step=999))


@pytest.mark.parametrize("poison", [NAN, math.inf])
def test_adam_non_finite(cabi, poison):
    """One NaN gradient makes every parameter NaN, as clip_grad_norm_ + Adam do; an inf gradient matches torch too."""
    _adam_run(cabi, 257, 1e-2, False, poison=poison)
    _report("bd_adam_step", f"poison={poison}", 0.0)


# ---- bd_polyak -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 1000, 262_145])
def test_polyak(cabi, n):
    g = _g(n)
    t, s = torch.randn(n, generator=g), 10 * torch.randn(n, generator=g)
    for w in (1.0, 0.005, 0.0):
        tb = R.Placed(1, n, n, 2)
        tb.view[0].copy_(t.cuda())
        si = _inp(s)
        cabi.check(cabi.lib.bd_polyak(tb.ptr, si.ptr, n, R.f32(w), cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(tb)
        ref, mag = R.polyak_ref(t, s, R.f32(w))
        _report("bd_polyak", f"n={n},w={w}", R.check_close("polyak", tb.view[0].cpu(), ref, mag))


# ---- Categorical head --------------------------------------------------------------------------------------------------

CS = [1, 2, 31, 32, 33, 64, 100, 128]


def _cat_logits(rows, D, C, seed, spread=80.0):
    g = _g(seed)
    x = spread * (2 * torch.rand(rows, D, C, generator=g) - 1)
    x.view(-1, C)[::3] = 0.25   # all-equal groups
    return x


def _run_cat_head(cabi, logits, q):
    rows, D, C = logits.shape
    n = logits.numel()
    li, qi = _inp(logits), _inp(q, 2)
    st, pr = _out(n, 1), _out(n, 2)
    cabi.check(cabi.lib.bd_categorical_head_forward(li.ptr, qi.ptr, rows, D, C, st.ptr, pr.ptr, cabi.stream()))
    torch.cuda.synchronize()
    _outside_ok(st, pr)
    return st.view[0].cpu().view(rows, D, C), pr.view[0].cpu().view(rows, D, C)


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("D", [1, 32])
def test_categorical_head(cabi, C, D):
    w = 0.0
    for rows in (1, 7, 2500):
        logits = _cat_logits(rows, D, C, rows * C + D)
        q = torch.empty(rows, D, C).exponential_(1.0, generator=_g(rows + C))
        state, probs = _run_cat_head(cabi, logits, q)
        pref, S, allow = R.cat_probs_ref(logits)
        w = max(w, R.check_close(f"cat probs C={C}", probs, pref, S, allow))
        assert torch.equal(state, R.expected_state(probs, q)), f"cat state C={C} rows={rows}"
        dstate = torch.randn(rows, D, C, generator=_g(C))
        di, pi, dl = _inp(dstate), _inp(probs, 3), _out(rows * D * C)
        cabi.check(cabi.lib.bd_categorical_head_backward(di.ptr, pi.ptr, rows, D, C, dl.ptr, cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(dl)
        ref, S = R.cat_head_bwd_ref(dstate, probs)
        w = max(w, R.check_close(f"cat head bwd C={C}", dl.view[0].cpu().view(rows, D, C), ref, S, R.TINY))
    _report("bd_categorical_head", f"C={C},D={D}", w)


@pytest.mark.parametrize("C", [2, 33, 64, 100, 128])
def test_categorical_argmax_ties(cabi, C):
    """Equal probabilities and crafted q: pairs (a, b), a < b, share the smallest q; the first maximum (a) must win,
    in one lane (b = a + 32), across lanes, and with the unique winner in the tail of a partial lane group."""
    pairs = [(0, 1), (0, C - 1), (C - 2, C - 1)]
    pairs += [(a, a + 32) for a in (0, 5, 31) if a + 32 < C] + [(a + 1, a + 32) for a in (3, 30) if a + 32 < C]
    pairs += [(5, 36), (1, 33), (33, 96), (97, 127)]
    pairs = [(a, b) for a, b in pairs if 0 <= a < b < C]
    rows = len(pairs) + 2
    logits = torch.zeros(rows, 1, C)
    q = torch.full((rows, 1, C), 2.0)
    want = []
    for i, (a, b) in enumerate(pairs):
        q[i, 0, a] = q[i, 0, b] = 0.5
        want.append(a)
    q[-2, 0, C - 1] = 0.25                      # unique winner: the last class (the tail lane group when C % 32 != 0)
    want.append(C - 1)
    want.append(0)                              # all equal: class 0
    state, probs = _run_cat_head(cabi, logits, q)
    assert torch.equal(probs, probs[..., :1].expand_as(probs)), "equal logits gave unequal probabilities"
    assert abs(float(probs[0, 0, 0]) - 1.0 / C) <= 4 * R.U / C
    assert torch.equal(state.argmax(-1).view(-1), torch.tensor(want)), (state.argmax(-1).view(-1), want)
    assert torch.equal(state.sum(-1), torch.ones(rows, 1))
    _report("bd_categorical_head", f"ties,C={C}", 0.0)


# ---- Categorical KL ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("D", [1, 32])
@pytest.mark.parametrize("kl_balance", [0.8, -1.0])
@pytest.mark.parametrize("branch", ["above", "below", "tie"])
def test_categorical_kl(cabi, C, D, kl_balance, branch):
    sum_form = kl_balance == -1
    w = 0.0
    for rows in ((1, 7, 2500) if (D == 1 or C == 33) else (1, 7, 300)):
        g = _g(rows * C + D)
        ql = 3 * torch.randn(rows, D, C, generator=g)
        pl = 3 * torch.randn(rows, D, C, generator=g)
        if branch == "tie" and sum_form:
            pl[::2] = ql[::2]                     # identical rows: KL exactly 0 = free nats; the others lie above
            near = R.O.kl_categorical(ql.double(), pl.double()).sum(-1) < 1e-3
            pl[near] = ql[near]                   # no row within fp32 error of the tie
        kl = R.O.kl_categorical(ql.double(), pl.double())
        if sum_form:
            rs = kl.sum(-1)
            fn = {"above": 0.5 * float(rs.min()) - 1e-3, "below": 2 * float(rs.max()) + 1, "tie": 0.0}[branch]
        else:
            mean = float(kl.mean())
            fn = {"above": 0.5 * mean, "below": 2 * mean + 1, "tie": mean}[branch]
        fn_k = fn_r = R.f32(fn)
        qi, pi = _inp(ql), _inp(pl, 2)
        red = Red(cabi)
        got = red.twice(cabi, lambda sc, slot, ws: cabi.lib.bd_kl_categorical_forward(
            qi.ptr, pi.ptr, rows, D, C, fn_k, int(sum_form), sc, slot, ws, cabi.stream()))
        inv_count = 1.0 / rows if sum_form else 1.0 / (rows * D)
        if branch == "tie" and not sum_form:
            fn_k = float(np.float32(got) * np.float32(inv_count))
            fn_r = mean
        weight = 0.75
        scalar, Ssc, _, dq_ref, Sq, dp_ref, Sp = R.cat_kl_ref(ql, pl, fn_r, kl_balance, weight)
        w = max(w, R.check_scalar("cat kl scalar", got, scalar, Ssc, R.red_c(D + 9 if sum_form else 9)))
        dq, dp = _out(ql.numel(), 1), _out(ql.numel(), 2)
        cabi.check(cabi.lib.bd_kl_categorical_backward(qi.ptr, pi.ptr, rows, D, C, fn_k, kl_balance, weight,
                                                       R.f32(inv_count), red.sc.data_ptr(), SLOT, dq.ptr, dp.ptr,
                                                       cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(dq, dp)
        w = max(w, R.check_close("cat kl dpost", dq.view[0].cpu().view(rows, D, C), dq_ref, Sq, R.TINY))
        w = max(w, R.check_close("cat kl dprior", dp.view[0].cpu().view(rows, D, C), dp_ref, Sp, R.TINY))
    _report("bd_kl_categorical", f"C={C},D={D},bal={kl_balance},{branch}", w)


def test_categorical_kl_backward_nan_mean_passes_gradient(cabi):
    rows, D, C = 3, 2, 33
    g = _g(11)
    ql, pl = 3 * torch.randn(rows, D, C, generator=g), 3 * torch.randn(rows, D, C, generator=g)
    qi, pi = _inp(ql), _inp(pl, 2)
    sc = torch.full((8,), R.SENTINEL, device="cuda")
    sc[SLOT] = NAN
    dq, dp = _out(ql.numel(), 1), _out(ql.numel(), 2)
    cabi.check(cabi.lib.bd_kl_categorical_backward(qi.ptr, pi.ptr, rows, D, C, 3.0, 0.8, 1.0, 1.0 / (rows * D),
                                                   sc.data_ptr(), SLOT, dq.ptr, dp.ptr, cabi.stream()))
    torch.cuda.synchronize()
    _, _, _, dq_ref, Sq, dp_ref, Sp = R.cat_kl_ref(ql, pl, -1.0, 0.8, 1.0)
    R.check_close("cat kl nan dpost", dq.view[0].cpu().view(rows, D, C), dq_ref, Sq, R.TINY)
    R.check_close("cat kl nan dprior", dp.view[0].cpu().view(rows, D, C), dp_ref, Sp, R.TINY)


# ---- bd_colsum -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [1, 3, 32, 33, 200, 256])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 65537, 4_000_000])
def test_colsum(cabi, N, M):
    M = min(M, 128_000_000 // N)        # <= 512 MB of input (M = 4e6 up to N = 32; 500k rows at N = 256)
    g = torch.Generator(device="cuda").manual_seed(M + N)
    xi = R.Placed(M, N, N, 3, float("nan"))
    xi.view.normal_(generator=g).add_(1.0)     # biased: a dropped block is not hidden in the noise
    x = xi.view
    out = _out(N, 2)
    ws = torch.full((int(R.K_COLSUM_BLOCKS * N),), NAN, device="cuda")
    assert int(cabi.lib.bd_colsum_ws_floats(N)) == ws.numel()
    vals = []
    for _ in range(2):
        out.buf.fill_(R.SENTINEL)
        cabi.check(cabi.lib.bd_colsum(xi.ptr, M, N, out.ptr, ws.data_ptr(), cabi.stream()))
        torch.cuda.synchronize()
        _outside_ok(out)
        vals.append(out.view[0].clone())
    assert torch.equal(vals[0], vals[1])
    ref, S = R.colsum_ref(x)
    c = (R.colsum_chain(M, N) + 8) * R.U
    _report("bd_colsum", f"N={N},M={M}", R.check_close("colsum", vals[0].double(), ref, S, c=c))
