"""GPU: bd_twohot_decode, bd_twohot_decode_backward and bd_twohot_nll (csrc/twohot.hip) on their own against the float64
restatement tests/twohot_ref.py, within the budgets measured there: every row count and bin count at which the kernels
take another path (one wave per row, four rows per workgroup, 4 or 16 registers per lane, pieces of 64), padded leading
dimensions, the fillings and targets of the restatement, guard rows and columns, the NULL forms, refused arguments, launch
determinism and the fixed-order sum of the row losses."""
import functools

import numpy as np
import pytest
import torch

from tests import reduce_ref as R
from tests import twohot_ref as T

pytestmark = pytest.mark.gpu

Z = T.Z_DEFAULT
SENT = -7777.0
GS = 0.25


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


@functools.lru_cache(maxsize=None)
def _case(name, rows, K, sweep=False):
    """Inputs and float64 results of one filling; made once and shared (read-only).  sweep: one row per target."""
    tg = T.targets(K, Z)
    if sweep:
        rows = tg.size
    rng = np.random.Generator(np.random.PCG64(1000 * K + rows))
    c = dict(l=T.filling(name, rows, K, Z), y=np.resize(tg, rows) if not sweep else tg,
             dv=rng.standard_normal(rows, dtype=np.float32), wr=rng.uniform(0.0, 1.0, rows).astype(np.float32))
    c["v"], c["m"] = T.decode(c["l"], Z)
    c["bwd"] = T.decode_backward(c["l"], c["dv"], Z)
    c["loss"], c["dl"] = T.nll(c["l"], c["y"], Z, c["wr"], GS)
    c["loss1"], c["dl1"] = T.nll(c["l"], c["y"], Z, None, GS)
    for v in c.values():
        v.setflags(write=False)
    return c


def _padded(x, ld, fill=np.nan):
    """[rows x K] -> device [rows x ld], the pad columns NaN: a kernel that read them would show it in every sum."""
    rows, K = x.shape
    out = torch.full((rows, ld), fill, dtype=torch.float32, device="cuda")
    out[:, :K] = torch.as_tensor(np.array(x)).cuda()
    return out


def _guarded(rows, width):
    """An output of `rows` rows with one guard row behind it, everything at the sentinel."""
    return torch.full((rows + 1, width), SENT, dtype=torch.float32, device="cuda")


def _check_guards(out, rows, K):
    assert torch.all(out[rows:] == SENT), "wrote beyond the last row"
    assert torch.all(out[:rows, K:] == SENT), "wrote beyond column K"


def _dev(x):
    return torch.as_tensor(np.array(x)).cuda()


def _run_all(cabi, c, K, ld, weighted=True, with_mean=True, with_value=True):
    """The three kernels on one case; returns numpy results after checking the guards."""
    lib, st = cabi.lib, cabi.stream()
    rows = c["l"].shape[0]
    l = _padded(c["l"], ld)
    val, mean, bwd = _guarded(rows, 1), _guarded(rows, 1), _guarded(rows, ld)
    cabi.check(lib.bd_twohot_decode(l.data_ptr(), ld, rows, K, Z, val.data_ptr(), mean.data_ptr() if with_mean else None, st))
    cabi.check(lib.bd_twohot_decode_backward(l.data_ptr(), ld, _dev(c["dv"]).data_ptr(), rows, K, Z, bwd.data_ptr(), ld, st))
    dl, val2, loss = _guarded(rows, ld), _guarded(rows, 1), _guarded(rows, 1)
    wr = _dev(c["wr"])
    cabi.check(lib.bd_twohot_nll(l.data_ptr(), ld, _dev(c["y"]).data_ptr(), wr.data_ptr() if weighted else None, rows, K, Z, GS,
                                 dl.data_ptr(), ld, val2.data_ptr() if with_value else None, loss.data_ptr(), st))
    torch.cuda.synchronize()
    for out, w in ((val, 1), (bwd, K), (dl, K), (loss, 1)) + (((mean, 1),) if with_mean else ()) + (((val2, 1),) if with_value else ()):
        _check_guards(out, rows, w)
    if not with_mean:
        assert torch.all(mean == SENT)
    if not with_value:
        assert torch.all(val2 == SENT)
    f = lambda t, w: t[:rows, :w].cpu().numpy().astype(np.float64)
    return dict(v=f(val, 1)[:, 0], m=f(mean, 1)[:, 0], bwd=f(bwd, K), dl=f(dl, K), loss=f(loss, 1)[:, 0], v2=f(val2, 1)[:, 0],
                loss_t=loss[:rows, 0].contiguous())


def _assert_case(tag, got, c, weighted=True, with_mean=True, with_value=True):
    loss, dl = (c["loss"], c["dl"]) if weighted else (c["loss1"], c["dl1"])
    wr = c["wr"] if weighted else np.ones_like(c["wr"])
    errs = dict(value=T.value_err(got["v"], c["v"]), decode_grad=T.grad_err(got["bwd"], c["bwd"]),
                loss=T.value_err(got["loss"], loss), nll_grad=T.grad_err(got["dl"], dl, T.NLL_GRAD_COND * GS * wr),
                nll_grad_to_weight=T.grad_err_to(got["dl"], dl, GS * wr))
    if with_mean:
        errs["mean"] = T.value_err(got["m"], c["m"])
    if with_value:
        errs["value2"] = T.value_err(got["v2"], c["v"])
    print("TWOHOT_WORST", tag, " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert errs["value"] <= T.VALUE_BUDGET and errs.get("value2", 0.0) <= T.VALUE_BUDGET, (tag, errs)
    assert errs.get("mean", 0.0) <= T.MEAN_BUDGET, (tag, errs)
    assert errs["decode_grad"] <= T.DECODE_GRAD_BUDGET, (tag, errs)
    assert errs["loss"] <= T.LOSS_BUDGET, (tag, errs)
    assert errs["nll_grad"] <= T.NLL_GRAD_BUDGET and errs["nll_grad_to_weight"] <= T.NLL_GRAD_TO_WEIGHT_BUDGET, (tag, errs)
    # the point of the head: the row L1 norm of the gradient is bounded by 2 grad_scale w_r whatever the target
    assert np.all(np.abs(got["dl"]).sum(-1) <= 2 * GS * wr * (1 + 1e-5) + 1e-30), tag


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("K", T.KS)
@pytest.mark.parametrize("rows", T.ROWS)
def test_kernels_against_the_restatement(cabi, rows, K, pad):
    for name in T.FILLINGS:
        c = _case(name, rows, K)
        _assert_case(f"{name} rows={rows} K={K} ld={K + pad}", _run_all(cabi, c, K, K + pad), c)


@pytest.mark.parametrize("K", T.KS)
def test_every_target(cabi, K):
    """One row per target -- 0, +-denormal, every bin centre and midpoint, both neighbours of every edge, +-1e9, +-FLT_MAX --
    on unit-normal logits and on the ramp next to +Z."""
    for name in ("normal", "ramp_hi"):
        c = _case(name, 0, K, sweep=True)
        _assert_case(f"targets {name} K={K}", _run_all(cabi, c, K, K + 3), c)


@pytest.mark.parametrize("K", [3, 255, 257])
def test_null_forms(cabi, K):
    c = _case("normal", 65, K)
    got = _run_all(cabi, c, K, K + 3, weighted=False, with_mean=False, with_value=False)
    _assert_case(f"null forms K={K}", got, c, weighted=False, with_mean=False, with_value=False)


def test_nan_target_gives_nan_loss(cabi):
    K, rows = 255, 5
    c = dict(_case("normal", rows, K))
    y = c["y"].copy()
    y[2] = np.nan
    c["y"] = y
    got = _run_all(cabi, c, K, K)
    assert np.isnan(got["loss"][2]) and np.isfinite(np.delete(got["loss"], 2)).all()
    keep = np.delete(np.arange(rows), 2)
    assert T.grad_err_to(got["dl"][keep], c["dl"][keep], GS * c["wr"][keep]) <= T.NLL_GRAD_TO_WEIGHT_BUDGET


def test_refused_arguments_leave_the_outputs_untouched(cabi):
    lib, st = cabi.lib, cabi.stream()
    rows, K, ld = 9, 63, 66
    c = _case("normal", rows, K)
    l, y, wr, dv = _padded(c["l"], ld), _dev(c["y"]), _dev(c["wr"]), _dev(c["dv"])
    dl, val, loss, mean = _guarded(rows, ld), _guarded(rows, 1), _guarded(rows, 1), _guarded(rows, 1)
    P = lambda t: t.data_ptr()
    good = dict(logits=P(l), ld=ld, rows=rows, K=K, zmax=Z, ldd=ld)
    bad = [dict(logits=None), dict(ld=K - 1), dict(ldd=K - 1), dict(K=1), dict(K=1025), dict(zmax=0.0), dict(zmax=-1.0),
           dict(zmax=80.5), dict(zmax=float("nan")), dict(rows=0), dict(rows=-3)]
    for change in bad:
        a = dict(good, **change)
        calls = [
            lambda: lib.bd_twohot_nll(a["logits"], a["ld"], P(y), P(wr), a["rows"], a["K"], a["zmax"], GS, P(dl), a["ldd"], P(val),
                                      P(loss), st),
            lambda: lib.bd_twohot_decode_backward(a["logits"], a["ld"], P(dv), a["rows"], a["K"], a["zmax"], P(dl), a["ldd"], st),
        ]
        if "ldd" not in change:
            calls.append(lambda: lib.bd_twohot_decode(a["logits"], a["ld"], a["rows"], a["K"], a["zmax"], P(val), P(mean), st))
        for call in calls:
            assert call() != 0, change
            assert b"bd_twohot" in lib.bd_last_error()
    for call in (lambda: lib.bd_twohot_nll(P(l), ld, None, P(wr), rows, K, Z, GS, P(dl), ld, P(val), P(loss), st),
                 lambda: lib.bd_twohot_nll(P(l), ld, P(y), P(wr), rows, K, Z, GS, None, ld, P(val), P(loss), st),
                 lambda: lib.bd_twohot_nll(P(l), ld, P(y), P(wr), rows, K, Z, GS, P(dl), ld, P(val), None, st),
                 lambda: lib.bd_twohot_decode(P(l), ld, rows, K, Z, None, P(mean), st),
                 lambda: lib.bd_twohot_decode_backward(P(l), ld, None, rows, K, Z, P(dl), ld, st),
                 lambda: lib.bd_twohot_decode_backward(P(l), ld, P(dv), rows, K, Z, None, ld, st)):
        assert call() != 0
    with pytest.raises(RuntimeError):
        cabi.check(lib.bd_twohot_decode(P(l), K - 1, rows, K, Z, P(val), None, st))
    torch.cuda.synchronize()
    for out in (dl, val, loss, mean):
        assert torch.all(out == SENT)


@pytest.mark.parametrize("K", [255, 1024])
def test_two_launches_are_bit_identical_and_the_loss_sum(cabi, K):
    rows = 257
    c = _case("normal", rows, K)
    a, b = _run_all(cabi, c, K, K + 3), _run_all(cabi, c, K, K + 3)
    for key in ("v", "m", "bwd", "dl", "loss", "v2"):
        assert np.array_equal(a[key], b[key]), key
    # value_loss: bd_sum of the row losses, the existing fixed-order reduction
    sc = torch.full((8,), R.SENTINEL, device="cuda")
    ws = torch.zeros(int(cabi.lib.bd_reduce_ws_floats()), device="cuda")
    cabi.check(cabi.lib.bd_sum(a["loss_t"].data_ptr(), rows, sc.data_ptr(), 5, ws.data_ptr(), cabi.stream()))
    torch.cuda.synchronize()
    ref, S = R.sum_ref(a["loss_t"].cpu())
    R.check_scalar(f"bd_sum(row_loss) K={K}", float(sc[5]), ref, S)
    assert abs(float(sc[5]) - float(c["loss"].sum())) <= T.LOSS_BUDGET * np.maximum(1.0, np.abs(c["loss"])).sum()
