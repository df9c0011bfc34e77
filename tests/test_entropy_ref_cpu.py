"""CPU tests of tests/entropy_ref.py, the float64 reference of the tanh-Normal entropy estimator: pinned to autograd of
the oracle's own tanh_normal_log_prob, its bound held by a torch-fp32 emulation of entropy_sample and missed by planted
faults, the input conditions of the GPU shape table, the candidate-y comparison of the in-between zone on the
emulation, and the host-side argument checks of bd_actor_entropy (no launch: every call is rejected before one).
Run with -s to see the ENTROPY_RATIOS lines."""
import ctypes as C
import json

import pytest
import torch

from oracle import dreamer_oracle as O
from tests import entropy_ref as E

D64 = torch.float64
TEETH_SHAPE = (2, 5, 3, 7)          # Hm, N, A, ns: ns != N (a swapped read differs), ns > 1, A > 1


def _oracle_autograd(mean, sd, eps):
    """entropy, d entropy / d mean, d entropy / d std as Dreamer.get_action composes them (oracle.get_action), float64."""
    m = mean.double().requires_grad_(True)
    s = sd.double().requires_grad_(True)
    e = eps.double()
    ents = []
    for t in range(e.shape[0]):
        y = torch.tanh(m[t].unsqueeze(0) + s[t].unsqueeze(0) * e[t])
        ents.append(-torch.mean(O.tanh_normal_log_prob(y, m[t].unsqueeze(0), s[t].unsqueeze(0)), 0))
    ent = torch.stack(ents)
    ent.sum().backward()
    return dict(entropy=ent.detach(), d_mean=m.grad, d_std=s.grad)


@pytest.mark.parametrize("regime", ["regular", "saturated"])
def test_reference_is_the_oracles_autograd(regime, monkeypatch):
    """estimate64 (exact = True: no fp32 rounding of u and y) equals float64 autograd of the oracle to 1e-12 relative;
    in the saturated regime with the oracle's clamp constant replaced by its fp32 value (in float64 the oracle would
    otherwise clamp at the double 0.99999997, which fp32 code never sees)."""
    if regime == "saturated":
        monkeypatch.setattr(O, "ATANH_CLAMP", E.CLAMP32)
    Hm, N, A, ns = 3, 7, 4, 9
    mean, sd, eps = E.MAKERS[regime](Hm, N, A, ns, seed=5)
    want = _oracle_autograd(mean, sd, eps)
    est = E.estimate64(mean, sd, eps, ns, exact=True)
    for k, t in est.items():
        scale = want[k].abs().clamp(min=1.0)
        assert float(((t.ref - want[k]).abs() / scale).max()) < 1e-12, k
    if regime == "saturated":           # the mask is what was compared: no gradient flows through xh
        s = E.sample64(mean.unsqueeze(1), sd.unsqueeze(1), eps, exact=True)
        xh_sat = 0.5 * torch.log(torch.tensor((1 + E.CLAMP32) / (1 - E.CLAMP32), dtype=D64))
        assert torch.allclose(s["dm"].ref, (xh_sat * torch.sign(mean).double() - mean.double()).unsqueeze(1) / 25.0, rtol=1e-9)


def test_clamp_constant_and_unreachable_softplus_branch():
    assert E.CLAMP32 == 1.0 - 2.0 ** -24 and E.CLAMP32 != E.CLAMP_DOUBLE
    assert float(torch.nextafter(torch.tensor(E.CLAMP32, dtype=torch.float32), torch.tensor(2.0))) == 1.0
    xh_max = 0.5 * torch.log(torch.tensor((1 + E.CLAMP32) / (1 - E.CLAMP32), dtype=D64))
    assert 2.0 * float(xh_max) < 20.0       # t = -2 xh never reaches F.softplus's threshold: a fault in that branch cannot be planted


@pytest.mark.parametrize("regime", E.REGIMES)
def test_fp32_emulation_stays_inside_the_bound(regime):
    """torch-fp32 emulation of entropy_sample against estimate64, 400 k draws per regime, per draw and as estimates."""
    Hm, N, A, ns = 4, 250, 4, 100
    mean, sd, eps = E.MAKERS[regime](Hm, N, A, ns, seed=1)
    lp, dm, ds = E.emulate(mean.unsqueeze(1), sd.unsqueeze(1), eps)
    rep = E.ratios(dict(lp=lp, dm=dm, ds=ds), E.sample64(mean.unsqueeze(1), sd.unsqueeze(1), eps), f"{regime} draw ")
    rep_est = E.ratios(E.emulate_estimate(mean, sd, eps), E.estimate64(mean, sd, eps, ns), f"{regime} estimate ")
    print("ENTROPY_RATIOS emulation", regime, json.dumps(dict(draw=rep, estimate=rep_est)))
    assert max(rep.values()) < 1.0 and max(rep_est.values()) < 1.0


def test_gpu_shape_table_holds_no_draw_between_the_regimes():
    """Every case of ENTROPY_SHAPES in every regime: the float64 u of every draw is regular or saturated, as the regime
    says; the mixed cases with ns >= 2 hold both kinds in every (row, action dim)."""
    for name, (Hm, N, A, ns) in E.ENTROPY_SHAPES.items():
        for i, regime in enumerate(E.REGIMES):
            mean, sd, eps = E.MAKERS[regime](Hm, N, A, ns, seed=E.case_seed(name, regime))
            r = E.regime_of(E.u64(mean, sd, eps))
            assert int((r == E.BETWEEN).sum()) == 0, (name, regime)
            if regime == "regular":
                assert bool((r == E.REGULAR).all())
            elif regime == "saturated":
                assert bool((r == E.SATURATED).all())
            elif ns >= 2:
                assert bool((r == E.REGULAR).any(1).all()) and bool((r == E.SATURATED).any(1).all()), name
            else:
                assert bool((r == E.REGULAR).any()) and bool((r == E.SATURATED).any()), name
    # the table reaches every lane layout and sample-part filling the kernel has
    assert {c[2] for c in E.ENTROPY_SHAPES.values()} == {1, 3, 6, 17, 32, 33, 64}
    assert {c[3] for c in E.ENTROPY_SHAPES.values()} == {1, 5, 16, 17, 100}
    for name, (Hm, N, A, ns) in E.ENTROPY_SHAPES.items():
        rows_pb = 64 // A
        if Hm * N > 1 and rows_pb > 1:
            assert (Hm * N) % rows_pb != 0 and Hm * N > rows_pb, name
    mean, sd, e = E.make_between_grid()
    u = mean.double() + sd.double() * e.double()
    assert bool((E.regime_of(u) == E.BETWEEN).all()) and bool((u > 0).any()) and bool((u < 0).any())
    assert int(((u.abs() >= 8) & (u.abs() <= 9.5)).sum()) >= 2048


def test_planted_faults_exceed_the_bound_tenfold():
    """Each wrong variant (float64, so the fault is the only error) misses the bound by >= 10x in at least one output of
    at least one regime."""
    Hm, N, A, ns = TEETH_SHAPE
    worst = {v: 0.0 for v in E.VARIANTS}
    where = {}
    for regime in E.REGIMES:
        mean, sd, eps = E.MAKERS[regime](Hm, N, A, ns, seed=2)
        est = E.estimate64(mean, sd, eps, ns)
        clean = E.emulate_estimate(mean, sd, eps, D64)
        for k, t in est.items():        # without a fault the float64 restatement is the reference up to its fp32-rounded u
            assert float(((clean[k] - t.ref).abs() / E.bound(t)).max()) < 0.05, (regime, k)
        for v in E.VARIANTS:
            got = E.emulate_estimate(mean, sd, eps, D64, variant=v)
            for k, t in est.items():
                r = float(((got[k] - t.ref).abs() / E.bound(t)).max())
                if r > worst[v]:
                    worst[v], where[v] = r, f"{regime}/{k}"
    print("ENTROPY_RATIOS teeth", json.dumps({v: f"{worst[v]:.3g} at {where.get(v)}" for v in E.VARIANTS}))
    for v in E.VARIANTS:
        assert worst[v] >= 10.0, (v, worst[v])


def test_unmasked_formula_is_the_masked_one_in_fp32():
    """CLAMP32 is the fp32 predecessor of 1: |y| > clamp means y = +-1, where 1 - y * y is exactly 0, so the kernel's J
    formula gives 0 there without the mask too.  (Recorded in DESIGN.md: the mask of entropy_sample is redundant in
    fp32; the variant with teeth is J = 1 outside the clamp.)"""
    for regime in E.REGIMES:
        mean, sd, eps = E.MAKERS[regime](*TEETH_SHAPE, seed=2)
        a = E.emulate(mean.unsqueeze(1), sd.unsqueeze(1), eps)
        b = E.emulate(mean.unsqueeze(1), sd.unsqueeze(1), eps, variant="unmasked_literal")
        assert all(torch.equal(x, y) for x, y in zip(a, b)), regime


def test_between_zone_candidates_accept_the_emulation_everywhere():
    """The candidate-y comparison of the GPU test on the torch-fp32 emulation: every grid point is explained by ONE fp32
    neighbour of the correctly rounded tanh(u) in all three outputs; and it rejects a planted fault."""
    mean, sd, e = E.make_between_grid()
    lp, dm, ds = E.emulate(mean, sd, e)
    off, worst = E.match_candidates(lp, dm, ds, mean, sd, e)
    hist = {int(k): int((off == k).sum()) for k in off.unique()}
    print("ENTROPY_RATIOS between emulation", json.dumps(dict(offsets=hist, worst=worst)))
    assert int((off == -99).sum()) == 0, hist
    # ("unmasked" cannot be told from a 1-ulp tanh here: y = 1 unmasked IS the candidate y = clamp, the same xh with J = 1)
    for v in ("ds_without_inv_sd", "dm_sign"):
        bad = E.emulate(mean, sd, e, D64, variant=v)
        off_v, _ = E.match_candidates(*bad, mean, sd, e)
        assert int((off_v == -99).sum()) > 0.2 * len(mean), v


def test_rng_gather_index_is_a_bijection_onto_used_words():
    """Draw k of (row, j) -> one element of the fill buffer: distinct elements, inside the buffer."""
    for Hm, N, A, ns in E.RNG_SHAPES:
        idx, n = E.rng_gather_index(Hm, N, A, ns)
        assert idx.shape == (Hm, ns, N, A) and int(idx.min()) >= 0 and int(idx.max()) < n
        assert idx.unique().numel() == idx.numel()


def test_actor_entropy_host_checks_without_gpu():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    p = C.c_void_p(16)      # never dereferenced: each call fails one host-side check before any launch

    def call(eps=p, stats=p, ent=p, Hm=2, N=5, A=3, ns=4):
        return lib.bd_actor_entropy(eps, stats, ent, Hm, N, A, ns, None)

    for kw in (dict(eps=None), dict(stats=None), dict(ent=None), dict(A=65), dict(A=0), dict(ns=0), dict(Hm=0), dict(N=0)):
        assert call(**kw) != 0, kw
        assert b"bd_actor_entropy: bad arguments" in lib.bd_last_error(), kw
    for kw in (dict(stats=None), dict(ent=None), dict(A=65), dict(ns=0)):
        a = dict(dict(stats=p, ent=p, Hm=2, N=5, A=3, ns=4), **kw)
        assert lib.bd_actor_entropy_rng(1, 2, 3, a["stats"], a["ent"], a["Hm"], a["N"], a["A"], a["ns"], None) != 0
        assert b"bd_actor_entropy_rng: bad arguments" in lib.bd_last_error(), kw
    with pytest.raises(RuntimeError, match="bd_actor_entropy"):
        _cabi.check(call(A=65))


# ---- the train-step case of test_entropy_kernels_gpu.py: its precondition and its control -----------------------------------

def _step_run(hp_over=None):
    import numpy as np
    from big_dreamer_amd import synth
    d, seed, hp, P = E.step_case()
    od = O.OracleDreamer(P, dict(hp, planning_horizon=d.H, **(hp_over or {})))
    batch = synth.make_batch(d, seed)
    out = []
    for step in range(2):
        nz = synth.make_noise(d, seed + step)
        actor_sd = {k: v.detach().clone() for k, v in od.P["actor"].items()}
        od.train_step(batch, nz)
        if step == 0:
            od.update_critic()
        gn = od.last["grad_norms"]["actor"]
        coef = min(1.0, od.hp["grad_clip_norm"] / (gn + 1e-6))
        out.append(dict(u=E.step_entropy_u(od, actor_sd, nz["entropy"]), grads=[(g * coef).numpy() for g in od.last["actor_grads"]],
                        ent=od.last["action_entropy"].double()))
    return out


def test_step_case_keeps_every_entropy_draw_regular():
    """Precondition of the GPU train-step test, on the oracle's run: no entropy draw of either step leaves the regular
    regime (so the estimator is well conditioned and the parity tolerances mean something), with margin."""
    for step, r in enumerate(_step_run()):
        u = r["u"]
        assert u.shape[1] == 100
        assert bool((E.regime_of(u) == E.REGULAR).all()), (step, float(u.abs().max()))
        print("ENTROPY_RATIOS step_case", step, f"max|u| {float(u.abs().max()):.3f}")
        assert float(u.abs().max()) < E.U_REG - 0.3


def test_step_case_entropy_term_is_visible():
    """The control: with entropy_weight = 0 the oracle's clipped actor gradient moves by more than 10x the tolerance the GPU
    test compares it at (2e-3 of the tensor's largest entry), in the last layer's weight and bias."""
    import numpy as np
    with_ent, without = _step_run(), _step_run(dict(entropy_weight=0.0))
    for step in range(2):
        for i in (-2, -1):
            want = with_ent[step]["grads"][i]
            tol = 2e-3 * float(np.abs(want).max()) + 1e-9
            moved = float(np.abs(without[step]["grads"][i] - want).max())
            print("ENTROPY_RATIOS step_control", step, i, f"moved {moved:.3e} tolerance {tol:.3e}")
            assert moved > 10.0 * tol, (step, i, moved, tol)
