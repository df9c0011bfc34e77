"""GPU tests of the tanh-Normal entropy estimator against tests/entropy_ref.py: bd_actor_entropy on explicit draws in the
regular, saturated and mixed regimes at every lane layout of its workgroup, bd_actor_entropy_rng bit for bit against
bd_actor_entropy on the draws gathered from bd_rng_fill, the zone between the regimes per sample against the candidate
values of tanh(u), the in-scan forms of bd_imagine_forward_scan and bd_imagine_cat_forward (sv_act_stats = NULL), the
bd_imagine_forward wrapper, and one whole train step whose actor gradient is dominated by the entropy term.  Outputs sit
in SENTINEL-padded buffers, inputs in NaN-padded ones; every launch is followed by a synchronise (which raises on a device
error); nothing retries.  Each test prints its worst err / bound per output as ENTROPY_RATIOS lines (run with -s)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import entropy_ref as E
from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.dense_ref import Placed, placed_input
from tests.test_scan_kernels_gpu import ImagineCase, cabi, pin, same_bits, sync

pytestmark = pytest.mark.gpu


def launch_entropy(mean, sd, eps, ns, rng=None):
    """bd_actor_entropy (rng = None) or bd_actor_entropy_rng (rng = (seed, step, stream id)) on statistics whose slots
    2, 3 hold (mean, sd) and whose slots 0, 1 hold other numbers.  Returns (stats Placed, entropy Placed)."""
    c = cabi()
    Hm, N, A = mean.shape
    M = Hm * N
    g = torch.Generator().manual_seed(7)
    s01 = torch.randn(M, 2 * A, generator=g).cuda()
    st = Placed(M, 4 * A, 4 * A)
    st.view.copy_(torch.cat([s01, mean.reshape(M, A).cuda(), sd.reshape(M, A).cuda()], 1))
    ent = Placed(M, 1, 1)
    if rng is None:
        e = placed_input(eps.reshape(-1, A).cuda().contiguous(), A)
        c.check(c.lib.bd_actor_entropy(e.ptr, st.ptr, ent.ptr, Hm, N, A, ns, c.stream()))
    else:
        c.check(c.lib.bd_actor_entropy_rng(rng[0], rng[1], rng[2], st.ptr, ent.ptr, Hm, N, A, ns, c.stream()))
    sync()
    assert st.outside_unchanged() and ent.outside_unchanged(), "written outside the rows"
    assert torch.equal(st.view[:, :2 * A], s01), "slots 0, 1 of the statistics changed"
    return st, ent


def outputs(st, ent, Hm, N, A):
    return dict(entropy=ent.view.reshape(Hm, N), d_mean=st.view[:, 2 * A:3 * A].reshape(Hm, N, A),
                d_std=st.view[:, 3 * A:].reshape(Hm, N, A))


# ---- a. bd_actor_entropy, explicit draws --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(E.ENTROPY_SHAPES))
def test_actor_entropy_against_float64(name):
    Hm, N, A, ns = E.ENTROPY_SHAPES[name]
    rep = {}
    for regime in E.REGIMES:
        mean, sd, eps = (x.cuda() for x in E.MAKERS[regime](Hm, N, A, ns, seed=E.case_seed(name, regime)))
        assert int((E.regime_of(E.u64(mean, sd, eps)) == E.BETWEEN).sum()) == 0
        st, ent = launch_entropy(mean, sd, eps, ns)
        got = outputs(st, ent, Hm, N, A)
        rep[regime] = E.ratios(got, E.estimate64(mean, sd, eps, ns), f"{name} {regime} ")
        st2, ent2 = launch_entropy(mean, sd, eps, ns)
        assert torch.equal(st.buf, st2.buf) and torch.equal(ent.buf, ent2.buf), f"{name} {regime}: second run differs"
    print("ENTROPY_RATIOS actor_entropy", name, json.dumps(rep))
    assert all(max(r.values()) < 1.0 for r in rep.values()), rep


# ---- b. bd_actor_entropy_rng, exactly ------------------------------------------------------------------------------------

def rng_fill_normal(n, seed, step, sid):
    c = cabi()
    buf = torch.zeros(n, device="cuda")
    a = c.RngFillArgs()
    a.n, a.seed, a.step = 1, seed, step
    a.t[0] = c.RngTensor(buf.data_ptr(), buf.numel(), c.BD_RNG_NORMAL, sid)
    c.check(c.lib.bd_rng_fill(C.byref(a), c.stream()))
    sync()
    return buf


@pytest.mark.parametrize("shape", E.RNG_SHAPES, ids=lambda s: "hm%d_n%d_a%d_ns%d" % s)
def test_in_kernel_draws_are_the_fill_kernels_draws_bit_for_bit(shape):
    """The Philox form draws sample k of (row, j) from the counter and word rng_gather_index restates; bd_actor_entropy
    on those draws, gathered from a bd_rng_fill buffer of the same seed, step and stream, gives the same bits."""
    Hm, N, A, ns = shape
    seed, step, sid = 0x1234567ABCDEF, 5, 4
    idx, n = E.rng_gather_index(Hm, N, A, ns)
    eps = rng_fill_normal(n, seed, step, sid)[idx.cuda()].contiguous()
    g = torch.Generator().manual_seed(9)
    mean = (torch.rand(Hm, N, A, generator=g) - 0.5).cuda()           # |mean| <= 0.5, sd <= 0.4: |u| <= 0.5 + 0.4 * 5.8 < 3
    sd = (0.1 + 0.3 * torch.rand(Hm, N, A, generator=g)).cuda()
    assert bool((E.regime_of(E.u64(mean, sd, eps)) == E.REGULAR).all()) and float(eps.abs().max()) < 5.8
    st_e, ent_e = launch_entropy(mean, sd, eps, ns)
    st_r, ent_r = launch_entropy(mean, sd, None, ns, rng=(seed, step, sid))
    assert torch.equal(ent_e.buf, ent_r.buf), "entropy differs between the explicit and the Philox form"
    assert torch.equal(st_e.buf, st_r.buf), "d entropy / d mean, d std differ between the explicit and the Philox form"
    rep = E.ratios(outputs(st_r, ent_r, Hm, N, A), E.estimate64(mean, sd, eps, ns), "rng ")
    print("ENTROPY_RATIOS actor_entropy_rng", shape, json.dumps(rep))


# ---- c. the zone between the regimes, per sample ---------------------------------------------------------------------------

def test_between_zone_matches_one_candidate_tanh_per_sample():
    """A = 1, ns = 1: (entropy, slot 2, slot 3) of a row are one draw's (-lp, -dm, -ds).  Each row must lie inside
    sample64's bound at ONE fp32 value y within TANH_ULPS ulps of the correctly rounded tanh(u), in all three outputs."""
    mean, sd, e = (x.cuda() for x in E.make_between_grid(4096))
    Hm, N = 4, 1024
    assert bool((E.regime_of(mean.double() + sd.double() * e.double()) == E.BETWEEN).all())
    st, ent = launch_entropy(mean.reshape(Hm, N, 1), sd.reshape(Hm, N, 1), e.reshape(Hm, 1, N, 1), 1)
    off, worst = E.match_candidates(-ent.view[:, 0], -st.view[:, 2], -st.view[:, 3], mean, sd, e)
    hist = {int(k): int((off == k).sum()) for k in off.unique()}
    print("ENTROPY_RATIOS between", json.dumps(dict(offsets=hist, worst=worst)))
    assert int((off == -99).sum()) == 0, hist


# ---- d. the in-scan forms ---------------------------------------------------------------------------------------------------

def in_scan_check(case, d, ns, tag):
    """Run 1 saves the statistics (checked layer by layer elsewhere); run 2 is the in-scan estimate on draws built from
    run 1's (mean, std): the same feat and action bits, the entropy inside estimate64's bound."""
    A = d.A
    run1 = case.forward()
    stats = run1["sv_act_stats"].view.reshape(d.T, d.B, 4 * A)
    mean, sd = stats[..., 2 * A:3 * A].clone(), stats[..., 3 * A:].clone()
    eps = E.eps_for_stats(mean, sd, ns, seed=ns)
    assert int((E.regime_of(E.u64(mean, sd, eps)) == E.BETWEEN).sum()) == 0
    run2 = case.forward(eps_entropy=pin(eps, A), n_samples=ns, stats=False)
    for k in ("feat", "action"):
        assert torch.equal(run1[k].buf, run2[k].buf), f"{tag}: {k} differs between the saved-statistics and the in-scan form"
    est = E.estimate64(mean, sd, eps, ns, chain=E.chain_scan(ns))
    return E.ratios(dict(entropy=run2["entropy"].view.reshape(d.T, d.B)), dict(entropy=est["entropy"]), tag + " ")


@pytest.mark.parametrize("name", E.SCAN_GAUSS)
def test_gaussian_scan_in_scan_entropy_against_float64(name):
    d = R.IMAGINE_SHAPES[name]
    case = ImagineCase(d, 21)
    rep = {ns: in_scan_check(case, d, ns, f"{name} ns={ns}") for ns in E.SCAN_NS}
    print("ENTROPY_RATIOS in_scan gaussian", name, json.dumps(rep))
    assert all(r["entropy"] < 1.0 for r in rep.values()), rep


@pytest.mark.parametrize("name", E.SCAN_CAT)
def test_categorical_scan_in_scan_entropy_against_float64(name):
    from tests.test_scan_cat_kernels_gpu import ImagineCase as CatImagineCase
    d = RC.IMAGINE_SHAPES[name]
    case = CatImagineCase(d, RC.SEEDS[2])
    rep = {ns: in_scan_check(case, d, ns, f"{name} ns={ns}") for ns in E.SCAN_NS}
    print("ENTROPY_RATIOS in_scan categorical", name, json.dumps(rep))
    assert all(r["entropy"] < 1.0 for r in rep.values()), rep


@pytest.mark.parametrize("name", E.SCAN_GAUSS)
def test_imagine_forward_is_the_scan_followed_by_actor_entropy(name):
    """bd_imagine_forward with statistics and draws == bd_imagine_forward_scan, then bd_actor_entropy: every output, bit
    for bit (the Gaussian twin of the check in test_scan_cat_kernels_gpu.py)."""
    d, ns = R.IMAGINE_SHAPES[name], 17
    case = ImagineCase(d, 21)
    g = torch.Generator().manual_seed(31)
    eps = pin(torch.randn(d.T, ns, d.B, d.A, generator=g).cuda(), d.A)
    whole = case.forward(eps_entropy=eps, n_samples=ns, wrapper=True)
    alone = case.forward()
    c = cabi()
    c.check(c.lib.bd_actor_entropy(eps.ptr, alone["sv_act_stats"].ptr, alone["entropy"].ptr, d.T, d.B, d.A, ns, c.stream()))
    sync()
    assert alone["sv_act_stats"].outside_unchanged() and alone["entropy"].outside_unchanged()
    same_bits(whole, alone, f"{name}: bd_imagine_forward against scan + bd_actor_entropy")
    assert bool(torch.isfinite(whole["entropy"].view).all())
    assert not torch.equal(whole["sv_act_stats"].view[:, 2 * d.A:], case.forward()["sv_act_stats"].view[:, 2 * d.A:])


# ---- e. one whole train step that can see the entropy gradient ---------------------------------------------------------------

def test_train_steps_with_a_visible_entropy_gradient_vs_oracle():
    """entropy_ref.step_case: synth.TINY, entropy_weight = 0.1, the actor's initial std lowered to 0.5 so that every
    entropy draw is regular (test_entropy_ref_cpu.py asserts that on the oracle's run, and that without the entropy term
    the actor gradient moves by more than 10x the tolerance used here).  Two train steps against OracleDreamer: logs,
    clipped actor gradients, post-Adam actor weights, at the tolerances of test_hip_parity."""
    from big_dreamer_amd import synth
    from big_dreamer_amd.engine import DreamerEngine
    from oracle import dreamer_oracle as O
    from tests.helpers import assert_close
    d, seed, hp, P = E.step_case()
    od = O.OracleDreamer(P, dict(hp, planning_horizon=d.H))
    eng = DreamerEngine(d, hp, "cuda", params=P)
    dev = lambda dct: {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}
    batch = synth.make_batch(d, seed)
    db = dev(batch)
    worst = {}

    def close(name, got, want, atol, rtol):
        got = np.asarray(got, dtype=np.float64).reshape(np.asarray(want).shape)
        want = np.asarray(want, dtype=np.float64)
        r = float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())
        key = name.split(".")[1]
        worst[key] = max(worst.get(key, 0.0), r)
        assert_close(name, got, want, atol, rtol)

    try:
        for step in range(2):
            nz = synth.make_noise(d, seed + step)
            ologs = od.train_step(batch, nz)
            logs = eng.train_step(db, dev(nz))
            if step == 0:
                od.update_critic()
                eng.update_critic()
            torch.cuda.synchronize()
            eng.cluster_status(d.B)
            for k, v in ologs.items():
                tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                close(f"s{step}.log.{k}", logs[k], v, tol[0], tol[1])
            gn = od.last["grad_norms"]["actor"]
            close(f"s{step}.gradnorm.actor", logs["grad_norm_actor"], gn, 1e-6, 1e-3)
            coef = min(1.0, od.hp["grad_clip_norm"] / (gn + 1e-6))
            for i, k in enumerate(od.P["actor"]):
                want = od.last["actor_grads"][i].numpy() * coef
                scale = float(np.abs(want).max()) + 1e-12
                close(f"s{step}.grad.actor.{k}", eng.G("actor", k).detach().cpu().numpy(), want, 2e-3 * scale + 1e-9, 2e-3)
            for k, p in od.P["actor"].items():
                close(f"s{step}.param.actor.{k}", eng.W("actor", k).detach().cpu().numpy(), p.detach().numpy(), 2e-5, 1e-5)
    finally:
        print("ENTROPY_RATIOS train_step (err / tolerance)", json.dumps(worst))
