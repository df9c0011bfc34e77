"""CPU: the yardstick of the Categorical planner tests -- the float32 oracle against the float64 one.

The reference cannot produce golden vectors for planning on Categorical latents (its Categorical
``TransitionModel.forward`` raises at HEAD; the shims that repair it live in ``oracle/gen_golden.py``), so the GPU tests
of tests/test_planner_cat_gpu.py pin the kernels to the CPU oracle composed in tests/planner_cat_oracle.py from
functions the reference's own runs already pin (``transition_forward_categorical``, ``dense_on_features``, the loop of
``mpc_planner``).  ``argmax(probs / q)`` is discontinuous, so those tests rest on two figures that are re-measured and
asserted here:
  * small cases: the margin of every draw exceeds planner_cat_oracle.MIN_GAP and the float32 oracle takes the float64
    oracle's index path on EVERY candidate of every iteration (what the GPU tests then demand of the kernel);
  * full size: float32 against float64 diverges on at most 2 of 1000 candidates per iteration (the GPU cap is 5), and
    the returns of the others agree to 1e-6 (two orders inside the GPU tolerance of 1e-4).
And ``synth.make_planner_noise`` still gives Gaussian ``Dims`` the stream the planner golden files were drawn from.
"""
import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import planner_cat_oracle as PO


def _both(name):
    d, B, H, iters, cand, top, pseed, nseed = PO.PLAN_CASES[name]
    c = PO.make_case(d, B, H, iters, cand, pseed, nseed)
    nz = c["noise"]
    t64, t32 = [], []
    PO.mpc_planner_categorical(c["P"], c["belief"], c["state"], d, H, iters, cand, top, nz["action"], nz["state"], t64,
                               torch.float64)
    if name != "full":
        PO.mpc_planner_categorical(c["P"], c["belief"], c["state"], d, H, iters, cand, top, nz["action"], nz["state"], t32,
                                   torch.float32)
    else:      # teacher-forced like the GPU test: every float32 iteration starts from the float64 loop's action belief
        mean, std = torch.zeros(H, B, d.A), torch.ones(H, B, d.A)
        for it in range(iters):
            t32.append(PO.rollout_categorical(c["P"], c["belief"], c["state"], d, mean, std, nz["action"][it], nz["state"][it],
                                              torch.float32))
            mean, std = t64[it]["mean"].float(), t64[it]["std"].float()
    return t64, t32


@pytest.mark.parametrize("name", ["cat_tiny", "cat_32"])
def test_small_cases_margin_and_exact_paths(name):
    t64, t32 = _both(name)
    margin = min(float(r["gap"].min()) for r in t64)
    print(f"{name}: smallest margin {margin:.3e} over {sum(r['gap'].numel() for r in t64)} draws")
    assert margin > PO.MIN_GAP[name]
    for it, (a, b) in enumerate(zip(t64, t32)):
        assert torch.equal(a["idx"], b["idx"]), f"iteration {it}: float32 took another index path"
        err = float((a["returns"] - b["returns"].double()).abs().max())
        assert err < 1e-6, f"iteration {it}: return error {err:.3e}"
        assert torch.equal(a["returns"].topk(PO.PLAN_CASES[name][5]).indices.sort().values,
                           b["returns"].topk(PO.PLAN_CASES[name][5]).indices.sort().values)


def test_full_size_divergence_of_the_yardstick():
    t64, t32 = _both("full")
    for it, (a, b) in enumerate(zip(t64, t32)):
        same = (a["idx"] == b["idx"]).all(dim=2).all(dim=0)
        n_div = int((~same).sum())
        err = float((a["returns"] - b["returns"].double()).abs()[same].max())
        print(f"full it{it}: {n_div} of {same.numel()} candidates diverged; max return error on the rest {err:.3e}")
        assert n_div <= 2 and err < 1e-6


def _old_planner_noise(d, B, horizon, iters, candidates, seed):
    """make_planner_noise as it was before Categorical latents (the stream order the golden files depend on)."""
    ns = synth.NoiseStream(seed)
    act = np.empty((iters, horizon, B, candidates, d.A), np.float32)
    st = np.empty((iters, horizon, B * candidates, d.S), np.float32)
    for it in range(iters):
        act[it] = ns.normal((horizon, B, candidates, d.A))
        for t in range(horizon):
            st[it, t] = ns.normal((B * candidates, d.S))
    return {"action": act, "state": st}


@pytest.mark.parametrize("d,B,H,iters,cand,seed", [(synth.TINY, 2, 5, 4, 64, 6), (synth.CONFIG2, 1, 15, 2, 1000, 7)])
def test_gaussian_planner_noise_unchanged(d, B, H, iters, cand, seed):
    got, want = synth.make_planner_noise(d, B, H, iters, cand, seed), _old_planner_noise(d, B, H, iters, cand, seed)
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)


def test_categorical_planner_noise_is_exponential_per_factor():
    d = synth.CAT_TINY
    nz = synth.make_planner_noise(d, 2, 3, 2, 8, 1)
    assert nz["state"].shape == (2, 3, 16, d.S) and (nz["state"] >= 0).all() and abs(float(nz["state"].mean()) - 1.0) < 0.1
    ns = synth.NoiseStream(1)
    ns.normal((3, 2, 8, d.A))
    assert np.array_equal(nz["state"][0, 0], ns.exponential((16 * d.cat_D, d.cat_C)).reshape(16, d.S))
