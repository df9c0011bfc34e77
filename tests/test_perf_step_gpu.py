"""GPU: the perf-mode train step (train_step(batch): Philox draws from Engine.make_noise and from inside the kernels) against
the explicit-noise step every parity test checks (train_step(batch, noise)).

Engine P is fresh, gets set_noise_seed(s) and runs train_step(batch) twice.  Engine E has the same parameters and runs
train_step(batch, noise_k) with noise_k built HERE from the scheme as tests/rng_ref.py states it -- never from P's
counters: key = s + 0x9E37...15 * (rank + 1); obs_post / action / img_prior are bd_rng_fill buffers (value-checked by
test_rng_values_gpu.py) of streams 1 / 2 / 3 at step k of the "wm" / "bh" / "bh" counters, Exp(1) where a Categorical
sampler consumes them; the tanh-Normal actor's entropy draws are gathered from a stream-4 Normal fill at step k through
rng_gather_index; obs_prior is arbitrary, and E runs twice with two different obs_prior arrays.  After every step
P.noise_state() must be what the scheme says.  Compared: every logged scalar, every parameter tensor, the clipped
gradients and both Adam moments of every group.

Outcomes (one MI355X): torch.equal throughout, in every case, serial and pipelined:
- Gaussian latents with the tanh-Normal actor (small, tiny_discount, small at gradient_mixing = 0.5, tiny_pixel, and small
  under the chunk plan (2, 2, 1)) and with the Categorical actor (discrete_tiny_a18); Categorical latents with the
  Categorical actor (discrete_cat_tiny_a18).  Both modes run the same arithmetic: the estimator's two forms
  (bd_actor_entropy on explicit draws, bd_actor_entropy_rng) add the same draws in the same order.
- cat_tiny (Categorical latents, tanh-Normal actor).  One might expect a difference in summation order here: the
  Categorical scan can estimate the entropy itself (ceil(ns / 32) draws per sample lane, two shuffles, eight waves), and
  perf mode runs it with eps_entropy = NULL and bd_actor_entropy_rng after it.  But the scan estimates in-line only when
  it is not asked to save the actor statistics (sv_act_stats == NULL: API rollouts); in a train step
  bd_imagine_cat_forward itself launches bd_actor_entropy behind the scan on the explicit draws.  So a train step
  estimates after the scan in both modes, with one kernel body, and the case is exact like the others.
- Two different obs_prior arrays give bit-identical results everywhere: nothing on the training path reads the
  observe step's prior sample, which is why perf mode does not draw it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import rng_ref as R
from tests.discrete_oracle import DISCRETE_GOLDEN
from tests.helpers import CASES, CAT_CASES

pytestmark = pytest.mark.gpu

def _case(name):
    if name in DISCRETE_GOLDEN:
        return DISCRETE_GOLDEN[name]
    return {**CASES, **CAT_CASES}[name][:3]


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _fill(key, step, count, kind, stream):
    from big_dreamer_amd import _cabi as cabi
    t = torch.zeros(count, device="cuda")
    a = cabi.RngFillArgs()
    a.n, a.seed, a.step = 1, key, step
    a.t[0] = cabi.RngTensor(t.data_ptr(), count, kind, stream)
    cabi.check(cabi.lib.bd_rng_fill(C.byref(a), cabi.stream()))
    return t


def scheme_noise(d, B, key, counters, obs_prior_seed):
    """The explicit noise of the train step whose counters are `counters` ("wm", "bh", "entropy"), from the scheme."""
    out = {}
    for name, (shape, kind, stream) in R.train_step_fills(d, B).items():
        out[name] = _fill(key, counters[R.STEP_COUNTER[name]], int(np.prod(shape)), kind, stream).view(*shape)
    if not d.discrete_actions:
        N = d.T * B
        idx, n = R.rng_gather_index(d.Hm, N, d.A, d.n_entropy)
        buf = _fill(key, counters[R.STEP_COUNTER["entropy"]], n, R.NORMAL, R.RNG_STREAMS["entropy"])
        out["entropy"] = buf[torch.from_numpy(idx).cuda()].contiguous()
        assert out["entropy"].shape == (d.Hm, d.n_entropy, N, d.A)
    g = torch.Generator().manual_seed(obs_prior_seed)
    out["obs_prior"] = (torch.randn(d.T, B, d.S, generator=g) * 3.0).cuda()
    return out


def _engine(name, pipeline, plan, hp_extra):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp = _case(name)
    eng = DreamerEngine(d, dict(hp, **(hp_extra or {})), "cuda", params=synth.make_params(d, seed))
    eng.pipeline = pipeline
    if plan is not None:
        eng.bh_chunks = plan
    return eng


def _state(eng):
    eng.join()
    torch.cuda.synchronize()
    out = {}
    for g, grp in eng.groups.items():
        out[g + ".p"] = grp.flat.clone()
        if grp.grad is not None:
            out.update({g + ".grad": grp.grad.clone(), g + ".m": grp.m.clone(), g + ".v": grp.v.clone()})
    return out


def _run(name, pipeline, plan, hp_extra, seed_s, explicit, obs_prior_seed=0, steps=2, in_flight=False):
    """-> [(logs, state) per step], the engine.  explicit = False: engine P; True: engine E on scheme_noise.
    in_flight (engine P): the steps are enqueued back to back with nothing read in between, so that the pipelined
    schedule has two of them under way at once; -> [(logs, state) after the last step]."""
    d, seed, _ = _case(name)
    eng = _engine(name, pipeline, plan, hp_extra)
    key = R.engine_key(seed_s, rank=0)
    if not explicit:
        eng.set_noise_seed(seed_s)
    out = []
    if in_flight:
        assert not explicit
        batches = [_dev(synth.make_batch(d, seed + k)) for k in range(steps)]
        for batch in batches:
            eng.train_step(batch, sync_logs=False)
        logs = eng.logs()
        assert eng.noise_state() == {"seed": key, "step": {"wm": steps, "bh": steps}, "entropy_step": steps - 1}
        return [(dict(logs), _state(eng))], eng
    for k in range(steps):
        batch = _dev(synth.make_batch(d, seed + k))
        if explicit:
            logs = eng.train_step(batch, scheme_noise(d, d.B, key, {"wm": k, "bh": k, "entropy": k}, obs_prior_seed + k))
        else:
            logs = eng.train_step(batch)
            assert eng.noise_state() == {"seed": key, "step": {"wm": k + 1, "bh": k + 1}, "entropy_step": k}, eng.noise_state()
        out.append((dict(logs), _state(eng)))
        assert np.isfinite(list(logs.values())).all(), logs
    return out, eng


def _assert_equal(a, b, what):
    for k, ((la, sa), (lb, sb)) in enumerate(zip(a, b)):
        assert set(la) == set(lb) and set(sa) == set(sb)
        for n in la:
            assert la[n] == lb[n], (what, f"step {k}", n, la[n], lb[n])
        for n in sa:
            assert torch.equal(sa[n], sb[n]), (what, f"step {k}", n, float((sa[n] - sb[n]).abs().max()))


# (id, case, extra hyper-parameters, chunk plan, pipelined?)
EXACT_CASES = [(f"{i}_{'pipelined' if pipe else 'serial'}", n, hp, None, pipe)
               for i, n, hp in (("small", "small", None), ("tiny_discount", "tiny_discount", None),
                                ("small_mixing0.5", "small", dict(gradient_mixing=0.5)),
                                ("discrete_cat_tiny_a18", "discrete_cat_tiny_a18", None),
                                ("discrete_tiny_a18", "discrete_tiny_a18", None), ("tiny_pixel", "tiny_pixel", None),
                                ("cat_tiny", "cat_tiny", None))
               for pipe in (False, True)] + [("small_plan221_pipelined", "small", None, (2, 2, 1), True)]


@pytest.mark.parametrize("case_id, name, hp_extra, plan, pipeline", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_perf_step_is_the_explicit_noise_step_bit_for_bit(case_id, name, hp_extra, plan, pipeline):
    s = 20240 + [c[0] for c in EXACT_CASES].index(case_id)
    perf, eng = _run(name, pipeline, plan, hp_extra, s, explicit=False)
    if plan is not None:
        assert eng._bh_plan_used == plan
    fed, _ = _run(name, pipeline, plan, hp_extra, s, explicit=True, obs_prior_seed=100)
    _assert_equal(perf, fed, f"{name}: perf mode against the scheme's explicit noise")
    fed2, _ = _run(name, pipeline, plan, hp_extra, s, explicit=True, obs_prior_seed=200)
    _assert_equal(fed, fed2, f"{name}: two different obs_prior arrays")
    if pipeline:
        flight, _ = _run(name, pipeline, plan, hp_extra, s, explicit=False, in_flight=True)
        _assert_equal(perf[-1:], flight, f"{name}: both steps in flight against one step at a time")
    # another seed gives another step: the comparison above is not vacuous
    other, _ = _run(name, pipeline, plan, hp_extra, s + 1, explicit=False, steps=1)
    assert other[0][0] != perf[0][0]
