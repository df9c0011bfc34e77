#!/usr/bin/env python3
"""Generate the discrete-action golden vectors (``tests/golden/discrete_*.npz``) by running the *reference itself*
(read-only, outside this repository; see ``oracle.gen_golden``) with ``action_distribution="Categorical"``.
TEST INFRASTRUCTURE: runs only where the reference exists, never on the GPU machine.

The reference's Categorical actor is unfinished, so it runs under two shims, applied AROUND its code:
  1. ``ActorModel.get_action_dist`` is not defined (src/models.py:518 calls it): the shim returns
     ``OneHotCategoricalStraightThrough(logits=out)``, the distribution the surrounding lines expect
     (``action_dist.sample()``, ``action_dist.probs``).  ``ActorModel.forward`` then runs unchanged: sample, then
     ``action + probs - probs.detach()`` (src/models.py:519-521).
  2. ``Dreamer.get_action`` (src/dreamer.py:429-444) assumes a tanh-Normal actor: the shim is
     ``action, dist = self.actor(belief, state); return action, dist.entropy()`` (the exact Categorical entropy).
Sampling goes through ``oracle.gen_golden.CategoricalShims``: its ``torch.multinomial`` replacement takes the Exp(1)
variates from the injected NoiseStream (after checking on the live call that ``argmax(probs / q)`` is the library's
draw).  It is needed for Gaussian latents too, where the actor is the only Categorical sampler; its two latent repairs
are inert there (``stack`` of a list without tuples is the original; the Gaussian posterior parameters are already a
tuple).  Noise order per train step: the observe draws, then per imagined step the action's Exp(1) draws (N, A) and the
prior draws -- no entropy draws (``synth.make_noise`` with ``discrete_actions``; asserted below).

    python tools/gen_discrete_golden.py            # writes every case of DISCRETE_RUNS
"""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from big_dreamer_amd import synth  # noqa: E402
from oracle import gen_golden as G  # noqa: E402


def _disc(d, A):
    return dataclasses.replace(d, A=A, discrete_actions=True)


# name -> (Dims, seed, top-level overrides, ActorCritic overrides); mirrored by tests/test_discrete_actions_*.py.
# entropy_weight = 0.1 makes the entropy term of the actor gradient visible at the tolerances of the comparisons.
DISCRETE_RUNS = {
    "discrete_tiny_a3": (_disc(synth.TINY, 3), 61, {}, {}),
    "discrete_tiny_a18": (_disc(synth.TINY, 18), 62, {}, dict(entropy_weight=0.1)),
    "discrete_cat_tiny_a3": (_disc(synth.CAT_TINY, 3), 63, dict(free_nats=0.0), {}),
    "discrete_cat_tiny_a18": (_disc(synth.CAT_TINY, 18), 64, dict(free_nats=0.0), dict(entropy_weight=0.1)),
    "discrete_tiny_discount_a3": (_disc(synth.TINY_DISCOUNT, 3), 65, {}, dict(entropy_weight=0.1)),
}


class DiscreteActorShims:
    """The two repairs of the module docstring."""

    def __enter__(self):
        import dreamer as ref_dreamer
        import models as ref_models
        self._had = hasattr(ref_models.ActorModel, "get_action_dist")
        self._gad = getattr(ref_models.ActorModel, "get_action_dist", None)
        self._ga = ref_dreamer.Dreamer.get_action
        ref_models.ActorModel.get_action_dist = \
            lambda self_, out: torch.distributions.OneHotCategoricalStraightThrough(logits=out)

        def get_action(self_, belief, state, deterministic=False):
            action, dist = self_.actor(belief, state)
            return action, dist.entropy()

        ref_dreamer.Dreamer.get_action = get_action
        return self

    def __exit__(self, *a):
        import dreamer as ref_dreamer
        import models as ref_models
        ref_dreamer.Dreamer.get_action = self._ga
        if self._had:
            ref_models.ActorModel.get_action_dist = self._gad
        else:
            del ref_models.ActorModel.get_action_dist


def expected_calls(d, seed):
    ns = synth.NoiseStream(seed)
    state = (lambda r: ns.exponential((r * d.cat_D, d.cat_C))) if d.categorical else (lambda r: ns.normal((r, d.S)))
    for _ in range(d.T):
        state(d.B); state(d.B)
    for _ in range(d.Hm):
        ns.exponential((d.N, d.A)); state(d.N)
    return ns.calls


def run(dreamer_mod, name, d, seed, over, ac_over):
    out = {}
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    tb = {k: torch.from_numpy(v) for k, v in batch.items()}
    ac = dict(G.ref_params(d)["ActorCritic"], **ac_over)
    agent = G.build_agent(dreamer_mod, d, P, action_distribution="Categorical", ActorCritic=ac, **over)
    assert agent.actor.action_distribution == "Categorical" and agent.gradient_mixing == -1
    assert agent.actor.model[-2].out_features == d.A
    agent.buffer.sample = lambda n, L: [tb["observations"], tb["actions"], tb["rewards"], tb["nonterminals"]]
    norms = []
    orig_clip = torch.nn.utils.clip_grad_norm_

    def rec_clip(params, max_norm, norm_type=2):
        r = orig_clip(params, max_norm, norm_type=norm_type)
        norms.append(float(r))
        return r

    torch.nn.utils.clip_grad_norm_ = rec_clip
    mods = ("transition_model", "observation_model", "reward_model", "encoder", "actor", "critic", "critic_target") + \
        (("discount_model",) if d.use_discount else ())
    try:
        for step in range(2):
            ns = synth.NoiseStream(seed + step)
            with G.Inject(ns), G.CategoricalShims(ns) as shims, DiscreteActorShims():
                logs = agent.train_step()
            assert shims.checked == 3
            assert ns.calls == expected_calls(d, seed + step), "reference RNG call order differs from synth.make_noise"
            if step == 0:
                agent.update_critic()
            for k, v in logs.items():
                out[f"step{step}.log.{k}"] = np.array(float(torch.as_tensor(v).detach()), dtype=np.float64)
            out[f"step{step}.grad_norms"] = np.array(norms[-3:], dtype=np.float64)
            for mod in mods:
                for k, p in getattr(agent, mod).state_dict().items():
                    out[f"step{step}.param.{mod}.{k}"] = G.t2n(p)
                if mod == "critic_target":
                    continue
                for k, p in getattr(agent, mod).named_parameters():
                    out[f"step{step}.grad.{mod}.{k}"] = G.t2n(p.grad)      # after clipping
    finally:
        torch.nn.utils.clip_grad_norm_ = orig_clip
    out["fingerprint.params"] = np.array(sum(float(np.abs(v.astype(np.float64)).sum()) for sd in P.values()
                                             for v in sd.values()))
    out["fingerprint.batch"] = np.array(sum(float(np.abs(v.astype(np.float64)).sum()) for v in batch.values()))
    nz = synth.make_noise(d, seed)
    out["fingerprint.noise"] = np.array(sum(float(np.abs(v.astype(np.float64)).sum()) for v in nz.values()))
    path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


def main():
    torch.set_num_threads(1)            # the reference's CPU reductions in one fixed order: regenerates bit-identically
    dreamer_mod, _ = G._import_reference()
    for name, (d, seed, over, ac_over) in DISCRETE_RUNS.items():
        run(dreamer_mod, name, d, seed, over, ac_over)


if __name__ == "__main__":
    main()
