"""CPU: the float64 restatement of the fused Categorical acting step (tests/act_cat_ref.py) against the composed CPU oracle
(oracle/dreamer_oracle.py's pieces, as tests/discrete_oracle.py and tests/planner_cat_oracle.py compose them), the margin
condition on the inputs of the GPU tests (tests/test_act_step_cat_gpu.py), and the known answer of the uniform draws."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from big_dreamer_amd import synth
from oracle import dreamer_oracle as O
from tests import act_cat_ref as R
from tests import scan_cat_ref as CR
from tests.discrete_oracle import discrete_head
from tests.helpers import assert_close
from tests.test_rng_cpu import KAT


def _oracle_step(P, d, belief, state, action, eps_post, eps_action, obs, explore, eps_explore):
    """One decision in float32 from the oracle's own functions: encoder, one step of TransitionModel.forward with an
    embedding, the actor on [h'; s'] and its sample, exploration as Dreamer.update_belief_and_act applies it."""
    t = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float32))
    tm = {k: t(v) for k, v in P["transition_model"].items()}
    belief, state, action = t(belief), t(state), t(action)
    B = belief.shape[0]
    emb = O.mlp(t(obs), {k: t(v) for k, v in P["encoder"].items()}).unsqueeze(0)
    ones = torch.ones(1, B, d.S)
    cat = (d.cat_D, d.cat_C) if d.categorical else None
    beliefs, _, _, posts, _ = O.transition_forward(tm, state, action.unsqueeze(0), belief, emb, None, ones,
                                                   t(eps_post).unsqueeze(0), cat)
    h2, s2 = beliefs[0], posts[0]
    actor = {k: t(v) for k, v in P["actor"].items()}
    if d.discrete_actions:
        act, _, _, _ = discrete_head(O.mlp(torch.cat([h2, s2], 1), actor), t(eps_action))
        if explore:     # big_dreamer_amd/dreamer.py update_belief_and_act: "explore_u" / "explore_k"
            u, v = t(eps_explore[:, 0]), t(eps_explore[:, 1])
            k = torch.clamp(torch.floor(v * d.A).long(), max=d.A - 1)
            act = torch.where((u < R.ACTION_NOISE).unsqueeze(1), F.one_hot(k, d.A).to(act.dtype), act)
    else:
        mean, std = O.actor_forward(h2, s2, actor)
        act = torch.tanh(mean + std * t(eps_action))
        if explore:
            act = torch.clamp(act + R.ACTION_NOISE * t(eps_explore), -1, 1)
    return h2.numpy(), s2.numpy(), act.numpy()


@pytest.fixture(scope="module")
def chains():
    """Every case's float64 chains, computed once: {(case, form, explore): chain}."""
    out = {}
    for name, (d, seed) in R.CASES.items():
        P, data = synth.make_params(d, R.PARAM_SEED), R.make_data(d, seed)
        for form, B in (("obs", R.ROWS), ("emb", 17)):
            for explore in (False, True):
                out[name, form, explore] = R.chain(P, d, data, B, explore, form)
    return out


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_matches_the_composed_oracle(chains, case, explore):
    """Three chained decisions: one-hot states and sampled / explored actions identical, the rest to float32 rounding."""
    d, seed = R.CASES[case]
    P, data = synth.make_params(d, R.PARAM_SEED), R.make_data(d, seed)
    b, s, a = data["belief"], data["state"], data["action"]
    for i, (wb, ws, wa, info) in enumerate(chains[case, "obs", explore]):
        b, s, a = _oracle_step(P, d, b, s, a, data["post"][i], data["act"][i], data["obs"][i], explore, data["exp"][i])
        assert_close(f"{case} belief{i}", b, wb, 2e-5, 2e-5)
        if d.categorical:
            assert np.array_equal(s, ws), f"{case} state{i}: one-hot states differ"
        else:
            assert_close(f"{case} state{i}", s, ws, 2e-5, 2e-5)
        if d.discrete_actions:
            assert np.array_equal(a.argmax(1), wa.argmax(1)), f"{case} action{i}: classes differ"
            assert float(np.abs(a - wa).max()) <= 1e-6
            if explore:     # explored rows are exact one-hots, and some rows explore while others do not
                hit = info["explored"]
                assert 0 < int(hit.sum()) < len(hit)
                assert np.array_equal(a[hit], wa[hit]) and set(np.unique(wa[hit])) <= {0.0, 1.0}
        else:
            assert_close(f"{case} action{i}", a, wa, 2e-5, 2e-5)


@pytest.mark.parametrize("case", list(R.CASES))
def test_inputs_leave_no_sample_to_rounding(chains, case):
    """The condition the GPU tests rest on: in every call of every chain of the case, no (row, factor) and no action row is
    ambiguous under the kernels' sampling margin (scan_cat_ref.sample_check), and the best ratio leads the runner-up by
    more than MIN_GAP, which also covers the fp32 error of the logits themselves."""
    d, _ = R.CASES[case]
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    for form in ("obs", "emb"):
        for explore in (False, True):
            for i, (_, _, _, info) in enumerate(chains[case, form, explore]):
                tag = f"{case} {form} explore={explore} call {i}: "
                if d.categorical:
                    amb, n, _ = CR.sample_check(tt(info["post_logits"]), tt(info["post_q"]), tt(info["post_idx"]), d.cat_D, d.cat_C,
                                                CR.sample_path(d.cat_C), tag)
                    assert amb == 0 and n == info["post_idx"].size, f"{tag}{amb} ambiguous (row, factor) pairs"
                if d.discrete_actions:
                    amb, n, _ = CR.sample_check(tt(info["actor_out"]), tt(info["actor_q"]), tt(info["actor_idx"]), 1, d.A, "libm", tag)
                    assert amb == 0 and n == len(info["actor_idx"]), f"{tag}{amb} ambiguous action rows"
                assert info["min_gap"] > R.MIN_GAP, f"{tag}smallest relative gap {info['min_gap']:.3e}"


def test_uniform_draws_known_answer():
    """rng_uniform4 / BD_RNG_UNIFORM: u = (word >> 8) * 2^-24 of the host twin's words, in [0, 1), exact in float32."""
    from big_dreamer_amd import _cabi as cabi
    assert cabi.BD_RNG_UNIFORM == 2 and (cabi.BD_RNG_NORMAL, cabi.BD_RNG_EXPONENTIAL) == (0, 1)
    words = philox_words(seed=0x0123456789ABCDEF, step=7, stream=10, groups=64)
    u = uniform_from_words(words)
    assert u.dtype == np.float32 and float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert np.array_equal((u.astype(np.float64) * 2.0 ** 24).astype(np.uint64), (words >> 8).astype(np.uint64))
    assert 0.4 < float(u.mean()) < 0.6
    # the published vectors (tests/test_rng_cpu.KAT) as uniforms: the all-zero counter's first word 0x6627e8d5 -> 0x6627e8 / 2^24
    ctr, key, want = KAT[0]
    out = (C.c_uint * 4)()
    assert cabi.lib.bd_philox4x32_10((C.c_uint * 4)(*ctr), (C.c_uint * 2)(*key), out) == 0 and list(out) == want
    assert float(uniform_from_words(np.array(list(out), dtype=np.uint32))[0]) == 0x6627e8 / 2.0 ** 24


def philox_words(seed, step, stream, groups):
    """The host twin's words of the first `groups` groups of four of (seed, step, stream): [groups * 4] uint32."""
    from big_dreamer_amd import _cabi as cabi
    key = (C.c_uint * 2)(seed & 0xFFFFFFFF, seed >> 32)
    out = (C.c_uint * 4)()
    words = np.zeros(groups * 4, dtype=np.uint32)
    for i in range(groups):
        ctr = (C.c_uint * 4)(i & 0xFFFFFFFF, i >> 32, stream, step & 0xFFFFFFFF)
        assert cabi.lib.bd_philox4x32_10(ctr, key, out) == 0
        words[4 * i:4 * i + 4] = list(out)
    return words


def uniform_from_words(words):
    return ((words >> 8).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
