"""float64 numpy restatement of one acting decision (Planet.update_belief_and_act, src/planet.py:370-403, with
Dreamer.get_action, src/dreamer.py:429-444) for the three configurations of bd_act_step_cat (csrc/act.hip):
Categorical latents with the tanh-Normal actor, Categorical latents with the Categorical actor, Gaussian latents with the
Categorical actor.  The shared parts (dense chains, the cell, the tanh-Normal tail) are tests/act_ref.py's; the samplers
are tests/scan_cat_ref.py's (`ratios64`, `first_max`, `one_hot_rows`).

    Categorical latents:  logits = posterior head on [h'; e];  per factor k = argmax(softmax(logits) / q), q ~ Exp(1), the
                          first maximum winning;  s' = one_hot(k)                      (src/models.py:101-117)
    Categorical actor:    out = actor([h'; s']);  p = softmax(out);  k = argmax(p / q);  a' = (one_hot(k) + p) - p
                          (src/models.py:518-522);  explore: with (u, v) uniform on [0, 1), u < action_noise replaces a'
                          by the exact one-hot of class min(floor(v A), A - 1), comparison and product in float32 as the
                          kernel and the composed path (torch.where on float32 tensors) make them

The prior head, get_action's prior sample and the actor's entropy are not evaluated: none feeds belief, state or action.

Every decision also returns what the GPU tests' precondition is stated on: the logits and draws of every sampler call and
the smallest relative gap between the best and the runner-up ratio (`min_gap`).  tests/test_act_cat_ref_cpu.py asserts for
every case of CASES that no (row, factor) and no action row is ambiguous (scan_cat_ref.sample_check) and that every gap is
above MIN_GAP, so the GPU tests may demand exact one-hots with nothing left out."""
import dataclasses

import numpy as np
import torch

from big_dreamer_amd import synth
from tests import act_ref
from tests import scan_cat_ref as CR
from tests.act_ref import _elu, _f64, _sigmoid, _softplus

ACTION_NOISE = 0.3      # conf/config.yaml

# Relative gap between the best and the runner-up probs / q that every sampler call of every case must show (float64).
# A gap g is a difference of two logits of g: the kernels' logits are Hd = 20-term fp32 sums of products below 1 on
# activations held to 2e-5, i.e. off by less than 5e-5 each way; 1e-4 covers both, as tests/planner_cat_oracle.MIN_GAP.
# That derivation is for the widths of CASES (Hd = 20) only.  At other widths the gap a row must show is derived from the
# row's own float64 operands: tests/act_shapes.py `logit_bound` / `required_gap` = max(MIN_GAP, 2 * bound), computed,
# printed and asserted per row by tests/test_act_shapes_cpu.py::test_no_sample_is_left_to_rounding.
MIN_GAP = 1e-4
ROWS = 33               # rows of data per case: B in {1, 16, 17, 33} takes the first B


def _dims(D=0, C=0, A=2, disc=False, S=6):
    """Be = 24, Hd = 20, E = 40, O = 5: no width is a multiple of 16 (synth.TINY / CAT_TINY)."""
    base = synth.CAT_TINY if D else synth.TINY
    return dataclasses.replace(base, S=D * C if D else S, cat_D=D, cat_C=C, A=A, discrete_actions=disc)


# name -> (dims, data seed).  A seed must meet the margin condition in both forms, explore off and on
# (tests/test_act_cat_ref_cpu.py asserts it); seed 0 does for every case.
CASES = {
    "cat3x5_tanh": (_dims(3, 5), 0),
    "cat3x5_disc2": (_dims(3, 5, 2, True), 0),
    "cat3x5_disc18": (_dims(3, 5, 18, True), 0),
    "cat32_tanh": (_dims(32, 32), 0),
    "cat32_disc2": (_dims(32, 32, 2, True), 0),
    "cat32_disc18": (_dims(32, 32, 18, True), 0),
    "gauss_disc2": (_dims(A=2, disc=True), 0),
    "gauss_disc18": (_dims(A=18, disc=True), 0),
}
PARAM_SEED = 11


def make_data(d, seed, n=ROWS, calls=3):
    """Inputs and noise of `calls` chained decisions for n environments (float32, as the kernels get them).  Categorical
    state: one class per factor, environment 0 all-zero (the collect loop's initial state, src/main.py:91-95)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    if d.categorical:
        state = np.eye(d.cat_C)[rng.integers(0, d.cat_C, (n, d.cat_D))].reshape(n, d.S)
        state[0] = 0.0
        post = rng.exponential(size=(calls, n, d.S))
    else:
        state = rng.standard_normal((n, d.S))
        post = rng.standard_normal((calls, n, d.S))
    if d.discrete_actions:
        action = np.eye(d.A)[rng.integers(0, d.A, n)]
        act = rng.exponential(size=(calls, n, d.A))
        exp = rng.random((calls, n, 2))                    # (u, v)
    else:
        action = rng.uniform(-1, 1, (n, d.A))
        act = rng.standard_normal((calls, n, d.A))
        exp = rng.standard_normal((calls, n, d.A))
    data = {"belief": rng.standard_normal((n, d.Be)), "state": state, "action": action,
            "obs": rng.standard_normal((calls, n, d.O)), "emb": rng.standard_normal((calls, n, d.E)),
            "post": post, "act": act, "exp": exp}
    data = {k: v.astype(np.float32) for k, v in data.items()}
    for k in ("post", "act"):       # Exp(1) draws stay in the normal range (scan_cat_ref.exp1)
        if (k == "post" and d.categorical) or (k == "act" and d.discrete_actions):
            data[k] = np.maximum(data[k], np.float32(1e-6))
    return data


def _sample(logits, q, D, C):
    """(classes [rows x D], smallest relative gap best / runner-up) of argmax(softmax(logits) / q), first maximum winning."""
    lt, qt = torch.from_numpy(np.ascontiguousarray(logits)), torch.from_numpy(np.ascontiguousarray(_f64(q)))
    idx = CR.first_max(lt, qt, D, C)
    gap = 1.0
    if C > 1:
        top = CR.ratios64(lt, qt, D, C)[0].topk(2, -1).values
        gap = float(((top[..., 0] - top[..., 1]) / top[..., 0]).min())
    return idx, gap


def act_step_cat(P, d, belief, state, action, eps_post, eps_action, obs=None, embedding=None, explore=False,
                 eps_explore=None, action_noise=ACTION_NOISE):
    """(belief (B,Be), state (B,S), previous action (B,A), obs (B,O) | embedding (B,E)) -> (belief', state', action', info).
    info: post_logits / post_q and actor_out / actor_q of the Categorical samplers that ran, min_gap over them, and
    `explored` (the rows epsilon-greedy replaced); post_hidden and actor_in, the posterior's hidden layer and the actor's
    input [h'; s'].  Every array is cast by `_f64` on the way in, so tests/act_shapes.float32_restatement can evaluate
    the same statements in float32."""
    tm = {k: _f64(v) for k, v in P["transition_model"].items()}
    h, s, a = _f64(belief), _f64(state), _f64(action)
    Be = h.shape[1]
    info = {"min_gap": 1.0}
    e = act_ref.dense(P["encoder"], _f64(obs)) if embedding is None else _f64(embedding)
    x = _elu(np.concatenate([s, a], 1) @ tm["fc_embed_state_action.0.weight"].T + tm["fc_embed_state_action.0.bias"])
    gi = x @ tm["rnn.weight_ih"].T + tm["rnn.bias_ih"]
    gh = h @ tm["rnn.weight_hh"].T + tm["rnn.bias_hh"]
    r = _sigmoid(gi[:, :Be] + gh[:, :Be])
    z = _sigmoid(gi[:, Be:2 * Be] + gh[:, Be:2 * Be])
    n = np.tanh(gi[:, 2 * Be:] + r * gh[:, 2 * Be:])
    h2 = (1.0 - z) * n + z * h
    q = _elu(np.concatenate([h2, e], 1) @ tm["belief_posterior.model.0.weight"].T + tm["belief_posterior.model.0.bias"])
    out = q @ tm["belief_posterior.model.2.weight"].T + tm["belief_posterior.model.2.bias"]
    if d.categorical:
        idx, gap = _sample(out, eps_post, d.cat_D, d.cat_C)
        s2 = _f64(CR.one_hot_rows(idx, d.cat_C).numpy())
        info.update(post_logits=out, post_q=np.asarray(eps_post), post_idx=idx.numpy(), min_gap=min(info["min_gap"], gap))
    else:
        s2 = out[:, :d.S] + (_softplus(out[:, d.S:]) + act_ref.MIN_STD_DEV) * _f64(eps_post)
    info.update(post_hidden=q, actor_in=np.concatenate([h2, s2], 1))      # operands of the two logit layers (logit_bound)
    ao = act_ref.dense(P["actor"], info["actor_in"])
    if d.discrete_actions:
        k, gap = _sample(ao, eps_action, 1, d.A)
        k = k.numpy()[:, 0]
        p = np.exp(ao - ao.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        act = (_f64(np.eye(d.A))[k] + p) - p
        info.update(actor_out=ao, actor_q=np.asarray(eps_action), actor_idx=k, min_gap=min(info["min_gap"], gap))
        if explore:
            u, v = np.float32(eps_explore[:, 0]), np.float32(eps_explore[:, 1])
            kr = np.minimum(np.floor(v * np.float32(d.A)).astype(np.int64), d.A - 1)
            hit = u < np.float32(action_noise)
            act = np.where(hit[:, None], _f64(np.eye(d.A))[kr], act)
            info["explored"] = hit
    else:
        A = d.A
        mean = act_ref.ACT_MEAN_SCALE * np.tanh(ao[:, :A] / act_ref.ACT_MEAN_SCALE)
        std = _softplus(ao[:, A:] + float(np.log(np.expm1(act_ref.ACT_INIT_STD)))) + act_ref.ACT_MIN_STD
        act = np.tanh(mean + std * _f64(eps_action))
        if explore:
            act = np.clip(act + action_noise * _f64(eps_explore), -1.0, 1.0)
    return h2, s2, act, info


def chain(P, d, data, B, explore, form="obs", calls=3):
    """`calls` chained decisions on the first B rows, outputs fed back as inputs: [(belief, state, action, info)]."""
    b, s, a = data["belief"][:B], data["state"][:B], data["action"][:B]
    outs = []
    for i in range(calls):
        kw = {"obs": data["obs"][i, :B]} if form == "obs" else {"embedding": data["emb"][i, :B]}
        b, s, a, info = act_step_cat(P, d, b, s, a, data["post"][i, :B], data["act"][i, :B], explore=explore,
                                     eps_explore=data["exp"][i, :B], **kw)
        outs.append((b, s, a, info))
    return outs
