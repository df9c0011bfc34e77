"""float64 numpy restatement of one acting decision (Planet.update_belief_and_act, src/planet.py:370-403, with
Dreamer.get_action, src/dreamer.py:429-444) from the weight dicts of ``synth.make_params``: what bd_act_step computes.

Steps: encoder chain (or a ready embedding) -> embed layer + GRU cell -> posterior head on [h'; embedding] and its sample ->
actor chain on [h'; s'] and the tanh-Normal sample -> exploration noise and clamp.  The prior head, get_action's prior
sample and the entropy estimate are not evaluated: none of them feeds the belief, the state or the action
(tests/test_act_ref_cpu.py pins that against the reference's recorded outputs)."""
import numpy as np

ACT_INIT_STD, ACT_MIN_STD, ACT_MEAN_SCALE = 5.0, 1e-4, 5.0     # ActorModel defaults (src/models.py:466-480)
MIN_STD_DEV = 0.1                                              # TransitionModel min_std_dev (src/models.py:131)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def _softplus(x):
    return np.logaddexp(0.0, x)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def dense(sd, x, n_hidden=4):
    """DenseModel / build_mlp: n_hidden x (Linear + ELU), then Linear (``model.{0,2,..}``, src/utils.py:368-404)."""
    for l in range(n_hidden):
        x = _elu(x @ _f64(sd[f"model.{2 * l}.weight"]).T + _f64(sd[f"model.{2 * l}.bias"]))
    return x @ _f64(sd[f"model.{2 * n_hidden}.weight"]).T + _f64(sd[f"model.{2 * n_hidden}.bias"])


def act_step(P, belief, state, action, eps_post, eps_action, obs=None, embedding=None, explore=False, eps_explore=None,
             action_noise=0.3):
    """(belief (B,Be), state (B,S), previous action (B,A), obs (B,O) | embedding (B,E)) -> (belief', state', action')."""
    tm = {k: _f64(v) for k, v in P["transition_model"].items()}
    h, s, a = _f64(belief), _f64(state), _f64(action)
    Be = h.shape[1]
    S = s.shape[1]
    # 1: embedding
    e = dense(P["encoder"], _f64(obs)) if embedding is None else _f64(embedding)
    # 2: x = ELU(W_e [s; a] + b), h' = GRUCell(x, h)   (src/models.py:251-252; gate order r, z, n)
    x = _elu(np.concatenate([s, a], 1) @ tm["fc_embed_state_action.0.weight"].T + tm["fc_embed_state_action.0.bias"])
    gi = x @ tm["rnn.weight_ih"].T + tm["rnn.bias_ih"]
    gh = h @ tm["rnn.weight_hh"].T + tm["rnn.bias_hh"]
    r = _sigmoid(gi[:, :Be] + gh[:, :Be])
    z = _sigmoid(gi[:, Be:2 * Be] + gh[:, Be:2 * Be])
    n = np.tanh(gi[:, 2 * Be:] + r * gh[:, 2 * Be:])
    h2 = (1.0 - z) * n + z * h
    # 3: posterior on [h'; e]   (src/models.py:266-267, :70-73)
    q = _elu(np.concatenate([h2, e], 1) @ tm["belief_posterior.model.0.weight"].T + tm["belief_posterior.model.0.bias"])
    out = q @ tm["belief_posterior.model.2.weight"].T + tm["belief_posterior.model.2.bias"]
    s2 = out[:, :S] + (_softplus(out[:, S:]) + MIN_STD_DEV) * _f64(eps_post)
    # 4: actor on [h'; s'], tanh-Normal sample   (src/models.py:506-517, src/dreamer.py:443)
    ao = dense(P["actor"], np.concatenate([h2, s2], 1))
    A = ao.shape[1] // 2
    mean = ACT_MEAN_SCALE * np.tanh(ao[:, :A] / ACT_MEAN_SCALE)
    std = _softplus(ao[:, A:] + np.log(np.expm1(ACT_INIT_STD))) + ACT_MIN_STD
    act = np.tanh(mean + std * _f64(eps_action))
    # 5: exploration   (src/planet.py:388-392)
    if explore:
        act = np.clip(act + action_noise * _f64(eps_explore), -1.0, 1.0)
    return h2, s2, act
