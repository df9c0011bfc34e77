"""GPU: the in-step training diagnostics of the engine (DreamerEngine.set_diagnostics, big_dreamer_amd/diagnostics.py).

- One diagnosed train step per configuration family against the CPU oracle: every scalar and list of the log dict is
  recomputed in float64 from what the oracle kept.  Tolerances are those the existing engine-vs-oracle tests apply to the
  TENSOR a statistic is formed from (cited at TOL below), carried to the statistic by first-order propagation:
  a mean moves by at most the mean of the elementwise tolerance, a min / max / population std by at most its maximum
  (|std(x + e) - std(x)| <= rms(e)), a sum of f(x) by at most sum |f'(x)| tol(x).
- Per-module gradient norms against the optimiser's own norm in the same dict, non-interference with the step, the
  cadence, independence of the schedule (pipeline, lazy logs, chunked heads) and the CLI.
"""
import dataclasses
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from big_dreamer_amd import diagnostics as dg
from big_dreamer_amd import synth
from tests import diag_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (atol, rtol) of the existing comparisons of each tensor with the oracle
TOL = {
    "latent": (2e-5, 2e-5),         # posterior / prior means and stds: tests/test_hip_parity.py:77-80; logits:
                                    # tests/test_categorical_scan_gpu.py:85-86
    "reward_pred": (5e-5, 5e-5),    # a dense head on the features, as imged_reward: tests/test_hip_parity.py:89
    "imged_reward": (5e-5, 5e-5),   # tests/test_hip_parity.py:89
    "value_pred": (5e-5, 5e-5),     # tests/test_hip_parity.py:90
    "returns": (2e-4, 5e-5),        # tests/test_hip_parity.py:91
    "critic_value": (5e-5, 5e-5),   # the critic on the imagined features, as value_pred: tests/test_hip_parity.py:90
    "action": (5e-5, 5e-5),         # the action is what the imagined features are computed from: tests/test_hip_parity.py:83-84
}
GRAD_TOL = (2e-3, 1e-9, 2e-3)       # 2e-3 * max|g| + 1e-9 absolute, 2e-3 relative: tests/test_hip_parity.py:154-156
BASE_KEYS = {"observation_loss", "reward_loss", "kl_loss", "model_loss", "actor_loss", "policy_entropy", "value_loss",
             "grad_norm_model", "grad_norm_actor", "grad_norm_critic"}


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _np(t):
    return t.detach().double().numpy()


def _tol(x, key):
    a, r = TOL[key]
    return a + r * np.abs(x)


class Checker:
    def __init__(self, logs):
        self.logs, self.seen, self.lines = logs, set(), []

    def close(self, key, want, tol):
        got = np.asarray(self.logs[key], dtype=np.float64)
        want = np.asarray(want, dtype=np.float64)
        err = np.abs(got - want)
        self.lines.append(f"DIAG {key:28s} got={got.ravel()[:3]} want={want.ravel()[:3]} err={err.max():.3e} tol={np.max(tol):.3e}")
        assert got.shape == want.shape and (err <= tol).all(), self.lines[-1]
        self.seen.add(key)

    def stats(self, prefix, x, key, which):
        s, t = R.stats_ref(x), _tol(x, key)
        for w in which:
            self.close(f"{prefix}_{w}", s[w], t.mean() if w == "mean" else t.max())

    def between(self, key, lo, hi):
        assert lo <= self.logs[key] <= hi, (key, self.logs[key], lo, hi)
        self.seen.add(key)


def _gauss_dynamics(c, inter, N):
    qm, qs, pm, ps = (_np(inter[k]).reshape(N, -1) for k in ("posterior_means", "posterior_stds", "prior_means", "prior_stds"))
    out, col, _, _ = R.latent_stats_ref(qm, qs, pm, ps)
    tq, ts, tp, tr = (_tol(a, "latent") for a in (qm, qs, pm, ps))
    diff = np.abs(qm - pm)
    klt = diff / ps ** 2 * (tq + tp) + np.abs(qs / ps ** 2 - 1 / qs) * ts + np.abs(1 / ps - (qs ** 2 + diff ** 2) / ps ** 3) * tr
    c.close("kl_raw", out[2] / N, klt.sum() / N)
    c.close("kl_per_dim", col / N, klt.sum(0) / N)
    c.between("kl_active_dims", int(((col - klt.sum(0)) / N > dg.ACTIVE_NATS).sum()), int(((col + klt.sum(0)) / N > dg.ACTIVE_NATS).sum()))
    c.close("post_entropy", out[0] / N, (ts / qs).sum() / N)
    c.close("prior_entropy", out[1] / N, (tr / ps).sum() / N)
    c.stats("post_std", qs, "latent", ("mean", "min"))
    c.stats("prior_std", ps, "latent", ("mean", "min"))


def _cat_dynamics(c, inter, N, D, Cn):
    xq, xp = (_np(inter[k]).reshape(N, D, Cn) for k in ("posterior_logits", "prior_logits"))
    out, col, used, _, _ = R.latent_stats_cat_ref(xq, xp)
    lq, lp = R.log_softmax(xq)[0], R.log_softmax(xp)[0]
    q, p = np.exp(lq), np.exp(lp)
    tq, tp = _tol(xq, "latent"), _tol(xp, "latent")
    kl, hq, hp = R.cat_kl(lq, lp), R.cat_entropy(lq), R.cat_entropy(lp)
    # d KL / d xq_c = q_c (lq_c - lp_c - KL), d KL / d xp_c = p_c - q_c, d H / d x_c = -q_c (lq_c + H), d max q / d x_c: |.| <= q_c
    klt = (np.abs(q * (lq - lp - kl[..., None])) * tq + np.abs(p - q) * tp).sum(-1)
    c.close("kl_raw", out[2] / N, klt.sum() / N)
    c.close("kl_per_dim", col / N, klt.sum(0) / N)
    c.between("kl_active_dims", int(((col - klt.sum(0)) / N > dg.ACTIVE_NATS).sum()), int(((col + klt.sum(0)) / N > dg.ACTIVE_NATS).sum()))
    c.close("post_entropy", out[0] / N, (np.abs(q * (lq + hq[..., None])) * tq).sum() / N)
    c.close("prior_entropy", out[1] / N, (np.abs(p * (lp + hp[..., None])) * tp).sum() / N)
    c.close("post_max_prob", out[3] / (N * D), (q * tq).sum() / (N * D) * 2)
    c.close("prior_max_prob", out[4] / (N * D), (p * tp).sum() / (N * D) * 2)
    # a class is certainly used if it is the argmax of a group by more than twice the logits' tolerance, possibly used if
    # it lies within that of the maximum
    gap = xq.max(-1, keepdims=True) - xq
    near = gap <= 2 * tq.max(-1, keepdims=True)
    sure = used.astype(bool) & ~((near.sum(-1) > 1)[..., None] & near).any(0)
    c.between("post_classes_used", sure.sum() / (D * Cn), near.any(0).sum() / (D * Cn))


def _grad_checks(c, od, eng, P, groups):
    for grp, mods, grads in groups:
        i = 0
        for mod in mods:
            sq = tol_sq = wsq = 0.0
            for k in od.P[mod]:
                g = _np(grads[i])
                t = GRAD_TOL[0] * np.abs(g).max() + GRAD_TOL[1] + GRAD_TOL[2] * np.abs(g)
                sq, tol_sq, wsq = sq + (g ** 2).sum(), tol_sq + (t ** 2).sum(), wsq + (P[mod][k].astype(np.float64) ** 2).sum()
                i += 1
            c.close(f"grad_norm/{mod}", math.sqrt(sq), math.sqrt(tol_sq))
            c.close(f"weight_norm/{mod}", math.sqrt(wsq), 1e-12 * math.sqrt(wsq))


def _behaviour_checks(c, od, d, batch_rewards, pre, nz):
    from oracle import dreamer_oracle as O
    last = od.last
    img_b, img_s = last["imged_beliefs"], last["imged_states"]
    with torch.no_grad():
        r = last["imged_reward"] if "imged_reward" in last else O.dense_on_features(img_b, img_s, od.P["reward_model"])
        v = last["value_pred"] if "value_pred" in last else O.dense_on_features(img_b, img_s, od.P["critic_target"])
        cv = last["critic_value"] if "critic_value" in last else O.dense_on_features(img_b, img_s, pre["critic"])
    r, v, cv, ret = _np(r).ravel(), _np(v).ravel(), _np(cv).ravel(), _np(last["returns"]).ravel()
    full = ("mean", "std", "min", "max")
    c.stats("imag_reward", r, "imged_reward", full)
    c.stats("imag_value", v, "value_pred", full)
    c.stats("imag_return", ret, "returns", full)
    c.stats("critic_value", cv, "critic_value", ("mean", "std"))
    # 1 - A / B, A = Var(ret - cv), B = Var(ret): |Var(x + e) - Var(x)| <= 2 std(x) max|e| + max|e|^2
    e_err, e_ret = (_tol(ret, "returns") + _tol(cv, "critic_value")).max(), _tol(ret, "returns").max()
    A, B = (ret - cv).var(), ret.var()
    dA, dB = 2 * math.sqrt(A) * e_err + e_err ** 2, 2 * math.sqrt(B) * e_ret + e_ret ** 2
    c.close("value_explained_variance", R.explained_variance_ref(ret, cv), (dA + A / B * dB) / (B - dB))
    # the imagined actions, from the kept beliefs and states with the actor as it was before its update
    N = img_b.shape[1]
    b_prev = torch.cat([pre["beliefs"].reshape(1, N, -1), img_b[:-1]], 0)
    s_prev = torch.cat([pre["states"].reshape(1, N, -1), img_s[:-1]], 0)
    eps = torch.as_tensor(nz["action"])
    acts = []
    with torch.no_grad():
        for t in range(img_b.shape[0]):
            if d.discrete_actions:
                from tests.discrete_oracle import discrete_head
                out = O.mlp(torch.cat([b_prev[t], s_prev[t]], dim=1), pre["actor"])
                acts.append(torch.nn.functional.one_hot(discrete_head(out, eps[t])[3], d.A).double())
            else:
                acts.append(O.get_action(b_prev[t], s_prev[t], pre["actor"], eps[t], torch.as_tensor(nz["entropy"])[t])[0])
    acts = _np(torch.stack(acts))
    if d.discrete_actions:      # the sampled indices are compared exactly (tests/test_discrete_actions_gpu.py:53)
        c.close("action_freq", acts.reshape(-1, d.A).mean(0), 1e-12)
    else:
        c.stats("action", acts, "action", full + ("rms",))


FAMILIES = {
    "gaussian": (synth.TINY, 0, {}),
    "categorical_latents": (synth.CAT_TINY, 51, dict(free_nats=0.0)),
    "categorical_actor": (dataclasses.replace(synth.TINY, A=6, discrete_actions=True), 0, {}),
    "use_discount": (synth.TINY_DISCOUNT, 9, {}),
    "tiny_pixel": (synth.TINY_PIXEL, 4, {}),
    "planet": (synth.TINY, 8, dict(kl_balance=-1, free_nats=0.05)),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_diagnosed_step_against_the_oracle(family):
    from big_dreamer_amd.engine import DreamerEngine
    from oracle import dreamer_oracle as O
    from tests.discrete_oracle import DiscreteOracleDreamer, oracle_hp
    d, seed, hp = FAMILIES[family]
    P, batch, nz = synth.make_params(d, seed), synth.make_batch(d, seed), synth.make_noise(d, seed)
    ohp = dict(hp, planning_horizon=d.H, **(dict(categorical=(d.cat_D, d.cat_C)) if d.categorical else {}))
    od = (DiscreteOracleDreamer(P, oracle_hp(d, hp)) if d.discrete_actions else O.OracleDreamer(P, ohp))
    eng = DreamerEngine(d, hp, "cuda", params=P, diagnostics_interval=1)
    planet = family == "planet"
    tb, tn = ({k: torch.as_tensor(v) for k, v in x.items()} for x in (batch, nz))
    with torch.no_grad():       # what the dynamics phase sees: the weights before any update
        inter = od.world_model_forward(tb, tn)[4]
    pre = dict(actor={k: v.detach().clone() for k, v in od.P["actor"].items()},
               critic={k: v.detach().clone() for k, v in od.P["critic"].items()},
               beliefs=inter["beliefs"].detach(), states=inter["posterior_states"].detach())
    if planet:
        od.planet_train_step(batch, nz, keep=True)
        logs = eng.world_model_step(_dev(batch), {k: v for k, v in _dev(nz).items() if k.startswith("obs_")})
    else:
        od.train_step(batch, nz, keep=True)
        logs = eng.train_step(_dev(batch), _dev(nz))
    inter = od.last.get("inter", inter)
    N = d.T * d.B
    c = Checker(logs)
    try:
        if d.categorical:
            _cat_dynamics(c, inter, N, d.cat_D, d.cat_C)
        else:
            _gauss_dynamics(c, inter, N)
        rew = batch["rewards"][:-1].astype(np.float64)
        c.close("reward_batch_mean", rew.mean(), 1e-12)
        c.close("reward_batch_std", rew.std(), 1e-12)
        c.stats("reward_pred", _np(inter["reward_pred"]), "reward_pred", ("mean", "std"))
        groups = [("model", od.model_modules, od.last["model_grads"])]
        if not planet:
            _behaviour_checks(c, od, d, rew, pre, nz)
            groups += [("actor", ("actor",), od.last["actor_grads"]), ("critic", ("critic",), od.last["critic_grads"])]
        _grad_checks(c, od, eng, P, groups)
    finally:
        print("\n".join(c.lines))
    extra = {k for k in logs if k not in BASE_KEYS and k != "discount_loss"}
    assert extra == c.seen, (sorted(extra - c.seen), sorted(c.seen - extra))
    assert not [k for k in logs if k.startswith("nonfinite/")]
    want = set(dg.DYNAMICS_KEYS + dg.REWARD_KEYS + (dg.CATEGORICAL_KEYS if d.categorical else dg.GAUSSIAN_KEYS))
    if not planet:
        want |= set(dg.BEHAVIOUR_KEYS + (dg.CATEGORICAL_ACTION_KEYS if d.discrete_actions else dg.TANH_ACTION_KEYS))
    assert want <= extra and all(k in want or k.startswith(("grad_norm/", "weight_norm/")) for k in extra)
    if planet:
        assert not [k for k in logs if k.endswith(("/actor", "/critic"))]


# ---- engine-level properties ------------------------------------------------------------------------------------------------
D = synth.TINY


@pytest.fixture(scope="module")
def case():
    return dict(P=synth.make_params(D, 3), batch=[_dev(synth.make_batch(D, 3 + i)) for i in range(3)],
                noise=[_dev(synth.make_noise(D, 3 + i)) for i in range(3)])


def _engine(case, interval, d=D, **attrs):
    from big_dreamer_amd.engine import DreamerEngine
    eng = DreamerEngine(d, None, "cuda", params=case["P"], diagnostics_interval=interval)
    for k, v in attrs.items():
        setattr(eng, k, v)
    return eng


def _state(eng):
    eng.flush_optimizers()
    eng.join()
    torch.cuda.synchronize()
    return {f"{g}.{b}": getattr(eng.groups[g], b).clone() for g in ("model", "actor", "critic") for b in ("flat", "m", "v")}


def _bits(logs):
    """The diagnostic entries of a log dict as bytes (NaN-safe, bit-exact comparison)."""
    return {k: np.asarray(v, dtype=np.float64).tobytes() for k, v in logs.items() if k not in BASE_KEYS}


def test_norms_of_the_modules_add_up_to_the_optimisers_norm(case):
    eng = _engine(case, 1)
    logs = eng.train_step(case["batch"][0], case["noise"][0])
    for opt, mods in (("model", synth.model_modules(D)), ("actor", ("actor",)), ("critic", ("critic",))):
        total = math.sqrt(sum(logs[f"grad_norm/{m}"] ** 2 for m in mods))
        # the slot is the fp32 rounding of the same fp64 sum of squares; its square root is taken in double
        assert abs(total - logs[f"grad_norm_{opt}"]) <= 2.0 ** -23 * total, (opt, total, logs[f"grad_norm_{opt}"])
        assert total > 0 and all(logs[f"weight_norm/{m}"] > 0 for m in mods)


def test_diagnostics_do_not_touch_the_step_and_follow_the_interval(case):
    off, on, two = _engine(case, 0), _engine(case, 1), _engine(case, 2)
    assert (off.diagnostics_interval, on.diagnostics_interval, two.diagnostics_interval) == (0, 1, 2)
    for i in range(3):
        a, b, c = (e.train_step(case["batch"][i], case["noise"][i]) for e in (off, on, two))
        assert set(a) == BASE_KEYS                                  # interval 0: exactly today's keys
        assert {k: a[k] for k in BASE_KEYS} == {k: b[k] for k in BASE_KEYS} == {k: c[k] for k in BASE_KEYS}
        assert set(b) > BASE_KEYS and "kl_raw" in b
        assert (set(c) > BASE_KEYS) == (i in (0, 2)), i             # interval 2: steps 0 and 2 only
        if i in (0, 2):
            assert _bits(b) == _bits(c)
    assert off._diag is None                                        # nothing was allocated
    sa, sb, sc = _state(off), _state(on), _state(two)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sc[k]), k
    with pytest.raises(ValueError):
        off.set_diagnostics(-1)


def test_set_diagnostics_takes_effect_on_the_next_step(case):
    eng = _engine(case, 0)
    assert "kl_raw" not in eng.train_step(case["batch"][0], case["noise"][0])
    eng.set_diagnostics(1)
    assert "kl_raw" in eng.train_step(case["batch"][1], case["noise"][1])
    eng.set_diagnostics(0)
    assert set(eng.train_step(case["batch"][2], case["noise"][2])) == BASE_KEYS


def _run(case, batches, noises, lazy, d=D, **attrs):
    eng = _engine(case, 1, d, **attrs)
    out = [eng.train_step(b, n, sync_logs="lazy" if lazy else True) for b, n in zip(batches, noises)]
    out = [dict(o.items()) for o in out]
    eng.join()
    torch.cuda.synchronize()
    return [_bits(o) for o in out], [{k: o[k] for k in BASE_KEYS} for o in out]


def test_schedule_does_not_change_the_diagnostic_bits(case):
    ref = _run(case, case["batch"], case["noise"], False, pipeline=True)
    assert all(len(b) > 20 for b in ref[0])
    for pipeline in (True, False):
        for lazy in (False, True):
            got = _run(case, case["batch"], case["noise"], lazy, pipeline=pipeline)
            assert got == ref, (pipeline, lazy)
    got = _run(case, case["batch"], case["noise"], True, pipeline=True, defer_opt=True)      # the held-back optimiser steps
    assert got == ref


def test_chunked_and_fused_heads_give_the_same_diagnostic_bits():
    d, seed = synth.SMALL, 1
    case = dict(P=synth.make_params(d, seed))
    batches = [_dev(synth.make_batch(d, seed + i)) for i in range(2)]
    noises = [_dev(synth.make_noise(d, seed + i)) for i in range(2)]
    ref = _run(case, batches, noises, True, d, bh_chunks=1)
    assert _run(case, batches, noises, True, d, bh_chunks=(2, 2, 1)) == ref


def test_agent_surface():
    from tests.test_planner_gpu import _agent
    agent, _, _ = _agent(D, 8, extra=("diagnostics_interval=3",))
    assert agent.diagnostics_interval == agent.engine.diagnostics_interval == 3
    agent.set_diagnostics(1)
    assert agent.diagnostics_interval == 1
    with pytest.raises(ValueError):
        agent.set_diagnostics(1.5)


def test_cli_prints_the_scalar_diagnostics():
    cmd = [sys.executable, os.path.join(ROOT, "src", "main.py"), "belief_size=32", "hidden_size=32", "embedding_size=64",
           "state_size=8", "batch_size=6", "seq_len=8", "planning_horizon=5", "experience_size=500", "seed_steps=100",
           "max_episode_length=30", "train_steps=140", "log_freq=10", "collect_interval=2", "diagnostics_interval=1"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "kl_raw" in out.stdout and "post_entropy" in out.stdout and "grad_norm/actor" in out.stdout
    assert "kl_per_dim" not in out.stdout                          # list-valued entries are left out of the line
