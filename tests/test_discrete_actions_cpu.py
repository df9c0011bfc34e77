"""CPU tests of the Categorical actor (action_distribution="Categorical", DESIGN.md "Discrete actions"): the closed-form
head gradients the kernels use against autograd, the straight-through value rule, the argument checks that run before
any GPU use, the synthetic discrete environment, and the parameter / noise layout."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from big_dreamer_amd import synth
from tests.discrete_oracle import DISCRETE_GOLDEN, DiscreteOracleDreamer, discrete_head, oracle_hp
from tests.helpers import assert_close, check_fingerprints, load_golden


def _rows(A, n=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = (torch.randn(n, A, generator=g, dtype=torch.float64) * 3.0)
    q = torch.empty(n, A, dtype=torch.float64).exponential_(generator=g)
    return out, q, g


@pytest.mark.parametrize("A", [2, 6, 18, 64])
def test_closed_form_head_gradients_vs_autograd(A):
    """d out of the straight-through action (softmax Jacobian), of the exact entropy, and of REINFORCE's norm[k]."""
    out, q, g = _rows(A, seed=A)
    x = out.clone().requires_grad_(True)
    a, H, norm, k = discrete_head(x, q)
    gact = torch.randn(out.shape, generator=g, dtype=torch.float64)
    p = torch.softmax(norm, -1).detach()
    nd, Hd = norm.detach(), H.detach().unsqueeze(-1)
    want, = torch.autograd.grad((a * gact).sum(), x, retain_graph=True)
    torch.testing.assert_close(want, p * (gact - (p * gact).sum(-1, keepdim=True)), rtol=1e-10, atol=1e-12)
    want, = torch.autograd.grad(H.sum(), x, retain_graph=True)
    torch.testing.assert_close(want, -p * (nd + Hd), rtol=1e-10, atol=1e-12)
    lp = norm.gather(-1, k.unsqueeze(-1)).sum()
    want, = torch.autograd.grad(lp, x)
    torch.testing.assert_close(want, F.one_hot(k, A).double() - p, rtol=1e-10, atol=1e-12)


def test_sample_is_argmax_p_over_q_first_maximum():
    out = torch.zeros(3, 4)
    q = torch.ones(3, 4)
    _, _, _, k = discrete_head(out, q)
    assert k.tolist() == [0, 0, 0]                    # ties: the first maximum wins
    q[1, 2] = 0.5
    assert discrete_head(out, q)[3].tolist() == [0, 2, 0]


def test_straight_through_value_rule_matches_reference_line():
    """a = (onehot + p) - sg(p), as `action = action + action_dist.probs - action_dist.probs.detach()`
    (reference src/models.py:520): not exactly one-hot in fp32."""
    g = torch.Generator().manual_seed(3)
    out = torch.randn(4096, 18, generator=g)
    q = torch.empty(4096, 18).exponential_(generator=g)
    a, _, _, k = discrete_head(out, q)
    dist = torch.distributions.OneHotCategoricalStraightThrough(logits=out)
    sample = F.one_hot(k, 18).float()
    ref = sample + dist.probs - dist.probs.detach()
    assert torch.equal(a, ref)
    hot = a.gather(1, k[:, None]).squeeze(1)
    p = dist.probs.gather(1, k[:, None]).squeeze(1)
    assert torch.equal(hot, (1 + p) - p)
    assert bool((hot != 1).any()) and float((hot - 1).abs().max()) <= 1.2e-7
    assert float(a.sum(-1).sub(1).abs().max()) <= 1.2e-7
    assert torch.equal(torch.distributions.Categorical(logits=out).entropy(), discrete_head(out, q)[1])


def test_param_shapes_and_noise_layout():
    d = dataclasses.replace(synth.TINY, A=18, discrete_actions=True)
    assert d.actor_out == 18 and synth.TINY.actor_out == 2 * synth.TINY.A
    shapes = dict(synth.param_shapes(d)["actor"])
    assert shapes["model.8.weight"] == (18, d.Hd) and shapes["model.8.bias"] == (18,)
    assert dict(synth.param_shapes(synth.TINY)["actor"])["model.8.weight"] == (2 * synth.TINY.A, synth.TINY.Hd)
    nz = synth.make_noise(d, 0)
    assert "entropy" not in nz and nz["action"].shape == (d.Hm, d.N, 18) and float(nz["action"].min()) >= 0.0
    b = synth.make_batch(d, 0)
    assert np.array_equal(b["actions"].sum(-1), np.ones((d.L, d.B), np.float32))
    # Gaussian draws unchanged by the discrete option
    assert "entropy" in synth.make_noise(synth.TINY, 0)


def test_restatement_two_steps_finite_and_rho_one_is_minus_one():
    d = dataclasses.replace(synth.CAT_TINY, A=18, discrete_actions=True)
    P = synth.make_params(d, 5)
    logs = {}
    for rho in (-1, 1, 0.0):
        od = DiscreteOracleDreamer(P, dict(planning_horizon=d.H, gradient_mixing=rho, categorical=(d.cat_D, d.cat_C)))
        for step in range(2):
            logs[rho] = od.train_step(synth.make_batch(d, 5), synth.make_noise(d, 5 + step))
        assert np.isfinite(list(logs[rho].values())).all()
    assert logs[-1] == logs[1]
    assert logs[0.0]["actor_loss"] != logs[-1]["actor_loss"]


def _params(**kw):
    from big_dreamer_amd.config import load_config
    p = load_config([])
    p.update(kw)
    return p


def test_argument_checks_run_before_gpu_use(monkeypatch):
    from big_dreamer_amd.dreamer import Dreamer
    from big_dreamer_amd.engine import check_action_distribution
    from big_dreamer_amd.env import SyntheticEnv
    from big_dreamer_amd.planet import Planet
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    env = SyntheticEnv(3, 2, 10, 2, 0)
    with pytest.raises(ValueError, match="action_distribution"):
        Dreamer(_params(action_distribution="Beta"), env)
    with pytest.raises(ValueError, match="CEM"):
        Dreamer(_params(action_distribution="Categorical", algorithm="planet"), env)
    with pytest.raises(ValueError, match="CEM"):
        Planet(_params(action_distribution="Categorical"), env)
    with pytest.raises(RuntimeError, match="MI355X"):       # valid settings reach the CUDA check
        Dreamer(_params(action_distribution="Categorical"), env)
    assert check_action_distribution("Gaussian") == "Gaussian"
    with pytest.raises(ValueError):
        check_action_distribution("categorical")


def test_actor_model_rejects_unknown_distribution():
    from big_dreamer_amd.models import ActorModel
    with pytest.raises(ValueError, match="action_distribution"):
        ActorModel(4, 3, 8, 2, action_distribution="Bernoulli", engine=None)


def test_synthetic_discrete_env():
    from big_dreamer_amd.env import Env, SyntheticDiscreteEnv
    env = Env(dict(action_distribution="Categorical", synthetic_env_action_size=18, max_episode_length=6,
                   action_repeat=2, seed=0))
    assert isinstance(env, SyntheticDiscreteEnv) and env.action_size == 18 and env.U.shape == (18, 1)
    for _ in range(5):
        a = env.sample_random_action()
        assert a.shape == (18,) and float(a.sum()) == 1.0 and set(a.unique().tolist()) <= {0.0, 1.0}
    # the control is the table row of argmax(action): a straight-through vector acts like its one-hot
    e1, e2 = (Env(dict(action_distribution="Categorical", synthetic_env_action_size=18, max_episode_length=6,
                       action_repeat=2, seed=0)) for _ in range(2))
    e1.reset(); e2.reset()
    hot = torch.zeros(18); hot[7] = 1.0
    soft = hot + 1e-3 * torch.rand(18)
    o1, r1, d1 = e1.step(hot)
    o2, r2, d2 = e2.step(soft)
    assert torch.equal(o1, o2) and r1 == r2 and d1 == d2 is False
    done = False
    for _ in range(3):
        _, _, done = e1.step(hot)
    assert done
    # pixel observations: the same discrete control over the rendered system
    from big_dreamer_amd.env import SyntheticDiscretePixelEnv
    pe = Env(dict(action_distribution="Categorical", pixel_observation=True, synthetic_env_action_size=6,
                  max_episode_length=6, action_repeat=2, seed=0))
    assert isinstance(pe, SyntheticDiscretePixelEnv) and pe.action_size == 6 and pe.observation_size == (3, 64, 64)
    assert pe.reset().shape == (1, 3, 64, 64)
    img, r, _ = pe.step(pe.sample_random_action())
    assert img.shape == (1, 3, 64, 64) and np.isfinite(r) and float(img.abs().max()) <= 0.5
    # the Gaussian environment is unchanged
    assert type(Env(dict(max_episode_length=6, action_repeat=2, seed=0))).__name__ == "SyntheticEnv"


# ------------------------------------------------------------------------------------------ pinned by the reference
@pytest.mark.parametrize("name", sorted(DISCRETE_GOLDEN))
def test_restatement_vs_reference_golden(name):
    """Two train steps of the restatement against the reference's own run (tools/gen_discrete_golden.py): logs, clipped
    gradients and gradient norms, post-Adam weights, at the tolerances of test_oracle_golden."""
    d, seed, hp = DISCRETE_GOLDEN[name]
    g = load_golden(name)
    P, batch = synth.make_params(d, seed), synth.make_batch(d, seed)
    check_fingerprints(g, P, batch, synth.make_noise(d, seed))
    od = DiscreteOracleDreamer(P, oracle_hp(d, hp))
    for step in range(2):
        logs = od.train_step(batch, synth.make_noise(d, seed + step))
        if step == 0:
            od.update_critic()
        assert set(logs) == {k.split(".log.")[1] for k in g if k.startswith(f"step{step}.log.")}
        for k, v in logs.items():
            assert_close(f"step{step}.{k}", v, g[f"step{step}.log.{k}"], 2e-6, 2e-5)
        gn = od.last["grad_norms"]
        assert_close(f"step{step}.grad_norms", [gn["model"], gn["actor"], gn["critic"]], g[f"step{step}.grad_norms"],
                     1e-6, 1e-4)
        for grp, mods, grads in (("model", od.model_modules, od.last["model_grads"]),
                                 ("actor", ("actor",), od.last["actor_grads"]),
                                 ("critic", ("critic",), od.last["critic_grads"])):
            coef = min(1.0, od.hp["grad_clip_norm"] / (gn[grp] + 1e-6))
            i = 0
            for mod in mods:
                for k in od.P[mod]:
                    want = g[f"step{step}.grad.{mod}.{k}"]
                    scale = float(np.abs(want).max()) + 1e-12
                    assert_close(f"step{step}.grad.{mod}.{k}", (grads[i] * coef).numpy(), want, 2e-5 * scale + 1e-9, 2e-4)
                    i += 1
        for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
            for k, p in od.P[mod].items():
                assert_close(f"step{step}.param.{mod}.{k}", p.detach().numpy(), g[f"step{step}.param.{mod}.{k}"],
                             2e-6, 1e-6)


def test_golden_entropy_term_is_visible():
    """The entropy_weight = 0.1 cases are what pin the entropy gradient: with it removed, the restatement's actor
    gradient leaves the golden's tolerance."""
    d, seed, hp = DISCRETE_GOLDEN["discrete_tiny_a18"]
    g = load_golden("discrete_tiny_a18")
    P, batch = synth.make_params(d, seed), synth.make_batch(d, seed)
    od = DiscreteOracleDreamer(P, oracle_hp(d, dict(hp, entropy_weight=0.0)))
    od.train_step(batch, synth.make_noise(d, seed))
    coef = min(1.0, od.hp["grad_clip_norm"] / (od.last["grad_norms"]["actor"] + 1e-6))
    want = g["step0.grad.actor.model.8.weight"]
    err = np.abs((od.last["actor_grads"][-2] * coef).numpy() - want).max()
    assert err > 100 * (2e-5 * np.abs(want).max() + 1e-9)
