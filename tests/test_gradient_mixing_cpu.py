"""CPU tests of ActorCritic.gradient_mixing: the restatement (tests/mixing_oracle.py) against the oracle at rho = 1,
the REINFORCE head gradient against its closed form, the range check of the surface and the host-side argument checks
of bd_actor_reinforce (no launch: every call here is rejected before one)."""
import ctypes as C

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from oracle import dreamer_oracle as O
from tests.mixing_oracle import MixingOracleDreamer, actor_head, tanh_normal_log_density


def _steps(od, d, seed):
    out = []
    for step in range(2):
        logs = od.train_step(synth.make_batch(d, seed), synth.make_noise(d, seed + step))
        if step == 0:
            od.update_critic()
        out.append((logs, {k: [g.clone() for g in od.last[k]] for k in ("model_grads", "actor_grads", "critic_grads")},
                    dict(od.last["grad_norms"])))
    return out


@pytest.mark.parametrize("d,hp", [(synth.TINY, {}), (synth.TINY_DISCOUNT, {})])
def test_restatement_at_rho_one_is_the_oracle(d, hp):
    """rho = 1 is the reference's objective: two steps give the oracle's logs, clipped gradients and weights exactly."""
    P = synth.make_params(d, 0)
    ref = O.OracleDreamer(P, dict(hp, planning_horizon=d.H))
    mix = MixingOracleDreamer(P, dict(hp, planning_horizon=d.H, gradient_mixing=1))
    for (la, ga, na), (lb, gb, nb) in zip(_steps(ref, d, 3), _steps(mix, d, 3)):
        assert la == lb
        assert na == nb
        for k in ga:
            assert all(torch.equal(x, y) for x, y in zip(ga[k], gb[k])), k
    for mod in ref.P:
        for k, p in ref.P[mod].items():
            assert torch.equal(p, mix.P[mod][k]), (mod, k)


def test_restatement_changes_the_actor_update_only():
    """rho = 0.3: the same world-model and critic steps (the critic sees the same returns), a different actor step."""
    d = synth.TINY
    P = synth.make_params(d, 0)
    ref = O.OracleDreamer(P, dict(planning_horizon=d.H))
    mix = MixingOracleDreamer(P, dict(planning_horizon=d.H, gradient_mixing=0.3))
    la = ref.train_step(synth.make_batch(d, 1), synth.make_noise(d, 1))
    lb = mix.train_step(synth.make_batch(d, 1), synth.make_noise(d, 1))
    for k in ("model_loss", "value_loss", "policy_entropy"):
        assert la[k] == lb[k], k
    assert la["actor_loss"] != lb["actor_loss"]
    assert not torch.equal(ref.P["actor"]["model.8.weight"], mix.P["actor"]["model.8.weight"])
    assert torch.equal(ref.P["critic"]["model.8.weight"], mix.P["critic"]["model.8.weight"])


def test_reinforce_head_gradient_matches_closed_form():
    """d l / d head: (eps / std) (1 - th^2) on the mean half, ((eps^2 - 1) / std) sigmoid(r + c0) on the std half --
    the closed form bd_actor_reinforce evaluates, against autograd of the restatement's log-density (float64)."""
    g = torch.Generator().manual_seed(5)
    rows, A = 37, 3
    out = (torch.randn(rows, 2 * A, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    eps = torch.randn(rows, A, generator=g, dtype=torch.float64)
    coef = torch.randn(rows, generator=g, dtype=torch.float64)           # -(1 - rho) w adv / count, per row
    mean, std = actor_head(out)
    u = (mean + std * eps).detach()
    (tanh_normal_log_density(u, mean, std) * coef).sum().backward()
    m, r = out.detach()[:, :A], out.detach()[:, A:]
    th = torch.tanh(m / O.ACT_MEAN_SCALE)
    sd = torch.nn.functional.softplus(r + O.RAW_INIT_STD) + O.ACT_MIN_STD
    sg = torch.sigmoid(r + O.RAW_INIT_STD)
    want = torch.cat([coef[:, None] * (eps / sd) * (1 - th * th), coef[:, None] * ((eps * eps - 1) / sd) * sg], 1)
    np.testing.assert_allclose(out.grad.numpy(), want.numpy(), rtol=1e-9, atol=1e-12)


def test_gradient_mixing_range():
    from big_dreamer_amd.engine import check_gradient_mixing
    for ok in (-1, 0, 0.3, 1, "0.5"):
        assert check_gradient_mixing(ok) == float(ok)
    for bad in (1.5, -0.5, 2, float("nan"), "x", None):
        with pytest.raises(ValueError):
            check_gradient_mixing(bad)


@pytest.mark.parametrize("bad", [1.5, -0.5, 2])
def test_surface_rejects_out_of_range_mixing_before_touching_a_gpu(bad):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import SyntheticEnv
    params = load_config([f"ActorCritic.gradient_mixing={bad}"])
    for cls in (Dreamer, DreamerV2):
        with pytest.raises(ValueError, match="gradient_mixing"):
            cls(params, SyntheticEnv(3, 1, 40, 2, 0), device="cpu")


def test_actor_reinforce_host_checks_without_gpu():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    # (no pointer here is ever dereferenced: each call fails one host-side check before any launch)
    p = C.c_void_p(16)
    ptrs = [p] * 7

    def call(ptrs_, Hm=2, N=5, A=3, rho=0.5):
        return lib.bd_actor_reinforce(*ptrs_, Hm, N, A, rho, 0.1, -1e-5, 0, p, p, 11, p, None)

    for i in range(5):              # eps, u/std, stats, returns, base0
        q = list(ptrs)
        q[i] = None
        assert call(q) != 0
        assert b"bd_actor_reinforce: missing pointers" in lib.bd_last_error()
    q = list(ptrs)
    q[5] = None                     # value: needed unless Hm == 1
    assert call(q) != 0 and b"missing pointers" in lib.bd_last_error()
    assert lib.bd_actor_reinforce(*ptrs, 2, 5, 3, 0.5, 0.1, -1e-5, 0, None, p, 11, p, None) != 0     # d_actor_out
    assert lib.bd_actor_reinforce(*ptrs, 2, 5, 3, 0.5, 0.1, -1e-5, 0, p, None, 11, p, None) != 0     # scalars
    assert lib.bd_actor_reinforce(*ptrs, 2, 5, 3, 0.5, 0.1, -1e-5, 0, p, p, 11, None, None) != 0     # workspace
    for A in (0, -2):
        assert call(ptrs, A=A) != 0 and b"bad dims" in lib.bd_last_error()
    assert call(ptrs, Hm=0) != 0 and b"bad dims" in lib.bd_last_error()
    assert call(ptrs, N=0) != 0 and b"bad dims" in lib.bd_last_error()
    for rho in (-0.1, 1.5, float("nan")):
        assert call(ptrs, rho=rho) != 0 and b"outside [0, 1]" in lib.bd_last_error()
    with pytest.raises(RuntimeError, match="bd_actor_reinforce"):
        _cabi.check(call(ptrs, rho=2.0))
