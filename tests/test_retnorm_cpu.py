"""CPU: percentile return normalisation (ActorCritic.return_normalization) -- the restatement (tests/retnorm_oracle.py)
against the reference-pinned mixing restatement, the running range (tests/retnorm_ref.py), the validation of the five keys
(before any device is touched) and the host-side refusals of bd_return_range / bd_return_seed (made before anything is
enqueued, so they need no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import retnorm_ref
from tests.helpers import CASES
from tests.mixing_oracle import MixingOracleDreamer
from tests.retnorm_oracle import RetnormOracleDreamer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracles(name, rho, state=None, ent_scale=1.0):
    d, seed, hp, _ = CASES[name]
    hp = dict(hp, planning_horizon=d.H, gradient_mixing=rho, entropy_weight=0.01)     # an entropy term that counts
    P = synth.make_params(d, seed)
    norm = RetnormOracleDreamer(P, dict(hp))
    if state is not None:
        norm.rn_state = dict(state)
    plain = MixingOracleDreamer(P, dict(hp, entropy_weight=hp["entropy_weight"] * ent_scale))
    batch, noise = synth.make_batch(d, seed), synth.make_noise(d, seed)
    return norm, plain, batch, noise


# ------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name,rho", [("tiny", -1), ("tiny", 0.5), ("tiny_discount", 0.1)])
def test_scale_one_reproduces_the_mixing_restatement(name, rho):
    """Empty range, floor 1: S = 1 and x / 1 is x, so logs, gradients and weights are those of MixingOracleDreamer, exactly."""
    norm, plain, batch, noise = _oracles(name, rho)
    ln, lp = norm.train_step(batch, noise), plain.train_step(batch, noise)
    assert ln["return_scale"] == 1.0 and ln["return_p_low"] == 0.0 and ln["return_p_high"] == 0.0
    assert set(ln) == set(lp) | {"return_scale", "return_p_low", "return_p_high"}
    for k, v in lp.items():
        assert ln[k] == v, k
    for grp in ("model_grads", "actor_grads", "critic_grads"):
        for a, b in zip(norm.last[grp], plain.last[grp]):
            assert torch.equal(a, b), grp
    assert norm.last["grad_norms"] == plain.last["grad_norms"]


@pytest.mark.parametrize("name,rho", [("tiny", -1), ("tiny", 0.0), ("tiny", 0.5), ("tiny_discount", 0.1)])
def test_preset_scale_is_the_mixing_restatement_with_scaled_entropy_weight(name, rho):
    """obj_S(eta) = (1 / S) obj_1(eta S): with a preset range the actor gradients are 1 / S times those of
    MixingOracleDreamer run with entropy_weight * S, and the loss likewise.  World model and critic do not see S.
    Tolerance: both sides are fp32 autograd over the same graph up to where 1 / S enters; the gradients are sums of up
    to ~10^3 products, so they agree to about 10^3 fp32 roundings (6e-8 each) of the largest element: 1e-4 of it."""
    state = dict(lo=-1.5, hi=6.0, count=3.0, skipped=0.0)
    S = float(retnorm_ref.scale(state, 1.0))
    assert S == 7.5
    norm, plain, batch, noise = _oracles(name, rho, state, ent_scale=S)
    ln, lp = norm.train_step(batch, noise), plain.train_step(batch, noise)
    assert ln["return_scale"] == 7.5 and ln["return_p_low"] == -1.5 and ln["return_p_high"] == 6.0
    assert abs(ln["actor_loss"] - lp["actor_loss"] / S) <= 1e-5 * abs(lp["actor_loss"] / S) + 1e-7
    for k in ("model_loss", "value_loss", "policy_entropy", "kl_loss"):
        assert ln[k] == lp[k], k
    worst = 0.0
    for a, b in zip(norm.last["actor_grads"], plain.last["actor_grads"]):
        want = b.double() / S
        tol = 1e-4 * float(want.abs().max()) + 1e-12
        worst = max(worst, float((a.double() - want).abs().max()) / tol)
        assert float((a.double() - want).abs().max()) <= tol
    print(f"worst error / tolerance = {worst:.3f}")
    assert float(sum(g.abs().sum() for g in norm.last["actor_grads"])) > 0
    for grp in ("model_grads", "critic_grads"):
        for a, b in zip(norm.last[grp], plain.last[grp]):
            assert torch.equal(a, b), grp
    # the step's own returns moved the range
    M = norm.last["returns"].numel()
    want = retnorm_ref.update(state, norm.last["returns"].numpy(), *retnorm_ref.ranks(M), 0.99)
    assert norm.rn_state == want and want["count"] == 4.0


def test_running_range_restatement():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(1001).astype(np.float32)
    k = retnorm_ref.ranks(1001)
    assert k == (50, 950) and retnorm_ref.ranks(1) == (0, 0) and retnorm_ref.ranks(2, 0.0, 1.0) == (0, 1)
    s0 = retnorm_ref.empty_state()
    assert retnorm_ref.scale(s0, 1.0) == np.float32(1.0) and retnorm_ref.scale(s0, 0.25) == np.float32(0.25)
    s1 = retnorm_ref.update(s0, x, *k, 0.99)
    srt = np.sort(x)
    assert s1 == dict(lo=float(srt[50]), hi=float(srt[950]), count=1.0, skipped=0.0)
    s2 = retnorm_ref.update(s1, 2 * x, *k, 0.5)
    assert s2["lo"] == 0.5 * s1["lo"] + 0.5 * float(2 * srt[50]) and s2["count"] == 2.0
    assert retnorm_ref.scale(s2, 1.0) == np.float32(s2["hi"] - s2["lo"])
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7] = bad
        assert retnorm_ref.update(s2, y, *k, 0.5) == dict(s2, skipped=1.0)


# ------------------------------------------------------------------------------------------ the keys
def test_config_defaults_and_overrides():
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.engine import DEFAULT_HP, RETURN_NORM_KEYS
    ac = load_config()["ActorCritic"]
    want = dict(return_normalization="none", return_norm_low=0.05, return_norm_high=0.95, return_norm_decay=0.99,
                return_norm_floor=1.0)
    assert {k: ac[k] for k in RETURN_NORM_KEYS} == want == {k: DEFAULT_HP[k] for k in RETURN_NORM_KEYS}
    ac = load_config(["ActorCritic.return_normalization=percentile", "ActorCritic.return_norm_decay=0.9"])["ActorCritic"]
    assert ac["return_normalization"] == "percentile" and ac["return_norm_decay"] == 0.9


def test_check_return_normalization():
    from big_dreamer_amd.engine import check_return_normalization as chk
    assert chk() == ("none", 0.05, 0.95, 0.99, 1.0)
    assert chk("percentile", 0, 1, 0, 2) == ("percentile", 0.0, 1.0, 0.0, 2.0)
    assert chk("none", algorithm="planet")[0] == "none"
    for bad in (dict(mode="quantile"), dict(mode=None), dict(mode="Percentile"), dict(low=0.5, high=0.5),
                dict(low=0.6, high=0.4), dict(low=-0.1), dict(high=1.1), dict(decay=1.0), dict(decay=-0.1), dict(floor=0.0),
                dict(floor=-1.0), dict(floor=float("nan")), dict(floor=float("inf")), dict(decay="0.5"), dict(low=True),
                dict(mode="percentile", algorithm="planet")):
        with pytest.raises(ValueError):
            chk(**bad)


@pytest.mark.parametrize("override,algo", [("return_normalization=median", "dreamer"), ("return_norm_low=0.95", "dreamer"),
                                           ("return_norm_decay=1.0", "dreamerV2"), ("return_norm_floor=0", "dreamer"),
                                           ("return_normalization=percentile", "planet")])
def test_bad_keys_raise_before_a_device_is_touched(override, algo, monkeypatch):
    """Engine, agent and command line: ValueError, with every way into the GPU runtime closed."""
    import importlib.util
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.engine import RETURN_NORM_KEYS, DreamerEngine
    from big_dreamer_amd.planet import Planet

    def touched(*a, **k):
        raise AssertionError("a device was touched")

    for fn in ("is_available", "current_device", "set_device", "init", "_lazy_init", "current_stream", "Stream"):
        monkeypatch.setattr(torch.cuda, fn, touched)
    ov = [f"ActorCritic.{override}", f"algorithm={algo}"]
    params = load_config(ov)
    with pytest.raises(ValueError, match="return_norm"):
        {"planet": Planet, "dreamer": Dreamer, "dreamerV2": DreamerV2}[algo](params, env=None)
    if algo != "planet":
        with pytest.raises(ValueError, match="return_norm"):
            DreamerEngine(synth.TINY, {k: params["ActorCritic"][k] for k in RETURN_NORM_KEYS}, "cuda")
    spec = importlib.util.spec_from_file_location("bd_cli_main", os.path.join(ROOT, "src", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(ValueError, match="return_norm"):
        cli.my_app(ov)


# ------------------------------------------------------------------------------------------ the C ABI
def test_kernels_are_declared_and_exported():
    from big_dreamer_amd import _cabi
    hdr = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    for name in ("bd_return_range", "bd_return_seed", "bd_actor_reinforce_norm", "bd_actor_reinforce_cat_norm"):
        assert re.search(rf"^int\s+{name}\s*\(", hdr, flags=re.M), name
        assert name in _cabi.EXPORTED and hasattr(_cabi.lib, name)
    assert "retnorm.hip" in open(os.path.join(ROOT, "big_dreamer_amd", "csrc", "Makefile")).read()


def test_return_range_refuses_bad_arguments_before_any_launch():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    x = (C.c_float * 16)()                       # never read: every call below is refused first
    st = (C.c_double * 4)()
    rg = (C.c_float * 4)()
    px, ps, pr = C.addressof(x), C.addressof(st), C.addressof(rg)

    def call(*a):
        return lib.bd_return_range(*a, None), lib.bd_last_error().decode()

    good = [px, 16, 0, 15, 0.99, 1.0, ps, pr]
    cases = [({1: 0}, "M = 0"), ({1: -3}, "M = -3"), ({2: -1}, "ranks (-1, 15)"), ({2: 9, 3: 8}, "ranks (9, 8)"),
             ({3: 16}, "ranks (0, 16)"), ({4: 1.0}, "decay 1 outside"), ({4: -0.5}, "decay -0.5 outside"),
             ({4: float("nan")}, "decay"), ({5: 0.0}, "floor 0"), ({5: -1.0}, "floor -1"), ({5: float("inf")}, "floor inf"),
             ({0: None}, "returns is null"), ({0: px + 2}, "returns is null or not 4-byte aligned"),
             ({6: None}, "state is null"), ({6: ps + 4}, "state is null or not 8-byte aligned"),
             ({7: None}, "range is null"), ({7: pr + 1}, "range is null or not 4-byte aligned")]
    for change, text in cases:
        a = list(good)
        for i, v in change.items():
            a[i] = v
        rc, msg = call(*a)
        assert rc != 0 and msg.startswith("bd_return_range:") and text in msg, (change, msg)
        assert "launch failed" not in msg
    assert all(v == 0 for v in st) and all(v == 0 for v in rg)


def test_return_seed_refuses_bad_arguments_before_any_launch():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    buf = (C.c_float * 16)()
    p = C.addressof(buf)

    def call(*a):
        return lib.bd_return_seed(*a, None), lib.bd_last_error().decode()

    good = [p, -0.1, None, 8, p, p, 12]
    cases = [({0: None}, "range is null"), ({0: p + 2}, "range is null or not 4-byte aligned"),
             ({4: None}, "null dreturns with n = 8"), ({4: p + 1}, "not 4-byte aligned"), ({2: p + 3}, "not 4-byte aligned"),
             ({5: p + 2}, "not 4-byte aligned"), ({6: -1}, "slot = -1"), ({3: 0, 4: None, 5: None}, "nothing to write")]
    for change, text in cases:
        a = list(good)
        for i, v in change.items():
            a[i] = v
        rc, msg = call(*a)
        assert rc != 0 and msg.startswith("bd_return_seed:") and text in msg, (change, msg)
        assert "launch failed" not in msg
    assert all(v == 0 for v in buf)


def test_reinforce_norm_refuses_a_misaligned_scale():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    rc = lib.bd_actor_reinforce_norm(p, p, p, p, p, p, None, p + 2, 2, 5, 3, 0.5, 0.1, -1e-5, 0, p, p, 11, p, None)
    assert rc != 0 and b"ret_scale is not 4-byte aligned" in lib.bd_last_error()
    rc = lib.bd_actor_reinforce_cat_norm(p, p, p, p, p, None, p + 2, 2, 5, 3, 0.5, 0.1, -1e-5, 0, p, p, 11, p, None)
    assert rc != 0 and b"ret_scale is not 4-byte aligned" in lib.bd_last_error()
    rc = lib.bd_actor_reinforce_norm(p, p, p, p, p, p, None, p, 2, 5, 3, 1.5, 0.1, -1e-5, 0, p, p, 11, p, None)
    assert rc != 0 and b"gradient mixing 1.5 outside" in lib.bd_last_error()
