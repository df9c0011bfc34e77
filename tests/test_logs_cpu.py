"""CPU: the formulas from scalar board to log dict (big_dreamer_amd/logs.py: logs_from) against the reference's
expressions written out in float64, and the import boundary of big_dreamer_amd.config (no HIP library to validate an
option)."""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from big_dreamer_amd import logs as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's defaults but for an entropy term that counts
HP = dict(kl_balance=0.8, kl_loss_weight=0.1, free_nats=3.0, entropy_weight=0.01, discount_weight=5.0)
COUNTS = dict(N=49 * 50, Mi=49 * 50 * 15, S=30)


def board(scale):
    """A hand-filled board: raw sums of the size a step of N = 2450 rows and Mi = 36750 imagined rows leaves; all the sums of
    one expression have one sign, so no expression cancels."""
    s = np.zeros(L.N_SLOTS, dtype=np.float32)
    s[L.SLOT_OBS], s[L.SLOT_REW], s[L.SLOT_KL], s[L.SLOT_DISC] = 61234.5, 2210.125, 301777.0, 1530.75
    s[L.SLOT_RET], s[L.SLOT_ENT], s[L.SLOT_VAL] = 412345.25, 98765.5, 35123.375
    s[L.SLOT_WOBJ], s[L.SLOT_RF] = 377001.5, 20917.75
    s[L.SLOT_GN_MODEL], s[L.SLOT_GN_ACTOR], s[L.SLOT_GN_CRITIC] = 1234.5, 0.03125, 77.25
    s[L.SLOT_RN], s[L.SLOT_RN + 1], s[L.SLOT_RN + 2] = scale, -1.5, 6.25
    return s


def expected(s, c, hp, world, use_discount, mix, return_norm):
    """The log dict in float64, from the reference: src/dreamer.py:293-296 (the model losses; _kl_loss, src/dreamer.py:122-144),
    359-360 (actor_loss = -objective.mean(), the entropy mean) and 383 (value_loss); the board holds the SUMS of the
    reference's means.  DESIGN.md, "Mixed actor gradient" and "Return normalisation", for the terms the reference lacks."""
    s = s.astype(np.float64)
    N, Mi = float(c["N"]), float(c["Mi"])
    obs, rew = s[L.SLOT_OBS] / N, s[L.SLOT_REW] / N
    if c["sum_form"]:                       # kl_balance == -1: the mean over rows of max(div, free_nats), summed by the kernel
        kl = s[L.SLOT_KL] / N
    else:                                   # the mean over every element of every rank, then free nats, then the balance
        m = max(s[L.SLOT_KL] / (N * c["S"] * world), hp["free_nats"])
        kl = hp["kl_balance"] * m + (1 - hp["kl_balance"]) * m
    model = obs + rew + kl * hp["kl_loss_weight"]
    scale = s[L.SLOT_RN] if return_norm and s[L.SLOT_RN] > 0 else 1.0
    rho = 1.0 if mix is None else mix
    if use_discount:                        # the discount-weighted objective is summed on the device; REINFORCE joins it
        objective = s[L.SLOT_WOBJ] + (1 - rho) * s[L.SLOT_RF] / scale
    else:
        objective = (rho * s[L.SLOT_RET] + (1 - rho) * s[L.SLOT_RF]) / scale + hp["entropy_weight"] * s[L.SLOT_ENT]
    out = dict(observation_loss=obs, reward_loss=rew, kl_loss=kl, actor_loss=-objective / Mi,
               policy_entropy=s[L.SLOT_ENT] / Mi, value_loss=s[L.SLOT_VAL] / Mi,
               grad_norm_model=math.sqrt(s[L.SLOT_GN_MODEL]), grad_norm_actor=math.sqrt(s[L.SLOT_GN_ACTOR]),
               grad_norm_critic=math.sqrt(s[L.SLOT_GN_CRITIC]))
    if use_discount:
        out["discount_loss"] = s[L.SLOT_DISC] / N
        model = model + out["discount_loss"] * hp["discount_weight"]
    out["model_loss"] = model
    if return_norm:
        out.update(return_scale=s[L.SLOT_RN], return_p_low=s[L.SLOT_RN + 1], return_p_high=s[L.SLOT_RN + 2])
    return out


@pytest.mark.parametrize("mix,use_discount,return_norm,sum_form,world",
                         list(itertools.product((None, 0.5), (False, True), (False, True), (0, 1), (1, 2))))
def test_log_formulas_against_float64(mix, use_discount, return_norm, sum_form, world):
    """Every key within float32 rounding of its expression: 4 ulp (float32) of the float64 value -- each expression is a sum
    of at most four one-signed terms, each term a few float32 operations on exact inputs."""
    s, c = board(7.75), dict(COUNTS, sum_form=sum_form)
    hp = dict(HP, kl_balance=-1 if sum_form else 0.8)
    got = L.logs_from(s, c, hp, world, use_discount, mix, return_norm)
    want = expected(s, c, hp, world, use_discount, mix, return_norm)
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert isinstance(got[k], float)
        assert abs(got[k] - w) <= 4 * float(np.spacing(np.float32(abs(w)))), (k, got[k], w)


@pytest.mark.parametrize("mix,use_discount", [(None, False), (0.5, False), (0.5, True)])
def test_scale_slot_zero_divides_by_one(mix, use_discount):
    """Slot SLOT_RN at 0 -- no behaviour phase has run -- is a scale of 1, not a division by zero."""
    s, c = board(0.0), dict(COUNTS, sum_form=0)
    got = L.logs_from(s, c, HP, 1, use_discount, mix, True)
    want = expected(s, c, HP, 1, use_discount, mix, False)
    assert math.isfinite(got["actor_loss"]) and got["return_scale"] == 0.0
    assert abs(got["actor_loss"] - want["actor_loss"]) <= 4 * float(np.spacing(np.float32(abs(want["actor_loss"]))))


def test_config_validates_options_without_the_hip_library():
    code = ("import sys, big_dreamer_amd.config as c\n"
            "assert 'big_dreamer_amd._cabi' not in sys.modules, 'config pulled in the HIP library'\n"
            "for n in ('check_return_normalization', 'check_critic_head', 'check_gradient_mixing', 'check_cnn_activation',\n"
            "          'check_dense_activation', 'check_action_distribution'):\n"
            "    assert callable(getattr(c, n)), n\n"
            "assert c.RETURN_NORM_KEYS[0] == 'return_normalization' and c.CRITIC_HEAD_KEYS[0] == 'critic_head'\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    from big_dreamer_amd import config, engine
    assert engine.check_critic_head is config.check_critic_head and engine.RETURN_NORM_KEYS is config.RETURN_NORM_KEYS
