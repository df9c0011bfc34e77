"""Config loading with the reference CLI's surface (`python src/main.py key=value ...`, Hydra-style dotted
overrides such as ``ActorCritic.entropy_weight=1e-4``) without Hydra/OmegaConf, which are not installed."""
from __future__ import annotations

import math
import os
from typing import Any, Dict, List

import numpy as np
import yaml

from .synth import CNN_ACTIVATIONS

ACTION_MODES = ("sample", "mode", "mean")        # eval_action, and action_mode of the acting step

REPLICA_POLICIES = ("raise", "resync")           # replica_on_mismatch


def check_replica_options(interval, policy):
    """replica_check_interval: an integer >= 0 (0 = off); replica_on_mismatch: one of REPLICA_POLICIES."""
    if isinstance(interval, bool) or not isinstance(interval, (int, float)) or int(interval) != interval or interval < 0:
        raise ValueError(f"replica_check_interval={interval!r} is not an integer >= 0")
    if policy not in REPLICA_POLICIES:
        raise ValueError(f"replica_on_mismatch={policy!r} is none of {REPLICA_POLICIES}")
    return int(interval), policy


def check_diagnostics_interval(interval) -> int:
    """diagnostics_interval: an integer >= 0 (0 = off), validated like replica_check_interval."""
    if isinstance(interval, bool) or not isinstance(interval, (int, float)) or int(interval) != interval or interval < 0:
        raise ValueError(f"diagnostics_interval={interval!r} is not an integer >= 0")
    return int(interval)


RETURN_NORMALIZATIONS = ("none", "percentile")
RETURN_NORM_KEYS = ("return_normalization", "return_norm_low", "return_norm_high", "return_norm_decay", "return_norm_floor")


def check_return_normalization(mode="none", low=0.05, high=0.95, decay=0.99, floor=1.0, algorithm=None) -> tuple:
    """ActorCritic.return_normalization and its four numbers ("Return normalisation"): "none" (the reference's
    objective) or "percentile" -- the returns of the actor objective divided by max(floor, P_high - P_low) of the imagined
    lambda-returns, smoothed with `decay`.  Quantiles 0 <= low < high <= 1, 0 <= decay < 1, floor > 0.  PlaNet
    (`algorithm`) has no actor and refuses "percentile".  Returns the five values, the numbers as floats."""
    if mode not in RETURN_NORMALIZATIONS:
        raise ValueError(f"return_normalization must be one of {RETURN_NORMALIZATIONS}, got {mode!r}")
    num = {}
    for key, v in (("return_norm_low", low), ("return_norm_high", high), ("return_norm_decay", decay),
                   ("return_norm_floor", floor)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{key} must be a finite number, got {v!r}")
        num[key] = float(v)
    low, high, decay, floor = num.values()
    if not 0.0 <= low < high <= 1.0:
        raise ValueError(f"return_norm_low / return_norm_high must satisfy 0 <= low < high <= 1, got {low!r}, {high!r}")
    if not 0.0 <= decay < 1.0:
        raise ValueError(f"return_norm_decay must be in [0, 1), got {decay!r}")
    if not 0.0 < floor <= 3.0e38:
        raise ValueError(f"return_norm_floor must be a positive fp32 number, got {floor!r}")
    if mode != "none" and algorithm == "planet":
        raise ValueError("return_normalization=percentile: PlaNet has no actor objective to normalise")
    return mode, low, high, decay, floor


CRITIC_HEAD_KEYS = ("critic_head", "critic_bins", "critic_bin_range")
CRITIC_HEAD_DEFAULTS = dict(critic_head="normal", critic_bins=255, critic_bin_range=20.0)
CRITIC_BINS_MAX = 1024
CRITIC_BIN_RANGE_MAX = 80.0        # expm1 of more overflows fp32


def check_critic_head(head="normal", bins=255, bin_range=20.0, algorithm=None) -> tuple:
    """ActorCritic.critic_head and its two numbers ("Two-hot critic"): "normal" (the reference's width-1 critic
    under a Normal(v, 1) loss) or "twohot" -- `bins` logits over bins uniform in symlog space on [-bin_range, bin_range],
    decoded as symexp of the softmax mean, trained with the cross-entropy against the two-hot encoding of symlog(return).
    bins: integer K, 2 <= K <= 1024; bin_range: Z, 0 < Z <= 80.  PlaNet (`algorithm`) has no critic and refuses "twohot".
    Returns (head, int K, float Z)."""
    from .synth import CRITIC_HEADS
    if head not in CRITIC_HEADS:
        raise ValueError(f"critic_head must be one of {CRITIC_HEADS}, got {head!r}")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= CRITIC_BINS_MAX:
        raise ValueError(f"critic_bins must be an integer in [2, {CRITIC_BINS_MAX}], got {bins!r}")
    if (isinstance(bin_range, bool) or not isinstance(bin_range, (int, float)) or not math.isfinite(bin_range)
            or not 0.0 < bin_range <= CRITIC_BIN_RANGE_MAX):
        raise ValueError(f"critic_bin_range must be a number in (0, {CRITIC_BIN_RANGE_MAX:g}], got {bin_range!r}")
    if head != "normal" and algorithm == "planet":
        raise ValueError("critic_head=twohot: PlaNet has no critic")
    return head, int(bins), float(bin_range)


REWARD_HEAD_KEYS = ("reward_head", "reward_bins", "reward_bin_range")
REWARD_HEAD_DEFAULTS = dict(reward_head="normal", reward_bins=255, reward_bin_range=20.0)
REWARD_BINS_MAX = CRITIC_BINS_MAX
REWARD_BIN_RANGE_MAX = CRITIC_BIN_RANGE_MAX


def check_reward_head(head="normal", bins=255, bin_range=20.0, algorithm=None) -> tuple:
    """reward_head and its two numbers ("World-model heads on any scale"): "normal" (the reference's width-1
    reward model under a Normal(r, 1) loss) or "twohot" -- `bins` logits over bins uniform in symlog space on
    [-bin_range, bin_range], decoded as symexp of the softmax mean, trained with the cross-entropy against the two-hot
    encoding of symlog(reward).  bins: integer K, 2 <= K <= 1024; bin_range: Z, 0 < Z <= 80.  PlaNet (`algorithm`) plans
    with a fused width-1 reward model and refuses "twohot".  Returns (head, int K, float Z)."""
    from .synth import REWARD_HEADS
    if head not in REWARD_HEADS:
        raise ValueError(f"reward_head must be one of {REWARD_HEADS}, got {head!r}")
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= REWARD_BINS_MAX:
        raise ValueError(f"reward_bins must be an integer in [2, {REWARD_BINS_MAX}], got {bins!r}")
    if (isinstance(bin_range, bool) or not isinstance(bin_range, (int, float)) or not math.isfinite(bin_range)
            or not 0.0 < bin_range <= REWARD_BIN_RANGE_MAX):
        raise ValueError(f"reward_bin_range must be a number in (0, {REWARD_BIN_RANGE_MAX:g}], got {bin_range!r}")
    if head != "normal" and algorithm == "planet":
        raise ValueError("reward_head=twohot: PlaNet's CEM rollout evaluates a width-1 reward model")
    return head, int(bins), float(bin_range)


def check_symlog_observations(value=False, pixel=False, algorithm=None) -> bool:
    """symlog_observations ("World-model heads on any scale"): a boolean; true makes the encoder read
    symlog(obs) and observation_loss the Normal(., 1) loss against symlog(obs).  Vector observations only (pixels are
    bounded already: DreamerV3 applies symlog to vector inputs), and not with PlaNet (`algorithm`)."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"symlog_observations must be a boolean, got {value!r}")
    if value and pixel:
        raise ValueError("symlog_observations=true: pixel observations are bounded already; symlog applies to vector "
                         "observations (pixel_observation=false)")
    if value and algorithm == "planet":
        raise ValueError("symlog_observations=true: PlaNet is not supported (its planner and train step read raw observations)")
    return bool(value)


def check_gradient_mixing(value) -> float:
    """ActorCritic.gradient_mixing: -1 (the reference's objective, backpropagation through the learned dynamics) or
    rho in [0, 1], DreamerV2's ``actor_grad_mix`` -- the weight of the dynamics term against REINFORCE (1 = -1)."""
    try:
        rho = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"gradient_mixing must be -1 or a number in [0, 1], got {value!r}") from None
    if not (rho == -1 or 0.0 <= rho <= 1.0):
        raise ValueError(f"gradient_mixing must be -1 or a number in [0, 1], got {value!r}")
    return rho


def check_cnn_activation(value) -> str:
    """cnn_activation_function: the activation of CnnImageEncoder / ObservationModel, a torch.nn class name as in the
    reference (src/planet.py:186-192): "ELU" (default), "ReLU" or "Tanh" (epilogue codes of csrc/conv.hip)."""
    if value not in CNN_ACTIVATIONS:
        raise ValueError(f"cnn_activation_function must be one of {CNN_ACTIVATIONS}, got {value!r}")
    return value


def check_dense_activation(value) -> str:
    """dense_activation_function: ELU is written into the epilogues of the scan, head and planner kernels."""
    if value != "ELU":
        raise NotImplementedError("the HIP path implements the reference default activation (ELU)")
    return value


ACTION_DISTRIBUTIONS = ("Gaussian", "Categorical")


def check_action_distribution(value) -> str:
    """action_distribution: "Gaussian" (the tanh-Normal actor) or "Categorical" (one-hot actions over A classes with a
    straight-through sample, DESIGN.md "Discrete actions")."""
    if value not in ACTION_DISTRIBUTIONS:
        raise ValueError(f"action_distribution must be one of {ACTION_DISTRIBUTIONS}, got {value!r}")
    return value


DEFAULT_CONFIG =os.path.join(os.path.dirname(os.path.abspath(__file__)), "conf", "config.yaml")


def _coerce(x: Any) -> Any:
    """PyYAML (YAML 1.1) reads '2e-4' as a string; OmegaConf reads a float.  Match OmegaConf."""
    if isinstance(x, dict):
        return {k: _coerce(v) for k, v in x.items()}
    if isinstance(x, str):
        try:
            return float(x)
        except ValueError:
            return x
    return x


def _parse_value(text: str) -> Any:
    return _coerce(yaml.safe_load(text))


def load_config(overrides: List[str] = (), path: str = DEFAULT_CONFIG) -> Dict[str, Any]:
    with open(path) as f:
        cfg = _coerce(yaml.safe_load(f))
    for ov in overrides:
        if "=" not in ov:
            raise ValueError(f"override '{ov}' is not of the form key=value")
        key, val = ov.split("=", 1)
        node = cfg
        parts = key.split(".")
        for p in parts[:-1]:
            if p not in node or not isinstance(node[p], dict):
                raise KeyError(f"unknown config group '{p}' in override '{ov}'")
            node = node[p]
        if parts[-1] not in node:
            raise KeyError(f"unknown config key '{key}' (the reference's Hydra config rejects unknown keys too)")
        node[parts[-1]] = _parse_value(val)
    if cfg.get("eval_action", "sample") not in ACTION_MODES:
        raise ValueError(f"eval_action={cfg['eval_action']!r} is none of {ACTION_MODES}")
    if not isinstance(cfg.get("eval_state_mean", False), bool):
        raise ValueError(f"eval_state_mean={cfg['eval_state_mean']!r} is not a boolean")
    if not isinstance(cfg.get("sample_on_device", False), bool):
        raise ValueError(f"sample_on_device={cfg['sample_on_device']!r} is not a boolean")
    check_replica_options(cfg.get("replica_check_interval", 0), cfg.get("replica_on_mismatch", "raise"))
    check_diagnostics_interval(cfg.get("diagnostics_interval", 0))
    check_reward_head(*(cfg.get(k, REWARD_HEAD_DEFAULTS[k]) for k in REWARD_HEAD_KEYS), algorithm=cfg.get("algorithm"))
    check_symlog_observations(cfg.get("symlog_observations", False), bool(cfg.get("pixel_observation", False)),
                              cfg.get("algorithm"))
    if not isinstance(cfg.get("replica_sync_at_start", False), bool):
        raise ValueError(f"replica_sync_at_start={cfg['replica_sync_at_start']!r} is not a boolean")
    return cfg
