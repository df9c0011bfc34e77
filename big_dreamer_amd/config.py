"""Config loading with the reference CLI's surface (`python src/main.py key=value ...`, Hydra-style dotted
overrides such as ``ActorCritic.entropy_weight=1e-4``) without Hydra/OmegaConf, which are not installed."""
from __future__ import annotations

import os
from typing import Any, Dict, List

import yaml

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
    if not isinstance(cfg.get("replica_sync_at_start", False), bool):
        raise ValueError(f"replica_sync_at_start={cfg['replica_sync_at_start']!r} is not a boolean")
    return cfg
