"""Training diagnostics, host side: the layout of the per-step diagnostic block the engine fills on the device
(csrc/diag.hip) and its conversion into log entries.  Everything here is float64 numpy on a few hundred numbers.

The block is one array of doubles in three regions -- ``model``, ``actor``, ``critic``, one per optimiser phase, each written
on that phase's stream and copied to the host behind it.  A region is a sequence of named fields (`Layout.fields`); a
"sextuple" is what bd_moments writes: count of finite values, their sum, sum of squares, min, max, count of non-finite values.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .config import check_diagnostics_interval

# A latent dimension (Gaussian) or factor (Categorical) is ACTIVE when its KL, averaged over the batch, exceeds this many
# nats (Burda et al. 2016 use the same 0.01 on the posterior mean's variance).  A definition, not a tolerance.
ACTIVE_NATS = 0.01

SEXT = 6                       # BD_MOMENTS_WORDS
LATENT_WORDS, LATENT_CAT_WORDS = 15, 5
REGIONS = ("model", "actor", "critic")

DYNAMICS_KEYS = ("kl_raw", "kl_per_dim", "kl_active_dims", "post_entropy", "prior_entropy")
GAUSSIAN_KEYS = ("post_std_mean", "post_std_min", "prior_std_mean", "prior_std_min")
CATEGORICAL_KEYS = ("post_max_prob", "prior_max_prob", "post_classes_used")
REWARD_KEYS = ("reward_batch_mean", "reward_batch_std", "reward_pred_mean", "reward_pred_std")
BEHAVIOUR_KEYS = tuple(f"imag_{w}_{s}" for w in ("reward", "value", "return") for s in ("mean", "std", "min", "max")) + (
    "critic_value_mean", "critic_value_std", "value_explained_variance")
TANH_ACTION_KEYS = ("action_mean", "action_std", "action_min", "action_max", "action_rms")
CATEGORICAL_ACTION_KEYS = ("action_freq",)


check_interval = check_diagnostics_interval


class Layout:
    """Where each field of the diagnostic block lies.  fields[name] = (offset, doubles); region[r] = (begin, end)."""

    def __init__(self, categorical: bool, n_latent: int, n_classes: int, behaviour: bool, discrete_actions: bool,
                 action_size: int, modules: Dict[str, Sequence[str]]):
        self.categorical, self.n_latent, self.n_classes = bool(categorical), int(n_latent), int(n_classes)
        self.behaviour, self.discrete_actions, self.action_size = bool(behaviour), bool(discrete_actions), int(action_size)
        self.modules = {g: tuple(m) for g, m in modules.items()}
        self.fields: Dict[str, Tuple[int, int]] = {}
        self.region: Dict[str, Tuple[int, int]] = {}
        off = 0

        def add(name: str, n: int) -> None:
            nonlocal off
            self.fields[name] = (off, n)
            off += n

        begin = off
        add("latent", LATENT_CAT_WORDS if categorical else LATENT_WORDS)
        add("kl_cols", self.n_latent)
        if categorical:
            add("used", (self.n_latent * self.n_classes + 1) // 2)            # 32-bit words, two to a double
        add("mom_wm", 2 * SEXT)                                                # rewards of the batch, reward predictions
        add("gsq_model", len(self.modules["model"]))
        add("wsq_model", len(self.modules["model"]))
        self.region["model"] = (begin, off)
        begin = off
        if behaviour:
            add("mom_bh", (3 if discrete_actions else 4) * SEXT)               # imagined reward, value, return (, action)
            if discrete_actions:
                add("act_freq", (self.action_size + 1) // 2)                   # fp32 column sums, two to a double
            add("gsq_actor", len(self.modules["actor"]))
            add("wsq_actor", len(self.modules["actor"]))
        self.region["actor"] = (begin, off)
        begin = off
        if behaviour:
            add("mom_cr", 2 * SEXT)                                            # critic value, return - critic value
            add("gsq_critic", len(self.modules["critic"]))
            add("wsq_critic", len(self.modules["critic"]))
        self.region["critic"] = (begin, off)
        self.size = off

    def get(self, block: np.ndarray, name: str) -> np.ndarray:
        off, n = self.fields[name]
        return block[off:off + n]


def moments(sext: np.ndarray) -> Dict[str, float]:
    """count, mean, std (population; variance clamped at 0), min, max, rms, var and nonfinite of one sextuple.  No finite
    value: mean, std, rms and var are NaN, min = +inf, max = -inf."""
    n, s, ss, mn, mx, nf = (float(v) for v in sext)
    if n > 0:
        mean = s / n
        var = max(ss / n - mean * mean, 0.0)
        std, rms = math.sqrt(var), math.sqrt(ss / n)
    else:
        mean = var = std = rms = math.nan
    return {"count": n, "mean": mean, "std": std, "var": var, "min": mn, "max": mx, "rms": rms, "nonfinite": nf}


def explained_variance(ret: Dict[str, float], err: Dict[str, float]) -> float:
    """1 - Var(returns - v) / Var(returns); NaN when the returns do not vary (or nothing is finite)."""
    if not ret["var"] > 0.0:
        return math.nan
    return 1.0 - err["var"] / ret["var"]


def _put(out: dict, prefix: str, m: Dict[str, float], stats: Sequence[str], name: Optional[str] = None) -> None:
    for s in stats:
        out[f"{prefix}_{s}"] = m[s]
    if m["nonfinite"] > 0:
        out[f"nonfinite/{name or prefix}"] = m["nonfinite"]


def entries(block: np.ndarray, lay: Layout, rows: int, imag_rows: int = 0, regions: Sequence[str] = REGIONS) -> Dict[str, object]:
    """Log entries of one diagnosed step.  block: the `lay.size` doubles; rows: posterior rows T * B of the step;
    imag_rows: imagined decisions Hm * N.  Only the `regions` named are read (PlaNet has the model region alone)."""
    block = np.asarray(block, dtype=np.float64)
    out: Dict[str, object] = {}
    if "model" in regions:
        lat, cols = lay.get(block, "latent"), lay.get(block, "kl_cols")
        per_dim = cols / rows
        out["kl_raw"] = float(lat[2] / rows)
        out["kl_per_dim"] = [float(v) for v in per_dim]
        out["kl_active_dims"] = int(np.count_nonzero(per_dim > ACTIVE_NATS))
        out["post_entropy"] = float(lat[0] / rows)
        out["prior_entropy"] = float(lat[1] / rows)
        if lay.categorical:
            groups = rows * lay.n_latent
            out["post_max_prob"] = float(lat[3] / groups)
            out["prior_max_prob"] = float(lat[4] / groups)
            used = lay.get(block, "used").view(np.uint32)[:lay.n_latent * lay.n_classes]
            out["post_classes_used"] = float(np.count_nonzero(used)) / (lay.n_latent * lay.n_classes)
        else:
            _put(out, "post_std", moments(lat[3:9]), ("mean", "min"))
            _put(out, "prior_std", moments(lat[9:15]), ("mean", "min"))
        wm = lay.get(block, "mom_wm")
        _put(out, "reward_batch", moments(wm[:SEXT]), ("mean", "std"))
        _put(out, "reward_pred", moments(wm[SEXT:]), ("mean", "std"))
    ret = None
    if "actor" in regions and lay.behaviour:
        bh = lay.get(block, "mom_bh")
        full = ("mean", "std", "min", "max")
        _put(out, "imag_reward", moments(bh[:SEXT]), full)
        _put(out, "imag_value", moments(bh[SEXT:2 * SEXT]), full)
        ret = moments(bh[2 * SEXT:3 * SEXT])
        _put(out, "imag_return", ret, full)
        if lay.discrete_actions:
            freq = lay.get(block, "act_freq").view(np.float32)[:lay.action_size].astype(np.float64)
            out["action_freq"] = [float(v) for v in freq / imag_rows]
        else:
            _put(out, "action", moments(bh[3 * SEXT:]), full + ("rms",))
    if "critic" in regions and lay.behaviour:
        cr = lay.get(block, "mom_cr")
        _put(out, "critic_value", moments(cr[:SEXT]), ("mean", "std"))
        err = moments(cr[SEXT:])
        if err["nonfinite"] > 0:
            out["nonfinite/value_error"] = err["nonfinite"]
        if ret is not None:
            out["value_explained_variance"] = explained_variance(ret, err)
    for group in REGIONS:
        if group in regions and (group == "model" or lay.behaviour):
            for kind, field in (("grad_norm", "gsq_"), ("weight_norm", "wsq_")):
                for mod, v in zip(lay.modules[group], lay.get(block, field + group)):
                    out[f"{kind}/{mod}"] = float(math.sqrt(v)) if v >= 0 else math.nan
    return out


def scalar_items(logs) -> List[Tuple[str, float]]:
    """The entries of a log dict a one-line printout shows: everything but the list-valued ones."""
    return [(k, v) for k, v in logs.items() if not isinstance(v, (list, tuple))]
