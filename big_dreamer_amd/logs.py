"""Log records of the train step: the scalar-board slots, the pinned host records lazy log dicts are read from (a ring of
eight) and the formulas from scalar board to the reference's log dict.  No kernel is launched here: the engine passes in
the scalar board, the cluster error word and the diagnostic block."""
from __future__ import annotations

import collections.abc
import math
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import diagnostics

# scalar-board slots (raw sums; see include/bigdreamer_hip.h "losses")
SLOT_OBS, SLOT_REW, SLOT_KL, SLOT_RET, SLOT_ENT, SLOT_VAL, SLOT_GN_MODEL, SLOT_GN_ACTOR, SLOT_GN_CRITIC = range(9)
SLOT_DISC, SLOT_WOBJ = 9, 10       # use_discount=True: Bernoulli loss sum (model phase); weighted actor objective sum
SLOT_RF = 11                       # gradient_mixing in [0, 1): sum of w * log pi(a) * (R - b), the REINFORCE objective
SLOT_RN = 12                       # return_normalization=percentile: the scale, low and high the step used (slots 12..14)
N_SLOTS = 16


class _LogRecord:
    """Pinned host copy of the scalar board of ONE train step, filled by three asynchronous D2H copies (one per
    optimiser phase, each on the stream that wrote the slots) -- reading it never stalls the pipeline streams."""

    ROW = {"model": 0, "actor": 1, "critic": 2}

    def __init__(self):
        self.host = torch.zeros(3, N_SLOTS + 1, dtype=torch.float32).pin_memory()     # last column: cluster error word
        self.events: List[Optional[torch.cuda.Event]] = [None, None, None]
        self.counts: Optional[dict] = None
        self.owner = None          # weakref to the LazyLogs handed to the caller
        self.need = (0, 1, 2)
        # diagnosed steps only: pinned copy of the step's diagnostic block, a region per phase behind the same three events
        self.diag: Optional[torch.Tensor] = None
        self.diag_mem: Optional[torch.Tensor] = None

    def snapshot(self, row: int, scalars: torch.Tensor, error_word: Optional[Callable], diag) -> None:
        """Asynchronous D2H of the scalar board (+ the cluster scan's sticky error word, `error_word()`, + this phase's
        region of the diagnostic block `diag`) into the record, on the current stream, behind the kernels of this phase that
        wrote its slots."""
        self.host[row, :N_SLOTS].copy_(scalars, non_blocking=True)
        if error_word is not None:
            self.host[row, N_SLOTS:].copy_(error_word(), non_blocking=True)
        if self.diag is not None:
            lo, hi = diag.lay.region[diagnostics.REGIONS[row]]
            self.diag[lo:hi].copy_(diag.block[lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self.events[row] = ev

    def read(self) -> Tuple[np.ndarray, int]:
        """Wait for the three copies -> (the board with every slot from the phase that wrote it, the cluster error word)."""
        for row in self.need:
            assert self.events[row] is not None, "log record read before its step was queued"
            self.events[row].synchronize()
        h = self.host.numpy()
        s = h[0, :N_SLOTS].copy()
        for slot in (SLOT_RET, SLOT_ENT, SLOT_GN_ACTOR, SLOT_WOBJ, SLOT_RF, SLOT_RN, SLOT_RN + 1, SLOT_RN + 2):
            s[slot] = h[1, slot]
        for slot in (SLOT_VAL, SLOT_GN_CRITIC):
            s[slot] = h[2, slot]
        return s, int(h[0, N_SLOTS:].view(np.uint32)[0])


class LazyLogs(collections.abc.MutableMapping):
    """The reference's log dict (src/dreamer.py:293-296,359-360,383), resolved on first read.

    ``Dreamer.train_step`` returns one per step; nothing synchronises until a key is read, so the reference loop's
    ``for _ in range(collect_interval): logs = model.train_step()`` (src/main.py:105-108) runs the cross-step pipeline
    and only the burst's last dict -- the one the loop reads -- waits for the GPU.  Keys and values are exactly those
    of the eager dict; extra keys may be written (``logs["weight_update_per_sec"] = ...``, src/main.py:108)."""

    def __init__(self, resolve: Callable[[_LogRecord], Dict[str, float]], rec: _LogRecord, drop_prefix: Tuple[str, ...] = ()):
        self._resolve, self._rec, self._drop = resolve, rec, drop_prefix
        self._vals: Optional[Dict[str, float]] = None
        self._extra: Dict[str, object] = {}

    def resolve(self) -> Dict[str, float]:
        if self._vals is None:
            vals = self._resolve(self._rec)
            self._vals = {k: v for k, v in vals.items() if not k.startswith(self._drop)} if self._drop else vals
            self._rec = None
        return self._vals

    def __getitem__(self, k):
        return self._extra[k] if k in self._extra else self.resolve()[k]

    def __setitem__(self, k, v):
        self._extra[k] = v

    def __delitem__(self, k):
        del self._extra[k]

    def __iter__(self):
        yield from self.resolve()
        yield from (k for k in self._extra if k not in self._vals)

    def __len__(self):
        return len(set(self.resolve()) | set(self._extra))

    def __repr__(self):
        return repr(dict(self.items()))


class LogRing:
    """The records of lazily read steps, a ring of eight, and `cur`: the record of the step being queued."""

    def __init__(self):
        self._ring: List[_LogRecord] = []
        self._i = 0
        self.cur: Optional[_LogRecord] = None

    def new_record(self, diag) -> _LogRecord:
        """Next record of the ring; a record still referenced by an unread LazyLogs is resolved first.  `diag`: the
        diagnostics of a diagnosed step, else None."""
        if len(self._ring) < 8:
            self._ring.append(_LogRecord())
            rec = self._ring[-1]
        else:
            rec = self._ring[self._i]
            self._i = (self._i + 1) % 8
            owner = rec.owner() if rec.owner is not None else None
            if owner is not None and owner._vals is None:
                owner.resolve()
        rec.events = [None, None, None]
        rec.owner, rec.counts = None, None
        rec.diag = None
        if diag is not None:
            if rec.diag_mem is None or rec.diag_mem.numel() != diag.lay.size:
                rec.diag_mem = torch.zeros(diag.lay.size, dtype=torch.float64).pin_memory()
            rec.diag = rec.diag_mem
        return rec


def logs_from(s: np.ndarray, c: dict, hp: dict, world_size: int, use_discount: bool, mix: Optional[float],
              return_norm: bool) -> Dict[str, float]:
    """Scalar board `s` (N_SLOTS raw sums) and counts `c` (N, Mi, S, sum_form) -> the reference's log dict
    (src/dreamer.py:293-296,359-360,383), fp32 arithmetic as in the reference.  mix: gradient_mixing rho where it changes
    the objective (0 <= rho < 1), else None; return_norm: percentile return normalisation is on."""
    f32 = np.float32
    N, Mi = f32(c["N"]), f32(c["Mi"])
    obs, rew = s[SLOT_OBS] / N, s[SLOT_REW] / N
    if c["sum_form"]:
        kl = s[SLOT_KL] / N
    else:
        mean = s[SLOT_KL] / f32(c["N"] * c["S"] * world_size)
        x = np.maximum(mean, f32(hp["free_nats"]))
        kl = f32(hp["kl_balance"]) * x + f32(1 - hp["kl_balance"]) * x
    ew = f32(hp["entropy_weight"]) if hp["entropy_weight"] != -1 else f32(0)
    model_loss = obs + rew + kl * f32(hp["kl_loss_weight"])
    # return normalisation: the return terms over the scale the step used; the entropy term is not divided
    scale = s[SLOT_RN] if return_norm and s[SLOT_RN] > 0 else f32(1)      # (0: no behaviour phase has run)
    if mix is None:
        objective = s[SLOT_RET] / scale + ew * s[SLOT_ENT]
    else:           # w (rho R + (1 - rho) log pi(a) sg(R - b) + eta H), summed ("Mixed actor gradient")
        objective = (f32(mix) * s[SLOT_RET] + f32(1 - mix) * s[SLOT_RF]) / scale + ew * s[SLOT_ENT]
    out = {}
    if use_discount:         # src/dreamer.py:287-290, 346-352
        disc = s[SLOT_DISC] / N
        model_loss = model_loss + disc * f32(hp["discount_weight"])
        out["discount_loss"] = float(disc)
        objective = s[SLOT_WOBJ] if mix is None else s[SLOT_WOBJ] + f32(1 - mix) * s[SLOT_RF] / scale
    out.update({
        "observation_loss": float(obs), "reward_loss": float(rew), "kl_loss": float(kl),
        "model_loss": float(model_loss),
        "actor_loss": float(-objective / Mi),
        "policy_entropy": float(s[SLOT_ENT] / Mi),
        "value_loss": float(s[SLOT_VAL] / Mi),
        "grad_norm_model": float(math.sqrt(s[SLOT_GN_MODEL])), "grad_norm_actor": float(math.sqrt(s[SLOT_GN_ACTOR])),
        "grad_norm_critic": float(math.sqrt(s[SLOT_GN_CRITIC])),
    })
    if return_norm:
        out.update(return_scale=float(s[SLOT_RN]), return_p_low=float(s[SLOT_RN + 1]), return_p_high=float(s[SLOT_RN + 2]))
    return out
