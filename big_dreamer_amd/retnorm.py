"""Device state of the percentile return normalisation ("Return normalisation")."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch


class _ReturnNorm:
    """Device side of the percentile return normalisation ("Return normalisation"), built only when it is on:
    the running range `state` = (lo, hi, count, skipped) in fp64, and `range`, two rows of (scale, lo, hi) in fp32.  A step
    reads row `cur` -- the range as it stood before the step -- and bd_return_range writes the other row for the next
    step, so two steps in flight never share a row.  `ev` is the end of the latest bd_return_range."""

    KEYS = ("lo", "hi", "count", "skipped")

    def __init__(self, eng):
        hp = eng.hp
        self.eng = eng
        self.decay, self.floor = hp["return_norm_decay"], hp["return_norm_floor"]
        self.q = (hp["return_norm_low"], hp["return_norm_high"])
        self.state = torch.zeros(4, dtype=torch.float64, device=eng.dev)
        self.range = torch.zeros(2, 4, dtype=torch.float32, device=eng.dev)
        self.cur = 0
        self.ev: Optional[torch.cuda.Event] = None
        self.load(dict(lo=0.0, hi=0.0, count=0.0, skipped=0.0))

    def ranks(self, M: int) -> Tuple[int, int]:
        """k_q = floor(q (M - 1)), in Python floats."""
        return tuple(int(math.floor(q * (M - 1))) for q in self.q)

    def load(self, d: dict) -> None:
        lo, hi = float(d["lo"]), float(d["hi"])
        self.state.copy_(torch.tensor([lo, hi, float(d["count"]), float(d["skipped"])], dtype=torch.float64))
        row = torch.tensor([max(self.floor, hi - lo), lo, hi, 0.0], dtype=torch.float64).to(torch.float32)
        self.range.copy_(row.expand(2, 4))

    def _join(self) -> None:
        """The engine's join(), and the latest bd_return_range wherever it was queued."""
        self.eng.join()
        if self.ev is not None:
            torch.cuda.current_stream().wait_event(self.ev)

    def state_dict(self) -> dict:
        self._join()
        return dict(zip(self.KEYS, self.state.cpu().tolist()))

    def load_state(self, d: dict) -> None:
        lo, hi, count, skipped = (float(d[k]) for k in self.KEYS)
        if not (math.isfinite(lo) and math.isfinite(hi) and count >= 0 and skipped >= 0):
            raise ValueError(f"load_return_norm_state: not a range state: {d!r}")
        self._join()
        self.load(dict(lo=lo, hi=hi, count=count, skipped=skipped))
        self.ev = torch.cuda.Event()
        self.ev.record(torch.cuda.current_stream())

    def broadcast(self, dp, src: int) -> None:
        """Every rank takes rank `src`'s running range (a collective on the caller's communicator)."""
        self._join()
        self.load(dict(zip(self.KEYS, dp.broadcast_(self.state.clone(), src).cpu().tolist())))
