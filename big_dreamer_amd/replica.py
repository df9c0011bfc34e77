"""The replica watch of the data-parallel engine ("Replica agreement").  The data-parallel step is exact only
while every rank holds bit-identical weights, Adam moments and step counts; one bd_fingerprint launch reduces each flat
buffer to a 64-bit word (and a count of non-finite elements) on the device, one small MAX all-reduce compares the words."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _cabi as cabi
from .config import check_replica_options

lib = cabi.lib


class ReplicaMismatch(RuntimeError):
    """Data-parallel replicas no longer hold bit-identical weights, Adam moments or step counts."""


class _ReplicaVerdict:
    """One periodic replica check in flight: pinned host memory for the step counts going up and the verdict coming
    down, and the event behind the D2H copy."""

    def __init__(self, n_buf: int):
        self.steps = torch.zeros(3, dtype=torch.int64).pin_memory()
        self.host = torch.zeros(2 * (2 * n_buf + 3), dtype=torch.int64).pin_memory()     # max | min over ranks of the words
        self.event: Optional[torch.cuda.Event] = None
        self.step = 0
        self.collective = False


class ReplicaWatch:
    """Fingerprint, agreement check and resync of one engine's replicas, and the periodic check of its train_step.
    Nothing but the two options is touched while `interval` is 0.  set, fingerprint, check, sync and resolve are
    documented on the engine methods that forward to them."""

    _FP_BUFFERS = tuple((g, b) for g in ("model", "actor", "critic") for b in ("flat", "m", "v")) + (("critic_target", "flat"),)
    _STEP_GROUPS = ("model", "actor", "critic")

    def __init__(self, eng, interval: int = 0, on_mismatch: str = "raise"):
        self.eng = eng
        self.set(interval, on_mismatch)
        self._fp: Optional[tuple] = None                     # (buffer names, bd_fingerprint argument block)
        self._checks_out: List[_ReplicaVerdict] = []         # issued, not yet read; oldest first
        self._check_pool: List[_ReplicaVerdict] = []
        self._ev_fp: Optional[torch.cuda.Event] = None       # end of the latest periodic fingerprint
        self._fp_wait: set = set()                           # optimisers that have not yet been ordered behind it
        self._resync_warned = False

    def set(self, interval: int = 0, on_mismatch: str = "raise") -> None:
        self.interval, self.on_mismatch = check_replica_options(interval, on_mismatch)

    def _fp_table(self):
        if self._fp is None:
            a = cabi.FingerprintArgs()
            a.n_buf = len(self._FP_BUFFERS)
            for i, (g, b) in enumerate(self._FP_BUFFERS):
                t = getattr(self.eng.groups[g], b)
                a.buf[i].p, a.buf[i].n = t.data_ptr(), t.numel()
            self._fp = (self._FP_BUFFERS, a)
        return self._fp

    def _fingerprint_into(self, out: torch.Tensor) -> None:
        """ONE launch over every flat buffer, on the current stream."""
        cabi.check(lib.bd_fingerprint(C.byref(self._fp_table()[1]), out.data_ptr(), cabi.stream()))

    def fingerprint(self):
        eng = self.eng
        eng.flush_optimizers()
        eng.join()
        names = self._fp_table()[0]
        out = torch.empty(len(names), 2, dtype=torch.int64, device=eng.dev)
        self._fingerprint_into(out)
        return out, list(names)

    def _replica_words(self, fp: torch.Tensor, steps: torch.Tensor) -> torch.Tensor:
        """What the ranks compare: the hashes, the three Adam step counts, then the non-finite counts (whose maximum over
        ranks tells every rank about a NaN on any).  Not the Philox key or counters: they differ per rank by design."""
        return torch.cat([fp[:, 0], steps, fp[:, 1]])

    def _replica_names(self) -> List[str]:
        return [f"{g}.{b}" for g, b in self._FP_BUFFERS] + [f"{g}.step" for g in self._STEP_GROUPS]

    def _read_verdict(self, hi: np.ndarray, lo: np.ndarray) -> dict:
        n, names = len(self._FP_BUFFERS), self._replica_names()
        mismatch = [names[i] for i in range(n + 3) if hi[i] != lo[i]]
        nonfinite = {names[i]: int(hi[n + 3 + i]) for i in range(n) if hi[n + 3 + i] != 0}
        return {"agree": not mismatch, "mismatch": mismatch, "nonfinite": nonfinite}

    def check(self) -> dict:
        eng = self.eng
        self.resolve()
        fp, _ = self.fingerprint()
        steps = torch.tensor([eng.groups[g].step for g in self._STEP_GROUPS], dtype=torch.int64, device=eng.dev)
        hi, lo = eng.dp.max_min_(self._replica_words(fp, steps))
        return self._read_verdict(hi.cpu().numpy(), lo.cpu().numpy())

    def sync(self, src: int = 0) -> None:
        eng = self.eng
        self.resolve()
        eng.flush_optimizers()
        eng.join()
        if eng.world_size > 1:
            for g, b in self._FP_BUFFERS:
                eng.dp.broadcast_(getattr(eng.groups[g], b), src)
            keys = ("lr", "eps", "weight_decay")
            meta = [float(eng.groups[g].step) for g in self._STEP_GROUPS]
            for g in self._STEP_GROUPS:
                ov = eng._opt_over.get(g) or {}
                meta += [x for k in keys for x in (float(k in ov), float(ov.get(k, 0.0)))]
            meta = eng.dp.broadcast_(torch.tensor(meta, dtype=torch.float64, device=eng.dev), src).cpu().tolist()
            for i, g in enumerate(self._STEP_GROUPS):
                eng.groups[g].step = int(meta[i])
                part = meta[3 + 6 * i:9 + 6 * i]
                ov = {k: part[2 * j + 1] for j, k in enumerate(keys) if part[2 * j]}
                if ov:
                    eng._opt_over[g] = ov
                else:
                    eng._opt_over.pop(g, None)
        for g in ("model", "actor", "critic", "critic_target"):
            eng.pack(g)
        if eng._rn is not None and eng.world_size > 1:      # each rank's own shard's range until now
            eng._rn.broadcast(eng.dp, src)
        torch.cuda.current_stream().synchronize()

    def due(self) -> bool:
        """Is this train step one that issues the periodic check?  If so, first read the verdicts train_step has not read
        (without the host throttle nothing else reads them), on the caller's stream: "resync" is a collective there."""
        eng, k = self.eng, self.interval
        if k <= 0 or eng._n_train_steps % k:
            return False
        if self._checks_out:
            throttled = eng.pipeline and eng.host_ahead > 0
            self.resolve(eng._n_train_steps - eng.host_ahead if throttled else None)
        return True

    def enqueue(self) -> None:
        """Fingerprint + agree + asynchronous D2H of the verdict, on the current stream, which the caller has ordered behind
        the optimiser steps issued so far.  One rank: the fingerprint alone (the NaN watch), no collective."""
        eng, n = self.eng, len(self._FP_BUFFERS)
        rec = self._check_pool.pop() if self._check_pool else _ReplicaVerdict(n)
        rec.step, rec.collective = eng._n_train_steps, eng.world_size > 1 or eng.dp.force
        fp = torch.empty(n, 2, dtype=torch.int64, device=eng.dev)
        self._fingerprint_into(fp)
        self._ev_fp = torch.cuda.Event()
        self._ev_fp.record(torch.cuda.current_stream())
        self._fp_wait = set(self._STEP_GROUPS)
        if rec.collective:
            for i, g in enumerate(self._STEP_GROUPS):
                rec.steps[i] = eng.groups[g].step
            steps = rec.steps.to(eng.dev, non_blocking=True)
            # the critic's communicator, from the critic's stream: behind the critic all-reduce of the previous step and
            # before this step's, never in front of a KL / world-model collective
            hi, lo = eng.dp.max_min_(self._replica_words(fp, steps), "critic")
            rec.host.copy_(torch.cat([hi, lo]), non_blocking=True)
        else:
            rec.host[:2 * n].copy_(fp.view(-1), non_blocking=True)
        rec.event = torch.cuda.Event()
        rec.event.record(torch.cuda.current_stream())
        self._checks_out.append(rec)

    def order_write(self, group: str) -> None:
        """Order this optimiser's write, about to be queued on the current stream, behind the latest periodic fingerprint,
        which read the group's buffers on another stream."""
        if group in self._fp_wait:
            self._fp_wait.discard(group)
            torch.cuda.current_stream().wait_event(self._ev_fp)

    def resolve(self, upto: Optional[int] = None) -> None:
        while self._checks_out and (upto is None or self._checks_out[0].step <= upto):
            rec = self._checks_out.pop(0)
            rec.event.synchronize()
            h, n = rec.host.numpy(), len(self._FP_BUFFERS)
            if rec.collective:
                v = self._read_verdict(h[:2 * n + 3].copy(), h[2 * n + 3:].copy())
            else:
                names = self._replica_names()
                v = {"mismatch": [], "nonfinite": {names[i]: int(h[2 * i + 1]) for i in range(n) if h[2 * i + 1] != 0}}
            self._check_pool.append(rec)
            if v["nonfinite"]:       # under both policies: copying NaNs around repairs nothing
                raise FloatingPointError(f"replica check at train step {rec.step}: non-finite values in "
                                         + ", ".join(f"{k} ({c})" for k, c in v["nonfinite"].items()))
            if v["mismatch"]:
                text = (f"replica check at train step {rec.step}: the ranks differ in " + ", ".join(v["mismatch"])
                        + " (data-parallel replicas must be bit-identical)")
                if self.on_mismatch == "raise":
                    raise ReplicaMismatch(text)
                if not self._resync_warned:
                    import warnings
                    warnings.warn(text + ": broadcasting rank 0's state (replica_on_mismatch='resync')")
                    self._resync_warned = True
                for r in self._checks_out:           # issued before the repair: stale
                    r.event.synchronize()
                self._check_pool += self._checks_out
                self._checks_out = []
                self.sync(0)
