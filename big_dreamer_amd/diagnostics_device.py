"""Device side of the training diagnostics ("Training diagnostics"); diagnostics.py, the layout and the
entries of the log dict, stays free of the HIP library."""
from __future__ import annotations

import ctypes as C

import torch

from . import _cabi as cabi
from . import diagnostics
from .params import ParamGroup

lib = cabi.lib
ptr = cabi.ptr


class _Diagnostics:
    """Device side of the training diagnostics ("Training diagnostics"), built when the interval is first set
    above 0: the diagnostic block (diagnostics.Layout), one reduction workspace per phase stream, and the per-module
    segment tables of the three optimisers' flat buffers."""

    def __init__(self, eng):
        d = eng.d
        segs = {g: eng.groups[g].module_segments() for g in diagnostics.REGIONS}
        self.lay = diagnostics.Layout(d.categorical, d.cat_D if d.categorical else d.S, d.cat_C, True, d.discrete_actions,
                                      d.A, {g: names for g, (names, _) in segs.items()})
        self.block = torch.zeros(self.lay.size, dtype=torch.float64, device=eng.dev)
        n_ws = int(lib.bd_diag_ws_floats())
        self.ws = {g: torch.zeros(n_ws, dtype=torch.float32, device=eng.dev) for g in diagnostics.REGIONS}
        self.offsets = {g: (C.c_size_t * len(offs))(*offs) for g, (_, offs) in segs.items()}
        self.n_seg = {g: len(names) for g, (names, _) in segs.items()}
        self.colsum_ws = (torch.zeros(int(lib.bd_colsum_ws_floats(d.A)), dtype=torch.float32, device=eng.dev)
                          if d.discrete_actions else None)

    def at(self, field: str, word: int = 0) -> int:
        """Device address of double `word` of a field of the block."""
        return self.block.data_ptr() + 8 * (self.lay.fields[field][0] + word)

    def moments(self, group: str, field: str, entries) -> None:
        """One bd_moments launch on the current stream: entries = [(p, q or None), ...] -> consecutive sextuples of `field`."""
        a = cabi.MomentsArgs()
        a.n_buf = len(entries)
        for i, (p, q) in enumerate(entries):
            a.buf[i].p, a.buf[i].q, a.buf[i].n = ptr(p), ptr(q), p.numel()
        cabi.check(lib.bd_moments(C.byref(a), self.at(field), ptr(self.ws[group]), cabi.stream()))

    def norms(self, group: str, g: ParamGroup) -> None:
        """Per-module sums of squares of the group's gradient and weights, on the current stream."""
        for field, buf in (("gsq_", g.grad), ("wsq_", g.flat)):
            cabi.check(lib.bd_segment_sumsq(ptr(buf), self.n_seg[group], self.offsets[group], self.at(field + group),
                                            ptr(self.ws[group]), cabi.stream()))
