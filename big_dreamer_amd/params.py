"""Flat parameter / gradient / Adam-moment storage of one optimiser and its torch.optim.Adam state_dict form."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch


class ParamGroup:
    """Flat parameter / gradient / Adam-moment buffers of one optimiser, with named views.

    With `conv_storage`, 4-D (convolution) tensors are STORED permuted (d0, d2, d3, d1) -- Conv2d (co, ky, kx, ci),
    ConvTranspose2d (ci, ky, kx, co): the layout the hand-written conv kernels use as plain [N][K] matrices
    (csrc/conv.hip) -- while `p` / `g` stay views with the reference's logical shape (state_dict, tests); `ps` / `gs`
    are the contiguous storage views.  Clip, Adam and the all-reduce act on the flat buffers and do not care."""

    def __init__(self, specs: List[Tuple[str, str, Tuple[int, ...]]], device, with_opt: bool = True,
                 conv_storage: bool = False):
        self.specs = specs
        # every tensor starts on a 16-byte boundary of the flat buffers (pad floats stay zero: zero gradient, zero Adam
        # update): 16-byte vector loads and LDS-DMA of a weight matrix as it lies in the buffer (csrc/gemm.hip)
        al = lambda k: (k + 3) & ~3
        n = sum(al(int(np.prod(s))) for _, _, s in specs)
        self.numel = n
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.grad = torch.zeros(n, dtype=torch.float32, device=device) if with_opt else None
        self.m = torch.zeros(n, dtype=torch.float32, device=device) if with_opt else None
        self.v = torch.zeros(n, dtype=torch.float32, device=device) if with_opt else None
        self.step = 0
        self.p: Dict[Tuple[str, str], torch.Tensor] = {}
        self.g: Dict[Tuple[str, str], torch.Tensor] = {}
        self.ps: Dict[Tuple[str, str], torch.Tensor] = {}
        self.gs: Dict[Tuple[str, str], torch.Tensor] = {}
        self._layout: Dict[Tuple[str, str], tuple] = {}
        off = 0
        for mod, name, shape in specs:
            k = int(np.prod(shape))
            perm = conv_storage and len(shape) == 4
            sshape = (shape[0], shape[2], shape[3], shape[1]) if perm else shape
            self._layout[(mod, name)] = (off, k, sshape, perm)

            def views(buf):
                st = buf[off:off + k].view(sshape)
                return st, (st.permute(0, 3, 1, 2) if perm else st)

            self.ps[(mod, name)], self.p[(mod, name)] = views(self.flat)
            if with_opt:
                self.gs[(mod, name)], self.g[(mod, name)] = views(self.grad)
            off += al(k)

    def module_segments(self) -> Tuple[List[str], List[int]]:
        """The modules of the group in storage order and the n + 1 element offsets of their contiguous stretches of the flat
        buffers (pad floats belong to the module they follow; the last stretch ends at `numel`)."""
        names: List[str] = []
        offsets: List[int] = []
        for mod, name, _ in self.specs:
            if not names or names[-1] != mod:
                assert mod not in names, f"module {mod} is not contiguous in the flat buffer"
                names.append(mod)
                offsets.append(self._layout[(mod, name)][0])
        return names, offsets + [self.numel]

    def logical(self, buf: torch.Tensor, mod: str, name: str) -> torch.Tensor:
        """View of `buf` (a flat buffer laid out like `flat`: grad, m, v) with the reference's shape of (mod, name)."""
        off, k, sshape, perm = self._layout[(mod, name)]
        st = buf[off:off + k].view(sshape)
        return st.permute(0, 3, 1, 2) if perm else st


def _adam_state_dict(g: ParamGroup, lr: float, hp: dict, over: Optional[dict] = None) -> dict:
    """The group's optimiser state in torch.optim.Adam's state_dict layout (parameter index = reference parameter
    order, moments in the reference's logical shapes), so that the reference's ``model_optimizer.load_state_dict``
    accepts it (src/planet.py:114)."""
    state = {}
    for i, (mod, name, _shape) in enumerate(g.specs):
        state[i] = {"step": torch.tensor(float(g.step)), "exp_avg": g.logical(g.m, mod, name).detach().cpu().clone().contiguous(),
                    "exp_avg_sq": g.logical(g.v, mod, name).detach().cpu().clone().contiguous()}
    over = over or {}
    group = {"lr": over.get("lr", lr), "betas": (0.9, 0.999), "eps": over.get("eps", hp["adam_epsilon"]),
             "weight_decay": over.get("weight_decay", hp["weight_decay"]), "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(g.specs)))}
    return {"state": state, "param_groups": [group]}


def _load_adam_state_dict(g: ParamGroup, sd: dict) -> Optional[dict]:
    """Restore moments + step; returns the checkpoint's param_group hyper-parameters (lr, eps, weight_decay) -- torch's
    ``Optimizer.load_state_dict`` adopts them (src/planet.py:114), so the caller does too."""
    pg = (sd.get("param_groups") or [None])[0]
    hyper = {k: float(pg[k]) for k in ("lr", "eps", "weight_decay") if pg and k in pg} or None
    if pg and tuple(pg.get("betas", (0.9, 0.999))) != (0.9, 0.999):
        raise NotImplementedError(f"Adam betas {pg['betas']} in the checkpoint: the kernels implement (0.9, 0.999), the "
                                  "reference's only setting (src/dreamer.py:56-67)")
    st = sd["state"]
    if not st:                      # a freshly built optimiser: nothing to restore
        g.m.zero_(); g.v.zero_(); g.step = 0
        return hyper
    assert len(st) == len(g.specs), f"optimizer state has {len(st)} parameters, this group {len(g.specs)}"
    steps = set()
    for i, (mod, name, shape) in enumerate(g.specs):
        e = st[i] if i in st else st[str(i)]
        assert tuple(e["exp_avg"].shape) == tuple(shape), (mod, name, tuple(e["exp_avg"].shape), shape)
        g.logical(g.m, mod, name).copy_(e["exp_avg"].to(torch.float32))
        g.logical(g.v, mod, name).copy_(e["exp_avg_sq"].to(torch.float32))
        steps.add(int(float(e["step"])))
    assert len(steps) == 1, f"per-parameter Adam step counts differ: {steps}"
    g.step = steps.pop()
    return hyper
