"""References for cnn_activation_function (ELU / ReLU / Tanh in the pixel conv stacks).  Plain helpers, not a conftest.

The CPU oracle (oracle/dreamer_oracle.py) writes ELU into its two conv stacks.  ``oracle_cnn_act`` swaps those two
functions for the ones below -- plain torch.nn.functional calls with the activation as an argument -- for the duration of a
``with`` block, so the rest of the oracle's train step (RSSM, heads, Adam) runs unchanged around them.  ``oracle64``
lifts an OracleDreamer to float64.  Golden files of the two new activations come from the reference itself
(tests/gen_golden_cnn_act.py).
"""
from __future__ import annotations

import contextlib
import dataclasses

import numpy as np
import torch
import torch.nn.functional as F

from big_dreamer_amd import synth
from tests.dense_ref import C_TOL

# name -> (Dims, seed, golden file); the seeds of the two new files are chosen by tests/gen_golden_cnn_act.py --search
# (ReLU: no conv pre-activation of the two train steps within its fp32 bound of 0, tests/test_cnn_activation_cpu.py)
CNN_ACT_CASES = {
    "ELU": (synth.TINY_PIXEL, 4, "tiny_pixel"),
    "ReLU": (dataclasses.replace(synth.TINY_PIXEL, cnn_act="ReLU"), 91, "tiny_pixel_relu"),
    "Tanh": (dataclasses.replace(synth.TINY_PIXEL, cnn_act="Tanh"), 22, "tiny_pixel_tanh"),
}


def act64(name: str, x: torch.Tensor) -> torch.Tensor:
    if name == "ELU":
        return torch.where(x > 0, x, torch.expm1(x))
    if name == "ReLU":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if name == "Tanh":
        return torch.tanh(x)
    assert name == "none", name
    return x


def act_grad_from_out64(name: str, y: torch.Tensor) -> torch.Tensor:
    """f'(x) through the saved output y = f(x), as the kernels take it (csrc/bd_device.h)."""
    y = y.double()
    if name == "ELU":
        return torch.where(y > 0, torch.ones_like(y), y + 1.0)
    if name == "ReLU":
        return torch.where(y > 0, torch.ones_like(y), torch.zeros_like(y))
    if name == "Tanh":
        return 1.0 - y * y
    assert name == "none", name
    return torch.ones_like(y)


def _act(name: str, x: torch.Tensor) -> torch.Tensor:
    return {"ELU": F.elu, "ReLU": F.relu, "Tanh": torch.tanh}[name](x)


def make_stacks(act: str, record=None):
    """(cnn_encoder, cnn_decoder) with the oracle's signatures.  record(tag, pre, S): every conv pre-activation and the
    contraction of the absolute operands sum|a*b| (bias included) behind it, detached."""

    def conv(x, w, b, tag):
        pre = F.conv2d(x, w, b, stride=2)
        if record is not None:
            with torch.no_grad():
                record(tag, pre.detach(), F.conv2d(x.abs(), w.abs(), b.abs(), stride=2))
        return pre

    def convT(x, w, b, tag, rec=True):
        pre = F.conv_transpose2d(x, w, b, stride=2)
        if record is not None and rec:
            with torch.no_grad():
                record(tag, pre.detach(), F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2))
        return pre

    def cnn_encoder(obs, sd):
        lead = obs.shape[:-3]
        x = obs.reshape(-1, *obs.shape[-3:])
        for i in range(4):
            x = _act(act, conv(x, sd[f"model.{2 * i}.weight"], sd[f"model.{2 * i}.bias"], f"encoder.model.{2 * i}"))
        x = x.flatten(1)
        if "model.9.weight" in sd:
            x = F.linear(x, sd["model.9.weight"], sd["model.9.bias"])
        return x.reshape(*lead, -1)

    def cnn_decoder(belief, state, sd):
        lead = belief.shape[:-1]
        x = F.linear(torch.cat([belief, state], dim=-1), sd["decoder.0.weight"], sd["decoder.0.bias"])
        x = x.reshape(-1, x.shape[-1], 1, 1)
        for idx in (2, 4, 6, 8):
            x = convT(x, sd[f"decoder.{idx}.weight"], sd[f"decoder.{idx}.bias"], f"decoder.{idx}", rec=idx != 8)
            if idx != 8:
                x = _act(act, x)
        return x.reshape(*lead, 3, 64, 64)

    return cnn_encoder, cnn_decoder


@contextlib.contextmanager
def oracle_cnn_act(act: str, record=None, float64: bool = False):
    """The oracle module with its conv stacks on `act` (and, float64=True, its fresh tensors in float64)."""
    from oracle import dreamer_oracle as O
    saved = O.cnn_encoder, O.cnn_decoder, torch.get_default_dtype()
    O.cnn_encoder, O.cnn_decoder = make_stacks(act, record)
    if float64:
        torch.set_default_dtype(torch.float64)
    try:
        yield O
    finally:
        O.cnn_encoder, O.cnn_decoder = saved[0], saved[1]
        torch.set_default_dtype(saved[2])


def oracle64(od) -> None:
    """Lift an OracleDreamer's parameters and Adam state to float64 in place."""
    from oracle import dreamer_oracle as O
    od.P = {mod: {k: v.detach().double().requires_grad_(mod != "critic_target") for k, v in sd.items()}
            for mod, sd in od.P.items()}
    od.model_params = [p for mod in od.model_modules for p in od.P[mod].values()]
    od.actor_params = list(od.P["actor"].values())
    od.critic_params = list(od.P["critic"].values())
    od.opt = {"model": O.AdamState(od.model_params), "actor": O.AdamState(od.actor_params),
              "critic": O.AdamState(od.critic_params)}


def to64(dct):
    return {k: np.asarray(v, dtype=np.float64) for k, v in dct.items()}


def conv_margins(act: str, d: synth.Dims, seed: int):
    """Two train steps of the float64 oracle with the conv stacks on `act`.  Returns (count, smallest |pre| / m, total,
    logs per step, with the conv stacks' post-Adam weights): count = conv pre-activations with |pre| <= m, m = C_TOL * sum|a*b| the fp32 bound of that contraction."""
    from oracle import dreamer_oracle  # noqa: F401  (imported by oracle_cnn_act)
    stats = {"count": 0, "ratio": float("inf"), "total": 0}

    def record(tag, pre, S):
        m = C_TOL * S
        stats["count"] += int((pre.abs() <= m).sum())
        stats["ratio"] = min(stats["ratio"], float((pre.abs() / m).min()))
        stats["total"] += pre.numel()

    P = synth.make_params(d, seed)
    batch = to64(synth.make_batch(d, seed))
    logs = []
    with oracle_cnn_act(act, record, float64=True) as O:
        od = O.OracleDreamer(P, dict(planning_horizon=d.H))
        oracle64(od)
        for step in range(2):
            log = od.train_step(batch, to64(synth.make_noise(d, seed + step)), keep=False)
            # post-Adam weights of the two conv stacks ride along under "param.<module>.<name>"
            log.update({f"param.{mod}.{k}": v.detach().numpy().copy() for mod in ("encoder", "observation_model")
                        for k, v in od.P[mod].items()})
            logs.append(log)
            if step == 0:
                od.update_critic()
    return stats["count"], stats["ratio"], stats["total"], logs
