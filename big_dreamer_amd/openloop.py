"""Open-loop prediction (DreamerV1's image_summaries, DreamerV2's video_pred): filter a few replay sequences on a short
context, roll the PRIOR forward from there on the recorded actions alone, decode every step, and compare with what was
recorded -- as an error curve over the prediction horizon and, for pixel agents, as a truth / model / error video assembled on
the device (bd_openl_video, bd_openl_error; csrc/video.hip) and copied to the host once.

``run_open_loop`` needs only ``encoder``, ``transition_model``, ``observation_model``, ``device``, ``belief_size``,
``state_size``, ``eval()`` / ``train()`` and ``engine.openl_video`` / ``engine.openl_error`` of the agent, so a stub drives it
on the CPU."""
from __future__ import annotations

from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

IMG, BANDS = 64, 3           # a column block: 64 wide; truth over model over error, 64 rows each


def video_shape(T: int, n: int) -> Tuple[int, int, int, int]:
    """(T, 3, 192, 64 n) of the open-loop video of `n` sequences over `T` steps: frame t, columns 64 k .. 64 k + 63 hold
    sequence k -- rows 0-63 the truth, 64-127 the model, 128-191 the error; no padding."""
    return int(T), 3, BANDS * IMG, IMG * int(n)


def check_open_loop(seq_len: int, n: int, context: int) -> None:
    """A batch of `n` sequences of `seq_len` records gives T = seq_len - 1 steps, of which `context` are filtered and at
    least one is predicted: seq_len >= 3, 1 <= context <= seq_len - 2, n >= 1."""
    if seq_len < 3:
        raise ValueError(f"open_loop: seq_len must be at least 3 (one context step and one open-loop step), got {seq_len}")
    if not 1 <= context <= seq_len - 2:
        raise ValueError(f"open_loop: context must be in [1, seq_len - 2] = [1, {seq_len - 2}], got {context}")
    if n < 1:
        raise ValueError(f"open_loop: at least one sequence, got {n}")


@torch.no_grad()
def run_open_loop(agent, batch: Sequence[torch.Tensor], context: int, video: Optional[bool] = None,
                  _noise: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, Any]:
    """`batch`: time-major [obs (L, n, ...), actions (L, n, A), rewards, nonterminals (L, n, 1)] as ExperienceReplay.sample
    returns it.  With T = L - 1 and c = `context`, in the train step's convention (step t consumes actions[t] and
    nonterminals[t] and predicts obs[t + 1]):
      context    transition_model(0, actions[:c], 0, encoder(obs[1:c+1]), nonterminals[:c]) -> beliefs b[0:c], POSTERIOR
                 states s[0:c];
      open loop  transition_model(s[c-1], actions[c:T], b[c-1], None, nonterminals[c:T]) -> b[c:T], sampled PRIOR states s[c:T];
      decode     model[t] = observation_model(b[t], s[t]), all T n rows in one pass; truth[t] = obs[t + 1].
    With ``symlog_observations`` the world model lives in symlog(obs) space: the context is filtered on
    ``agent.encoder_input(obs)`` = symlog(obs), and the decoder's output goes through bd_symexp before the error, so the curve
    stays in observation units and is comparable across settings.
    `_noise` (tests): {"post": (c, n, S), "prior": (T - c, n, S)} -- standard normals, or Exp(1) variates for Categorical
    latents -- in place of the draws the two forward calls make.  `video`: None = for pixel observations; state observations
    have none.  Returns ``openl_obs_mse`` (T,) float32 -- per step the mean of (model - truth)^2 over the sequences and all
    observation elements --, ``openl_mse_context`` / ``openl_mse_open`` (its means over steps < c and >= c), ``context``,
    ``video`` (uint8 ``video_shape(T, n)`` or None) and the device tensors ``beliefs`` (T, n, Be) and ``states`` (T, n, S)
    that were decoded."""
    dev = agent.device
    obs, actions, _, nonterminals = (x.to(dev) for x in batch)
    L, n = int(actions.shape[0]), int(actions.shape[1])
    check_open_loop(L, n, context)
    T, c = L - 1, int(context)
    pixel = obs.dim() == 5
    want_video = pixel and (video is None or bool(video))
    agent.eval()
    symlog = bool(getattr(agent, "symlog_observations", False))     # the world model lives in symlog(obs) space
    embedding = agent.encoder(agent.encoder_input(obs[1:c + 1]) if symlog else obs[1:c + 1])
    kw_post = {} if _noise is None else {"_noise": (_noise["post"], _noise["post"])}     # (unused prior draw, posterior draw)
    kw_prior = {} if _noise is None else {"_noise": (_noise["prior"],)}
    b_ctx, _, _, s_ctx, _ = agent.transition_model(torch.zeros(n, agent.state_size, device=dev), actions[:c],
                                                   torch.zeros(n, agent.belief_size, device=dev), embedding,
                                                   nonterminals[:c], **kw_post)
    b_open, s_open, _, _, _ = agent.transition_model(s_ctx[c - 1], actions[c:T], b_ctx[c - 1], None, nonterminals[c:T],
                                                     **kw_prior)
    beliefs, states = torch.cat([b_ctx, b_open], dim=0), torch.cat([s_ctx, s_open], dim=0)
    truth = obs[1:]
    frames = None
    if pixel:       # decode once: both kernels read the conv stack's own NHWC buffer
        feat = torch.cat([beliefs, states], dim=-1).reshape(T * n, -1)
        frames = torch.empty(video_shape(T, n), dtype=torch.uint8, device=dev) if want_video else None
        model = agent.engine.openl_video(truth, feat, frames)
        curve = agent.engine.openl_error(truth, model, T, n, 3 * IMG * IMG, True)
    else:
        model = agent.observation_model(beliefs, states)
        if symlog:          # back to observation units: the curve stays comparable across settings
            model = model.contiguous()
            model = agent.engine.symexp(model, torch.empty_like(model))
        curve = agent.engine.openl_error(truth, model, T, n, int(model.shape[-1]), False)
    agent.train()
    curve = curve.cpu().numpy().astype(np.float32, copy=False)
    return {"openl_obs_mse": curve, "openl_mse_context": float(curve[:c].mean()), "openl_mse_open": float(curve[c:].mean()),
            "context": c, "video": None if frames is None else frames.cpu().numpy(), "beliefs": beliefs, "states": states}
