"""Evaluation episodes (src/main.py:191-283): `n` environments side by side, no exploration noise, the returns'
min / avg / max / std -- and for pixel agents the real-vs-predicted video, assembled on the device one launch per decision
(bd_eval_frame, csrc/video.hip) and copied to the host once.

``run_evaluation`` needs only ``update_belief_and_act``, ``device``, ``belief_size``, ``state_size``, ``action_size``,
``eval()`` / ``train()`` of the agent (and ``engine.eval_frame`` for the video), so a stub drives it on the CPU."""
from __future__ import annotations

from typing import Any, Callable, Dict, Optional, Tuple

import numpy as np
import torch

TILE_H, TILE_W, GRID_COLS, GRID_PAD = 64, 128, 5, 2     # a tile: real | predicted, 3 x 64 x 128; make_grid(nrow=5, padding=2)


def frame_shape(n: int) -> Tuple[int, int, int]:
    """(3, GH, GW) of one video frame of `n` environments: the tile itself for n == 1 (make_grid leaves a single image as
    it is), else the padded grid, five tiles per row."""
    if n == 1:
        return 3, TILE_H, TILE_W
    xmaps = min(GRID_COLS, n)
    ymaps = -(-n // xmaps)
    return 3, ymaps * (TILE_H + GRID_PAD) + GRID_PAD, xmaps * (TILE_W + GRID_PAD) + GRID_PAD


@torch.no_grad()
def run_evaluation(agent, envs, max_steps: int, video: bool = False,
                   _noise: Optional[Callable[[int], Dict[str, torch.Tensor]]] = None, action_mode: str = "sample",
                   state_mean: bool = False) -> Dict[str, Any]:
    """The reference's test loop (src/main.py:199-272) on `envs` (an EnvBatcher): at most `max_steps` decisions from the
    zero belief / state / action, ``explore=False``, stopping once every environment is done.  `_noise(step)` (parity
    tests) is handed to ``update_belief_and_act`` as its ``_noise``; None passes no such keyword (Planet has none).
    `action_mode` ("sample", "mode", "mean") and `state_mean` are the evaluation policy (Dreamer.update_belief_and_act);
    they are passed on only when they differ from the defaults, so a Planet or a stub without them evaluates as before.
    Returns Eval_{min,avg,max,std}_return (floats; std is the population std), ``returns`` (n,), ``steps`` and ``video``:
    uint8 (steps, 3, GH, GW) -- frame t pairs the observations decision t consumed with the reconstruction from the belief
    and posterior it produced -- or None."""
    from .config import ACTION_MODES
    if action_mode not in ACTION_MODES:
        raise ValueError(f"action_mode {action_mode!r} is none of {ACTION_MODES}")
    n, dev = envs.n, agent.device
    policy = {} if (action_mode == "sample" and not state_mean) else {"action_mode": action_mode, "state_mean": bool(state_mean)}
    agent.eval()
    observation = envs.reset()
    total = np.zeros((n,))
    belief = torch.zeros(n, agent.belief_size, device=dev)
    posterior_state = torch.zeros(n, agent.state_size, device=dev)      # (Categorical latents: dimensions * classes)
    action = torch.zeros(n, agent.action_size, device=dev)
    frames = torch.empty((max_steps,) + frame_shape(n), dtype=torch.uint8, device=dev) if video else None
    steps = 0
    for t in range(max_steps):
        observation = observation.to(device=dev)       # the one upload: the encoder and the frame kernel both read it
        kw = dict(policy) if _noise is None else dict(policy, _noise=_noise(t))
        belief, posterior_state, action, next_observation, reward, done = agent.update_belief_and_act(
            envs, belief, posterior_state, action, observation, explore=False, **kw)
        total += reward.numpy()
        if video:
            agent.engine.eval_frame(observation, belief, posterior_state, frames, t)
        observation = next_observation
        steps = t + 1
        if done.sum().item() == n:
            break
    envs.close()
    agent.train()
    return {"Eval_min_return": total.min().item(), "Eval_avg_return": total.mean().item(),
            "Eval_max_return": total.max().item(), "Eval_std_return": total.std().item(),
            "returns": total, "steps": steps, "video": frames[:steps].cpu().numpy() if video else None}
