"""Plain helpers of the evaluation tests (tests/test_evaluate_cpu.py, tests/test_evaluate_gpu.py, tests/gen_golden_eval.py):
a numpy restatement of the video frame (bd_eval_frame, csrc/video.hip), a scripted environment class for EnvBatcher, and a
stub agent with the surface evaluate.run_evaluation asks for.  Nothing here imports the package under test."""
import numpy as np
import torch


# ---- the frame: make_grid(cat([obs, dec], dim=3) + 0.5, nrow=5) as bytes --------------------------------------------------
def quantise(v):
    """postprocess_observation(v, 8) (src/utils.py:320-337): uint8(clip(floor((v + 0.5) * 256), 0, 255)), fp32 arithmetic."""
    v = np.asarray(v, dtype=np.float32)
    return np.clip(np.floor((v + np.float32(0.5)) * np.float32(256.0)), 0, 255).astype(np.uint8)


def frame_geometry(n):
    """(GH, GW, [(row, column) of tile k's top-left pixel])."""
    if n == 1:
        return 64, 128, [(0, 0)]
    xmaps = min(5, n)
    ymaps = (n + xmaps - 1) // xmaps
    return ymaps * 66 + 2, xmaps * 130 + 2, [((k // xmaps) * 66 + 2, (k % xmaps) * 130 + 2) for k in range(n)]


def frame_reference(obs, dec):
    """obs, dec: (n, 3, 64, 64) float32, NCHW both -> uint8 (3, GH, GW).  Tile k: obs[k] in columns 0-63, dec[k] in 64-127."""
    obs, dec = np.asarray(obs, dtype=np.float32), np.asarray(dec, dtype=np.float32)
    n = obs.shape[0]
    assert obs.shape == (n, 3, 64, 64) and dec.shape == (n, 3, 64, 64)
    GH, GW, origins = frame_geometry(n)
    frame = np.zeros((3, GH, GW), np.uint8)
    for k, (r, c) in enumerate(origins):
        frame[:, r:r + 64, c:c + 64] = quantise(obs[k])
        frame[:, r:r + 64, c + 64:c + 128] = quantise(dec[k])
    return frame


# ---- scripted environments ------------------------------------------------------------------------------------------------
SCRIPT_N, SCRIPT_STEPS = 4, 6
SCRIPT_FINISH = (2, 4, 0, 2)          # the step() call at which each environment reports done; 0: never


def script_params(finish=SCRIPT_FINISH):
    """The `env_params` of EnvBatcher(ScriptedEnv, params, n): every instance takes the next index from it."""
    return {"finish": tuple(finish), "made": 0, "closed": 0}


def script_observation(i, t):
    return torch.tensor([[100.0 * i + 10.0 * t + j + 1.0 for j in range(3)]], dtype=torch.float32)      # (1, 3), never 0


def script_reward(i, t):
    return (i + 1) + 0.125 * t           # exact in binary, distinct per (environment, step), never 0


class ScriptedEnv:
    """Environment i of a batch: observation and reward are functions of (i, number of step() calls); done is reported by
    exactly ONE call (finish[i]), so a batcher must remember it; it keeps answering when stepped after that."""
    action_size, observation_size = 2, 3

    def __init__(self, params):
        self.p, self.i = params, params["made"]
        params["made"] += 1
        self.t, self.actions = 0, []

    def reset(self):
        self.t = 0
        return script_observation(self.i, 0)

    def step(self, action):
        self.t += 1
        self.actions.append(np.asarray(action, dtype=np.float32).copy())
        return script_observation(self.i, self.t), script_reward(self.i, self.t), self.t == self.p["finish"][self.i]

    def close(self):
        self.p["closed"] += 1


def script_actions(t, n=SCRIPT_N):
    return torch.full((n, 2), float(t)) + torch.arange(n, dtype=torch.float32).unsqueeze(1) / 8


# ---- stub agent -----------------------------------------------------------------------------------------------------------
class StubAgent:
    """What run_evaluation needs of an agent, on the CPU: records every call."""

    def __init__(self, belief_size=5, state_size=12, action_size=2, takes_noise=True):
        self.device = torch.device("cpu")
        self.belief_size, self.state_size, self.action_size = belief_size, state_size, action_size
        self.calls, self.modes, self.takes_noise = [], [], takes_noise

    def eval(self):
        self.modes.append("eval")

    def train(self):
        self.modes.append("train")

    def update_belief_and_act(self, env, belief, posterior_state, action, observation, explore=False, **kw):
        if kw and not self.takes_noise:
            raise TypeError(f"unexpected keyword arguments {sorted(kw)}")
        self.modes.append("act")
        self.calls.append(dict(belief=belief.clone(), state=posterior_state.clone(), action=action.clone(),
                               observation=observation.clone(), explore=explore, kw=dict(kw)))
        t = len(self.calls)
        next_observation, reward, done = env.step(script_actions(t, belief.shape[0]))
        return belief + 1, posterior_state + 2, script_actions(t, belief.shape[0]), next_observation, reward, done
