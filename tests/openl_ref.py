"""Plain helpers of the open-loop prediction tests (tests/test_openloop_cpu.py, tests/test_openloop_gpu.py): numpy restatements
of the truth / model / error video (bd_openl_video, csrc/video.hip) and of the error curve (bd_openl_error), and a stub agent
with the surface openloop.run_open_loop asks for.  Nothing here imports the package under test."""
import numpy as np
import torch


# ---- the video: (T, 3, 192, 64 n) -- per sequence a 64-wide column block, truth over model over error ---------------------
def quantise(v):
    """uint8(clip(floor((v + 0.5) * 256), 0, 255)), fp32 arithmetic: the evaluation video's quantiser."""
    v = np.asarray(v, dtype=np.float32)
    return np.clip(np.floor((v + np.float32(0.5)) * np.float32(256.0)), 0, 255).astype(np.uint8)


def quantise_error(model, truth):
    """e = ((model - truth) + 1) * 0.5, then uint8(clip(floor(e * 256), 0, 255)); every operation rounded to fp32."""
    model, truth = np.asarray(model, dtype=np.float32), np.asarray(truth, dtype=np.float32)
    e = ((model - truth) + np.float32(1.0)) * np.float32(0.5)
    return np.clip(np.floor(e * np.float32(256.0)), 0, 255).astype(np.uint8)


def video_reference(truth, model):
    """truth, model: (T, n, 3, 64, 64) float32, NCHW both -> uint8 (T, 3, 192, 64 n)."""
    truth, model = np.asarray(truth, dtype=np.float32), np.asarray(model, dtype=np.float32)
    T, n = truth.shape[:2]
    assert truth.shape == (T, n, 3, 64, 64) and model.shape == truth.shape
    video = np.zeros((T, 3, 192, 64 * n), np.uint8)
    for k in range(n):
        cols = slice(64 * k, 64 * k + 64)
        video[:, :, 0:64, cols] = quantise(truth[:, k])
        video[:, :, 64:128, cols] = quantise(model[:, k])
        video[:, :, 128:192, cols] = quantise_error(model[:, k], truth[:, k])
    return video


def error_reference(truth, model):
    """(T, ...) both, the same layout -> (T,) float64: the mean of (model - truth)^2 over everything but the first axis."""
    truth, model = np.asarray(truth, dtype=np.float64), np.asarray(model, dtype=np.float64)
    assert truth.shape == model.shape
    T = truth.shape[0]
    return ((model - truth) ** 2).reshape(T, -1).mean(axis=1)


def error_chain(n, width):
    """The longest chain of additions behind one element of bd_openl_error's output, as the kernel's comment states it:
    ceil(n width / 256) per-lane additions, 6 across the wave, 2 across the four waves."""
    return -(-(n * width) // 256) + 8


def error_bound(n, width, want):
    """|got - want| <= (chain + 4) 2^-24 want: every addition of the chain rounds once, relative to a partial sum of
    non-negative terms that never exceeds the total; the 4: the subtraction (twice, as it is squared), the square and the
    final division."""
    return (error_chain(n, width) + 4) * 2.0 ** -24 * np.asarray(want, dtype=np.float64)


# ---- stub agent -----------------------------------------------------------------------------------------------------------
class _StubEngine:
    def __init__(self, log):
        self.log = log

    def openl_video(self, truth, feat, video):
        self.log.append(("openl_video", dict(truth=truth.clone(), feat=feat.clone(), video=video)))
        if video is not None:
            video.fill_(7)
        Tn = feat.shape[0]
        return feat[:, :1].reshape(Tn, 1, 1, 1).expand(Tn, 64, 64, 3).contiguous()       # "NHWC": pixel = the row's first belief

    def openl_error(self, truth, model, T, n, width, nhwc):
        self.log.append(("openl_error", dict(truth=truth.clone(), model=model.clone(), T=T, n=n, width=width, nhwc=nhwc)))
        m = model.reshape(T, n, 64, 64, 3).permute(0, 1, 4, 2, 3) if nhwc else model
        return ((m.reshape(T, -1) - truth.reshape(T, -1)) ** 2).mean(dim=1)


class StubAgent:
    """What run_open_loop needs of an agent, on the CPU: records every call with its arguments.  The context call returns
    beliefs 10 + t, posterior states 20 + t (and prior states 90 + t, which must not be used); the open-loop call returns
    beliefs 100 + t and prior states 200 + t."""

    def __init__(self, pixel=False, belief_size=5, state_size=4, embedding_size=7, observation_size=3):
        self.device = torch.device("cpu")
        self.belief_size, self.state_size = belief_size, state_size
        self.embedding_size, self.observation_size, self.pixel = embedding_size, observation_size, pixel
        self.log = []
        self.engine = _StubEngine(self.log)

    def eval(self):
        self.log.append(("eval", {}))

    def train(self):
        self.log.append(("train", {}))

    def encoder(self, obs):
        self.log.append(("encoder", dict(obs=obs.clone())))
        lead = obs.shape[:2]
        return obs.reshape(*lead, -1)[..., :1].expand(*lead, self.embedding_size) + 0.5

    def transition_model(self, init_state, actions, init_belief, embeddings=None, nonterminals=None, **kw):
        self.log.append(("transition_model", dict(init_state=init_state.clone(), actions=actions.clone(),
                                                  init_belief=init_belief.clone(),
                                                  embeddings=None if embeddings is None else embeddings.clone(),
                                                  nonterminals=nonterminals.clone(), kw=dict(kw))))
        steps, n = actions.shape[:2]
        ramp = torch.arange(steps, dtype=torch.float32).view(steps, 1, 1) + torch.arange(n, dtype=torch.float32).view(1, n, 1) / 8
        full = lambda base, width: (base + ramp).expand(steps, n, width).clone()
        if embeddings is None:
            return full(100.0, self.belief_size), full(200.0, self.state_size), None, None, None
        return full(10.0, self.belief_size), full(90.0, self.state_size), None, full(20.0, self.state_size), None

    def observation_model(self, belief, state):
        self.log.append(("observation_model", dict(belief=belief.clone(), state=state.clone())))
        return (belief[..., :1] + state[..., :1]).expand(*belief.shape[:-1], self.observation_size).clone()


def stub_batch(L, n, pixel=False, A=2, O=3, seed=0):
    """A time-major batch in ExperienceReplay.sample's layout with every element distinct."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.rand((L, n, 3, 64, 64) if pixel else (L, n, O), generator=g) - 0.5
    actions = torch.rand((L, n, A), generator=g)
    rewards = torch.rand((L, n), generator=g)
    nonterminals = (torch.rand((L, n, 1), generator=g) > 0.2).float()
    return [obs, actions, rewards, nonterminals]
