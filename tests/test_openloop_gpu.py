"""GPU: open-loop prediction -- the video kernel alone (csrc/video.hip: bd_openl_video) bit for bit against
tests/openl_ref.py's video_reference, the error kernel (bd_openl_error) against float64 within its summation order's bound,
Dreamer.open_loop / Planet.open_loop against the composition of the public modules' forward() written out by hand, and the
CLI's openl_freq."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.openl_ref import error_bound, error_chain, error_reference, video_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


# ---------------------------------------------------------------------------------------------- the video kernel alone
def _special_values():
    """The exact bin edges k / 256 - 0.5 of the truth / model bytes, their fp32 neighbours on both sides and the clip bounds."""
    edges = np.arange(257, dtype=np.float32) / np.float32(256) - np.float32(0.5)
    return np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(1)),
                           np.array([-0.5, 0.5, -3.0, 7.0, 0.0, -0.0], np.float32)])


def _video_inputs(rng, T, n):
    """truth and model (T, n, 3, 64, 64), NCHW both: uniform values reaching past both clip bounds, and at random places (no
    place used twice) _special_values() in each, and pairs whose (model - truth + 1) / 2 is a bin edge k / 256 of the error
    byte or one of its fp32 neighbours -- model - truth = d exactly with truth 0, up to the rounding of d + 0.125 with truth
    0.125 -- or past its clip bounds."""
    shape = (T, n, 3, 64, 64)
    truth, model = (rng.uniform(-0.75, 0.75, shape).astype(np.float32) for _ in range(2))
    special = _special_values()
    d = np.arange(257, dtype=np.float32) / np.float32(128) - np.float32(1)              # (d + 1) / 2 = k / 256
    d = np.concatenate([d, np.nextafter(d, np.float32(-2)), np.nextafter(d, np.float32(2)), np.array([-1.5, 1.5, 3.0], np.float32)])
    where = rng.permutation(truth.size)[:2 * special.size + 2 * d.size]
    tf, mf = truth.reshape(-1), model.reshape(-1)
    a, b, c = special.size, 2 * special.size, 2 * special.size + d.size
    tf[where[:a]] = special
    mf[where[a:b]] = special
    tf[where[b:c]], mf[where[b:c]] = 0.0, d
    tf[where[c:]], mf[where[c:]] = 0.125, d + np.float32(0.125)
    return truth, model


def _nhwc(model):
    T, n = model.shape[:2]
    return np.ascontiguousarray(model.transpose(0, 1, 3, 4, 2)).reshape(T * n, 64, 64, 3)


@pytest.mark.parametrize("T,n", [(1, 1), (3, 3), (2, 6)])
def test_openl_video_kernel_is_bit_identical_to_the_reference(T, n):
    from big_dreamer_amd import _cabi as cabi
    from big_dreamer_amd.openloop import video_shape
    rng = np.random.default_rng(100 * T + n)
    truth, model = _video_inputs(rng, T, n)
    want = video_reference(truth, model)
    assert want.shape == video_shape(T, n) and want.max() == 255 and want.min() == 0
    assert len(np.unique(want[:, :, 128:])) == 256                          # every error byte occurs
    size = want.size
    buf = torch.full((GUARD + size + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    video = buf.data_ptr() + GUARD
    tr, mo = torch.from_numpy(truth).cuda(), torch.from_numpy(_nhwc(model)).cuda()
    cabi.check(cabi.lib.bd_openl_video(tr.data_ptr(), mo.data_ptr(), T, n, video, cabi.stream()))
    got = buf.cpu().numpy()
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + size:] == 0xA5).all()          # the guard bytes are untouched
    body = got[GUARD:GUARD + size].reshape(want.shape)
    assert np.array_equal(body, want), int((body != want).sum())
    # argument checks come back as error codes, before any launch
    t, m = tr.data_ptr(), mo.data_ptr()
    for bad in ((None, m, T, n, video), (t, None, T, n, video), (t, m, T, n, None), (t, m, 0, n, video), (t, m, T, 0, video),
                (t, m, -1, n, video), (t, m, T, n, video + 1), (t, m, T, n, video + 2), (t, m, 1 << 20, 1 << 20, video)):
        assert cabi.lib.bd_openl_video(*bad, cabi.stream()) != 0, bad
    assert np.array_equal(buf.cpu().numpy(), got)


# ---------------------------------------------------------------------------------------------- the error kernel alone
def _error(truth, model, T, n, width, nhwc):
    from big_dreamer_amd import _cabi as cabi
    out = torch.full((T + 2,), -7.0, device="cuda")
    cabi.check(cabi.lib.bd_openl_error(truth.data_ptr(), model.data_ptr(), T, n, width, nhwc, out[1:].data_ptr(), cabi.stream()))
    assert out[0].item() == -7.0 and out[T + 1].item() == -7.0              # nothing but out[0:T] is written
    return out[1:T + 1].clone()


def _check_error(got, want, n, width):
    got = got.cpu().numpy().astype(np.float64)
    bound = error_bound(n, width, want)
    print("openl_error n", n, "width", width, "chain", error_chain(n, width), "|got - want| / bound", np.abs(got - want) / bound)
    assert (want > 0).all() and (np.abs(got - want) <= bound).all(), (got, want, bound)


@pytest.mark.parametrize("n", [1, 3])
def test_openl_error_pixel_form_against_float64(n):
    T, width = 3, 12288
    rng = np.random.default_rng(7 + n)
    truth = rng.uniform(-0.5, 0.5, (T, n, 3, 64, 64)).astype(np.float32)
    model = (truth + rng.normal(0, 0.2, truth.shape)).astype(np.float32)
    nhwc = _nhwc(model)
    tr, mo = torch.from_numpy(truth).cuda(), torch.from_numpy(nhwc).cuda()
    want = error_reference(truth, model)
    assert error_chain(n, width) == -(-n * width // 256) + 8 == 48 * n + 8   # per-lane terms + 6 (wave) + 2 (four waves)
    got = _error(tr, mo, T, n, width, 1)
    _check_error(got, want, n, width)
    assert torch.equal(got, _error(tr, mo, T, n, width, 1))                 # a fixed order: the same bits again
    # the bound discriminates: the NHWC buffer read as if it were NCHW is outside it
    wrong = error_reference(truth, nhwc.reshape(truth.shape))
    assert (np.abs(wrong - want) > error_bound(n, width, want)).all(), (wrong, want)
    assert (np.abs(got.cpu().numpy() - wrong) > error_bound(n, width, wrong)).all()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("width", [3, 5, 257])
def test_openl_error_dense_form_against_float64(width, n):
    T = 3
    rng = np.random.default_rng(31 * width + n)
    truth = rng.normal(0, 1, (T, n, width)).astype(np.float32)
    model = rng.normal(0, 1, (T, n, width)).astype(np.float32)
    tr, mo = torch.from_numpy(truth).cuda(), torch.from_numpy(model).cuda()
    got = _error(tr, mo, T, n, width, 0)
    _check_error(got, error_reference(truth, model), n, width)
    assert torch.equal(got, _error(tr, mo, T, n, width, 0))


def test_openl_error_rejects_bad_arguments_before_any_launch():
    from big_dreamer_amd import _cabi as cabi
    x = torch.zeros(3 * 2 * 12288, device="cuda")
    out = torch.full((3,), -7.0, device="cuda")
    p, o = x.data_ptr(), out.data_ptr()
    for bad in ((None, p, 3, 2, 5, 0, o), (p, None, 3, 2, 5, 0, o), (p, p, 3, 2, 5, 0, None), (p, p, 0, 2, 5, 0, o),
                (p, p, 3, 0, 5, 0, o), (p, p, 3, 2, 0, 0, o), (p, p, 3, 2, 5, 1, o), (p, p, 3, 2, 12288, 2, o),
                (p, p, 3, 1 << 20, 1 << 12, 0, o)):
        assert cabi.lib.bd_openl_error(*bad, cabi.stream()) != 0, bad
    assert (out == -7.0).all()


# ---------------------------------------------------------------------------------------------- agents
TINY = ["belief_size=32", "hidden_size=32", "embedding_size=64", "state_size=6", "synthetic_env_action_size=2",
        "synthetic_env_observation_size=3", "batch_size=3", "seq_len=6", "planning_horizon=4", "experience_size=100",
        "max_episode_length=8", "action_repeat=2", "seed_steps=48"]
PIXEL = ["pixel_observation=true", "embedding_size=1024"]
AGENTS = {
    "state": ([], "dreamer"),
    "pixel": (PIXEL, "dreamer"),
    "pixel_categorical": (PIXEL + ["algorithm=dreamerV2", "latent_distribution=Categorical", "discrete_latent_dimensions=4",
                                   "discrete_latent_classes=4"], "dreamerV2"),
    "planet": (["algorithm=planet", "MPC.optimisation_iters=2", "MPC.candidates=32", "MPC.top_candidates=4"], "planet"),
}


@functools.lru_cache(maxsize=None)
def _agent_and_batch(name):
    """A tiny agent with a filled replay buffer, and ONE batch of 3 sequences of 6 records, shared by the tests."""
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import Env
    from big_dreamer_amd.planet import Planet
    extra, cls = AGENTS[name]
    params = load_config(TINY + list(extra))
    torch.manual_seed(3)                                         # the weights: PyTorch's default initialisation
    np.random.seed(3)
    agent = {"dreamer": Dreamer, "dreamerV2": DreamerV2, "planet": Planet}[cls](params, Env(params))
    agent.randomly_initialize_replay_buffer()
    batch = [x.clone() for x in agent.buffer.sample(3, 6)]
    return agent, batch


def _noise(agent, T, n, c, seed=5):
    g = torch.Generator().manual_seed(seed)
    categorical = agent.latent_distribution == "Categorical"
    draw = lambda steps: (torch.empty(steps, n, agent.state_size).exponential_(generator=g) if categorical
                          else torch.randn(steps, n, agent.state_size, generator=g)).cuda()
    return {"post": draw(c), "prior": draw(T - c)}


def _by_hand(agent, batch, c, noise):
    """Section "Semantics" of the open-loop prediction, written out on the modules' public forward()."""
    obs, actions, _, nonterminals = batch
    L, n = actions.shape[:2]
    T, dev = L - 1, agent.device
    emb = agent.encoder(obs[1:c + 1])
    b0, _, _, s0, _ = agent.transition_model(torch.zeros(n, agent.state_size, device=dev), actions[:c],
                                             torch.zeros(n, agent.belief_size, device=dev), emb, nonterminals[:c],
                                             _noise=(torch.ones_like(noise["post"]), noise["post"]))
    b1, s1, _, _, _ = agent.transition_model(s0[c - 1], actions[c:T], b0[c - 1], None, nonterminals[c:T],
                                             _noise=(noise["prior"],))
    beliefs, states = torch.cat([b0, b1]), torch.cat([s0, s1])
    model = agent.observation_model(beliefs, states)             # (T, n, 3, 64, 64) NCHW, or (T, n, O)
    truth = obs[1:]
    video = video_reference(truth.cpu().numpy(), model.cpu().numpy()) if agent.pixel_observation else None
    return beliefs, states, error_reference(truth.cpu().numpy(), model.cpu().numpy()), video


def _open_loop_equals_the_hand_composition(name, c):
    from big_dreamer_amd.openloop import video_shape
    agent, batch = _agent_and_batch(name)
    L, n = batch[1].shape[:2]
    T = L - 1
    assert (L, n) == (6, 3)
    noise = _noise(agent, T, n, c)
    res = agent.open_loop(batch=batch, context=c, _noise=noise)
    beliefs, states, want, video = _by_hand(agent, batch, c, noise)
    assert tuple(res["beliefs"].shape) == (T, n, agent.belief_size) and torch.equal(res["beliefs"], beliefs)
    assert tuple(res["states"].shape) == (T, n, agent.state_size) and torch.equal(res["states"], states)
    assert not torch.equal(beliefs[c - 1], beliefs[c]) and torch.isfinite(beliefs).all()
    width = batch[0][0, 0].numel()
    curve = res["openl_obs_mse"]
    assert curve.dtype == np.float32 and curve.shape == (T,)
    print(name, "c", c, "|got - want| / bound", np.abs(curve - want) / error_bound(n, width, want))
    assert (want > 0).all() and (np.abs(curve.astype(np.float64) - want) <= error_bound(n, width, want)).all(), (curve, want)
    assert res["context"] == c
    assert res["openl_mse_context"] == float(curve[:c].mean()) and res["openl_mse_open"] == float(curve[c:].mean())
    if agent.pixel_observation:
        assert res["video"].dtype == np.uint8 and res["video"].shape == video_shape(T, n)
        assert np.array_equal(res["video"], video), int((res["video"] != video).sum())
        assert len({f.tobytes() for f in res["video"]}) == T                 # the frames differ from step to step
        assert agent.open_loop(batch=batch, context=c, video=False, _noise=noise)["video"] is None
    else:
        assert res["video"] is None
        assert agent.open_loop(batch=batch, context=c, video=True, _noise=noise)["video"] is None
    return agent, batch, res


@pytest.mark.parametrize("name", ["state", "pixel", "pixel_categorical", "planet"])
def test_open_loop_equals_the_hand_composition(name):
    agent, _, _ = _open_loop_equals_the_hand_composition(name, 2)
    assert agent.latent_distribution == ("Categorical" if name == "pixel_categorical" else "Gaussian")
    assert agent.state_size == (16 if name == "pixel_categorical" else 6)


@pytest.mark.parametrize("c", [1, 4])
def test_open_loop_shortest_and_longest_context(c):
    _open_loop_equals_the_hand_composition("state", c)


def test_open_loop_rejects_contexts_past_the_bounds():
    agent, batch = _agent_and_batch("state")
    for c in (0, 5, -1):
        with pytest.raises(ValueError, match="open_loop"):
            agent.open_loop(batch=batch, context=c)
    with pytest.raises(ValueError, match="open_loop"):
        agent.open_loop(sequences=0, context=2)


@pytest.mark.parametrize("name", ["state", "pixel"])
def test_open_loop_draws_its_own_noise_reproducibly(name):
    agent, batch = _agent_and_batch(name)
    runs = []
    for _ in range(2):
        torch.manual_seed(11)
        agent.engine.set_noise_seed(11)
        runs.append(agent.open_loop(batch=batch, context=2))
    a, b = runs
    assert np.array_equal(a["openl_obs_mse"], b["openl_obs_mse"]) and np.isfinite(a["openl_obs_mse"]).all()
    assert torch.equal(a["beliefs"], b["beliefs"]) and torch.equal(a["states"], b["states"])
    assert (a["video"] is None) == (name == "state")
    if name == "pixel":
        assert np.array_equal(a["video"], b["video"])
    torch.manual_seed(12)                                        # ... and another seed gives other states
    assert not torch.equal(agent.open_loop(batch=batch, context=2)["states"], a["states"])


def test_open_loop_samples_its_own_batch():
    agent, _ = _agent_and_batch("state")
    res = agent.open_loop(sequences=4, context=3)
    assert res["openl_obs_mse"].shape == (5,) and tuple(res["beliefs"].shape) == (5, 4, 32) and res["context"] == 3


# ---------------------------------------------------------------------------------------------- the CLI
CLI = [a for a in TINY if not a.startswith(("seq_len", "seed_steps"))] + PIXEL + [
    "seq_len=4", "seed_steps=48", "train_steps=53", "log_freq=10", "collect_interval=1", "experience_size=300",
    "openl_sequences=2", "openl_context=1"]


def _main(*extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "src", "main.py"), *CLI, *extra], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout


def test_cli_openl_freq_switch(tmp_path):
    from big_dreamer_amd.openloop import video_shape
    on_dir, off_dir = tmp_path / "on", tmp_path / "off"
    on = _main("openl_freq=2", f"eval_video_dir={on_dir}")
    first = int(re.search(r"Initialized with \d+ episodes and (\d+) steps", on).group(1))
    steps = [step for step in range(first, 53) if step % 2 == 0]
    assert len(steps) >= 2
    assert sorted(os.listdir(on_dir)) == sorted(f"Openl_{step}.npy" for step in steps)
    for step in steps:
        video = np.load(on_dir / f"Openl_{step}.npy")
        assert video.dtype == np.uint8 and video.shape == video_shape(4 - 1, 2)
    for key in ("openl_mse_context", "openl_mse_open"):
        values = re.findall(rf"^{key} : (\S+)$", on, flags=re.M)
        assert len(values) == len(steps), (key, values)
        assert all(np.isfinite(float(v)) and float(v) > 0 for v in values)
    off = _main(f"eval_video_dir={off_dir}")                                  # the default openl_freq: nothing of it
    assert "openl_" not in off and "model_loss" in off
    assert not os.path.exists(off_dir) or not [f for f in os.listdir(off_dir) if f.startswith("Openl_")]
