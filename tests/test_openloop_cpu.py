"""CPU: the open-loop prediction's host side -- check_open_loop's bounds, the three configuration keys, video_shape, the numpy
statement of the video (tests/openl_ref.py: video_reference, what bd_openl_video is held to on the GPU) against a second,
per-pixel construction, openloop.run_open_loop under a stub agent, and the two C entry points' argument checks."""
import math

import numpy as np
import pytest
import torch

from tests.openl_ref import (StubAgent, error_chain, error_reference, quantise, quantise_error, stub_batch, video_reference)


# ---------------------------------------------------------------------------------------------- bounds, config, shape
def test_check_open_loop_bounds():
    from big_dreamer_amd.openloop import check_open_loop
    for seq_len, n, context in ((3, 1, 1), (50, 6, 1), (50, 6, 48), (7, 1, 5), (4, 1000, 2)):
        check_open_loop(seq_len, n, context)
    for seq_len, n, context in ((2, 1, 1), (2, 1, 0), (3, 1, 0), (3, 1, 2), (50, 6, 49), (50, 6, -1), (7, 0, 3), (7, -2, 3)):
        with pytest.raises(ValueError, match="open_loop"):
            check_open_loop(seq_len, n, context)


def test_config_keys():
    from big_dreamer_amd.config import load_config
    p = load_config([])
    assert p["openl_freq"] == -1 and p["openl_sequences"] == 6 and p["openl_context"] == 5
    q = load_config(["openl_freq=500", "openl_sequences=4", "openl_context=3"])
    assert q["openl_freq"] == 500 and q["openl_sequences"] == 4 and q["openl_context"] == 3
    assert all(type(q[k]) is int for k in ("openl_freq", "openl_sequences", "openl_context"))


def test_video_shape():
    from big_dreamer_amd.openloop import video_shape
    assert video_shape(49, 6) == (49, 3, 192, 384)
    assert video_shape(1, 1) == (1, 3, 192, 64)
    assert video_shape(3, 3) == (3, 3, 192, 192)


# ---------------------------------------------------------------------------------------------- the video's reference
def _byte(x):
    """uint8(clip(floor(x), 0, 255)) of one fp32 number, by hand."""
    return min(max(math.floor(float(x)), 0), 255)


def test_video_reference_against_a_per_pixel_construction():
    T, n = 2, 3
    rng = np.random.default_rng(5)
    truth = rng.uniform(-0.75, 0.75, (T, n, 3, 64, 64)).astype(np.float32)
    model = rng.uniform(-0.75, 0.75, (T, n, 3, 64, 64)).astype(np.float32)
    model[0, 1, 2, 5, :] = truth[0, 1, 2, 5, :] + np.float32(1.5)           # error past the upper clip bound
    model[1, 2, 0, :, 9] = truth[1, 2, 0, :, 9] - np.float32(1.5)           # ... and the lower one
    video = video_reference(truth, model)
    assert video.shape == (T, 3, 192, 64 * n) and video.dtype == np.uint8
    half, one, scale = np.float32(0.5), np.float32(1.0), np.float32(256.0)
    slow = np.empty_like(video)
    for t in range(T):
        for c in range(3):
            for row in range(192):
                band, y = divmod(row, 64)
                for col in range(64 * n):
                    k, x = divmod(col, 64)
                    tr, mo = truth[t, k, c, y, x], model[t, k, c, y, x]
                    if band == 0:
                        b = _byte((tr + half) * scale)
                    elif band == 1:
                        b = _byte((mo + half) * scale)
                    else:
                        b = _byte((((mo - tr) + one) * half) * scale)
                    slow[t, c, row, col] = b
    assert np.array_equal(video, slow)
    assert (video[0, 2, 128 + 5, 64:128] == 255).all() and (video[1, 0, 128:192, 128 + 9] == 0).all()
    # the three bands of a block are what the two quantisers give, nothing is padded
    assert np.array_equal(video[1, :, 0:64, 64:128], quantise(truth[1, 1]))
    assert np.array_equal(video[1, :, 64:128, 64:128], quantise(model[1, 1]))
    assert np.array_equal(video[1, :, 128:192, 64:128], quantise_error(model[1, 1], truth[1, 1]))


def test_error_reference_and_chain():
    truth = np.zeros((2, 3, 4), np.float32)
    model = np.stack([np.full((3, 4), 2.0, np.float32), np.arange(12, dtype=np.float32).reshape(3, 4)])
    got = error_reference(truth, model)
    assert got.dtype == np.float64 and np.array_equal(got, [4.0, sum(i * i for i in range(12)) / 12])
    assert error_chain(1, 3) == 9 and error_chain(1, 256) == 9 and error_chain(1, 257) == 10 and error_chain(6, 12288) == 296


# ---------------------------------------------------------------------------------------------- run_open_loop
def _names(agent):
    return [name for name, _ in agent.log]


def _calls(agent, name):
    return [args for called, args in agent.log if called == name]


def test_run_open_loop_state_stub_call_sequence_and_slices():
    from big_dreamer_amd.openloop import run_open_loop
    L, n, c = 7, 3, 2
    T = L - 1
    agent, batch = StubAgent(), stub_batch(L, n)
    obs, actions, _, nonterminals = batch
    noise = {"post": torch.full((c, n, 4), 3.0), "prior": torch.full((T - c, n, 4), 4.0)}
    res = run_open_loop(agent, batch, c, _noise=noise)
    assert _names(agent) == ["eval", "encoder", "transition_model", "transition_model", "observation_model", "openl_error",
                             "train"]
    assert torch.equal(_calls(agent, "encoder")[0]["obs"], obs[1:c + 1])
    ctx, opn = _calls(agent, "transition_model")
    # the context: zero state and belief, actions[:c], the encoder's output, nonterminals[:c], the posterior draw second
    assert tuple(ctx["init_state"].shape) == (n, 4) and not ctx["init_state"].any()
    assert tuple(ctx["init_belief"].shape) == (n, 5) and not ctx["init_belief"].any()
    assert torch.equal(ctx["actions"], actions[:c]) and torch.equal(ctx["nonterminals"], nonterminals[:c])
    assert torch.equal(ctx["embeddings"], agent.encoder(obs[1:c + 1]))
    assert len(ctx["kw"]["_noise"]) == 2 and ctx["kw"]["_noise"][1] is noise["post"]
    # the open loop: from the LAST context step's belief and POSTERIOR state, no embeddings, the remaining actions
    assert opn["embeddings"] is None
    assert (opn["init_belief"] == 10 + (c - 1) + torch.arange(n).view(n, 1) / 8).all() and tuple(opn["init_belief"].shape) == (n, 5)
    assert (opn["init_state"] == 20 + (c - 1) + torch.arange(n).view(n, 1) / 8).all() and tuple(opn["init_state"].shape) == (n, 4)
    assert torch.equal(opn["actions"], actions[c:T]) and torch.equal(opn["nonterminals"], nonterminals[c:T])
    assert len(opn["kw"]["_noise"]) == 1 and opn["kw"]["_noise"][0] is noise["prior"]
    # one decoder pass over all T steps: context beliefs / posterior states, then open-loop beliefs / prior states
    dec = _calls(agent, "observation_model")[0]
    assert tuple(dec["belief"].shape) == (T, n, 5) and tuple(dec["state"].shape) == (T, n, 4)
    assert dec["belief"][:, 0, 0].tolist() == [10, 11, 100, 101, 102, 103]
    assert dec["state"][:, 0, 0].tolist() == [20, 21, 200, 201, 202, 203]
    assert torch.equal(res["beliefs"], dec["belief"]) and torch.equal(res["states"], dec["state"])
    err = _calls(agent, "openl_error")[0]
    assert (err["T"], err["n"], err["width"], bool(err["nhwc"])) == (T, n, 3, False)
    assert torch.equal(err["truth"], obs[1:])
    assert torch.equal(err["model"], agent.observation_model(dec["belief"], dec["state"]))
    # the results
    curve = res["openl_obs_mse"]
    assert curve.dtype == np.float32 and curve.shape == (T,)
    want = error_reference(obs[1:].numpy(), err["model"].numpy())
    assert np.allclose(curve, want, rtol=1e-5, atol=0)
    assert type(res["openl_mse_context"]) is float and type(res["openl_mse_open"]) is float
    assert res["openl_mse_context"] == float(curve[:c].mean()) and res["openl_mse_open"] == float(curve[c:].mean())
    assert res["context"] == c and res["video"] is None
    assert set(res) == {"openl_obs_mse", "openl_mse_context", "openl_mse_open", "context", "video", "beliefs", "states"}


def test_run_open_loop_state_stub_has_no_video_and_passes_noise_only_when_given():
    from big_dreamer_amd.openloop import run_open_loop
    for video in (None, True, False):
        agent = StubAgent()
        res = run_open_loop(agent, stub_batch(5, 2), 1, video=video)
        assert res["video"] is None and "openl_video" not in _names(agent)
        assert all(call["kw"] == {} for call in _calls(agent, "transition_model"))
        assert _names(agent)[0] == "eval" and _names(agent)[-1] == "train"


def test_run_open_loop_pixel_stub_decodes_once_for_both_kernels():
    from big_dreamer_amd.openloop import run_open_loop, video_shape
    L, n, c = 4, 2, 2
    T = L - 1
    agent, batch = StubAgent(pixel=True), stub_batch(L, n, pixel=True)
    res = run_open_loop(agent, batch, c)                                     # video=None: pixel observations get one
    assert _names(agent) == ["eval", "encoder", "transition_model", "transition_model", "openl_video", "openl_error", "train"]
    vid, err = _calls(agent, "openl_video")[0], _calls(agent, "openl_error")[0]
    assert torch.equal(vid["truth"], batch[0][1:]) and tuple(vid["feat"].shape) == (T * n, 5 + 4)
    assert vid["feat"][:, 0].tolist() == [10, 10.125, 11, 11.125, 100, 100.125]         # row t n + k: step t of sequence k
    assert vid["feat"][:, 5].tolist() == [20, 20.125, 21, 21.125, 200, 200.125]
    assert tuple(vid["video"].shape) == video_shape(T, n) and vid["video"].dtype == torch.uint8
    assert (err["T"], err["n"], err["width"], bool(err["nhwc"])) == (T, n, 12288, True)
    assert tuple(err["model"].shape) == (T * n, 64, 64, 3)                   # openl_video's buffer, as it is
    assert res["video"].shape == video_shape(T, n) and res["video"].dtype == np.uint8 and (res["video"] == 7).all()
    assert res["openl_obs_mse"].shape == (T,)
    agent = StubAgent(pixel=True)
    res = run_open_loop(agent, batch, 1, video=False)                        # still one decode for the error curve
    assert res["video"] is None and _calls(agent, "openl_video")[0]["video"] is None


def test_run_open_loop_rejects_a_bad_context_before_any_call():
    from big_dreamer_amd.openloop import run_open_loop
    for L, c in ((5, 4), (5, 0), (2, 1)):
        agent = StubAgent()
        with pytest.raises(ValueError, match="open_loop"):
            run_open_loop(agent, stub_batch(L, 2), c)
        assert agent.log == []


# ---------------------------------------------------------------------------------------------- the C ABI's host half
def test_openl_entry_points_reject_bad_arguments_without_gpu():
    from big_dreamer_amd import _cabi as cabi
    a = 64                                                                   # (addresses are never dereferenced here)
    for change in ({"truth": None}, {"model": None}, {"video": None}, {"T": 0}, {"T": -1}, {"n": 0}, {"n": -3},
                   {"video": a + 1}, {"video": a + 2}, {"T": 1 << 20, "n": 1 << 20}, {"T": 1, "n": 58255},
                   {"T": 2 ** 31 - 1, "n": 2 ** 31 - 1}):
        args = dict(truth=a, model=a, T=3, n=2, video=a)
        args.update(change)
        assert cabi.lib.bd_openl_video(args["truth"], args["model"], args["T"], args["n"], args["video"], None) != 0, change
        assert b"bd_openl_video" in cabi.lib.bd_last_error(), change
    for change in ({"truth": None}, {"model": None}, {"out": None}, {"T": 0}, {"T": -1}, {"n": 0}, {"width": 0}, {"width": -5},
                   {"nhwc": 1}, {"nhwc": 1, "width": 12287}, {"nhwc": 2, "width": 12288}, {"nhwc": -1},
                   {"n": 1 << 20, "width": 1 << 12}, {"n": 2 ** 31 - 1, "width": 2 ** 31 - 1}):
        args = dict(truth=a, model=a, T=3, n=2, width=5, nhwc=0, out=a)
        args.update(change)
        rc = cabi.lib.bd_openl_error(args["truth"], args["model"], args["T"], args["n"], args["width"], args["nhwc"],
                                     args["out"], None)
        assert rc != 0, change
        assert b"bd_openl_error" in cabi.lib.bd_last_error(), change
        with pytest.raises(RuntimeError, match="bd_openl_error"):
            cabi.check(rc)
