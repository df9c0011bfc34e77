"""CPU: the two-hot critic head without a GPU -- the three entry points in the header and the ctypes table, the checks
of the new keys, the shapes that follow from them, and the properties of the float64 restatement tests/twohot_ref.py that
make it a specification: q is a two-hot encoding whose mean is clamp(symlog y), symexp inverts symlog, uniform logits
decode to exactly 0, the stated gradients are the derivatives (central differences), the gradient of the loss is bounded
whatever the target, and q is continuous across every bin edge."""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import twohot_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = T.FLT_MAX

SIGNATURES = {
    "bd_twohot_decode": "int bd_twohot_decode(const float* logits, int ld, int rows, int K, float zmax, float* value, float* mean, "
                        "void* stream);",
    "bd_twohot_decode_backward": "int bd_twohot_decode_backward(const float* logits, int ld, const float* dvalue, int rows, int K, "
                                 "float zmax, float* dlogits, int ldd, void* stream);",
    "bd_twohot_nll": "int bd_twohot_nll(const float* logits, int ld, const float* target, const float* weight, int rows, int K, "
                     "float zmax, float grad_scale, float* dlogits, int ldd, float* value, float* row_loss, void* stream);",
}


# ------------------------------------------------------------------------------------------ the C ABI
def test_kernels_are_declared_and_exported():
    from big_dreamer_amd import _cabi
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read())
    P, I, F = C.c_void_p, C.c_int, C.c_float
    ctype = {"const float*": P, "float*": P, "void*": P, "int": I, "float": F}
    for name, sig in SIGNATURES.items():
        assert sig in hdr, name
        assert name in _cabi.EXPORTED and hasattr(_cabi.lib, name)
        args = [a.rsplit(" ", 1)[0] for a in sig[sig.index("(") + 1:sig.index(")")].split(", ")]
        fn = getattr(_cabi.lib, name)
        assert fn.restype is I and list(fn.argtypes) == [ctype[a] for a in args], name
    assert "twohot.hip" in open(os.path.join(ROOT, "big_dreamer_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from big_dreamer_amd import _cabi
    lib = _cabi.lib
    buf = (C.c_float * 64)()                     # never read: every call below is refused first
    p = C.addressof(buf)
    for K, ld, zmax, rows in ((1, 8, 20.0, 4), (1025, 2048, 20.0, 4), (8, 7, 20.0, 4), (8, 8, 0.0, 4), (8, 8, 80.5, 4),
                              (8, 8, float("nan"), 4), (8, 8, 20.0, 0), (8, 8, 20.0, -1)):
        assert lib.bd_twohot_decode(p, ld, rows, K, zmax, p, None, None) != 0
        assert b"bd_twohot_decode" in lib.bd_last_error()
        assert lib.bd_twohot_decode_backward(p, ld, p, rows, K, zmax, p, ld, None) != 0
        assert lib.bd_twohot_nll(p, ld, p, None, rows, K, zmax, 1.0, p, ld, None, p, None) != 0
        assert b"bd_twohot_nll" in lib.bd_last_error()
    assert lib.bd_twohot_decode(None, 8, 4, 8, 20.0, p, None, None) != 0
    assert lib.bd_twohot_decode(p, 8, 4, 8, 20.0, None, None, None) != 0
    assert lib.bd_twohot_nll(p, 8, p, None, 4, 8, 20.0, 1.0, p, 7, None, p, None) != 0      # ldd < K
    assert lib.bd_twohot_nll(p, 8, p, None, 4, 8, 20.0, 1.0, p, 8, None, None, None) != 0


# ------------------------------------------------------------------------------------------ keys and shapes
def test_check_critic_head():
    from big_dreamer_amd.engine import check_critic_head as chk
    assert chk() == ("normal", 255, 20.0)
    assert chk("twohot", 2, 80) == ("twohot", 2, 80.0) and chk("twohot", 1024, 1e-3) == ("twohot", 1024, 1e-3)
    assert chk("normal", algorithm="planet")[0] == "normal"
    for bad in (dict(head="two_hot"), dict(head=None), dict(head="Twohot"), dict(bins=1), dict(bins=1025), dict(bins=255.0),
                dict(bins="255"), dict(bins=True), dict(bin_range=0.0), dict(bin_range=-1.0), dict(bin_range=80.5),
                dict(bin_range=float("nan")), dict(bin_range=float("inf")), dict(bin_range="20"), dict(bin_range=True),
                dict(head="twohot", algorithm="planet")):
        with pytest.raises(ValueError):
            chk(**bad)


def test_config_defaults_and_overrides():
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.engine import CRITIC_HEAD_DEFAULTS, CRITIC_HEAD_KEYS
    ac = load_config()["ActorCritic"]
    assert {k: ac[k] for k in CRITIC_HEAD_KEYS} == dict(critic_head="normal", critic_bins=255, critic_bin_range=20.0) \
        == CRITIC_HEAD_DEFAULTS
    ac = load_config(["ActorCritic.critic_head=twohot", "ActorCritic.critic_bins=7"])["ActorCritic"]
    assert ac["critic_head"] == "twohot" and ac["critic_bins"] == 7


@pytest.mark.parametrize("override,algo", [("critic_head=onehot", "dreamer"), ("critic_bins=1", "dreamer"),
                                           ("critic_bins=1025", "dreamerV2"), ("critic_bin_range=81", "dreamer"),
                                           ("critic_head=twohot", "planet")])
def test_bad_keys_raise_before_a_device_is_touched(override, algo, monkeypatch):
    import importlib.util
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.planet import Planet

    def touched(*a, **k):
        raise AssertionError("a device was touched")

    for fn in ("is_available", "current_device", "set_device", "init", "_lazy_init", "current_stream", "Stream"):
        monkeypatch.setattr(torch.cuda, fn, touched)
    ov = [f"ActorCritic.{override}", f"algorithm={algo}"]
    params = load_config(ov)
    with pytest.raises(ValueError, match="critic_"):
        {"planet": Planet, "dreamer": Dreamer, "dreamerV2": DreamerV2}[algo](params, env=None)
    spec = importlib.util.spec_from_file_location("bd_cli_main", os.path.join(ROOT, "src", "main.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    with pytest.raises(ValueError, match="critic_"):
        cli.my_app(ov)


def test_critic_out_and_shape_tables():
    d = synth.TINY
    assert (d.critic_head, d.critic_bins, d.critic_bin_range, d.critic_out, d.twohot) == ("normal", 255, 20.0, 1, False)
    feat = d.Be + d.S
    for K in (255, 7):
        t = dataclasses.replace(d, critic_head="twohot", critic_bins=K)
        assert t.critic_out == K and t.twohot
        shapes = dict(synth.param_shapes(t)["critic"])
        assert shapes["model.8.weight"] == (K, d.Hd) and shapes["model.8.bias"] == (K,)
        assert shapes["model.0.weight"] == (d.Hd, feat)
        P = synth.make_params(t, 0)
        assert P["critic"]["model.8.weight"].shape == P["critic_target"]["model.8.weight"].shape == (K, d.Hd)
        assert dict(synth.param_shapes(t)["reward_model"])["model.8.weight"] == (1, d.Hd)
    assert dict(synth.param_shapes(d)["critic"])["model.8.weight"] == (1, d.Hd)
    with pytest.raises(ValueError):
        dataclasses.replace(d, critic_head="gaussian")


# ------------------------------------------------------------------------------------------ the restatement
def _targets():
    rng = np.random.default_rng(0)
    wide = rng.standard_normal(400) * np.exp(rng.uniform(-20, 40, 400))
    return np.concatenate([wide, [0.0, -0.0, 1e-42, -1e-42, 1.0, -1.0, 1e9, -1e9, FLT_MAX, -FLT_MAX]])


@pytest.mark.parametrize("K", T.KS)
@pytest.mark.parametrize("Z", [20.0, 1.0, 80.0])
def test_encoding_is_two_hot_with_the_right_mean(K, Z):
    y = _targets()
    q = T.encode(y, K, Z)
    assert (q >= 0).all() and np.abs(q.sum(-1) - 1).max() <= 4e-16 and ((q > 0).sum(-1) <= 2).all()
    mean = (q * T.bins(K, Z)).sum(-1)
    assert np.abs(mean - np.clip(T.symlog(y), -Z, Z)).max() <= 1e-13 * Z
    z = T.bins(K, Z)
    assert z[0] == -Z and z[-1] == Z and np.array_equal(z, -z[::-1])
    assert np.abs(z - (-Z + np.arange(K) * (2 * Z / (K - 1)))).max() <= 1e-14 * Z


def test_symexp_inverts_symlog():
    y = _targets()
    back = T.symexp(T.symlog(y))
    assert np.all(np.abs(back - y) <= 1e-13 * np.abs(y))
    assert T.symlog(0.0) == 0.0 and T.symexp(0.0) == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", T.KS)
def test_uniform_logits_decode_to_exactly_zero(K, dtype):
    for c in (0.0, 0.37, -1e4, 80.0):
        v, m = T.decode(np.full((3, K), c), 20.0, dtype)
        assert np.all(v == 0) and np.all(m == 0), (K, c)


def _central(f, l, h=1e-6):
    g = np.zeros_like(l)
    for i in range(l.shape[-1]):
        e = np.zeros(l.shape[-1])
        e[i] = h
        g[..., i] = (f(l + e) - f(l - e)) / (2 * h)
    return g


@pytest.mark.parametrize("K", [2, 3, 7, 65, 255])
def test_gradients_are_the_derivatives(K):
    rng = np.random.default_rng(K)
    Z = 5.0
    l = rng.standard_normal((6, K))
    dv = rng.standard_normal(6)
    want = _central(lambda x: T.decode(x, Z)[0] * dv, l)
    got = T.decode_backward(l, dv, Z)
    assert np.abs(got - want).max() <= 1e-7 * max(1.0, np.abs(want).max())
    y = np.array([0.0, 0.3, -2.0, 50.0, -1e9, 7.0])
    wr = rng.uniform(0.2, 1.0, 6)
    want = 0.5 * _central(lambda x: T.nll(x, y, Z, wr)[0], l)
    got = T.nll(l, y, Z, wr, 0.5)[1]
    assert np.abs(got - want).max() <= 1e-8


@pytest.mark.parametrize("K", T.KS)
def test_gradient_is_bounded_whatever_the_target(K):
    """The point of the head: the row L1 norm of dlogits is at most 2 grad_scale w_r for targets from 0 to +-FLT_MAX (the
    Normal(v, 1) critic's gradient grows with the error)."""
    rng = np.random.default_rng(K)
    mag = np.concatenate([[0.0], np.logspace(-45, np.log10(FLT_MAX), 300), [FLT_MAX]])
    y = np.concatenate([mag, -mag])
    wr = rng.uniform(0.0, 2.0, y.size)
    gs = 0.125
    for name in ("normal", "spike", "ramp_lo"):
        l = T.filling(name, y.size, K)
        for dtype in (np.float64, np.float32):
            loss, dl = T.nll(l, y, 20.0, wr, gs, dtype)
            assert np.isfinite(loss).all() and np.isfinite(dl).all()
            assert np.all(np.abs(dl.astype(np.float64)).sum(-1) <= 2 * gs * wr * (1 + 1e-5) + 1e-300), (name, dtype)


def test_nan_target_gives_nan_loss():
    loss, _ = T.nll(np.zeros((2, 5)), np.array([np.nan, 1.0]), 20.0)
    assert np.isnan(loss[0]) and np.isfinite(loss[1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("K", T.KS)
def test_encoding_is_continuous_across_every_bin_edge(K, dtype):
    """nextafter on both sides of every edge symexp(z_i): q moves by no more than the format resolves (w -> 1 at k is w = 0 at
    k + 1), although k itself may differ."""
    Z = 20.0
    z = T.bins(K, Z)
    with np.errstate(over="ignore"):
        edge = T.symexp(z).astype(dtype)
    edge = edge[np.isfinite(edge)]
    lo, hi = np.nextafter(edge, dtype(-np.inf)), np.nextafter(edge, dtype(np.inf))
    q0, ql, qh = (T.encode(v, K, Z, dtype).astype(np.float64) for v in (edge, lo, hi))
    # one ulp of y moves symlog(y) by at most ulp(|t| + 1) and w by that over delta; (t + Z) itself is rounded once more
    eps = np.finfo(dtype).eps
    tol = 4 * eps * (2 * Z + 1) / (2 * Z / (K - 1))
    assert np.abs(ql - q0).max() <= tol and np.abs(qh - q0).max() <= tol, (np.abs(ql - q0).max(), np.abs(qh - q0).max(), tol)
    # and across precisions: the float32 encoding of the same targets agrees with float64 although k may differ
    if dtype is np.float32:
        q64 = T.encode(edge.astype(np.float64), K, Z)
        assert np.abs(q0 - q64).max() <= tol
