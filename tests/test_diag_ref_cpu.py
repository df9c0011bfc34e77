"""CPU tests of the training diagnostics: the float64 restatements of the kernels (tests/diag_ref.py) against
torch.distributions, the config key, the argument block against the header, the entry points' refusals (nothing is launched)
and diagnostics.py's derivations on hand-made raw blocks."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.distributions as td

from big_dreamer_amd import diagnostics as dg
from big_dreamer_amd.config import load_config
from tests import diag_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- restatements vs torch
def _gauss_case(rows=23, S=7, seed=0):
    rng = np.random.default_rng(seed)
    qm, pm = (rng.standard_normal((rows, S)).astype(np.float32) for _ in range(2))
    qs, ps = (np.exp(rng.uniform(np.log(1e-3), np.log(1e2), (rows, S))).astype(np.float32) for _ in range(2))
    return qm, qs, pm, ps


def test_gaussian_restatement_matches_torch_distributions():
    qm, qs, pm, ps = _gauss_case()
    q = td.Normal(torch.from_numpy(qm).double(), torch.from_numpy(qs).double())
    p = td.Normal(torch.from_numpy(pm).double(), torch.from_numpy(ps).double())
    out, col, _, _ = R.latent_stats_ref(qm, qs, pm, ps)
    kl = td.kl_divergence(q, p)
    np.testing.assert_allclose(out[0], float(q.entropy().sum()), rtol=1e-13)
    np.testing.assert_allclose(out[1], float(p.entropy().sum()), rtol=1e-13)
    np.testing.assert_allclose(out[2], float(kl.sum()), rtol=1e-12)
    np.testing.assert_allclose(col, kl.sum(0).numpy(), rtol=1e-12)
    assert out[3] == qs.size and out[6] == qs.min() and out[7] == qs.max() and out[8] == 0
    np.testing.assert_allclose(out[10], ps.astype(np.float64).sum(), rtol=1e-14)


def _cat_case(rows=11, D=4, Cn=6, seed=1):
    rng = np.random.default_rng(seed)
    ql, pl = ((rng.standard_normal((rows, D, Cn)) * 3).astype(np.float32) for _ in range(2))
    ql[0, 0] = np.where(np.arange(Cn) == 2, 80.0, -80.0)          # near one-hot
    ql[1, 1] = 0.5                                                # an exact tie of all classes
    ql[2, 2, 1] = ql[2, 2, 4] = ql[2, 2].max() + 1                # an exact tie of two maxima: class 1 wins
    return ql, pl


def test_categorical_restatement_matches_torch_distributions():
    ql, pl = _cat_case()
    q = td.OneHotCategorical(logits=torch.from_numpy(ql).double())
    p = td.OneHotCategorical(logits=torch.from_numpy(pl).double())
    out, col, used, _, _ = R.latent_stats_cat_ref(ql, pl)
    kl = td.kl_divergence(q, p)
    np.testing.assert_allclose(out[0], float(q.entropy().sum()), rtol=1e-12)
    np.testing.assert_allclose(out[1], float(p.entropy().sum()), rtol=1e-12)
    np.testing.assert_allclose(out[2], float(kl.sum()), rtol=1e-12)
    np.testing.assert_allclose(col, kl.sum(0).numpy(), rtol=1e-12)
    np.testing.assert_allclose(out[3], float(q.probs.max(-1).values.sum()), rtol=1e-13)
    np.testing.assert_allclose(out[4], float(p.probs.max(-1).values.sum()), rtol=1e-13)
    expect = torch.zeros(4, 6)
    expect[torch.arange(4).expand(11, 4).reshape(-1), torch.from_numpy(ql).argmax(-1).reshape(-1)] = 1
    assert (used == expect.numpy()).all()
    assert used[0, 2] == 1 and used[1, 0] == 1 and used[2, 1] == 1


def test_moments_and_segments_restatements():
    x = np.array([1.0, -2.0, np.nan, 4.0, np.inf], dtype=np.float32)
    out, S1, S2 = R.moments_ref(x)
    assert list(out) == [3, 3, 21, -2, 4, 2] and S1 == 7 and S2 == 21
    out, _, _ = R.moments_ref(x[:2], np.array([0.5, 0.5], dtype=np.float32))
    assert list(out) == [2, -2, 0.25 + 6.25, -2.5, 0.5, 0]
    assert list(R.moments_ref(np.zeros(0, dtype=np.float32))[0]) == [0, 0, 0, np.inf, -np.inf, 0]
    assert list(R.segment_sumsq_ref(np.arange(6, dtype=np.float32), [1, 1, 3, 6])) == [0, 5, 50]


# ---------------------------------------------------------------------------------------------- config
def test_diagnostics_interval_config_key():
    assert load_config([])["diagnostics_interval"] == 0
    assert load_config(["diagnostics_interval=25"])["diagnostics_interval"] == 25
    for bad in ("-1", "2.5", "true", "often"):
        with pytest.raises(ValueError, match="diagnostics_interval"):
            load_config([f"diagnostics_interval={bad}"])
    with pytest.raises(KeyError):
        load_config(["diagnostic_interval=1"])
    assert dg.check_interval(3.0) == 3
    for bad in (-1, 0.5, True, None):
        with pytest.raises(ValueError):
            dg.check_interval(bad)


# ---------------------------------------------------------------------------------------------- the argument block
def test_moments_argument_block_matches_the_header():
    from big_dreamer_amd import _cabi as cabi
    text = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    m = re.search(r"typedef struct \{\s*int n_buf;\s*struct \{([^}]*)\} buf\[BD_MOMENTS_MAX_BUFFERS\];\s*\} bd_moments_args;", text)
    inner = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in inner.split(";"))):
        mm = re.fullmatch(r"(.*?)(\*?)\s*(\w+)", decl)
        fields.append((mm.group(3), C.c_void_p if mm.group(2) else {"size_t": C.c_size_t}[mm.group(1).strip()]))
    assert fields == list(cabi.MomentsBuf._fields_) == [("p", C.c_void_p), ("q", C.c_void_p), ("n", C.c_size_t)]
    consts = {k: int(v) for k, v in re.findall(r"#define (BD_MOMENTS_MAX_BUFFERS|BD_MOMENTS_WORDS|BD_LATENT_WORDS|"
                                              r"BD_LATENT_CAT_WORDS|BD_SEGMENTS_MAX) (\d+)", text)}
    assert consts == dict(BD_MOMENTS_MAX_BUFFERS=cabi.BD_MOMENTS_MAX_BUFFERS, BD_MOMENTS_WORDS=cabi.BD_MOMENTS_WORDS,
                          BD_LATENT_WORDS=cabi.BD_LATENT_WORDS, BD_LATENT_CAT_WORDS=cabi.BD_LATENT_CAT_WORDS,
                          BD_SEGMENTS_MAX=cabi.BD_SEGMENTS_MAX)
    twin_buf = type("TwinBuf", (C.Structure,), {"_fields_": fields})
    twin = type("Twin", (C.Structure,), {"_fields_": [("n_buf", C.c_int), ("buf", twin_buf * consts["BD_MOMENTS_MAX_BUFFERS"])]})
    assert C.sizeof(cabi.MomentsArgs) == C.sizeof(twin) == 8 + 16 * 24
    assert cabi.MomentsArgs.buf.offset == twin.buf.offset == 8
    assert (dg.SEXT, dg.LATENT_WORDS, dg.LATENT_CAT_WORDS) == (cabi.BD_MOMENTS_WORDS, cabi.BD_LATENT_WORDS,
                                                               cabi.BD_LATENT_CAT_WORDS)
    for name in ("bd_diag_ws_floats", "bd_moments", "bd_latent_stats", "bd_latent_stats_categorical", "bd_segment_sumsq"):
        assert name in cabi.EXPORTED
    assert cabi.lib.bd_diag_ws_floats() >= 2 * 256 * 16 * 6


# ---------------------------------------------------------------------------------------------- refusals
def _refused(cabi, rc, text):
    assert rc != 0
    err = cabi.lib.bd_last_error().decode()
    assert text in err, err


def test_entry_points_refuse_bad_arguments_without_a_launch():
    from big_dreamer_amd import _cabi as cabi
    lib, A = cabi.lib, 4096                                   # (addresses are never dereferenced by a refusal)
    a = cabi.MomentsArgs()
    a.n_buf = 1
    a.buf[0].p, a.buf[0].n = A, 10
    _refused(cabi, lib.bd_moments(None, A, A, None), "bd_moments: null argument block")
    _refused(cabi, lib.bd_moments(C.byref(a), None, A, None), "bd_moments: output is null")
    _refused(cabi, lib.bd_moments(C.byref(a), A + 4, A, None), "not 8-byte aligned")
    _refused(cabi, lib.bd_moments(C.byref(a), A, None, None), "bd_moments: workspace is null")
    a.n_buf = 17
    _refused(cabi, lib.bd_moments(C.byref(a), A, A, None), "bd_moments: 17 buffers (max 16)")
    a.n_buf = -1
    _refused(cabi, lib.bd_moments(C.byref(a), A, A, None), "n_buf = -1 is negative")
    a.n_buf, a.buf[0].p = 1, None
    _refused(cabi, lib.bd_moments(C.byref(a), A, A, None), "buffer 0 is null with n = 10")
    a.buf[0].p = A + 2
    _refused(cabi, lib.bd_moments(C.byref(a), A, A, None), "buffer 0 is not 4-byte aligned")

    offs = (C.c_size_t * 34)(*range(34))
    _refused(cabi, lib.bd_segment_sumsq(A, 33, offs, A, A, None), "bd_segment_sumsq: 33 segments (max 32)")
    _refused(cabi, lib.bd_segment_sumsq(A, 2, offs, None, A, None), "bd_segment_sumsq: output is null")
    _refused(cabi, lib.bd_segment_sumsq(A, 2, None, A, A, None), "bd_segment_sumsq: null offsets")
    _refused(cabi, lib.bd_segment_sumsq(A, 2, (C.c_size_t * 3)(0, 9, 8), A, A, None), "offsets decrease at segment 1 (9 > 8)")
    _refused(cabi, lib.bd_segment_sumsq(None, 2, offs, A, A, None), "bd_segment_sumsq: null buffer")
    _refused(cabi, lib.bd_segment_sumsq(A, -1, offs, A, A, None), "n_seg = -1 is negative")

    _refused(cabi, lib.bd_latent_stats(A, A, A, None, 3, 3, A, A, A, None), "bd_latent_stats: null input")
    _refused(cabi, lib.bd_latent_stats(A, A, A, A, 3, 3, None, A, A, None), "bd_latent_stats: output is null")
    _refused(cabi, lib.bd_latent_stats(A, A, A, A, 3, 3, A, None, A, None), "bd_latent_stats: colsum is null")
    _refused(cabi, lib.bd_latent_stats(A, A, A, A, 0, 3, A, A, A, None), "bad dims (rows=0 S=3)")
    _refused(cabi, lib.bd_latent_stats(A, A, A, A, 3, 0, A, A, A, None), "bad dims (rows=3 S=0)")
    cat = lib.bd_latent_stats_categorical
    _refused(cabi, cat(A, None, 3, 2, 2, A, A, A, A, None), "bd_latent_stats_categorical: null input")
    _refused(cabi, cat(A, A, 3, 2, 2, A, A, None, A, None), "null `used`")
    _refused(cabi, cat(A, A, 3, 2, 129, A, A, A, A, None), "129 classes (max 128)")
    _refused(cabi, cat(A, A, 3, 2, 0, A, A, A, A, None), "0 classes (max 128)")
    _refused(cabi, cat(A, A, 3, 0, 2, A, A, A, A, None), "bad dims (rows=3 D=0)")


# ---------------------------------------------------------------------------------------------- diagnostics.py
MODULES = {"model": ("transition_model", "reward_model"), "actor": ("actor",), "critic": ("critic",)}


def _sext(v):
    return R.moments_ref(np.asarray(v, dtype=np.float32))[0]


def _gauss_block(lay, rows, kl_cols, returns, values, actions):
    b = np.zeros(lay.size)
    rng = np.random.default_rng(0)
    qs, ps = rng.uniform(0.1, 2, (rows, lay.n_latent)), rng.uniform(0.1, 2, (rows, lay.n_latent))
    lat = lay.get(b, "latent")
    lat[0], lat[1], lat[2] = R.gauss_entropy(qs).sum(), R.gauss_entropy(ps).sum(), np.sum(kl_cols)
    lat[3:9], lat[9:15] = _sext(qs), _sext(ps)
    lay.get(b, "kl_cols")[:] = kl_cols
    lay.get(b, "mom_wm")[:] = np.concatenate([_sext([1, 2, 3]), _sext([2, 2, 2])])
    lay.get(b, "mom_bh")[:] = np.concatenate([_sext([0.5, 1.5]), _sext(values), _sext(returns), _sext(actions)])
    lay.get(b, "mom_cr")[:] = np.concatenate([_sext(values), R.moments_ref(np.float32(returns), np.float32(values))[0]])
    for g, v in (("model", [9.0, 16.0]), ("actor", [4.0]), ("critic", [0.0])):
        lay.get(b, "gsq_" + g)[:] = v
        lay.get(b, "wsq_" + g)[:] = [4 * x for x in v]
    return b, qs, ps


def test_entries_of_a_hand_made_gaussian_block():
    lay = dg.Layout(False, 3, 0, True, False, 2, MODULES)
    rows = 10
    # the ACTIVE_NATS boundary: a mean KL of exactly 0.01 nat is not active, the next double above is
    kl_cols = np.array([rows * dg.ACTIVE_NATS, rows * np.nextafter(dg.ACTIVE_NATS, 1), 0.0])
    returns, values, actions = [1.0, 2.0, 4.0, 7.0], [1.5, 1.5, 4.5, 6.0], [-1.0, 0.0, 0.5, 1.0]
    b, qs, ps = _gauss_block(lay, rows, kl_cols, returns, values, actions)
    e = dg.entries(b, lay, rows, 4)
    assert e["kl_per_dim"] == [dg.ACTIVE_NATS, np.nextafter(dg.ACTIVE_NATS, 1), 0.0] and e["kl_active_dims"] == 1
    assert e["kl_raw"] == pytest.approx(kl_cols.sum() / rows, rel=1e-15)
    assert e["post_entropy"] == pytest.approx(R.gauss_entropy(qs).sum() / rows, rel=1e-14)
    assert e["post_std_mean"] == pytest.approx(np.float32(qs).astype(np.float64).mean(), rel=1e-14)
    assert e["prior_std_min"] == float(np.float32(ps).min())
    assert (e["reward_batch_mean"], e["reward_pred_mean"], e["reward_pred_std"]) == (2.0, 2.0, 0.0)
    assert e["reward_batch_std"] == pytest.approx(math.sqrt(2 / 3), rel=1e-14)
    sr, sa = R.stats_ref(returns), R.stats_ref(actions)
    for k in ("mean", "std", "min", "max"):
        assert e[f"imag_return_{k}"] == pytest.approx(sr[k], rel=1e-14)
        assert e[f"action_{k}"] == pytest.approx(sa[k], rel=1e-14)
    assert e["action_rms"] == pytest.approx(sa["rms"], rel=1e-14)
    assert e["critic_value_mean"] == pytest.approx(np.mean(values), rel=1e-14)
    assert e["value_explained_variance"] == pytest.approx(R.explained_variance_ref(returns, values), rel=1e-13)
    assert (e["grad_norm/transition_model"], e["grad_norm/reward_model"], e["grad_norm/actor"], e["grad_norm/critic"]) == (3, 4, 2, 0)
    assert (e["weight_norm/transition_model"], e["weight_norm/actor"]) == (6, 4)
    assert not [k for k in e if k.startswith("nonfinite/")]
    assert set(dg.DYNAMICS_KEYS + dg.GAUSSIAN_KEYS + dg.REWARD_KEYS + dg.BEHAVIOUR_KEYS + dg.TANH_ACTION_KEYS) <= set(e)
    # PlaNet: the model region alone
    m = dg.entries(b, lay, rows, 0, regions=("model",))
    assert "imag_return_mean" not in m and "grad_norm/actor" not in m and m["grad_norm/reward_model"] == 4
    assert [k for k, _ in dg.scalar_items(e)] == [k for k in e if k != "kl_per_dim"]


def test_zero_variance_returns_give_nan_explained_variance():
    lay = dg.Layout(False, 3, 0, True, False, 2, MODULES)
    b, _, _ = _gauss_block(lay, 10, np.ones(3), [2.0, 2.0, 2.0], [1.0, 2.0, 3.0], [0.0])
    e = dg.entries(b, lay, 10, 3)
    assert math.isnan(e["value_explained_variance"]) and e["imag_return_std"] == 0.0


def test_empty_finite_sets_and_nonfinite_counts():
    lay = dg.Layout(False, 3, 0, True, False, 2, MODULES)
    b, _, _ = _gauss_block(lay, 10, np.ones(3), [np.nan, np.inf], [1.0, np.nan], [np.nan])
    e = dg.entries(b, lay, 10, 2)
    assert math.isnan(e["imag_return_mean"]) and math.isnan(e["imag_return_std"])
    assert e["imag_return_min"] == math.inf and e["imag_return_max"] == -math.inf
    assert math.isnan(e["value_explained_variance"]) and math.isnan(e["action_rms"])
    assert e["nonfinite/imag_return"] == 2 and e["nonfinite/imag_value"] == 1 and e["nonfinite/action"] == 1
    assert e["nonfinite/critic_value"] == 1 and e["nonfinite/value_error"] == 2
    assert "nonfinite/imag_reward" not in e
    m = dg.moments(np.array([0, 0, 0, np.inf, -np.inf, 0.0]))
    assert math.isnan(m["mean"]) and m["count"] == 0


def test_entries_of_a_hand_made_categorical_block():
    lay = dg.Layout(True, 2, 3, True, True, 3, MODULES)
    assert lay.fields["used"][1] == 3 and lay.fields["act_freq"][1] == 2 and "mom_bh" in lay.fields
    b = np.zeros(lay.size)
    rows, imag = 5, 8
    lay.get(b, "latent")[:] = [3.0, 4.0, 1.0, 7.0, 6.0]
    lay.get(b, "kl_cols")[:] = [0.9, 0.1]
    lay.get(b, "used").view(np.uint32)[:6] = [1, 0, 1, 0, 0, 1]
    lay.get(b, "mom_wm")[:] = np.concatenate([_sext([1.0]), _sext([2.0])])
    lay.get(b, "mom_bh")[:] = np.concatenate([_sext([1.0, 2.0])] * 3)
    lay.get(b, "act_freq").view(np.float32)[:3] = [4, 0, 4]
    lay.get(b, "mom_cr")[:] = np.concatenate([_sext([1.0, 2.0]), _sext([0.0, 0.0])])
    e = dg.entries(b, lay, rows, imag)
    assert e["post_max_prob"] == 0.7 and e["prior_max_prob"] == 0.6 and e["post_classes_used"] == 0.5
    assert e["kl_per_dim"] == [0.18, 0.02] and e["kl_active_dims"] == 2 and e["kl_raw"] == 0.2
    assert e["action_freq"] == [0.5, 0.0, 0.5] and "action_mean" not in e and "post_std_mean" not in e
    assert e["value_explained_variance"] == 1.0
    assert set(dg.CATEGORICAL_KEYS + dg.CATEGORICAL_ACTION_KEYS) <= set(e)
