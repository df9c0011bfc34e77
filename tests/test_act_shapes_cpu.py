"""CPU: what the GPU tests of the acting step's shape table (tests/act_shapes.py, tests/test_act_shapes_gpu.py) rest on,
shown without a kernel: every row is a shape the entry points take and its first refused neighbours are refused in their
own words; the LDS rule for Categorical latents, restated from the header comment of csrc/act.hip; the float64
restatement against the composed float32 oracle at every row; per row the gap every Categorical sampler call shows
against the logit error the forward tolerance allows (so exact one-hots may be demanded with nothing left out); the
conditioning of the rows (a float32 evaluation of the restatement uses a few per cent of the tolerance); and the sharpness
condition -- the last input column of every width moves an output by more than ten tolerances or changes a sampled class,
so a kernel that drops a ragged tail fails the GPU test."""
import ctypes as C
import itertools
import json

import numpy as np
import pytest
import torch

from tests import act_cat_ref as R
from tests import act_mode_ref as MR
from tests import act_ref
from tests import act_shapes as T
from tests import scan_cat_ref as CR
from tests.helpers import assert_close, split_scratch_floats
from tests.test_act_cat_ref_cpu import _oracle_step

MAX_LDS = 160 * 1024
NAMES = list(T.ROWS)
SAMPLER_ROWS = [n for n in NAMES if T.samplers(T.ROWS[n].dims)]


def _dims_args(d, O=None):
    return d.Be, d.cat_D, d.cat_C, d.S, d.A, d.Hd, d.E, d.O if O is None else O


# ---------------------------------------------------------------------------------------------- predicates, the LDS rule
def _cat_rule(Be, D, C, S, A, Hd, E, O, scratch):
    """bd_act_step_cat_supported for Categorical latents, from the header comment of csrc/act.hip ("LDS budget") and the
    refusal's words: S = D * C, C <= 256, S <= 256 or (256 % C == 0 and S % 16 == 0), A <= 64, widths up to 2^20, and
        t0, t1, t2           3 * max(Kb_h, Kb_hd) * 256
        ef | logits image    max(max(Kb_e, Kb_o) * 256, 16 * (ceil(S / 16) * 16 + 8))
        state                2 * 16 * D
        action fragments     Kb_a * 256
        split-K scratch
    floats within the 160 KiB of a workgroup."""
    if min(Be, S, A, Hd, E, D, C) <= 0 or O < 0 or max(Be, Hd, E, O, S, D) > 1 << 20 or A > 64 or C > 256:
        return 0
    if D * C != S or not (S <= 256 or (256 % C == 0 and S % 16 == 0)):
        return 0
    kb = lambda x: -(-x // 16)
    n_ef = max(max(kb(E), kb(O)) * 256, 16 * (kb(S) * 16 + 8))
    floats = 3 * max(kb(Be), kb(Hd)) * 256 + n_ef + 2 * 16 * D + kb(A) * 256 + scratch
    return int(floats * 4 <= MAX_LDS)


# the first refused neighbours of the table: entry point, overrides of a complete block, the refusal's words
REFUSED = {
    "gauss_S65": ("bd_act_step", dict(S=65, A=2), "state width above 64"),
    "gauss_A65": ("bd_act_step", dict(S=6, A=65), "action width above 64"),
    "disc_A65": ("bd_act_step_cat", dict(S=6, A=65, actor_cat=1), "action width above 64"),
    "cat_C257": ("bd_act_step_cat", dict(D=1, C=257, S=257, A=2, latent_cat=1), "latents unsupported"),
    "cat_16x17": ("bd_act_step_cat", dict(D=16, C=17, S=272, A=2, latent_cat=1), "latents unsupported"),
    "cat_S_not_DC": ("bd_act_step_cat", dict(D=3, C=5, S=16, A=2, latent_cat=1), "latents unsupported"),
    "cat_lds": ("bd_act_step_cat", dict(D=3, C=5, S=15, A=2, latent_cat=1, Hd=1 << 16), "LDS"),
    "gauss_lds": ("bd_act_step", dict(S=6, A=2, Hd=1 << 16), "LDS"),
}


def test_every_row_is_supported():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    for name, row in T.ROWS.items():
        d = row.dims
        for O in (d.O, 0):                                          # observation form, embedding form
            if d.categorical or d.discrete_actions:
                got = lib.bd_act_step_cat_supported(*_dims_args(d, O), int(d.categorical), int(d.discrete_actions))
            else:
                got = lib.bd_act_step_supported(d.Be, d.S, d.A, d.Hd, d.E, O)
            assert got == 1, (name, O)
        kb = lambda x: -(-x // 16)
        if row.big:     # above 64 KiB already without state and action: t0..t2, the embedding, the scratch
            assert (3 * max(kb(d.Be), kb(d.Hd)) * 256 + kb(d.E) * 256 + split_scratch_floats()) * 4 > 64 * 1024, name


def test_lds_rule_for_categorical_latents():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    scratch = split_scratch_floats()
    grid = [_dims_args(r.dims) for r in T.ROWS.values() if r.dims.categorical]
    grid += [_dims_args(r.dims, 0) for r in T.ROWS.values() if r.dims.categorical]
    grid += [(24, 1, 257, 257, 2, 20, 40, 5), (24, 16, 17, 272, 2, 20, 40, 5), (24, 3, 5, 16, 2, 20, 40, 5), (24, 3, 5, 15, 65, 20, 40, 5),
             (24, 3, 5, 15, 2, 1 << 16, 40, 5), (200, 32, 32, 1024, 18, 200, 1024, 3), (200, 32, 32, 1024, 18, 200, 1024, 0)]
    for Be, (D, C), A, Hd, E, O in itertools.product((24, 200, 1 << 13), ((3, 5), (32, 32), (16, 16), (17, 16), (16, 17), (136, 2),
                                                                            (1, 256), (2, 256), (1, 257), (16, 1), (0, 5), (2048, 16)),
                                                     (1, 64, 65), (20, 200, 1 << 14), (40, 1024, 1 << 15), (0, 5, 4000)):
        grid.append((Be, D, C, D * C, A, Hd, E, O))
    seen = {0: 0, 1: 0}
    for Be, D, C, S, A, Hd, E, O in grid:
        want = _cat_rule(Be, D, C, S, A, Hd, E, O, scratch)
        seen[want] += 1
        for ac in (0, 1):
            assert lib.bd_act_step_cat_supported(Be, D, C, S, A, Hd, E, O, 1, ac) == want, (Be, D, C, S, A, Hd, E, O, ac)
    assert seen[0] > 20 and seen[1] > 20
    # the image, not the embedding, sizes the region at 32 x 32 with a small E; the rule's overflow is an LDS overflow
    assert 16 * (1024 + 8) > 3 * 256 and _cat_rule(24, 2048, 16, 2048 * 16, 2, 20, 40, 5, scratch) == 0


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_neighbours_name_the_entry_point(case):
    """Each is refused by the predicate and by the entry point itself, before any launch (the block's pointers are fake),
    in the refusal's own words."""
    from big_dreamer_amd import _cabi as cabi
    entry, over, words = REFUSED[case]
    a = cabi.ActArgs()
    for name, typ in a._fields_:
        if typ is cabi.P:
            setattr(a, name, 4096)
        elif name in ("w_enc", "b_enc", "w_a", "b_a"):
            for i in range(len(getattr(a, name))):
                getattr(a, name)[i] = 4096
    a.embedding = None
    a.belief_out, a.state_out, a.action_out = 8192, 12288, 16384
    a.B, a.Be, a.D, a.C, a.Hd, a.E, a.O = 1, 24, 0, 0, 20, 40, 5
    for k, v in over.items():
        setattr(a, k, v)
    if entry == "bd_act_step":
        assert cabi.lib.bd_act_step_supported(a.Be, a.S, a.A, a.Hd, a.E, a.O) == 0
    else:
        assert cabi.lib.bd_act_step_cat_supported(a.Be, a.D, a.C, a.S, a.A, a.Hd, a.E, a.O, a.latent_cat, a.actor_cat) == 0
    assert getattr(cabi.lib, entry)(C.byref(a), None) != 0, case
    err = cabi.lib.bd_last_error().decode()
    assert err.startswith(entry + ":") and words in err, (case, err)


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("name", [n for n in NAMES if not T.samplers(T.ROWS[n].dims)])
def test_gaussian_tanh_rows_are_act_ref(name):
    """With Gaussian latents and the tanh-Normal actor act_cat_ref.act_step_cat is act_ref.act_step."""
    d, P, data = T.inputs(name)
    for form in ("obs", "emb"):
        n = T.form_rows(name, form)
        b, s, a = data["belief"][:n], data["state"][:n], data["action"][:n]
        for i, (wb, ws, wa, _) in enumerate(T.chain(name, form, True)):
            kw = {"obs": data["obs"][i, :n]} if form == "obs" else {"embedding": data["emb"][i, :n]}
            b, s, a = act_ref.act_step(P, b, s, a, data["post"][i, :n], data["act"][i, :n], explore=True,
                                       eps_explore=data["exp"][i, :n], action_noise=R.ACTION_NOISE, **kw)
            assert np.array_equal(b, wb) and np.array_equal(s, ws) and np.array_equal(a, wa), (name, form, i)


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_composed_oracle(name, explore):
    """tests/test_act_cat_ref_cpu.py's comparison at every row: three chained decisions of the observation form, one-hot
    states and sampled / explored actions identical, the rest to float32 rounding."""
    d, P, data = T.inputs(name)
    n = T.form_rows(name, "obs")
    b, s, a = data["belief"][:n], data["state"][:n], data["action"][:n]
    for i, (wb, ws, wa, info) in enumerate(T.chain(name, "obs", explore)):
        b, s, a = _oracle_step(P, d, b, s, a, data["post"][i, :n], data["act"][i, :n], data["obs"][i, :n], explore, data["exp"][i, :n])
        assert_close(f"{name} belief{i}", b, wb, 2e-5, 2e-5)
        if d.categorical:
            assert np.array_equal(s, ws), f"{name} state{i}: one-hot states differ"
        else:
            assert_close(f"{name} state{i}", s, ws, 2e-5, 2e-5)
        if d.discrete_actions:
            assert np.array_equal(a.argmax(1), wa.argmax(1)), f"{name} action{i}: classes differ"
            assert float(np.abs(a - wa).max()) <= 1e-6
            if explore:
                hit = info["explored"]
                assert np.array_equal(a[hit], wa[hit]) and set(np.unique(wa[hit])) <= {0.0, 1.0}
        else:
            assert_close(f"{name} action{i}", a, wa, 2e-5, 2e-5)


# ---------------------------------------------------------------------------------------------- sampler margins
def _check_samplers(d, P, info, tag):
    """One decision: no sampler call ambiguous under the kernels' margin; -> (smallest gap, allowed logit error)."""
    tt = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    if d.categorical:
        amb, n, _ = CR.sample_check(tt(info["post_logits"]), tt(info["post_q"]), tt(info["post_idx"]), d.cat_D, d.cat_C,
                                    CR.sample_path(d.cat_C), tag)
        assert amb == 0 and n == info["post_idx"].size, f"{tag}{amb} ambiguous (row, factor) pairs"
    if d.discrete_actions:
        amb, n, _ = CR.sample_check(tt(info["actor_out"]), tt(info["actor_q"]), tt(info["actor_idx"]), 1, d.A, "libm", tag)
        assert amb == 0 and n == len(info["actor_idx"]), f"{tag}{amb} ambiguous action rows"
    return info["min_gap"], T.logit_bound(P, d, info)


@pytest.mark.parametrize("name", SAMPLER_ROWS)
def test_no_sample_is_left_to_rounding(name):
    """Both forms, explore off and on, every call of the chain: the best ratio leads the runner-up by more than
    max(MIN_GAP, 2 * bound), bound = the logit error a kernel within the forward tolerance may show at this row
    (act_shapes.logit_bound, from the float64 operands of the layer that makes the logits)."""
    d, P, _ = T.inputs(name)
    gap, bound = 1.0, 0.0
    for form in ("obs", "emb"):
        for explore in (False, True):
            for i, (_, _, _, info) in enumerate(T.chain(name, form, explore)):
                g, b = _check_samplers(d, P, info, f"{name} {form} explore={explore} call {i}: ")
                gap, bound = min(gap, g), max(bound, b)
    print("ACT_GAP", name, json.dumps({"seed": T.ROWS[name].seed, "bound": bound, "required": T.required_gap(bound), "gap": gap}))
    assert gap > T.required_gap(bound), f"{name}: smallest gap {gap:.3e} against {T.required_gap(bound):.3e}: choose another seed"


@pytest.mark.parametrize("name", T.EVAL_ROWS)
def test_evaluation_runs_meet_their_conditions(name):
    """The conditions tests/test_act_mode_ref_cpu.py states for the evaluation policy's inputs, at the rows run with one:
    every Categorical sampler at q = 1 (where the policy puts it there) is decided by more than the row's gap; for the
    tanh-Normal actor the draws made for the float64 statistics are regular or saturated and at most MULTI_CAP of the
    rows have more than one admissible index."""
    d, P, data = T.inputs(name)
    for B, form in T.eval_runs(name):
        for state_mean in (False, True):
            h2, s2, a2, info, mean, std = MR.policy_ref(P, d, data, B, form, state_mean)
            if T.samplers(d):
                gap, bound = _check_samplers(d, P, info, f"{name} B={B} {form} state_mean={state_mean}: ")
                assert gap > T.required_gap(bound), (name, B, form, state_mean, gap, bound)
            if d.discrete_actions or state_mean:
                continue
            m, s = torch.from_numpy(mean).float(), torch.from_numpy(std).float()
            eps = MR.eps_for_stats(m, s, d.n_entropy, seed=500 + B)
            assert bool(MR.regular_or_saturated(m, s, eps).all())
            share = MR.multi_share(m, s, eps)
            assert share <= MR.MULTI_CAP, f"{name} B={B} {form}: {share:.3f} of the rows have more than one admissible index"


# ---------------------------------------------------------------------------------------------- conditioning, sharpness
@pytest.mark.parametrize("name", NAMES)
def test_float32_evaluation_uses_a_few_per_cent_of_the_tolerance(name):
    """The same restatement with every operand, product and activation in float32 stays within 5 % of the GPU tolerance of
    the float64 chain, and samples the same classes: a correct fp32 kernel meets 2e-5 with a wide margin at this row."""
    d, P, data = T.inputs(name)
    worst = 0.0
    for form in ("obs", "emb"):
        want = T.chain(name, form, True)
        with T.float32_restatement():
            got = R.chain(P, d, data, T.form_rows(name, form), True, form)
        assert got[0][0].dtype == np.float32 and got[-1][1].dtype == np.float32
        ratio, flipped = T.moved(d, got, want)
        assert not flipped, f"{name} {form}: the float32 evaluation samples another class"
        worst = max(worst, ratio)
    print("ACT_FP32", name, f"{100 * worst:.2f} % of the tolerance")
    assert worst <= 0.05, f"{name}: float32 evaluation at {100 * worst:.1f} % of the tolerance"


@pytest.mark.parametrize("width", T.WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_every_tail_column_matters(name, width):
    d, P, _ = T.inputs(name)
    why = T.exempt(name, width)
    form = T.sharp_form(name)
    ratio, flipped = T.moved(d, T.chain(name, form, True, P=T.drop_last_column(P, d, width)), T.chain(name, form, True))
    if why is not None:
        assert ratio == 0.0 and not flipped, f"{name} {width}: exempt ({why}), yet the column moves an output"
        return
    assert ratio > 10.0 or flipped, (f"{name}: dropping the last column of {width} moves the outputs by {ratio:.2f} tolerances "
                                     "and changes no class: change the row's seed")
