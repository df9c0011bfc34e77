"""GPU: the fused acting step (csrc/act.hip: bd_act_step, bd_act_step_cat; all eight instantiations of act_step_kernel)
at the shape table tests/act_shapes.py -- widths at and one past the 16-wide tile, heads that leave the split-K form,
both sources of Kb_g and Kb_io, gru_tile's 13-block form, every sampler path of the Categorical latents, launches above
64 KiB -- against the float64 restatement (tests/act_ref.py, tests/act_cat_ref.py) and, with an evaluation policy,
tests/act_mode_ref.py.

Tolerances are those of the one-point tests: 2e-5 abs + rel on beliefs, Gaussian states and tanh-Normal actions (the
project's fp32 forward tolerance); one-hot states, sampled classes and explored one-hots EXACT; straight-through action
values to 1e-6.  Exact comparisons rest on tests/test_act_shapes_cpu.py: every sampler call of every row is decided by
more than the logit error that tolerance allows, and the last column of every width moves an output by more than ten
tolerances, so a dropped tail cannot pass.

Every call runs between guard rows: inputs and noise are the first B rows of buffers with NaN in front and behind, and
the engine's named output buffers are seeded with views into sentinel-filled slabs whose interior reads NaN before the
call.  After every call the slabs are unchanged outside the B rows and no output holds a NaN."""
import json

import numpy as np
import pytest
import torch

from tests import act_cat_ref as R
from tests import act_shapes as T
from tests import test_act_mode_gpu as AM
from tests import test_act_step_cat_gpu as SC
from tests.dense_ref import Placed, placed_input
from tests.test_act_step_gpu import cu

pytestmark = pytest.mark.gpu

TOL, ST_TOL = T.TOL, SC.ST_TOL
NAMES = ("belief", "state", "action")
OFF = 16                    # floats in front of every guarded buffer (keeps the 64-byte alignment of a fresh allocation)
INDEX_SENTINEL = -7777


@pytest.fixture(scope="module")
def rows():
    """Per row of the table, built on first use: (engine, parameters, data, memo of the evaluation references)."""
    from big_dreamer_amd.engine import DreamerEngine
    made = {}

    def get(name):
        if name not in made:
            d, P, data = T.inputs(name)
            made[name] = (DreamerEngine(d, None, "cuda", params=P), P, data, {})
        return made[name]
    return get


def nan_behind(x):
    """[B x w] -> the same values as a contiguous device view with NaN in front of the first and behind the last row."""
    x = x if torch.is_tensor(x) else cu(x)
    x = x.cuda().float()
    return placed_input(x.reshape(x.shape[0], -1), x[0].numel(), OFF).view.view(x.shape)


class Guard:
    """The engine's output buffers of a B-row call -- both alternating sets, the actor statistics, the mode index -- as
    views into sentinel-filled slabs."""

    def __init__(self, eng, B):
        d = eng.d
        self.eng, self.B = eng, B
        self.out = {f"act{p}_{n}": Placed(B, w, w, OFF) for p in (0, 1) for n, w in zip(NAMES, (d.Be, d.S, d.A))}
        self.out["act_stats"] = Placed(B, 2 * d.A, 2 * d.A, OFF)
        self.index = torch.full((OFF + B + OFF,), INDEX_SENTINEL, dtype=torch.int32, device="cuda")

    def arm(self):
        """Before a call: the engine finds these buffers under their names, and what the call must write reads NaN."""
        for key, p in self.out.items():
            p.view.fill_(float("nan"))
            self.eng._buf[key] = p.view
        self.eng._buf["act_mode_index"] = self.index[OFF:OFF + self.B]

    def check(self, tag, outs):
        torch.cuda.synchronize()
        for key, p in self.out.items():
            assert p.outside_unchanged(), f"{tag}: wrote outside the {self.B} rows of {key}"
        outside = torch.cat([self.index[:OFF], self.index[OFF + self.B:]])
        assert bool((outside == INDEX_SENTINEL).all()), f"{tag}: wrote outside the {self.B} mode indices"
        for t in outs:
            if t is not None and t.is_floating_point():
                assert not bool(torch.isnan(t).any()), f"{tag}: an output holds a NaN"


def _step_of(eng):
    return eng.act_step_cat if T.samplers(eng.d) else eng.act_step


def _chain_gpu(eng, data, B, explore, form, tag):
    """Three chained decisions on the first B rows, every call between guard rows; cloned results per call."""
    guard, step = Guard(eng, B), _step_of(eng)
    b, s, a = (nan_behind(data[k][:B]) for k in NAMES)
    outs = []
    for i in range(3):
        nz = {"post": nan_behind(data["post"][i, :B]), "action": nan_behind(data["act"][i, :B]),
              "explore": nan_behind(data["exp"][i, :B])}
        kw = {"obs": nan_behind(data["obs"][i, :B])} if form == "obs" else {"embedding": nan_behind(data["emb"][i, :B])}
        guard.arm()
        out = step(b, s, a, explore=explore, action_noise=R.ACTION_NOISE, noise=nz, **kw)
        assert {t.data_ptr() for t in out} <= {p.view.data_ptr() for p in guard.out.values()}, "the outputs are not the guarded buffers"
        guard.check(f"{tag} call {i}", out)
        out = tuple(t.clone() for t in out)
        outs.append(out)
        b, s, a = (nan_behind(t) for t in out)
    return outs


def _note(d, got, want, acc):
    """Worst err / tol per tensor of one decision into acc (exactly compared tensors: the number of mismatches)."""
    gb, gs, ga = (t.cpu().numpy().astype(np.float64) for t in got)
    wb, ws, wa = (np.asarray(w, np.float64) for w in want[:3])
    rel = lambda g, w: float((np.abs(g - w) / (TOL + TOL * np.abs(w))).max())
    worst = lambda key, v: acc.__setitem__(key, max(acc.get(key, 0.0), v))
    worst("belief", rel(gb, wb))
    if d.categorical:
        acc["state_mismatches"] = acc.get("state_mismatches", 0) + int((gs != ws).sum())
    else:
        worst("state", rel(gs, ws))
    if d.discrete_actions:
        acc["class_mismatches"] = acc.get("class_mismatches", 0) + int((ga.argmax(1) != wa.argmax(1)).sum())
        worst("action_straight_through", float(np.abs(ga - wa).max()) / ST_TOL)
    else:
        worst("action", rel(ga, wa))


def test_guard_rows_notice_a_stray_write(rows):
    """The guards themselves: one float behind the last row, one mode index behind the last, and an output element the
    call left unwritten are each reported (the writes here are torch's, into this test's own slabs)."""
    eng = rows("ones")[0]
    guard = Guard(eng, 3)
    guard.arm()
    for p in guard.out.values():
        p.view.zero_()
    guard.check("clean", tuple(p.view for p in guard.out.values()))
    assert eng.buf("act1_state", 3, eng.d.S).data_ptr() == guard.out["act1_state"].view.data_ptr()
    guard.out["act1_state"].full[3, 0] = 0.0
    with pytest.raises(AssertionError, match="outside the 3 rows of act1_state"):
        guard.check("stray float", ())
    guard = Guard(eng, 3)
    guard.index[OFF + 3] = 0
    with pytest.raises(AssertionError, match="mode indices"):
        guard.check("stray index", ())
    guard = Guard(eng, 3)
    guard.arm()
    with pytest.raises(AssertionError, match="NaN"):
        guard.check("unwritten", (guard.out["act0_belief"].view,))


# ---------------------------------------------------------------------------------------------- float64, guards, tiles
@pytest.mark.parametrize("name", list(T.ROWS))
def test_three_chained_decisions_against_float64(rows, name):
    """Per row: the observation form at every row count of the row (act_shapes.obs_B) and the embedding form at 17 (the
    big rows: 3), explore off and on; rows 0..15 of the 17-row run equal the 16-row run bit for bit."""
    eng, _, data, _ = rows(name)
    d = eng.d
    assert eng.act_step_cat_supported == bool(T.samplers(d)) and eng.act_step_supported == (not T.samplers(d))
    acc = {}
    try:
        for form, B in [("obs", B) for B in T.obs_B(name)] + [("emb", T.form_rows(name, "emb"))]:
            for explore in (False, True):
                tag = f"{name} {form} B={B} explore={explore}"
                got, want = _chain_gpu(eng, data, B, explore, form, tag), T.first_rows(T.chain(name, form, explore), B)
                for i in range(3):
                    _note(d, got[i], want[i], acc)
                for i in range(3):
                    SC._compare(d, f"{tag} call {i}", got[i], want[i], want[i][3].get("explored"))
                if form == "obs" and B == 17:     # a tile must not depend on its neighbours
                    alone = _chain_gpu(eng, data, 16, explore, form, tag + " (16 rows)")
                    for i in range(3):
                        for n, t, w in zip(NAMES, got[i], alone[i]):
                            assert torch.equal(t[:16], w), f"{tag} {n}{i}: rows 0..15 of the 17-row run differ from the 16-row run"
    finally:
        print("ACT_RATIOS", name, json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in acc.items()}))


# ---------------------------------------------------------------------------------------------- evaluation instantiations
@pytest.mark.parametrize("name", T.EVAL_ROWS)
def test_evaluation_policy(rows, name, monkeypatch):
    """action_mode "mean" and "mode" and state_mean at the rows of act_shapes.EVAL_ROWS: the checks of
    tests/test_act_mode_gpu.py::test_fused_step_with_a_policy (belief', state', last_act_stats and the action against
    float64, the mode's index admissible, bitwise against the sampling step where the two coincide), every call between
    guard rows.  The conditions on these inputs are asserted by tests/test_act_shapes_cpu.py."""

    class GuardedRunner(AM.Runner):
        def __init__(self, eng, data, B, form):
            super().__init__(eng, data, B, form)
            self.ins = tuple(nan_behind(t) for t in self.ins)
            self.kw = {k: nan_behind(v) for k, v in self.kw.items()}
            self.post, self.act, self.exp = nan_behind(self.post), nan_behind(self.act), nan_behind(self.exp)
            self.guard, self.tag = Guard(eng, B), f"{name} B={B} {form}"

        def __call__(self, action_mode="sample", state_mean=False, noise=(), explore=False):
            self.guard.arm()
            out, stats, index = super().__call__(action_mode, state_mean, noise, explore)
            self.guard.check(f"{self.tag} {action_mode} state_mean={state_mean}", out + (stats,))
            return out, stats, index

    monkeypatch.setattr(AM, "Runner", GuardedRunner)
    for B, form in T.eval_runs(name):
        AM.test_fused_step_with_a_policy(rows, name, B, form)


# ---------------------------------------------------------------------------------------------- in-kernel noise
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("name", T.NOISE_ROWS)
def test_in_kernel_noise_is_the_rng_fill_stream(rows, name, B):
    """The body of the one-point tests at widths that are no multiples of 4: element e of a draw tensor is word e & 3 of
    Philox group e >> 2, so a group of four straddles two rows."""
    from big_dreamer_amd import _cabi as cabi
    eng, _, data, _ = rows(name)
    d, step = eng.d, _step_of(eng)
    assert d.S % 4 and d.A % 4
    eng.set_noise_seed(1234)
    ins = tuple(nan_behind(data[k][:B]) for k in NAMES)
    obs = nan_behind(data["obs"][0, :B])
    normal, exp1 = cabi.BD_RNG_NORMAL, cabi.BD_RNG_EXPONENTIAL
    shapes = [("post", "act_post", (B, d.S), exp1 if d.categorical else normal),
              ("action", "act_action", (B, d.A), exp1 if d.discrete_actions else normal),
              ("explore", "act_explore", (B, 2), cabi.BD_RNG_UNIFORM) if d.discrete_actions else
              ("explore", "act_explore", (B, d.A), normal)]
    guard = Guard(eng, B)

    def run(explore, noise):
        guard.arm()
        out = step(*ins, obs=obs, explore=explore, action_noise=R.ACTION_NOISE, noise=noise)
        guard.check(f"{name} B={B} explore={explore}", out)
        return tuple(t.clone() for t in out)

    k = eng._rng_step.get("act", 0)
    plain = run(False, None)
    assert eng._rng_step["act"] == k + 1, "the decision counter advances by one per call"
    fed = run(False, SC._rng_fill(eng, k, shapes))
    for n, x, y in zip(NAMES, plain, fed):
        assert torch.equal(x, y), f"explore=0 {n}: in-kernel draws differ from bd_rng_fill's"
    eng._rng_step["act"] = k
    noisy = run(True, None)
    buf = SC._rng_fill(eng, k, shapes)
    fed = run(True, buf)
    for n, x, y in zip(NAMES, noisy, fed):
        assert torch.equal(x, y), f"explore=1 {n}: in-kernel draws differ from bd_rng_fill's"
    assert torch.equal(noisy[0], plain[0]) and torch.equal(noisy[1], plain[1]), "exploration touches the action alone"
    if not d.discrete_actions:
        want = torch.clamp(plain[2] + R.ACTION_NOISE * buf["explore"], -1, 1)
        assert float((noisy[2] - want).abs().max()) <= 1e-6 and not torch.equal(noisy[2], plain[2])
    nxt = run(False, None)
    assert eng._rng_step["act"] == k + 2
    assert torch.equal(nxt[0], plain[0]), "the belief takes no noise"
    if B == 17 or not d.categorical:        # (seven factors of one row can repeat by chance)
        assert not torch.equal(nxt[1], plain[1]), "decision k + 1 drew the same state"
