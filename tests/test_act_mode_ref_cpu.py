"""CPU tests of the evaluation policy: the float64 selection reference tests/act_mode_ref.py (the input conditions of the
GPU cases, an fp32 emulation of the kernel's rule held to it), and what the feature adds outside the kernels -- the two
config keys, the refusals, the argument block's tail against the header.

The reference's own recorded action (tests/golden/action_mode.npz, the draws of synth.NoiseStream(12)) is NOT checked
against the admissible set here: its actor is freshly initialised, std = 4.8 .. 5.2, so u = mean + std e leaves the
regular regime (|u| <= 3) for most draws without reaching the saturated one (|u| >= 16), and none of its 9 rows has all
its draws in a regime the bounds cover (test_golden_rows_are_outside_the_bounds_regimes pins that fact)."""
import os
import re

import pytest
import torch

from big_dreamer_amd import synth
from tests import act_mode_ref as R
from tests import entropy_ref as ER
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(N, A, n, kind) for (N, A, n) in R.SIZES for kind in R.kinds_of(A)]


# ---------------------------------------------------------------------------------------------- the reference and its inputs
def test_golden_rows_are_outside_the_bounds_regimes():
    """Why the recorded action is not held to the admissible set: every one of the 9 rows has draws between the regimes."""
    d = synth.SMALL
    g = load_golden("action_mode")
    N = g["belief"].shape[0]
    eps = torch.from_numpy(synth.NoiseStream(12).normal((d.n_entropy, N, d.A)))
    ok = R.regular_or_saturated(torch.from_numpy(g["mean"]), torch.from_numpy(g["std"]), eps)
    left_out = int((~ok).sum())
    print(f"rows of action_mode.npz left out: {left_out} of {N}")
    assert N == 9 and left_out > 3, "rows qualify now: check the recorded action against the admissible set"
    # the recorded action is still one of its draws, to the golden's tolerance, in every row
    mean, sd = torch.from_numpy(g["mean"]).double(), torch.from_numpy(g["std"]).double()
    y = torch.tanh(mean.unsqueeze(0) + sd.unsqueeze(0) * eps.double())
    miss = (y - torch.from_numpy(g["action"]).double().unsqueeze(0)).abs().amax(-1).min(0).values
    assert float(miss.max()) <= 2e-5


@pytest.mark.parametrize("N, A, n, kind", CASES)
def test_gpu_case_inputs(N, A, n, kind):
    """Conditions on the inputs of tests/test_act_mode_kernels_gpu.py, on the float64 side: every draw regular or
    saturated; at most MULTI_CAP of the rows with more than one admissible index; the float64 winner admissible; an fp32
    emulation of the kernel's rule (entropy_ref.emulate, column-order fp32 sum, first maximum) admissible in every row."""
    mean, sd, eps = R.make_case(N, A, n, kind)
    assert mean.shape == (N, A) and eps.shape == (n, N, A)
    assert bool(R.regular_or_saturated(mean, sd, eps).all())
    u = mean.double().unsqueeze(0) + sd.double().unsqueeze(0) * eps.double()
    if kind == "mixed":
        reg = ER.regime_of(u)
        assert bool((reg == ER.SATURATED).any()) and bool((reg == ER.REGULAR).any())
    adm = R.admissible(mean, sd, eps)
    share = R.multi_share(mean, sd, eps)
    assert share <= R.MULTI_CAP, f"{share:.3f} of the rows have more than one admissible index"
    w = R.winner(mean, sd, eps)
    assert bool(torch.gather(adm, 0, w.view(1, N)).all())
    lp = ER.emulate(mean.unsqueeze(0), sd.unsqueeze(0), eps)[0]
    tot = torch.zeros(n, N)
    for c in range(A):
        tot = tot + lp[..., c]
    got = tot.argmax(0)                      # (first maximum: ties in fp32 are checked against the planted cases below)
    assert bool(torch.gather(adm, 0, got.view(1, N)).all()), "the fp32 emulation's index is not admissible: the bound is too tight"
    if n == 1:
        assert bool(adm.all()) and bool((w == 0).all())


@pytest.mark.parametrize("N, A, n, kind", [c for c in CASES if c[2] in R.TIES])
def test_planted_ties(N, A, n, kind):
    """The planted draws j1 < j2 are identical, stay in their regimes, are the float64 winners (first: j1), and are the
    ONLY admissible indices in at least 1 - MULTI_CAP of the rows (the GPU test demands j1 there, and never j2 anywhere)."""
    mean, sd, eps0 = R.make_case(N, A, n, kind)
    for j1, j2 in R.TIES[n]:
        eps = R.plant_tie(mean, sd, eps0, j1, j2)
        assert j1 < j2 < n and torch.equal(eps[j1], eps[j2])
        assert bool(R.regular_or_saturated(mean, sd, eps).all())
        assert torch.equal(R.winner(mean, sd, eps), torch.full((N,), j1))
        adm = R.admissible(mean, sd, eps)
        assert bool(adm[j1].all()) and bool(adm[j2].all())
        others = (adm.sum(0) > 2).double().mean()
        assert float(others) <= R.MULTI_CAP, f"{float(others):.3f} of the rows admit a third index"


def test_admissible_has_teeth():
    """A log-density evaluated wrongly is caught: the winner under a dropped log-det term, or under a std-less quadratic,
    is inadmissible in most rows of a case."""
    mean, sd, eps = R.make_case(70, 3, 100, "regular")
    adm = R.admissible(mean, sd, eps)
    u = mean.double().unsqueeze(0) + sd.double().unsqueeze(0) * eps.double()
    no_logdet = (-0.5 * eps.double() ** 2).sum(-1).argmax(0)                                   # Normal.log_prob alone
    no_std = (-0.5 * (u - mean.double()) ** 2 + 2 * (u + torch.nn.functional.softplus(-2 * u))).sum(-1).argmax(0)
    last_max = 99 - torch.flip(R.draw_terms(mean, sd, eps)[0], (0,)).argmax(0)                 # control: the true winner
    for name, idx, lo in (("no log-det", no_logdet, 0.5), ("quadratic without 1 / sd^2", no_std, 0.5)):
        bad = 1.0 - float(torch.gather(adm, 0, idx.view(1, -1)).double().mean())
        assert bad >= lo, f"{name}: only {bad:.2f} of the rows inadmissible"
    assert bool(torch.gather(adm, 0, last_max.view(1, -1)).all())


def test_fused_case_samplers_are_decided_outside_the_rounding():
    """tests/test_act_mode_gpu.py compares sampled classes exactly: every Categorical sampler of its fused cases, at q = 1
    where the policy puts it there, shows act_cat_ref.MIN_GAP between the best and the runner-up (float64)."""
    from tests import act_cat_ref as CR
    for name, (d, seed) in R.fused_cases().items():
        P, data = synth.make_params(d, R.FUSED_PARAM_SEED), CR.make_data(d, seed)
        for B in R.FUSED_B:
            for form in ("obs", "emb"):
                for state_mean in (False, True):
                    gap = R.policy_ref(P, d, data, B, form, state_mean)[3]["min_gap"]
                    assert gap > CR.MIN_GAP, (name, B, form, state_mean, gap)


# ---------------------------------------------------------------------------------------------- config, refusals, the block
def test_config_keys():
    from big_dreamer_amd.config import load_config
    cfg = load_config([])
    assert cfg["eval_action"] == "sample" and cfg["eval_state_mean"] is False
    cfg = load_config(["eval_action=mode", "eval_state_mean=true"])
    assert cfg["eval_action"] == "mode" and cfg["eval_state_mean"] is True
    assert load_config(["eval_action=mean"])["eval_action"] == "mean"
    with pytest.raises(ValueError, match="eval_action"):
        load_config(["eval_action=best"])
    with pytest.raises(ValueError, match="eval_state_mean"):
        load_config(["eval_state_mean=perhaps"])


def test_planet_refuses_the_evaluation_policy():
    """PlaNet plans its actions: refused before anything of the agent is touched (no agent is needed to see it)."""
    from big_dreamer_amd.planet import Planet
    with pytest.raises(ValueError, match="PlaNet plans"):
        Planet.update_belief_and_act(None, None, None, None, None, None, action_mode="mode")
    with pytest.raises(ValueError, match="PlaNet plans"):
        Planet.update_belief_and_act(None, None, None, None, None, None, state_mean=True)


def test_run_evaluation_passes_the_policy_and_refuses_an_unknown_one():
    """run_evaluation hands action_mode / state_mean to update_belief_and_act only when they differ from the defaults."""
    from big_dreamer_amd.evaluate import run_evaluation
    seen = []

    class Envs:
        n = 2

        def reset(self):
            return torch.zeros(2, 3)

        def close(self):
            pass

    class Agent:
        device, belief_size, state_size, action_size = "cpu", 4, 3, 1

        def eval(self):
            pass

        def train(self):
            pass

        def update_belief_and_act(self, envs, b, s, a, o, explore=False, **kw):
            seen.append(kw)
            return b, s, a, o, torch.ones(2), torch.ones(2)

    run_evaluation(Agent(), Envs(), 3)
    run_evaluation(Agent(), Envs(), 3, action_mode="mean", state_mean=True)
    run_evaluation(Agent(), Envs(), 3, state_mean=True)
    assert seen == [{}, {"action_mode": "mean", "state_mean": True}, {"action_mode": "sample", "state_mean": True}]
    with pytest.raises(ValueError, match="action_mode"):
        run_evaluation(Agent(), Envs(), 3, action_mode="best")


def _header_struct_fields(name):
    """Field names of a typedef struct of include/bigdreamer_hip.h in declaration order, with 'ptr' / the C type."""
    text = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const float\*|float\*|int\*|unsigned long long|unsigned|float|int) (.*)", decl)
        assert m, decl
        kind = "ptr" if m.group(1).endswith("*") else m.group(1)
        for item in m.group(2).split(","):
            item = item.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", item)
            out.append((arr.group(1), kind, int(arr.group(2))) if arr else (item, kind, 1))
    return out


def test_struct_tail_matches_the_header():
    import ctypes as C
    from big_dreamer_amd import _cabi as cabi
    ctype = {"ptr": (cabi.P,), "int": (C.c_int,), "unsigned": (C.c_uint,), "float": (C.c_float,),
             "unsigned long long": (C.c_ulonglong,)}
    want = _header_struct_fields("bd_act_args")
    got = cabi.ActArgs._fields_
    assert [f[0] for f in got] == [w[0] for w in want]
    for (name, typ), (_, kind, count) in zip(got, want):
        if count > 1:
            assert typ._length_ == count and typ._type_ in ctype[kind], name
        else:
            assert typ in ctype[kind], name
    tail = [f[0] for f in got][-7:]
    assert tail == ["action_mode", "latent_mean", "n_mode", "eps_mode", "stream_mode", "act_stats_out", "mode_index_out"]
    assert [f[0] for f in got][-8] == "action_out", "the evaluation fields are appended behind the sampling step's block"
    a = cabi.ActArgs()                                   # a zeroed tail: the sampling step
    assert a.action_mode == cabi.BD_POLICY_SAMPLE == 0 and a.latent_mean == 0 and a.eps_mode is None
    assert cabi.ACTION_MODES == {"sample": 0, "mode": 1, "mean": 2}
    assert "bd_tanh_normal_mode" in cabi.EXPORTED
    text = open(os.path.join(ROOT, "include", "bigdreamer_hip.h")).read()
    for k, v in (("BD_POLICY_SAMPLE", 0), ("BD_POLICY_MODE", 1), ("BD_POLICY_MEAN", 2)):
        assert re.search(rf"#define {k} {v}\b", text)


def test_entry_points_refuse_bad_policy_arguments():
    """Refusals without a launch: an unknown action_mode, the mode without a draw count, bd_tanh_normal_mode's sizes."""
    import ctypes as C
    from big_dreamer_amd import _cabi as cabi
    a = cabi.ActArgs()
    for name, typ in a._fields_:
        if typ is cabi.P:
            setattr(a, name, 4096)
        elif name in ("w_enc", "b_enc", "w_a", "b_a"):
            for i in range(len(getattr(a, name))):
                getattr(a, name)[i] = 4096
    a.embedding = None
    a.belief_out, a.state_out, a.action_out = 8192, 12288, 16384
    a.B, a.Be, a.S, a.A, a.Hd, a.E, a.O = 1, 24, 6, 2, 20, 40, 5
    for over, text in ((dict(action_mode=3), "action_mode 3"), (dict(action_mode=1, n_mode=0), "n_mode 0"),
                       (dict(action_mode=1, n_mode=100, eps_mode=None), "noise buffers")):
        for k, v in over.items():
            setattr(a, k, v)
        assert cabi.lib.bd_act_step(C.byref(a), None) != 0
        assert text in cabi.lib.bd_last_error().decode(), (over, cabi.lib.bd_last_error())
    for N, A, n in ((0, 2, 10), (1, 65, 10), (1, 2, 0)):
        assert cabi.lib.bd_tanh_normal_mode(4096, 8192, None, 0, 0, 0, N, A, n, 12288, None, None) != 0
        assert "bd_tanh_normal_mode: bad dims" in cabi.lib.bd_last_error().decode()
