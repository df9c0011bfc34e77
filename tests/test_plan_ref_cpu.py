"""CPU: tests/plan_ref.py pinned and shown to discriminate (no GPU).

- The float64 step reference, chained over a whole rollout and a whole CEM loop with fill_layers, equals the float64 oracle
  (oracle.dreamer_oracle.mpc_planner, planner_cat_oracle) to 1e-12 and the reference's own run (golden planner_tiny.npz)
  at the planner tests' tolerances.
- A torch-fp32 emulation of the kernels (same formulas; the refit two-pass with the kernel's lane-strided sum and shuffle
  tree) stays inside the bound for every case of the GPU tables; each planted fault misses it.  Worst ratios and miss
  factors are printed as PLAN_REF lines (run with -s) and recorded in DESIGN.md.
- The ambiguous share of every Categorical case and seed of the GPU test, on the float64 reference.
- PlanDims::lds_floats restated (plan_ref.lds_bytes) against the worked figures in planner.hip's header comment."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from big_dreamer_amd import synth
from oracle import dreamer_oracle as O
from tests import plan_ref as PR
from tests import planner_cat_oracle as PO
from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.dense_ref import C_TOL
from tests.helpers import CSRC, PLANNER_CASES, assert_close, load_golden

MIN_STD = 0.1


def _w64(P):
    return R.to64(PR.weights_of(P))


def _worst(layers, K):
    """check_layers without the assertion: name -> worst err / bound (inf where a zero bound is missed)."""
    rep = {}
    for name, t, sl, ref, S, allow in layers:
        err, bound = (K[name][t][:, sl] - ref).abs(), C_TOL * S + allow
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0).to(err.dtype))
        key = name if name != "feat" else ("h" if sl.start == 0 else "s")
        rep[key] = max(rep.get(key, 0.0), float(ratio.max()))
    return rep


# ---- pins ---------------------------------------------------------------------------------------------------------------

def test_chained_reference_equals_the_gaussian_oracle_and_the_golden_run():
    d0, B, H, iters, cand, top, seed, _ = PLANNER_CASES["planner_tiny"]
    g = load_golden("planner_tiny")
    P = synth.make_params(d0, seed)
    nz = synth.make_planner_noise(d0, B, H, iters, cand, seed)
    tP = {m: {k: torch.as_tensor(v).double() for k, v in sd.items()} for m, sd in P.items()}
    trace = []
    with torch.no_grad():
        want = O.mpc_planner(tP, torch.as_tensor(g["belief"]).double(), torch.as_tensor(g["state"]).double(), d0.A, H, iters,
                             cand, top, torch.as_tensor(nz["action"]).double(), torch.as_tensor(nz["state"]).double(), trace)
    d = PR.PDims(H, B, cand, d0.Be, d0.S, d0.A, d0.Hd)
    W = _w64(P)
    mean, std = torch.zeros(H, B, d.A, dtype=R.D64), torch.ones(H, B, d.A, dtype=R.D64)
    for it in range(iters):
        I = R.to64(dict(init_belief=torch.as_tensor(g["belief"]), init_state=torch.as_tensor(g["state"]), act_mean=mean,
                        act_std=std, eps_action=torch.as_tensor(nz["action"][it]).reshape(H, B * cand, d.A),
                        eps_state=torch.as_tensor(nz["state"][it])))
        K = PR.empty_set(d)
        R.fill_layers(PR.rollout_layers(d, W, I, K, MIN_STD, min_std_f32=False), K)
        ret = K["returns"][0, :, 0]
        assert float((ret - trace[it][0]).abs().max()) <= 1e-12
        assert_close(f"returns{it} (golden)", ret.numpy(), g[f"returns{it}"], 1e-4, 1e-4)
        mean, std, _, _, _ = PR.refit_ref(ret.numpy()[None], K["actions"], H, B, cand, top, d.A)
        assert float((mean - trace[it][1].squeeze(2)).abs().max()) <= 1e-12
        assert float((std - trace[it][2].squeeze(2)).abs().max()) <= 1e-12
    assert float((mean[0] - want).abs().max()) <= 1e-12
    assert_close("action (golden)", mean[0].numpy(), g["action"], 2e-4, 2e-4)


def test_chained_reference_equals_the_categorical_oracle():
    d0, B, H, iters, cand, top, pseed, nseed = PO.PLAN_CASES["cat_tiny"]
    c = PO.make_case(d0, B, H, iters, cand, pseed, nseed)
    nz = c["noise"]
    trace = []
    want = PO.mpc_planner_categorical(c["P"], c["belief"], c["state"], d0, H, iters, cand, top, nz["action"], nz["state"], trace,
                                      torch.float64)
    d = PR.PCDims(H, B, cand, d0.Be, d0.cat_D, d0.cat_C, d0.A, d0.Hd)
    W = _w64(c["P"])
    mean, std = torch.zeros(H, B, d.A, dtype=R.D64), torch.ones(H, B, d.A, dtype=R.D64)
    for it in range(iters):
        I = R.to64(dict(init_belief=torch.as_tensor(c["belief"]), init_state=torch.as_tensor(c["state"]), act_mean=mean,
                        act_std=std, eps_action=torch.as_tensor(nz["action"][it]).reshape(H, B * cand, d.A),
                        eps_state=torch.as_tensor(nz["state"][it])))
        K = PR.empty_set(d)
        R.fill_layers(PR.rollout_layers(d, W, I, K, chain=True), K)
        one = PO.rollout_categorical(c["P"], c["belief"], c["state"], d0, mean, std, nz["action"][it], nz["state"][it], torch.float64)
        for r in (one, trace[it]):
            assert torch.equal(K["sidx"], r["idx"])
            assert float((K["returns"][0, :, 0] - r["returns"]).abs().max()) <= 1e-12
            assert float((K["actions"] - r["actions"]).abs().max()) <= 1e-12
            assert float((K["feat"][..., :d.Be] - r["beliefs"]).abs().max()) <= 1e-12
        mean, std, _, _, _ = PR.refit_ref(K["returns"][0, :, 0].numpy()[None], K["actions"], H, B, cand, top, d.A)
        assert float((mean - trace[it]["mean"]).abs().max()) <= 1e-12 and float((std - trace[it]["std"]).abs().max()) <= 1e-12
    assert float((mean[0] - want).abs().max()) <= 1e-12


def test_refit_selection_follows_the_documented_order():
    nan = float("nan")
    r = np.array([[1.0, nan, 3.0, 3.0, -0.0, 0.0, np.inf, nan, -np.inf, 0.0]], np.float32)
    assert PR.refit_select(r, 10)[0].tolist() == [1, 7, 6, 2, 3, 0, 4, 5, 9, 8]
    # the kernel's sum: from +0, so a candidate whose every step is -0 has the return +0, bit for bit
    s = PR.refit_returns(np.array([[-0.0, 1.0], [-0.0, -1.0]], np.float32), 1, 2)
    assert s.dtype == np.float32 and not np.signbit(s).any()
    assert np.isnan(PR.refit_returns(np.array([[np.inf], [-np.inf]], np.float32), 1, 1)).all()


# ---- the fp32 emulation and its planted faults ----------------------------------------------------------------------------

def emulate(d, W, I, min_std, fault=None):
    """The rollout kernel's formulas in torch fp32 (W, I fp32).  Returns the kernel's outputs as a float64 tensor set."""
    rows, Be, H = d.rows, d.Be, d.H
    ms = torch.tensor(min_std, dtype=torch.float32)
    env = torch.arange(rows) // d.cand
    if fault == "tile_env":           # every per-environment lookup by the tile's first row
        env = (torch.arange(rows) // 16 * 16) // d.cand
    h, s = I["init_belief"][env], I["init_state"][env]
    w0 = s.view(rows, d.D, d.C).abs().max(-1).values if d.cat else None      # the start state's weight per factor
    hist = [h]
    K = PR.empty_set(d)
    ret = torch.zeros(rows)
    Bp = 16 * R.cdiv(Be, 16)
    for t in range(H):
        a = I["act_mean"][t][env] + I["act_std"][t][env] * I["eps_action"][t]
        x = F.elu(torch.cat([s, a], 1) @ W["W_e"].t() + W["b_e"])
        hp = hist[-2] if (fault == "carry" and t == 1) else h
        gi, gh = x @ W["W_ih"].t() + W["b_ih"], hp @ W["W_hh"].t() + W["b_hh"]
        r, z = torch.sigmoid(gi[:, :Be] + gh[:, :Be]), torch.sigmoid(gi[:, Be:2 * Be] + gh[:, Be:2 * Be])
        if fault == "rz":
            r, z = z, r
        n = torch.tanh(gi[:, 2 * Be:] + r * gh[:, 2 * Be:])
        h = (1 - z) * n + z * hp
        hist.append(h)
        p = F.elu(h @ W["W_1"].t() + W["b_1"])
        if d.cat:
            logits = p @ W["W_2"].t() + W["b_2"]
            ratio = torch.softmax(logits.view(rows, d.D, d.C), -1) / I["eps_state"][t].view(rows, d.D, d.C)
            idx = ratio.argmax(-1)
            if fault == "last_max":
                idx = d.C - 1 - ratio.flip(-1).argmax(-1)
            K["sidx"][t] = idx
            s = RC.one_hot_rows(idx, d.C).float()
            sfeat = s
            if fault == "start_weight":
                s = (s.view(rows, d.D, d.C) * w0.unsqueeze(-1)).reshape(rows, -1)
        else:
            S_ = d.S
            b_raw = W["b_2"][:S_] if fault == "std_bias" else W["b_2"][S_:]
            mean, raw = p @ W["W_2"][:S_].t() + W["b_2"][:S_], p @ W["W_2"][S_:].t() + b_raw
            s = mean + (F.softplus(raw) + (0 if fault == "min_std" else ms)) * I["eps_state"][t]
            sfeat = s
        K["actions"][t], K["feat"][t] = a.double(), torch.cat([h, sfeat], 1).double()
        y = torch.cat([h, s], 1)
        if fault == "ff_offset":      # the state columns of ff at the next fragment block; the layer contracts over Be + S
            ff = torch.zeros(rows, Bp + d.S)
            ff[:, :Be], ff[:, Bp:] = h, s
            y = ff[:, :Be + d.S]
        for l in range(4):
            y = F.elu(y @ W["W_r"][l].t() + W["b_r"][l])
        if not (fault == "last_step" and t == H - 1):
            ret = ret + (y @ W["W_r"][4].t() + W["b_r"][4])[:, 0]
    K["returns"][0, :, 0] = ret.double()
    return K


def _case64(d, P, I):
    return _w64(P), R.to64(I), PR.weights_of(P)


def _emulated(d, P, I, fault=None):
    W64, I64, W32 = _case64(d, P, I)
    K = emulate(d, W32, I, MIN_STD, fault)
    return _worst(PR.rollout_layers(d, W64, I64, K, MIN_STD), K), (W64, I64, K)


@pytest.mark.parametrize("name", list(PR.GAUSS_CASES))
def test_emulation_is_inside_the_bound_gaussian(name):
    d, P, I = PR.gauss_case(name)
    rep, _ = _emulated(d, P, I)
    print("PLAN_REF emulation", name, json.dumps(rep))
    assert max(rep.values()) < 1.0, rep


@pytest.mark.parametrize("seed", PR.CAT_SEEDS)
@pytest.mark.parametrize("name", list(PR.CAT_CASES))
def test_emulation_and_ambiguous_share_categorical(name, seed):
    """The emulation inside the bound with every draw inside its margin, and -- on the float64 reference alone -- the
    ambiguous share of the case and seed at or below the cap."""
    d, P, I = PR.cat_case(name, seed)
    rep, (W64, I64, K) = _emulated(d, P, I)
    amb, n, high = PR.sample_checks(d, W64, I64, K)
    Kr = PR.empty_set(d)
    R.fill_layers(PR.rollout_layers(d, W64, I64, Kr, chain=True), Kr)
    amb_ref, n_ref, _ = PR.sample_checks(d, W64, I64, Kr)
    print("PLAN_REF emulation", name, seed, json.dumps(rep), f"ambiguous {amb} of {n}, reference {amb_ref} of {n_ref}")
    assert max(rep.values()) < 1.0, rep
    assert amb_ref <= PR.AMBIGUOUS_CAP * n_ref and amb <= PR.AMBIGUOUS_CAP * n, (amb_ref, amb, n)
    if d.C == 256:
        assert high > n // 2 and int(Kr["sidx"].max()) == 255, f"only {high} of {n} sampled classes are >= 128, or never 255"
    if name == "dup":
        assert RC.duplicate_check(d, torch.zeros(1, d.S), Kr["sidx"]) > 0, "the planted pair never won"
    # the four start kinds occur, and a start weight that is clearly not 1
    if name == "starts":
        w = I["init_state"].view(d.B, d.D, d.C).amax(-1)
        assert {0.0, 0.5, 1.0} <= set(w.flatten().tolist())


GAUSS_FAULTS = {"tile_env": "rows_3x7_h4", "carry": "rows_3x7_h4", "rz": "rows_2x21_h4", "min_std": "rows_2x21_h4",
                "std_bias": "rows_2x21_h4", "ff_offset": "rows_2x21_h4", "last_step": "rows_2x21_h4"}


@pytest.mark.parametrize("fault", list(GAUSS_FAULTS))
def test_planted_faults_miss_the_bound_gaussian(fault):
    d, P, I = PR.gauss_case(GAUSS_FAULTS[fault])
    rep, _ = _emulated(d, P, I, fault)
    print("PLAN_REF fault", fault, json.dumps(rep))
    assert max(rep.values()) > 1.0, (fault, rep)


def test_planted_faults_miss_the_bound_categorical():
    d, P, I = PR.cat_case("starts", PR.CAT_SEEDS[0])
    for fault in ("tile_env", "start_weight"):
        rep, _ = _emulated(d, P, I, fault)
        print("PLAN_REF fault cat", fault, json.dumps(rep))
        assert max(rep.values()) > 1.0, (fault, rep)
    d, P, I = PR.cat_case("dup", PR.CAT_SEEDS[0])
    W64, I64, W32 = _case64(d, P, I)
    K = emulate(d, W32, I, MIN_STD, "last_max")
    with pytest.raises(AssertionError, match="ties with it"):
        RC.duplicate_check(d, torch.zeros(1, d.S), K["sidx"])
    with pytest.raises(AssertionError, match="sample"):
        PR.sample_checks(d, W64, I64, K)


# ---- refit ----------------------------------------------------------------------------------------------------------------

def emulate_refit(ret, act, H, B, cand, top, A, fault=None):
    """cem_refit_kernel in fp32: the sequential return, the key order, the two-pass statistics with 64 lane-strided partial
    sums and the xor shuffle tree."""
    steps = ret.shape[0] - (1 if fault == "steps_minus_1" else 0)
    r = np.zeros(B * cand, np.float32)
    with np.errstate(invalid="ignore"):
        for t in range(steps):
            r = ret[t] if (fault == "neg_zero" and t == 0) else r + ret[t]
    r = r.reshape(B, cand)
    mean, std = torch.zeros(H, B, A), torch.zeros(H, B, A)
    xor = [torch.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]

    def wave_sum(v):                  # [n, H, A] -> [H, A]
        lanes = torch.zeros(64, *v.shape[1:])
        for j0 in range(0, v.shape[0], 64):
            c = v[j0:j0 + 64]
            lanes[:c.shape[0]] = lanes[:c.shape[0]] + c
        for p in xor:
            lanes = lanes + lanes[p]
        return lanes[0]

    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(top), dtype=torch.float32)
    for b in range(B):
        nan = np.isnan(r[b])
        val = np.where(nan, 0.0, -r[b].astype(np.float64))
        if fault != "neg_zero":
            val = val + 0.0
        else:
            val = np.where(np.signbit(r[b]) & (r[b] == 0), 1e-300, val + 0.0)       # -0 ranked strictly below +0
        idx = np.arange(cand) if fault != "tie_high" else -np.arange(cand)
        sel = np.lexsort((idx, val, nan if fault == "nan_last" else ~nan))[:top]
        x = torch.as_tensor(act[:, b * cand + sel]).transpose(0, 1)                  # [top, H, A]
        m = wave_sum(x) * inv
        if fault == "one_pass":
            v = wave_sum(x * x) * inv - m * m
        else:
            v = wave_sum((x - m) ** 2) * (1 / torch.tensor(float(top - 1)) if fault == "unbiased" else inv)
        mean[:, b], std[:, b] = m, v.clamp_min(0).sqrt()
    return mean, std


@pytest.mark.parametrize("case", PR.refit_cases(), ids=lambda c: c[0])
def test_refit_emulation_is_inside_the_bound(case):
    name, (H, B, cand, top, A), rs, rpat, apat, seed = case
    ret, act = PR.refit_inputs(H, B, cand, top, A, rs, seed, rpat, apat)
    ref = PR.refit_ref(ret, torch.as_tensor(act), H, B, cand, top, A)
    rep = {}
    PR.check_refit(name, *emulate_refit(ret, act, H, B, cand, top, A), ref, top, rep)
    print("PLAN_REF refit emulation", name, json.dumps(rep))
    # the patterns are what they claim to be
    r = PR.refit_returns(ret, B, cand)
    if rpat in ("ties", "all_equal", "zeros"):      # a block of equal returns straddles the cut in every environment
        for b in range(B):
            s = np.sort(-r[b])
            assert s[top - 1] == s[min(top, cand - 1)] or top == cand
    if rpat == "zeros":
        assert not np.signbit(r[r == 0]).any() and (np.signbit(ret) & (ret == 0)).any() and (r == 0).sum() > top
    if rpat == "nans_few":
        assert 0 < np.isnan(r).sum(1).min() and np.isnan(r).sum(1).max() < top
    if rpat in ("nans_many", "inf_minus_inf"):
        assert np.isnan(r).sum(1).min() > (top if rpat == "nans_many" else 0)
    if rpat in ("infs", "inf_minus_inf"):
        assert np.isinf(r).any()


REFIT_FAULTS = {"unbiased": ("normal", "normal", 1), "one_pass": ("normal", "offset", 1), "tie_high": ("ties", "normal", 1),
                "nan_last": ("nans_few", "normal", 5), "steps_minus_1": ("normal", "normal", 5), "neg_zero": ("zeros", "normal", 5)}


@pytest.mark.parametrize("fault", list(REFIT_FAULTS))
def test_refit_planted_faults_miss_the_bound(fault):
    rpat, apat, rs = REFIT_FAULTS[fault]
    H, B, cand, top, A = PR.REFIT_MID
    ret, act = PR.refit_inputs(H, B, cand, top, A, rs, 400, rpat, apat)
    ref = PR.refit_ref(ret, torch.as_tensor(act), H, B, cand, top, A)
    mean, std = emulate_refit(ret, act, H, B, cand, top, A, fault)
    miss = max(float(((mean.double() - ref[0]).abs() / ref[2]).max()), float(((std.double() - ref[1]).abs() / ref[3]).max()))
    print("PLAN_REF refit fault", fault, f"{miss:.3g}")
    with pytest.raises(AssertionError, match="refit"):
        PR.check_refit(fault, mean, std, ref, top)


# ---- host formulas ----------------------------------------------------------------------------------------------------------

def test_lds_formula_and_the_case_tables():
    with open(os.path.join(CSRC, "planner.hip")) as fh:
        src = fh.read()
    assert "31504 floats = 126 016 B" in src and "37648 floats = 150 592 B" in src
    assert PR.lds_bytes(200, 30, 6, 200) == 126016 and PR.lds_bytes(200, 1024, 6, 200, 32, 32) == 150592
    assert PR.lds_bytes(448, 6, 2, 20) == 162880 <= R.K_MAX_LDS < PR.lds_bytes(449, 6, 2, 20) == 165952
    assert all(PR.accepts(d) for d in PR.GAUSS_CASES.values()) and all(PR.accepts(d) for d in PR.CAT_CASES.values())
    assert not PR.accepts(PR.GAUSS_TOO_WIDE) and not PR.accepts(PR.GAUSS_CASES["s64"]._replace(S=65))
    # every form of the dual head, the 13-block GRU case and its neighbours, every sampler path
    forms = {PR.dual_head_form(d.S) for d in PR.GAUSS_CASES.values()}
    assert forms == {"splitk", "blocks+tail", "splitk+tail"} or forms == {"splitk", "blocks+tail"}, forms
    assert PR.dual_head_form(32) == "splitk" and PR.dual_head_form(33) == "blocks+tail" and PR.dual_head_form(48) == "blocks+tail"
    nb = {R.cdiv(d.Be, 16) for d in PR.GAUSS_CASES.values()}
    assert {12, 13, 14} - {12} <= nb and 13 in nb and {193, 208, 209} <= {d.Be for d in PR.GAUSS_CASES.values()}
    assert {RC.sample_path(d.C) for d in PR.CAT_CASES.values()} == {"hw", "libm"}
    assert any(d.S > 256 for d in PR.CAT_CASES.values()) and any(d.D == 1 for d in PR.CAT_CASES.values())
    assert any(d.Hd > d.Be for d in PR.CAT_CASES.values()) and any(d.Be > d.Hd for d in PR.CAT_CASES.values())
    assert {(d.D, d.C) for d in PR.CAT_CASES.values()} >= set(PR.CAT_DC)
