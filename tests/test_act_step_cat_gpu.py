"""GPU: the fused acting step for Categorical latents and / or the Categorical actor (csrc/act.hip: bd_act_step_cat;
Engine.act_step_cat, Dreamer.act_step_cat, the BD_ACT_FUSED_CAT route of Dreamer.update_belief_and_act) against the
float64 restatement tests/act_cat_ref.py at widths and row counts that are no multiples of the 16 x 16 tile, against the
composed path before and after a weight update, and the uniform kind of bd_rng_fill.

One-hot states, sampled classes and epsilon-greedy actions are compared EXACTLY: tests/test_act_cat_ref_cpu.py asserts that
no sampler call of any case here is decided within the kernels' rounding (act_cat_ref.MIN_GAP)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import act_cat_ref as R
from tests.helpers import assert_close
from tests.test_act_cat_ref_cpu import philox_words, uniform_from_words
from tests.test_act_step_gpu import StubEnv, _load, _tiny_agent, cu

pytestmark = pytest.mark.gpu

TOL = 2e-5              # beliefs, Gaussian states, tanh-Normal actions (tests/test_act_step_gpu.TOL)
ST_TOL = 1e-6           # straight-through action values (onehot + p) - p
NAMES = ("belief", "state", "action")


@pytest.fixture(scope="module")
def cases():
    """Per case of act_cat_ref.CASES, built on first use: engine, parameters, data, and the float64 chains by (B, explore,
    form) -- a reference is computed once and shared."""
    from big_dreamer_amd.engine import DreamerEngine
    made = {}

    def get(name):
        if name not in made:
            d, seed = R.CASES[name]
            P = synth.make_params(d, R.PARAM_SEED)
            made[name] = (DreamerEngine(d, None, "cuda", params=P), P, R.make_data(d, seed), {})
        return made[name]
    return get


def _ref(case, name, B, explore, form="obs"):
    eng, P, data, memo = case
    key = (B, explore, form)
    if key not in memo:
        memo[key] = R.chain(P, eng.d, data, B, explore, form)
    return memo[key]


def _chain_gpu(eng, data, B, explore, form="obs"):
    b, s, a = cu(data["belief"][:B]), cu(data["state"][:B]), cu(data["action"][:B])
    outs = []
    for i in range(3):
        nz = {"post": cu(data["post"][i, :B]), "action": cu(data["act"][i, :B]), "explore": cu(data["exp"][i, :B])}
        kw = {"obs": cu(data["obs"][i, :B])} if form == "obs" else {"embedding": cu(data["emb"][i, :B])}
        b, s, a = eng.act_step_cat(b, s, a, explore=explore, action_noise=R.ACTION_NOISE, noise=nz, **kw)
        outs.append(tuple(t.clone() for t in (b, s, a)))
    return outs


def _compare(d, tag, got, want, explored=None):
    """One decision against its reference under the tolerances of the module docstring."""
    gb, gs, ga = (t.cpu().numpy() for t in got)
    wb, ws, wa = want[:3]
    assert gb.shape == wb.shape and gs.shape == ws.shape and ga.shape == wa.shape
    assert_close(f"{tag} belief", gb, wb, TOL, TOL)
    if d.categorical:
        assert np.array_equal(gs, ws.astype(np.float32)), f"{tag} state: one-hot states differ"
    else:
        assert_close(f"{tag} state", gs, ws, TOL, TOL)
    if d.discrete_actions:
        assert np.array_equal(ga.argmax(1), wa.argmax(1)), f"{tag} action: sampled classes differ"
        assert float(np.abs(ga - wa).max()) <= ST_TOL, f"{tag} action: straight-through values off by {np.abs(ga - wa).max():.3e}"
        if explored is not None:
            assert np.array_equal(ga[explored], np.asarray(wa, dtype=np.float32)[explored]), f"{tag}: explored rows are exact one-hots"
    else:
        assert_close(f"{tag} action", ga, wa, TOL, TOL)


# ---------------------------------------------------------------------------------------------- 1, 2: float64
@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
@pytest.mark.parametrize("name", list(R.CASES))
def test_tile_edges_against_float64(cases, name, B, explore):
    case = cases(name)
    eng, _, data, _ = case
    assert eng.act_step_cat_supported and not eng.act_step_supported
    got, want = _chain_gpu(eng, data, B, explore), _ref(case, name, B, explore)
    for i in range(3):
        _compare(eng.d, f"{name} B={B} explore={explore} call {i}", got[i], want[i], want[i][3].get("explored"))
    if B == 17:     # a tile must not depend on its neighbours
        alone = _chain_gpu(eng, data, 16, explore)
        for i in range(3):
            for n, t, w in zip(NAMES, got[i], alone[i]):
                assert torch.equal(t[:16], w), f"{n}{i}: rows 0..15 of the 17-row run differ from the 16-row run"


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("name", list(R.CASES))
def test_embedding_form_against_float64(cases, name, B):
    case = cases(name)
    eng, _, data, _ = case
    got, want = _chain_gpu(eng, data, B, True, form="emb"), _ref(case, name, B, True, form="emb")
    for i in range(3):
        _compare(eng.d, f"{name} embedding form B={B} call {i}", got[i], want[i], want[i][3].get("explored"))


# ---------------------------------------------------------------------------------------------- 3: the composed path
AGENT_KINDS = {      # kind -> (dims, config overrides)
    "cat_tanh": (synth.CAT_TINY, ["latent_distribution=Categorical", "discrete_latent_dimensions=3", "discrete_latent_classes=5"]),
    "cat_disc": (dataclasses.replace(synth.CAT_TINY, A=3, discrete_actions=True),
                 ["latent_distribution=Categorical", "discrete_latent_dimensions=3", "discrete_latent_classes=5",
                  "action_distribution=Categorical"]),
    "gauss_disc": (dataclasses.replace(synth.TINY, A=3, discrete_actions=True), ["action_distribution=Categorical"]),
}


def _agent_inputs(d, B, seed):
    """Inputs and the composed route's `_noise` of one decision; explore_u straddles action_noise."""
    data = R.make_data(d, seed, n=B, calls=1)
    ins = [cu(data["belief"]), cu(data["state"]), cu(data["action"])]
    nz = {"prior": torch.ones(B, d.S).cuda(), "post": cu(data["post"][0]), "action": cu(data["act"][0])}
    if d.discrete_actions:
        u = data["exp"][0, :, 0]
        u[0], u[1] = 0.01, 0.99          # row 0 explores, row 1 does not, whatever action_noise in (0.01, 0.99) is configured
        nz["explore_u"] = cu(u)
        nz["explore_k"] = torch.as_tensor(np.arange(B) % d.A).cuda()
    else:
        nz["entropy"] = torch.randn(d.n_entropy, B, d.A, generator=torch.Generator().manual_seed(seed)).cuda()
        nz["explore"] = cu(data["exp"][0])
    return ins, torch.from_numpy(data["obs"][0]), nz


def _min_gap(agent, d, ins, obs, nz):
    """Smallest sampler gap of the decision under the agent's CURRENT weights (float64 restatement)."""
    mods = ("transition_model", "encoder", "actor")
    P = {m: {k: v.detach().cpu().numpy() for k, v in getattr(agent, m).state_dict().items()} for m in mods}
    n = lambda t: t.cpu().numpy()
    return R.act_step_cat(P, d, *(n(t) for t in ins), n(nz["post"]), n(nz["action"]), obs=obs.numpy())[3]["min_gap"]


def _same_decision(d, tag, got, want, min_gap):
    """Exact one-hots are demanded where the float64 restatement shows them decided outside the kernels' rounding."""
    assert min_gap > R.MIN_GAP, f"{tag}: a sample of these inputs is decided within {min_gap:.2e}: choose another data seed"
    for n, t, w in zip(NAMES, got, want):
        t, w = t.cpu().numpy(), w.cpu().numpy()
        if (n == "state" and d.categorical):
            assert np.array_equal(t, w), f"{tag} {n}: one-hot states differ"
        elif n == "action" and d.discrete_actions:
            assert np.array_equal(t.argmax(1), w.argmax(1)) and float(np.abs(t - w).max()) <= ST_TOL, f"{tag} {n}"
        else:
            assert_close(f"{tag} {n}", t, w, TOL, TOL)


@pytest.mark.parametrize("kind", list(AGENT_KINDS))
def test_agent_equals_the_composed_path_before_and_after_a_train_step(kind, monkeypatch):
    d, extra = AGENT_KINDS[kind]
    monkeypatch.delenv("BD_ACT_FUSED_CAT", raising=False)
    B = 5
    env = StubEnv(d, batched=B)
    agent = _tiny_agent(d, extra, env=env)
    assert agent.dims.A == d.A and agent.dims.discrete_actions == d.discrete_actions
    _load(agent, synth.make_params(d, 3))
    assert 0.01 < agent.action_noise < 0.99
    ins, obs, nz = _agent_inputs(d, B, 21)
    assert not agent.act_fused and not agent.act_fused_cat
    before = [t.clone() for t in agent.act_step_cat(*ins, obs, explore=True, _noise=nz)]
    want = agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)[:3]
    _same_decision(d, kind, before, want, _min_gap(agent, d, ins, obs, nz))
    if d.discrete_actions:      # the explored row took its class exactly, the other row kept the actor's sample
        a = before[2].cpu().numpy()
        assert np.array_equal(a[0], np.eye(d.A, dtype=np.float32)[0])
    agent.engine.hp.update(model_learning_rate=1e-2, actor_learning_rate=1e-2)
    agent.engine.train_step({k: cu(v) for k, v in synth.make_batch(d, 4).items()},
                            {k: cu(v) for k, v in synth.make_noise(d, 4).items()})
    got = [t.clone() for t in agent.act_step_cat(*ins, obs, explore=True, _noise=nz)]
    assert float((got[0] - before[0]).abs().max()) > 1e-3, "the train step did not move the decision: the test shows nothing"
    want = agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)[:3]
    _same_decision(d, f"{kind} after train_step", got, want, _min_gap(agent, d, ins, obs, nz))


# ---------------------------------------------------------------------------------------------- 4: in-kernel noise
def _rng_fill(eng, step, shapes):
    from big_dreamer_amd import _cabi as cabi
    r = cabi.RngFillArgs()
    r.n, r.seed, r.step = len(shapes), eng.rng_seed, step
    out = {}
    for i, (key, stream, shape, kind) in enumerate(shapes):
        t = out[key] = torch.zeros(*shape, device="cuda")
        r.t[i] = cabi.RngTensor(t.data_ptr(), t.numel(), kind, eng.RNG_STREAMS[stream])
    cabi.check(cabi.lib.bd_rng_fill(C.byref(r), cabi.stream()))
    return out


@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("name", ["cat3x5_tanh", "cat32_disc18", "gauss_disc2"])
def test_in_kernel_noise_is_the_rng_fill_stream(cases, name, B):
    from big_dreamer_amd import _cabi as cabi
    eng, _, data, _ = cases(name)
    d = eng.d
    eng.set_noise_seed(1234)
    ins = (cu(data["belief"][:B]), cu(data["state"][:B]), cu(data["action"][:B]))
    obs = cu(data["obs"][0, :B])
    shapes = [("post", "act_post", (B, d.S), cabi.BD_RNG_EXPONENTIAL if d.categorical else cabi.BD_RNG_NORMAL),
              ("action", "act_action", (B, d.A), cabi.BD_RNG_EXPONENTIAL if d.discrete_actions else cabi.BD_RNG_NORMAL),
              ("explore", "act_explore", (B, 2), cabi.BD_RNG_UNIFORM) if d.discrete_actions else
              ("explore", "act_explore", (B, d.A), cabi.BD_RNG_NORMAL)]
    run = lambda explore, noise: tuple(t.clone() for t in eng.act_step_cat(*ins, obs=obs, explore=explore,
                                                                            action_noise=R.ACTION_NOISE, noise=noise))
    k = eng._rng_step.get("act", 0)
    plain = run(False, None)
    assert eng._rng_step["act"] == k + 1, "the decision counter advances by one per call"
    fed = run(False, _rng_fill(eng, k, shapes))
    for n, x, y in zip(NAMES, plain, fed):
        assert torch.equal(x, y), f"explore=0 {n}: in-kernel draws differ from bd_rng_fill's"
    eng._rng_step["act"] = k
    noisy = run(True, None)
    fed = run(True, _rng_fill(eng, k, shapes))
    for n, x, y in zip(NAMES, noisy, fed):
        assert torch.equal(x, y), f"explore=1 {n}: in-kernel draws differ from bd_rng_fill's"
    assert torch.equal(noisy[0], plain[0]) and torch.equal(noisy[1], plain[1]), "exploration touches the action alone"
    nxt = run(False, None)
    assert eng._rng_step["act"] == k + 2
    assert torch.equal(nxt[0], plain[0]), "the belief takes no noise"
    if B == 17 or not d.categorical:        # (three factors of one row can repeat by chance)
        assert not torch.equal(nxt[1], plain[1]), "decision k + 1 drew the same state"


# ---------------------------------------------------------------------------------------------- 5: routing
@pytest.mark.parametrize("kind", list(AGENT_KINDS))
def test_update_belief_and_act_routes_by_the_switch(kind, monkeypatch):
    d, extra = AGENT_KINDS[kind]
    B = 2
    env = StubEnv(d, batched=B)
    agent = _tiny_agent(d, extra, env=env)
    _load(agent, synth.make_params(d, 8))
    ins, obs, nz = _agent_inputs(d, B, 22)
    calls = []
    real = agent.engine.act_step_cat
    monkeypatch.setattr(agent.engine, "act_step_cat", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.delenv("BD_ACT_FUSED_CAT", raising=False)
    agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)
    assert calls == [] and not agent.act_fused_cat, "the switch is off by default"
    monkeypatch.setenv("BD_ACT_FUSED_CAT", "1")           # read at every call
    assert agent.act_fused_cat and not agent.act_fused
    out = agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)
    assert calls == [1]
    assert np.array_equal(env.got[-1], out[2].cpu().numpy()), "the environment got another action than act_step_cat returned"
    monkeypatch.setenv("BD_ACT_FUSED_CAT", "0")
    agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)
    assert calls == [1]


def test_gaussian_tanh_agents_never_take_this_route(monkeypatch):
    from big_dreamer_amd import _cabi as cabi
    d = synth.TINY
    env = StubEnv(d)
    agent = _tiny_agent(d, env=env)
    monkeypatch.setenv("BD_ACT_FUSED_CAT", "1")
    assert not agent.engine.act_step_cat_supported and not agent.act_fused_cat
    assert cabi.lib.bd_act_step_cat_supported(d.Be, 0, 0, d.S, d.A, d.Hd, d.E, d.O, 0, 0) == 0
    monkeypatch.setattr(agent.engine, "act_step_cat", lambda *a, **k: pytest.fail("the Categorical kernel was called"))
    zeros = [torch.zeros(1, d.Be).cuda(), torch.zeros(1, d.S).cuda(), torch.zeros(1, d.A).cuda()]
    agent.update_belief_and_act(env, *zeros, torch.zeros(1, d.O), explore=True)
    assert len(env.got) == 1
    with pytest.raises(NotImplementedError, match="act_step_cat"):
        agent.act_step_cat(*zeros, torch.zeros(1, d.O))


# ---------------------------------------------------------------------------------------------- 6: argument checks
def test_argument_checks_reject_without_launching(cases):
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    eng = cases("cat3x5_disc18")[0]
    d = eng.d
    sup = lib.bd_act_step_cat_supported
    assert sup(d.Be, d.cat_D, d.cat_C, d.S, d.A, d.Hd, d.E, d.O, 1, 1) == 1
    for A, ac in ((18, 1), (17, 0)):        # BASELINE configs[4] sizes, observation form and embedding form
        assert sup(200, 32, 32, 1024, A, 200, 1024, 3, 1, ac) == 1 and sup(200, 32, 32, 1024, A, 200, 1024, 0, 1, ac) == 1
    assert sup(200, 0, 0, 30, 18, 200, 1024, 3, 0, 1) == 1
    assert sup(200, 32, 32, 1024, 65, 200, 1024, 3, 1, 1) == 0          # one lane per class
    assert sup(200, 32, 32, 1024, 18, 1 << 16, 1024, 3, 1, 1) == 0      # LDS
    assert sup(200, 32, 32, 1000, 18, 200, 1024, 3, 1, 1) == 0          # S != D * C
    assert sup(200, 3, 300, 900, 18, 200, 1024, 3, 1, 1) == 0           # C above 256
    assert sup(200, 0, 0, 30, 1, 200, 1024, 3, 0, 0) == 0               # bd_act_step's configuration

    def args(**over):
        """A complete argument block: every pointer names one (never launched on) device buffer."""
        a = cabi.ActCatArgs()
        a.B, a.Be, a.D, a.C, a.S, a.A, a.Hd, a.E, a.O = 1, d.Be, d.cat_D, d.cat_C, d.S, d.A, d.Hd, d.E, d.O
        a.latent_cat, a.actor_cat = 1, 1
        p = dummy.data_ptr()
        for name, typ in cabi.ActCatArgs._fields_:
            if typ is cabi.P:
                setattr(a, name, p)
            elif name in ("w_enc", "b_enc", "w_a", "b_a"):
                arr = getattr(a, name)
                for i in range(len(arr)):
                    arr[i] = p
        a.embedding = None
        a.belief_out, a.state_out, a.action_out = p + 64, p + 128, p + 192
        for k, v in over.items():
            setattr(a, k, v)
        return a

    dummy = torch.zeros(1024, device="cuda")
    torch.cuda.synchronize()
    for over, text in (({"action_out": None}, "missing outputs"), ({"Hd": 1 << 16}, "LDS"), ({"state": None}, "missing inputs"),
                       ({"belief_out": dummy.data_ptr()}, "aliases"), ({"eps_action": None}, "noise buffers"),
                       ({"embedding": dummy.data_ptr()}, "not both"), ({"w_q2": None}, "missing transition weights"),
                       ({"w_a0sT": None}, "missing actor weights"), ({"A": 65}, "action width"),
                       ({"latent_cat": 0, "actor_cat": 0, "S": 6}, "that configuration is bd_act_step")):
        rc = lib.bd_act_step_cat(C.byref(args(**over)), cabi.stream())
        assert rc < 0 and text in lib.bd_last_error().decode(), (over, rc, lib.bd_last_error())
    torch.cuda.synchronize()
    assert float(dummy.abs().max()) == 0.0
    # a factor with two non-zero classes cannot be carried as a class index: refused, not silently sampled
    data = cases("cat3x5_disc18")[2]
    bad = data["state"][:2].copy()
    bad[1, :2] = 1.0
    before = eng._rng_step.get("act", 0)
    with pytest.raises(ValueError, match="one-hot"):
        eng.act_step_cat(cu(data["belief"][:2]), cu(bad), cu(data["action"][:2]), obs=cu(data["obs"][0, :2]))
    assert eng._rng_step.get("act", 0) == before, "a refused call must not consume a decision index"


# ---------------------------------------------------------------------------------------------- 7: uniform draws
def test_rng_fill_uniform_kind():
    """BD_RNG_UNIFORM equals the host twin bit for bit; the other kinds, filled in the same launch, equal their fills alone."""
    from big_dreamer_amd import _cabi as cabi
    from tests.test_rng_gpu import _fill
    seed, step = 0x0123456789ABCDEF, 7
    n = 1030                                    # past one block of 1024, not a multiple of 4
    u, nrm, ex = (torch.zeros(n, device="cuda") for _ in range(3))
    _fill([(nrm, cabi.BD_RNG_NORMAL, 8), (u, cabi.BD_RNG_UNIFORM, 10), (ex, cabi.BD_RNG_EXPONENTIAL, 9)], seed, step)
    got = u.cpu().numpy()
    assert float(got.min()) >= 0.0 and float(got.max()) < 1.0
    assert np.array_equal(got, uniform_from_words(philox_words(seed, step, 10, (n + 3) // 4))[:n])
    # the normal and exponential kinds: the same bits as a fill of their own, and the values of the host words
    for t, kind, sid in ((nrm, cabi.BD_RNG_NORMAL, 8), (ex, cabi.BD_RNG_EXPONENTIAL, 9)):
        alone = torch.zeros(n, device="cuda")
        _fill([(alone, kind, sid)], seed, step)
        assert torch.equal(alone, t)
    w = philox_words(seed, step, 9, (n + 3) // 4)[:n]
    u01 = ((w >> 8).astype(np.float64) + 0.5) / 2.0 ** 24
    # float32 against float64: u01 rounds its 25th bit (2^-25 relative, 3e-8 in the logarithm), logf is 1 ulp
    assert_close("exponential kind", ex.cpu().numpy(), -np.log(u01), 1e-6, 1e-6)
    w = philox_words(seed, step, 8, (n + 3) // 4).reshape(-1, 2)
    u0, u1 = (((w[:, j] >> 8).astype(np.float64) + 0.5) / 2.0 ** 24 for j in (0, 1))
    r = np.sqrt(-2.0 * np.log(u0))
    want = np.stack([r * np.cos(2 * np.pi * u1), r * np.sin(2 * np.pi * u1)], 1).reshape(-1)[:n]
    # the angle 2 pi u is rounded to float32 (up to 6.28 * 2^-24 = 3.7e-7) and scaled by r <= sqrt(50 ln 2) = 5.9: 2.2e-6,
    # plus the 1-ulp errors of logf, sqrtf and sincosf relative to the value
    assert_close("normal kind", nrm.cpu().numpy(), want, 4e-6, 1e-6)
    bad = cabi.RngFillArgs()
    bad.n, bad.seed, bad.step = 1, seed, step
    bad.t[0] = cabi.RngTensor(u.data_ptr(), n, 3, 1)
    assert cabi.lib.bd_rng_fill(C.byref(bad), cabi.stream()) < 0 and b"bad descriptor" in cabi.lib.bd_last_error()
