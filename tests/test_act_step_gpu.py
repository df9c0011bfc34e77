"""GPU: the fused acting step (csrc/act.hip: bd_act_step; Engine.act_step, Dreamer.act_step, the BD_ACT_FUSED route of
Dreamer.update_belief_and_act) against the reference's recorded decisions (tests/golden/act.npz), against the float64
restatement tests/act_ref.py at widths and row counts that are no multiples of the 16 x 16 tile, and against the composed
path after a weight update."""
import ctypes as C

import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import act_ref
from tests.helpers import assert_close, load_golden
from tests.test_act_ref_cpu import ACTION_NOISE

pytestmark = pytest.mark.gpu

TOL = 2e-5
EDGE = synth.TINY       # Be=24, S=6, Hd=20, E=40, A=2, O=5: no width is a multiple of 16
NAMES = ("belief", "state", "action")


def cu(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).cuda().contiguous()


def _load(agent, P):
    for mod in ("transition_model", "observation_model", "reward_model", "encoder", "actor", "critic", "critic_target"):
        getattr(agent, mod).load_state_dict({k: torch.as_tensor(v) for k, v in P[mod].items()})


class StubEnv:
    """Records what update_belief_and_act hands to env.step; batched: looks like an EnvBatcher (src/env.py:343)."""

    def __init__(self, d, batched=0):
        self.action_size, self.observation_size = d.A, d.O
        self.got = []
        if batched:
            self.n, self.envs = batched, [None] * batched

    def step(self, a):
        self.got.append(a.numpy().copy())
        return None, 0.0, False


def _tiny_agent(d, extra=(), cls=None, env=None):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    ov = [f"belief_size={d.Be}", f"state_size={d.S}", f"hidden_size={d.Hd}", f"embedding_size={d.E}", f"batch_size={d.B}",
          f"seq_len={d.L}", f"planning_horizon={d.H}", "experience_size=100"] + list(extra)
    return (cls or Dreamer)(load_config(ov), env or StubEnv(d))


# ---------------------------------------------------------------------------------------------- golden
@pytest.mark.parametrize("case", ["b1_explore", "b10_eval"])
def test_act_step_matches_the_reference(case):
    """Dreamer.act_step at config-2 size on the reference's own draws: three chained calls, belief / state / action."""
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer
    g = load_golden("act")
    B, explore, seed = (int(x) for x in g[f"{case}.meta"])
    d = synth.CONFIG2
    agent = Dreamer(load_config(["experience_size=100"]), StubEnv(d))
    assert agent.engine.act_step_supported
    _load(agent, synth.make_params(d, seed))
    ns = synth.NoiseStream(seed)
    belief, state, action = torch.zeros(B, d.Be).cuda(), torch.zeros(B, d.S).cuda(), torch.zeros(B, d.A).cuda()
    for i in range(3):
        nz = {"prior": ns.normal((B, d.S)), "post": ns.normal((B, d.S)), "action": ns.normal((B, d.A)),
              "entropy": ns.normal((d.n_entropy, B, d.A))}
        if explore:
            nz["explore"] = ns.normal((B, d.A))
        belief, state, action = agent.act_step(belief, state, action, torch.from_numpy(g[f"{case}.obs"][i]),
                                               explore=bool(explore), _noise={k: cu(v) for k, v in nz.items()})
        for name, t in zip(NAMES, (belief, state, action)):
            assert_close(f"{case}.{name}{i}", t.cpu().numpy(), g[f"{case}.{name}{i}"], TOL, TOL)


# ---------------------------------------------------------------------------------------------- tile edges
@pytest.fixture(scope="module")
def edge():
    """One engine at the edge dims, inputs and noise for 33 rows x 3 calls, and the float64 decisions per (B, explore)."""
    from big_dreamer_amd.engine import DreamerEngine
    d = EDGE
    P = synth.make_params(d, 11)
    eng = DreamerEngine(d, None, "cuda", params=P)
    rng = np.random.Generator(np.random.PCG64(77))
    n = 33
    data = {"belief": rng.standard_normal((n, d.Be)), "state": rng.standard_normal((n, d.S)),
            "action": rng.uniform(-1, 1, (n, d.A)), "obs": rng.standard_normal((3, n, d.O)),
            "emb": rng.standard_normal((3, n, d.E)), "post": rng.standard_normal((3, n, d.S)),
            "act": rng.standard_normal((3, n, d.A)), "exp": rng.standard_normal((3, n, d.A))}
    data = {k: v.astype(np.float32) for k, v in data.items()}
    return eng, P, data


def _chain_gpu(eng, data, B, explore, form="obs"):
    """Three chained engine calls on the first B rows; outputs fed back as inputs.  Returns cloned results per call."""
    b, s, a = cu(data["belief"][:B]), cu(data["state"][:B]), cu(data["action"][:B])
    outs = []
    for i in range(3):
        nz = {"post": cu(data["post"][i, :B]), "action": cu(data["act"][i, :B]), "explore": cu(data["exp"][i, :B])}
        kw = {"obs": cu(data["obs"][i, :B])} if form == "obs" else {"embedding": cu(data["emb"][i, :B])}
        b, s, a = eng.act_step(b, s, a, explore=explore, action_noise=ACTION_NOISE, noise=nz, **kw)
        outs.append(tuple(t.clone() for t in (b, s, a)))
    return outs


def _chain_ref(P, data, B, explore, form="obs"):
    b, s, a = data["belief"][:B], data["state"][:B], data["action"][:B]
    outs = []
    for i in range(3):
        kw = {"obs": data["obs"][i, :B]} if form == "obs" else {"embedding": data["emb"][i, :B]}
        b, s, a = act_ref.act_step(P, b, s, a, data["post"][i, :B], data["act"][i, :B], explore=explore,
                                   eps_explore=data["exp"][i, :B], action_noise=ACTION_NOISE, **kw)
        outs.append((b, s, a))
    return outs


@pytest.mark.parametrize("explore", [False, True])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_tile_edges_against_float64(edge, B, explore):
    eng, P, data = edge
    got, want = _chain_gpu(eng, data, B, explore), _chain_ref(P, data, B, explore)
    for i in range(3):
        for name, t, w in zip(NAMES, got[i], want[i]):
            assert tuple(t.shape) == w.shape
            assert_close(f"B={B} explore={explore} {name}{i}", t.cpu().numpy(), w, TOL, TOL)
    if B == 17:     # a tile must not depend on its neighbours
        alone = _chain_gpu(eng, data, 16, explore)
        for i in range(3):
            for name, t, w in zip(NAMES, got[i], alone[i]):
                assert torch.equal(t[:16], w), f"{name}{i}: rows 0..15 of the 17-row run differ from the 16-row run"


@pytest.mark.parametrize("B", [1, 17])
def test_embedding_form_against_float64(edge, B):
    """obs = NULL and a ready embedding (what a pixel agent hands over after its conv stack)."""
    eng, P, data = edge
    got, want = _chain_gpu(eng, data, B, True, form="emb"), _chain_ref(P, data, B, True, form="emb")
    for i in range(3):
        for name, t, w in zip(NAMES, got[i], want[i]):
            assert_close(f"embedding form B={B} {name}{i}", t.cpu().numpy(), w, TOL, TOL)


# ---------------------------------------------------------------------------------------------- in-kernel noise
def _rng_fill(eng, step, shapes):
    """bd_rng_fill buffers of the act_* streams for decision `step`."""
    from big_dreamer_amd import _cabi as cabi
    r = cabi.RngFillArgs()
    r.n, r.seed, r.step = len(shapes), eng.rng_seed, step
    out = {}
    for i, (key, stream, shape) in enumerate(shapes):
        t = out[key] = torch.zeros(*shape, device="cuda")
        r.t[i] = cabi.RngTensor(t.data_ptr(), t.numel(), cabi.BD_RNG_NORMAL, eng.RNG_STREAMS[stream])
    cabi.check(cabi.lib.bd_rng_fill(C.byref(r), cabi.stream()))
    return out


@pytest.mark.parametrize("B", [1, 17])
def test_in_kernel_noise_is_the_rng_fill_stream(edge, B):
    eng, _, data = edge
    d = EDGE
    eng.set_noise_seed(1234)
    ins = (cu(data["belief"][:B]), cu(data["state"][:B]), cu(data["action"][:B]))
    obs = cu(data["obs"][0, :B])
    shapes = [("post", "act_post", (B, d.S)), ("action", "act_action", (B, d.A)), ("explore", "act_explore", (B, d.A))]
    run = lambda explore, noise: tuple(t.clone() for t in eng.act_step(*ins, obs=obs, explore=explore,
                                                                        action_noise=ACTION_NOISE, noise=noise))
    k = eng._rng_step.get("act", 0)
    plain = run(False, None)                                   # decision k, drawn in the kernel
    assert eng._rng_step["act"] == k + 1
    fed = run(False, _rng_fill(eng, k, shapes))
    for name, x, y in zip(NAMES, plain, fed):
        assert torch.equal(x, y), f"explore=0 {name}: in-kernel draws differ from bd_rng_fill's"
    eng._rng_step["act"] = k                                   # the same decision again, with exploration
    noisy = run(True, None)
    buf = _rng_fill(eng, k, shapes)
    fed = run(True, buf)
    for name, x, y in zip(NAMES, noisy, fed):
        assert torch.equal(x, y), f"explore=1 {name}: in-kernel draws differ from bd_rng_fill's"
    # explore = 0 left the un-noised action; explore = 1 is that action plus the clamp of the explore stream
    assert torch.equal(noisy[0], plain[0]) and torch.equal(noisy[1], plain[1])
    want = torch.clamp(plain[2] + ACTION_NOISE * buf["explore"], -1, 1)
    assert float((noisy[2] - want).abs().max()) <= 1e-6 and not torch.equal(noisy[2], plain[2])
    nxt = run(False, None)                                     # decision k + 1: other draws
    assert eng._rng_step["act"] == k + 2
    assert torch.equal(nxt[0], plain[0]), "the belief takes no noise"
    assert not torch.equal(nxt[1], plain[1]) and not torch.equal(nxt[2], plain[2])


# ---------------------------------------------------------------------------------------------- fresh weights
def test_act_step_reads_the_weights_a_train_step_wrote(monkeypatch):
    """One train step, then act_step: equal to the composed path of an agent loaded from the trained agent's state dicts.
    A kernel reading stale packed weights would miss by far more than the tolerance (lr 1e-2: every weight moves 1e-2)."""
    d = synth.TINY
    agent = _tiny_agent(d)
    _load(agent, synth.make_params(d, 3))
    B = 3
    rng = np.random.Generator(np.random.PCG64(5))
    ins = [cu(rng.standard_normal((B, d.Be))), cu(rng.standard_normal((B, d.S))), cu(rng.uniform(-1, 1, (B, d.A)))]
    obs = torch.from_numpy(rng.standard_normal((B, d.O)).astype(np.float32))
    nz = {"prior": cu(rng.standard_normal((B, d.S))), "post": cu(rng.standard_normal((B, d.S))),
          "action": cu(rng.standard_normal((B, d.A))), "entropy": cu(rng.standard_normal((d.n_entropy, B, d.A))),
          "explore": cu(rng.standard_normal((B, d.A)))}
    before = [t.clone() for t in agent.act_step(*ins, obs, explore=True, _noise=nz)]
    agent.engine.hp.update(model_learning_rate=1e-2, actor_learning_rate=1e-2)
    agent.engine.train_step({k: cu(v) for k, v in synth.make_batch(d, 4).items()},
                            {k: cu(v) for k, v in synth.make_noise(d, 4).items()})
    got = [t.clone() for t in agent.act_step(*ins, obs, explore=True, _noise=nz)]
    assert float((got[0] - before[0]).abs().max()) > 1e-3, "the train step did not move the decision: the test shows nothing"
    monkeypatch.setenv("BD_ACT_FUSED", "0")
    other = _tiny_agent(d, env=StubEnv(d, batched=B))
    assert not other.act_fused
    for mod in ("transition_model", "observation_model", "reward_model", "encoder", "actor", "critic", "critic_target"):
        getattr(other, mod).load_state_dict(getattr(agent, mod).state_dict())
    want = other.update_belief_and_act(other.env, *ins, obs, explore=True, _noise=nz)[:3]
    for name, t, w in zip(NAMES, got, want):
        assert_close(f"after train_step: {name}", t.cpu().numpy(), w.cpu().numpy(), TOL, TOL)


# ---------------------------------------------------------------------------------------------- routing
def test_update_belief_and_act_routes_through_act_step(monkeypatch):
    d = synth.TINY
    B = 2
    env = StubEnv(d, batched=B)
    agent = _tiny_agent(d, env=env)
    _load(agent, synth.make_params(d, 8))
    monkeypatch.setenv("BD_ACT_FUSED", "1")
    assert agent.act_fused
    rng = np.random.Generator(np.random.PCG64(6))
    ins = [cu(rng.standard_normal((B, d.Be))), cu(rng.standard_normal((B, d.S))), cu(rng.uniform(-1, 1, (B, d.A)))]
    obs = torch.from_numpy(rng.standard_normal((B, d.O)).astype(np.float32))
    nz = {"prior": cu(rng.standard_normal((B, d.S))), "post": cu(rng.standard_normal((B, d.S))),
          "action": cu(rng.standard_normal((B, d.A))), "entropy": cu(rng.standard_normal((d.n_entropy, B, d.A))),
          "explore": cu(rng.standard_normal((B, d.A)))}
    want = [t.clone() for t in agent.act_step(*ins, obs, explore=True, _noise=nz)]
    calls = []
    real = agent.engine.act_step
    monkeypatch.setattr(agent.engine, "act_step", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)
    assert calls == [1]
    for t, w in zip(out[:3], want):
        assert torch.equal(t, w)
    assert np.array_equal(env.got[-1], want[2].cpu().numpy()), "the environment got another action than act_step returned"
    # the switch off: the composed path, the same decision to the tolerance
    monkeypatch.setenv("BD_ACT_FUSED", "0")
    out0 = agent.update_belief_and_act(env, *ins, obs, explore=True, _noise=nz)
    assert calls == [1]
    for name, t, w in zip(NAMES, out0[:3], want):
        assert_close(f"composed {name}", t.cpu().numpy(), w.cpu().numpy(), TOL, TOL)


@pytest.mark.parametrize("kind", ["latent", "action"])
def test_categorical_agents_keep_the_composed_path(kind, monkeypatch):
    from big_dreamer_amd.dreamer import Dreamer
    d = synth.CAT_TINY if kind == "latent" else synth.TINY
    extra = (["latent_distribution=Categorical", f"discrete_latent_dimensions={d.cat_D}",
              f"discrete_latent_classes={d.cat_C}"] if kind == "latent" else ["action_distribution=Categorical"])
    env = StubEnv(d)
    agent = _tiny_agent(d, extra, cls=Dreamer, env=env)
    monkeypatch.setenv("BD_ACT_FUSED", "1")
    assert not agent.engine.act_step_supported and not agent.act_fused
    monkeypatch.setattr(agent.engine, "act_step", lambda *a, **k: pytest.fail("the fused kernel was called"))
    zeros = [torch.zeros(1, agent.belief_size).cuda(), torch.zeros(1, agent.state_size).cuda(), torch.zeros(1, d.A).cuda()]
    out = agent.update_belief_and_act(env, *zeros, torch.zeros(1, d.O), explore=True)
    assert tuple(out[0].shape) == (1, d.Be) and tuple(out[2].shape) == (1, d.A) and len(env.got) == 1
    with pytest.raises(NotImplementedError, match="act_step"):
        agent.act_step(*zeros, torch.zeros(1, d.O))


# ---------------------------------------------------------------------------------------------- argument checks
def test_argument_checks_reject_without_launching(edge):
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    d = EDGE
    assert lib.bd_act_step_supported(d.Be, d.S, d.A, d.Hd, d.E, d.O) == 1
    assert lib.bd_act_step_supported(d.Be, d.S, d.A, d.Hd, d.E, 0) == 1            # embedding form
    assert lib.bd_act_step_supported(200, 30, 1, 200, 1024, 3) == 1                # the reference's default sizes
    assert lib.bd_act_step_supported(d.Be, 1024, d.A, d.Hd, d.E, d.O) == 0         # 32 x 32 one-hot latents
    assert lib.bd_act_step_supported(d.Be, d.S, d.A, 1 << 16, d.E, d.O) == 0       # LDS
    assert lib.bd_act_step_supported(d.Be, d.S, 0, d.Hd, d.E, d.O) == 0

    def args(**over):
        """A complete argument block: every pointer names one (never launched on) device buffer."""
        a = cabi.ActArgs()
        a.B, a.Be, a.S, a.A, a.Hd, a.E, a.O = 1, d.Be, d.S, d.A, d.Hd, d.E, d.O
        p = dummy.data_ptr()
        for name, typ in cabi.ActArgs._fields_:
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
    for over, text in (({"action_out": None}, "missing outputs"), ({"Hd": 1 << 16}, "LDS"),
                       ({"belief_out": dummy.data_ptr()}, "aliases"), ({"eps_action": None}, "noise buffers"),
                       ({"embedding": dummy.data_ptr()}, "not both")):
        rc = lib.bd_act_step(C.byref(args(**over)), cabi.stream())
        assert rc < 0 and text in lib.bd_last_error().decode(), (over, rc, lib.bd_last_error())
    torch.cuda.synchronize()
    assert float(dummy.abs().max()) == 0.0
