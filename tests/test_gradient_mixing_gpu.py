"""GPU tests of ActorCritic.gradient_mixing (DreamerV2's REINFORCE / dynamics-backprop actor gradient): the
bd_actor_reinforce kernel against autograd, two whole train steps against the CPU restatement (tests/mixing_oracle.py)
for the three schedules, rho = 1 against -1 bit for bit, the pipelined schedule against the serial one, the launches the
rho = 0 schedule leaves out, and the drop-in surface."""
import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from oracle import dreamer_oracle as O
from tests.helpers import CASES, CAT_CASES, assert_close
from tests.mixing_oracle import MixingOracleDreamer, actor_head, tanh_normal_log_density

pytestmark = pytest.mark.gpu

SLOT = 11


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("A", [1, 3, 17])
@pytest.mark.parametrize("Hm,N", [(3, 37), (2, 700)])     # 111 rows (not a multiple of anything); several workgroups
@pytest.mark.parametrize("weighted", [False, True])
def test_actor_reinforce_kernel_vs_autograd(A, Hm, N, weighted):
    from big_dreamer_amd import _cabi
    lib, ptr = _cabi.lib, _cabi.ptr
    g = torch.Generator().manual_seed(A * 1000 + N + int(weighted))
    rows = Hm * N
    f64 = dict(generator=g, dtype=torch.float64)
    out = torch.randn(rows, 2 * A, **f64) * 2.0          # raw actor head outputs
    eps = torch.randn(rows, A, **f64).float().double()
    ret = torch.randn(rows, **f64).float().double()
    base0 = torch.randn(N, **f64).float().double()
    value = torch.randn(rows, **f64).float().double()
    w = (torch.rand(rows, **f64) * 0.99).float().double() if weighted else torch.ones(rows, dtype=torch.float64)
    dm, ds = torch.randn(rows, A, **f64).float().double(), torch.randn(rows, A, **f64).float().double()
    rho, inv, dent = 0.3, 1.0 / rows, -1e-2 / rows
    b = torch.cat([base0, value[:rows - N]])
    adv = ret - b
    c = -(1 - rho) * inv * w * adv
    # reference (float64 autograd): d/d head of  sum c l  and, in write mode, of the entropy term
    # sum dent w (dm mean + ds std)  (dm, ds: d entropy / d mean, d std as bd_actor_entropy leaves them)
    x = out.clone().requires_grad_(True)
    mean_r, std_r = actor_head(x)
    u = (mean_r + std_r * eps).detach()
    lp = tanh_normal_log_density(u, mean_r, std_r)
    g_rf, = torch.autograd.grad((c * lp).sum(), x, retain_graph=True)
    g_ent, = torch.autograd.grad((dent * w[:, None] * (dm * mean_r + ds * std_r)).sum(), x)
    lw = w * adv * lp.detach()
    ref_sum = float(lw.sum())
    # the kernel's inputs, as the forward scan and bd_actor_entropy leave them (fp32)
    m, r = out[:, :A], out[:, A:]
    th, sg = torch.tanh(m / O.ACT_MEAN_SCALE), torch.sigmoid(r + O.RAW_INIT_STD)
    stats = torch.cat([th, sg, dm, ds], 1)
    us = torch.cat([u, std_r.detach()], 1)
    d0 = torch.randn(rows, 2 * A, **f64).float()
    cu = lambda t: t.float().cuda().contiguous()
    dev = dict(eps=cu(eps), us=cu(us), stats=cu(stats), ret=cu(ret), base0=cu(base0), value=cu(value), w=cu(w))
    ws = torch.zeros(int(lib.bd_reduce_ws_floats()), device="cuda")
    results = {}
    for write in (0, 1):
        dout = d0.clone().cuda()
        sc = torch.zeros(16, device="cuda")
        _cabi.check(lib.bd_actor_reinforce(ptr(dev["eps"]), ptr(dev["us"]), ptr(dev["stats"]), ptr(dev["ret"]),
                                           ptr(dev["base0"]), ptr(dev["value"]), ptr(dev["w"]) if weighted else None,
                                           Hm, N, A, rho, inv, dent, write, ptr(dout), ptr(sc), SLOT, ptr(ws),
                                           _cabi.stream()))
        torch.cuda.synchronize()
        results[write] = (dout.cpu().double(), sc.cpu())
    want = {0: d0.double() + g_rf, 1: g_rf + g_ent}
    for write, (got, sc) in results.items():
        scale = float(want[write].abs().max())
        assert_close(f"d_actor_out(write={write})", got.numpy(), want[write].numpy(), 2e-5 * scale, 1e-4)
        assert_close("slot", float(sc[SLOT]), ref_sum, 1e-5 * float(lw.abs().sum()), 1e-5)
        assert float(sc[:SLOT].abs().sum()) == 0 and float(sc[SLOT + 1:].abs().sum()) == 0
    assert torch.equal(results[0][1], results[1][1]), "the sum must not depend on the mode"


# ------------------------------------------------------------------------------------------ whole train steps
_STEP_CASES = [("tiny", 0.0), ("tiny", 0.1), ("tiny", 0.5), ("small", 0.0), ("small", 0.1), ("small", 0.5),
               ("config1", 0.1), ("tiny_discount", 0.1), ("tiny_pixel", 0.1), ("cat_tiny", 0.0), ("cat_tiny", 0.1)]


def _case(name):
    if name in CAT_CASES:
        d, seed, hp, _ = CAT_CASES[name]
        return d, seed, dict(hp), dict(hp, categorical=(d.cat_D, d.cat_C))
    d, seed, hp, _ = CASES[name]
    return d, seed, dict(hp), dict(hp)


@pytest.mark.parametrize("name,rho", _STEP_CASES)
def test_train_steps_vs_restatement(name, rho):
    """Two whole train steps with mixing rho: logs, clipped gradients, gradient norms, post-Adam weights against the CPU
    restatement, at the tolerances of test_hip_parity.test_train_steps_vs_oracle_and_golden."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, ohp = _case(name)
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
    od = MixingOracleDreamer(P, dict(ohp, planning_horizon=d.H, gradient_mixing=rho))
    db = _dev(batch)
    rep = []

    def rel(tag, got, want, atol, rtol):
        got, want = np.asarray(got, dtype=np.float64).reshape(np.shape(want)), np.asarray(want, dtype=np.float64)
        rep.append(f"{tag:28s} max|err|={np.abs(got - want).max():.3e}  max|ref|={np.abs(want).max():.3e}")
        assert_close(tag, got, want, atol, rtol)

    try:
        for step in range(2):
            nz = synth.make_noise(d, seed + step)
            ologs = od.train_step(batch, nz)
            logs = eng.train_step(db, _dev(nz))
            if step == 0:
                od.update_critic()
                eng.update_critic()
            torch.cuda.synchronize()
            eng.cluster_status(d.B)
            assert set(ologs) <= set(logs)
            for k, v in ologs.items():
                tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                rel(f"s{step}.{k}", logs[k], v, *tol)
            gn = od.last["grad_norms"]
            rel(f"s{step}.grad_norms", [logs["grad_norm_model"], logs["grad_norm_actor"], logs["grad_norm_critic"]],
                [gn["model"], gn["actor"], gn["critic"]], 1e-6, 1e-3)
            coef = {k: min(1.0, od.hp["grad_clip_norm"] / (gn[k] + 1e-6)) for k in gn}
            groups = {"model": (od.model_modules, od.last["model_grads"]), "actor": (("actor",), od.last["actor_grads"]),
                      "critic": (("critic",), od.last["critic_grads"])}
            for grp, (mods, grads) in groups.items():
                i = 0
                for mod in mods:
                    for k in od.P[mod]:
                        want = grads[i].numpy() * coef[grp]
                        scale = float(np.abs(want).max()) + 1e-12
                        rel(f"s{step}.grad.{mod}.{k}", eng.G(mod, k).detach().cpu().numpy(), want, 2e-3 * scale + 1e-9,
                            2e-3)
                        i += 1
            for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
                for k, p in od.P[mod].items():
                    rel(f"s{step}.param.{mod}.{k}", eng.W(mod, k).detach().cpu().numpy(), p.detach().numpy(), 2e-5, 1e-5)
    finally:
        print("\n".join(rep[-200:]))


def _weights_equal(a, b):
    for grp in ("model", "actor", "critic", "critic_target"):
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat), grp
        if ga.grad is not None:
            assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp


@pytest.mark.parametrize("name", ["small", "cat_tiny"])
def test_rho_one_is_bit_identical_to_minus_one(name):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name)
    P = synth.make_params(d, seed)
    out = []
    for rho in (-1, 1):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        logs = []
        for step in range(2):
            logs.append(eng.train_step(_dev(synth.make_batch(d, seed + step)), _dev(synth.make_noise(d, seed + step))))
            if step == 0:
                eng.update_critic()
        torch.cuda.synchronize()
        out.append((eng, logs))
    _weights_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


@pytest.mark.parametrize("name", ["small", "cat_tiny"])
@pytest.mark.parametrize("rho", [0.0, 0.1])
def test_pipelined_schedule_is_bit_identical_to_serial(name, rho):
    """As test_hip_parity.test_pipelined_schedule_is_bit_identical_to_serial, with the mixed objective: four
    un-synchronised steps, lazy and synchronous logs, every weight, Adam moment and logged scalar."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name)
    P = synth.make_params(d, seed)
    engs = []
    for pipe, defer in ((True, False), (False, False), (True, True)):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.pipeline, eng.defer_opt = pipe, defer
        engs.append(eng)
    steps = 4
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    torch.cuda.synchronize()
    logs, lazy = [], []
    for eng in engs:
        for i in range(steps):
            lz = eng.train_step(batches[i], noises[i], sync_logs="lazy")
            if i == 1:
                eng.update_critic()
        lazy.append(dict(lz))
        logs.append(eng.logs())
        torch.cuda.synchronize()
    for i, a in enumerate(engs):
        _weights_equal(a, engs[1])
        assert logs[i] == logs[1], i
        assert lazy[i] == lazy[1] == logs[1], i
    assert np.isfinite(list(logs[0].values())).all()


@pytest.mark.parametrize("name", ["small", "cat_tiny"])
def test_rho_zero_runs_no_imagination_backward(name):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = _case(name)
    P = synth.make_params(d, seed)
    spans = {}
    for rho in (-1, 0.0, 0.1):
        eng = DreamerEngine(d, dict(hp, gradient_mixing=rho), "cuda", params=P)
        eng.enable_timers(True)
        eng.train_step(_dev(synth.make_batch(d, seed)), _dev(synth.make_noise(d, seed)))
        torch.cuda.synchronize()
        spans[rho] = set(eng.timer_summary())
    assert {"imagine_bwd", "img_heads_bwd"} <= spans[-1] and "actor_reinforce" not in spans[-1]
    assert {"imagine_bwd", "img_heads_bwd", "actor_reinforce"} <= spans[0.1]
    assert not {"imagine_bwd", "img_heads_bwd"} & spans[0.0], spans[0.0]
    assert {"imagine_fwd", "actor_reinforce", "actor_hidden_bwd", "wgrad_actor"} <= spans[0.0]


# ------------------------------------------------------------------------------------------ drop-in surface
@pytest.mark.parametrize("algo,rho", [("dreamerV2", 0.0), ("dreamer", 0.1)])
def test_surface_trains_and_acts_with_mixing(algo, rho):
    from big_dreamer_amd.config import load_config
    from big_dreamer_amd.dreamer import Dreamer, DreamerV2
    from big_dreamer_amd.env import SyntheticEnv
    d = synth.SMALL
    ov = [f"belief_size={d.Be}", f"hidden_size={d.Hd}", f"embedding_size={d.E}", f"batch_size={d.B}",
          f"seq_len={d.L}", f"planning_horizon={d.H}", "experience_size=400", "seed_steps=120", "max_episode_length=40",
          f"ActorCritic.gradient_mixing={rho}"]
    if algo == "dreamerV2":
        ov += ["algorithm=dreamerV2", "latent_distribution=Categorical", "discrete_latent_dimensions=4",
               "discrete_latent_classes=5", "state_size=20"]
    else:
        ov += [f"state_size={d.S}"]
    params = load_config(ov)
    env = SyntheticEnv(d.O, d.A, 40, 2, 0)
    torch.manual_seed(0)
    agent = (DreamerV2 if algo == "dreamerV2" else Dreamer)(params, env)
    assert agent.engine.hp["gradient_mixing"] == rho
    np.random.seed(0)
    agent.randomly_initialize_replay_buffer()
    for _ in range(2):
        logs = agent.train_step()
        assert set(logs) >= {"actor_loss", "policy_entropy", "value_loss", "model_loss"}
        assert all(np.isfinite(v) for v in logs.values()), logs
    agent.update_critic()
    obs = env.reset()
    S = agent.state_size
    belief, state, action = torch.zeros(1, d.Be).cuda(), torch.zeros(1, S).cuda(), torch.zeros(1, d.A).cuda()
    belief, state, action, _, reward, _ = agent.update_belief_and_act(env, belief, state, action, obs, explore=True)
    assert float(action.abs().max()) <= 1.0 and np.isfinite(reward)
    assert torch.isfinite(belief).all() and torch.isfinite(state).all()
