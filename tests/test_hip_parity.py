"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical inputs, and
against the golden vectors generated from the reference.  Tolerances are fp32 and stated per check."""
import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests.helpers import CASES, assert_close, check_fingerprints, compare_tensor, load_golden

pytestmark = pytest.mark.gpu


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _setup(name, cluster=True):
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, full = CASES[name]
    g = load_golden(name)
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    noise = synth.make_noise(d, seed)
    check_fingerprints(g, P, batch, noise)
    eng = DreamerEngine(d, hp, "cuda", params=P)
    if not cluster:
        eng.use_obs_cluster = False      # single-workgroup-per-tile observe kernels (observe.hip)
    return d, seed, hp, full, g, P, batch, noise, eng


def _rel(name, got, want, atol, rtol, report):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(want).shape)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    report.append(f"{name:28s} max|err|={err.max():.3e}  max|ref|={np.abs(want).max():.3e}")
    assert_close(name, got, want, atol, rtol)


@pytest.mark.parametrize("name", ["tiny", "small", "config1", "config2"])
def test_forward_pieces_vs_oracle(name):
    """R-enc, R1, R2, R4-R8 forward values on the initial weights."""
    from oracle import dreamer_oracle as O
    d, seed, hp, full, g, P, batch, noise, eng = _setup(name)
    od = O.OracleDreamer(P, dict(hp, planning_horizon=d.H))
    tb = {k: torch.as_tensor(v) for k, v in batch.items()}
    tn = {k: torch.as_tensor(v) for k, v in noise.items()}
    with torch.no_grad():
        _, _, _, _, inter = od.world_model_forward(tb, tn)
        ib, is_, (im, isd), ent = O.imagine_ahead(od.P, inter["posterior_states"], inter["beliefs"], d.H,
                                                  tn["action"], tn["entropy"], tn["img_prior"])
        r = O.dense_on_features(ib, is_, od.P["reward_model"])
        v = O.dense_on_features(ib, is_, od.P["critic_target"])
        ret = O.lambda_return(r, v, v[-1], od.hp["discount"], od.hp["disclam"])
    db, dn = _dev(batch), _dev(noise)
    T, B, N, Hm = d.T, d.B, d.N, d.Hm
    emb, pre = eng.encode(db["observations"][1:].reshape(N, d.O), N)
    feat, qm, qs = eng.observe(db["actions"][:-1], db["nonterminals"][:-1], pre, dn["obs_post"],
                               torch.zeros(B, d.Be, device="cuda"), torch.zeros(B, d.S, device="cuda"), T, B)
    pst, pm, ps = eng.prior_head(feat, N, dn["obs_prior"])
    ifeat, e_ent, act = eng.imagine(feat, N, Hm, dn)
    F = d.Be + d.S
    r_out, _, _ = eng.dense_forward("reward_model", "rew", "ir", ifeat, F, Hm * N, 1)
    v_out, _, _ = eng.dense_forward("critic_target", "tgt", "iv", ifeat, F, Hm * N, 1)
    returns = torch.zeros(Hm * N, device="cuda")
    from big_dreamer_amd import _cabi as cabi
    cabi.check(cabi.lib.bd_lambda_return_forward(r_out.data_ptr(), v_out.data_ptr(), Hm, N, eng.hp["discount"],
                                                 eng.hp["disclam"], returns.data_ptr(), cabi.stream()))
    torch.cuda.synchronize()
    rep = []
    c = lambda t: t.detach().cpu().numpy()
    try:
        # recurrent fp32 chains with a different summation order: 2e-5 abs / 2e-5 rel
        _rel("embeddings", c(emb), inter["embeddings"].reshape(N, -1), 2e-5, 2e-5, rep)
        f = c(feat).reshape(T, B, F)
        _rel("beliefs", f[..., :d.Be], inter["beliefs"], 2e-5, 2e-5, rep)
        _rel("posterior_states", f[..., d.Be:], inter["posterior_states"], 2e-5, 2e-5, rep)
        _rel("posterior_means", c(qm), inter["posterior_means"].reshape(N, -1), 2e-5, 2e-5, rep)
        _rel("posterior_stds", c(qs), inter["posterior_stds"].reshape(N, -1), 2e-5, 2e-5, rep)
        _rel("prior_means", c(pm), inter["prior_means"].reshape(N, -1), 2e-5, 2e-5, rep)
        _rel("prior_stds", c(ps), inter["prior_stds"].reshape(N, -1), 2e-5, 2e-5, rep)
        _rel("prior_states", c(pst), inter["prior_states"].reshape(N, -1), 2e-5, 2e-5, rep)
        fi = c(ifeat).reshape(Hm, N, F)
        _rel("imged_beliefs", fi[..., :d.Be], ib, 5e-5, 5e-5, rep)
        _rel("imged_states", fi[..., d.Be:], is_, 5e-5, 5e-5, rep)
        # entropy: 100-sample mean of a log-density with atanh near saturation: ill-conditioned per row
        # (1-ulp tanh differences move single rows by up to ~6e-3); mean is tight.
        _rel("action_entropy", c(e_ent).reshape(Hm, N), ent, 2e-2, 1e-3, rep)
        assert abs(float(c(e_ent).mean()) - float(ent.mean())) < 2e-4
        _rel("imged_reward", c(r_out).reshape(Hm, N, 1), r, 5e-5, 5e-5, rep)
        _rel("value_pred", c(v_out).reshape(Hm, N, 1), v, 5e-5, 5e-5, rep)
        _rel("returns", c(returns).reshape(Hm, N, 1), ret, 2e-4, 5e-5, rep)
    finally:
        print("\n".join(rep))


@pytest.mark.parametrize("name,cluster", [("tiny", True), ("small", True), ("tiny_klsum", True), ("tiny_freenats0", True),
                                          ("config1", True), ("config2", True), ("small", False),
                                          ("tiny_freenats0", False), ("config2", False),
                                          # the round-1 cluster form (GRU columns split, one all-gather per step)
                                          ("small", "round1"), ("tiny_freenats0", "round1"), ("config2", "round1"),
                                          ("tiny_pixel", True), ("tiny_pixel_lin", True),
                                          ("tiny_pixel", "miopen"), ("tiny_pixel_lin", "miopen"),
                                          ("config3", True), ("tiny_discount", True), ("tiny_discount", False)])
def test_train_steps_vs_oracle_and_golden(name, cluster, monkeypatch):
    """Two whole train steps: losses, clipped gradients, gradient norms, post-Adam weights -- with the observe
    scan run by the multi-CU cluster kernels (default) and by the single-workgroup kernels."""
    from oracle import dreamer_oracle as O
    from big_dreamer_amd import _cabi as cabi
    torch_convs = cluster == "miopen"
    if torch_convs:
        cluster = True
    # cluster=True: the K-split cluster scan (csrc/observe_ksplit.hip); "round1": observe_cluster.hip's form; False: one
    # workgroup per tile (observe.hip)
    cabi.check(cabi.lib.bd_observe_cluster_set_ksplit(0 if cluster == "round1" else -1))
    if cluster == "round1":
        cluster = True
    d, seed, hp, full, g, P, batch, noise, eng = _setup(name, cluster)
    if d.pixel:
        from big_dreamer_amd.conv_stack import ConvStacks
        assert isinstance(eng.conv, ConvStacks), "the product engine has ONE pixel path: csrc/conv.hip"
    if torch_convs:                 # comparator (test helper): the conv stacks on MIOpen through torch autograd
        from tests.torch_conv_stacks import TorchConvStacks
        eng.conv = TorchConvStacks(eng)
    od = O.OracleDreamer(P, dict(hp, planning_horizon=d.H))
    db = _dev(batch)
    rep = []
    try:
        for step in range(2):
            nz = synth.make_noise(d, seed + step)
            ologs = od.train_step(batch, nz)
            logs = eng.train_step(db, _dev(nz))
            if step == 0:
                od.update_critic()
                eng.update_critic()
            torch.cuda.synchronize()
            eng.cluster_status(d.B)          # no cluster member timed out waiting for its peers
            for k, v in ologs.items():
                # losses are means over up to 34300 rows; policy_entropy has the ill-conditioned tail
                tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                _rel(f"s{step}.{k}", logs[k], v, tol[0], tol[1], rep)
                _rel(f"s{step}.{k}(golden)", logs[k], g[f"step{step}.log.{k}"], tol[0], tol[1], rep)
            gn = od.last["grad_norms"]
            _rel(f"s{step}.grad_norms", [logs["grad_norm_model"], logs["grad_norm_actor"], logs["grad_norm_critic"]],
                 [gn["model"], gn["actor"], gn["critic"]], 1e-6, 1e-3, rep)
            coef = {k: min(1.0, od.hp["grad_clip_norm"] / (gn[k] + 1e-6)) for k in gn}
            groups = {"model": (od.model_modules, od.last["model_grads"]), "actor": (("actor",), od.last["actor_grads"]),
                      "critic": (("critic",), od.last["critic_grads"])}
            for grp, (mods, grads) in groups.items():
                i = 0
                for mod in mods:
                    for k in od.P[mod]:
                        want = grads[i].numpy() * coef[grp]
                        got = eng.G(mod, k).detach().cpu().numpy()
                        scale = float(np.abs(want).max()) + 1e-12
                        # gradients are long sums: tolerance relative to the tensor's own scale
                        _rel(f"s{step}.grad.{mod}.{k}", got, want, 2e-3 * scale + 1e-9, 2e-3, rep)
                        i += 1
            for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
                for k, p in od.P[mod].items():
                    got = eng.W(mod, k).detach().cpu().numpy()
                    # an Adam step moves a weight by <= lr (2e-4): agreement must be far below one step
                    _rel(f"s{step}.param.{mod}.{k}", got, p.detach().numpy(), 2e-5, 1e-5, rep)
                    compare_tensor(g, f"step{step}.param.{mod}.{k}", got, full, atol=2e-5, rtol=1e-5)
    finally:
        cabi.check(cabi.lib.bd_observe_cluster_set_ksplit(-1))
        print("\n".join(rep[-400:]))


@pytest.mark.parametrize("dims", [synth.Dims(B=5, L=4, H=4, Be=40, S=10, Hd=32, E=64, A=17, O=6),      # HumanoidStandup's action width
                                  synth.Dims(B=18, L=3, H=3, Be=200, S=30, Hd=200, E=1024, A=17, O=3),
                                  # widths that are NOT multiples of 4: lanes whose four consecutive columns straddle the edge
                                  # of a layer (transposed-accumulator epilogues, the K-split scan's row accessors)
                                  synth.Dims(B=5, L=4, H=4, Be=42, S=10, Hd=30, E=64, A=3, O=6),
                                  synth.Dims(B=20, L=3, H=3, Be=46, S=9, Hd=35, E=50, A=2, O=5)])
def test_wide_action_vectors_vs_oracle(dims):
    """A = 17 (configs[2-3]) needs two K blocks for the action operand and two column blocks for the actor's mean / std
    heads; the golden cases stop at A = 3.  Also: ragged layer widths.  Two train steps against the oracle."""
    from big_dreamer_amd.engine import DreamerEngine
    from oracle import dreamer_oracle as O
    d = dims
    P = synth.make_params(d, 41)
    od = O.OracleDreamer(P, dict(planning_horizon=d.H))
    eng = DreamerEngine(d, None, "cuda", params=P)
    batch = synth.make_batch(d, 41)
    rep = []
    try:
        for step in range(2):
            nz = synth.make_noise(d, 41 + step)
            ologs = od.train_step(batch, nz)
            logs = eng.train_step(_dev(batch), _dev(nz))
            torch.cuda.synchronize()
            for k, v in ologs.items():
                tol = (5e-4, 5e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                _rel(f"s{step}.{k}", logs[k], v, tol[0], tol[1], rep)
            gn = od.last["grad_norms"]
            coef = {k: min(1.0, od.hp["grad_clip_norm"] / (gn[k] + 1e-6)) for k in gn}
            groups = {"model": (od.model_modules, od.last["model_grads"]), "actor": (("actor",), od.last["actor_grads"]),
                      "critic": (("critic",), od.last["critic_grads"])}
            for grp, (mods, grads) in groups.items():
                i = 0
                for mod in mods:
                    for k in od.P[mod]:
                        want = grads[i].numpy() * coef[grp]
                        scale = float(np.abs(want).max()) + 1e-12
                        _rel(f"s{step}.grad.{mod}.{k}", eng.G(mod, k).cpu().numpy(), want, 2e-3 * scale + 1e-9, 2e-3, rep)
                        i += 1
            for mod in list(O.MODEL_MODULES) + ["actor", "critic"]:
                for k, p in od.P[mod].items():
                    _rel(f"s{step}.param.{mod}.{k}", eng.W(mod, k).cpu().numpy(), p.detach().numpy(), 2e-5, 1e-5, rep)
    finally:
        print("\n".join(rep[-80:]))


def test_wide_batch_uses_two_column_blocks_per_cluster_member(monkeypatch):
    """B = 320 sequences = 20 row tiles: 20 x 13 single-block members would not be co-resident on 256 CUs, so the observe
    scans run with 7 members per tile owning two GRU column blocks each (observe_cluster.hip, pick_cluster).  One whole
    train step at the config-2 model size against the oracle (no golden file at this batch size).  (140 members are
    above the engine's default cap of half the chip for the cluster scan: lifted here to exercise the kernel form.)"""
    monkeypatch.setenv("BD_OBS_CLUSTER_MAX_WGS", "256")
    from big_dreamer_amd import _cabi as cabi
    from big_dreamer_amd.engine import DreamerEngine
    from oracle import dreamer_oracle as O
    d = synth.Dims(B=320, L=5, H=3)
    assert int(cabi.lib.bd_observe_cluster_size(d.B, d.Be)) == 7
    P = synth.make_params(d, 31)
    batch, nz = synth.make_batch(d, 31), synth.make_noise(d, 31)
    od = O.OracleDreamer(P, dict(planning_horizon=d.H, free_nats=0.5))
    eng = DreamerEngine(d, dict(free_nats=0.5), "cuda", params=P)
    assert eng._cluster_ok(d.B)
    ologs = od.train_step(batch, nz)
    logs = eng.train_step(_dev(batch), _dev(nz))
    torch.cuda.synchronize()
    eng.cluster_status(d.B)
    rep = []
    try:
        for k, v in ologs.items():
            tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
            _rel(k, logs[k], v, tol[0], tol[1], rep)
        gn = od.last["grad_norms"]
        coef = min(1.0, od.hp["grad_clip_norm"] / (gn["model"] + 1e-6))
        i = 0
        for mod in O.MODEL_MODULES:
            for k, p in od.P[mod].items():
                want = od.last["model_grads"][i].numpy() * coef
                scale = float(np.abs(want).max()) + 1e-12
                _rel(f"grad.{mod}.{k}", eng.G(mod, k).cpu().numpy(), want, 2e-3 * scale + 1e-9, 2e-3, rep)
                _rel(f"param.{mod}.{k}", eng.W(mod, k).cpu().numpy(), p.detach().numpy(), 2e-5, 1e-5, rep)
                i += 1
    finally:
        print("\n".join(rep[-60:]))


@pytest.mark.parametrize("name", ["small", "config2"])
def test_pipelined_schedule_is_bit_identical_to_serial(name):
    """Cross-step pipeline (dynamics learning of step k+1 under behaviour learning of step k on two HIP streams,
    engine.py) vs the serial schedule: four un-synchronised steps, same batches and noise -> identical bits in
    every weight, Adam moment and logged scalar (same kernels, same operands; only the issue order differs)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _full = CASES[name]
    P = synth.make_params(d, seed)
    engs = []
    for pipe, defer in ((True, False), (False, False), (True, True)):
        eng = DreamerEngine(d, hp, "cuda", params=P)
        eng.pipeline = pipe
        eng.defer_opt = defer        # the data-parallel order of the optimiser steps (engine._optimizer_step_or_defer)
        engs.append(eng)
    steps = 4
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    torch.cuda.synchronize()
    logs = []
    for eng in engs:
        for i in range(steps):
            eng.train_step(batches[i], noises[i], sync_logs=False)
            if i == 1:
                eng.update_critic()
        logs.append(eng.logs())
        torch.cuda.synchronize()
        eng.cluster_status(d.B)
    b = engs[1]
    for i, a in enumerate(engs):
        for grp in ("model", "actor", "critic", "critic_target"):
            ga, gb = a.groups[grp], b.groups[grp]
            assert torch.equal(ga.flat, gb.flat), (i, grp)
            if ga.grad is not None:
                assert torch.equal(ga.grad, gb.grad) and torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), (i, grp)
        assert logs[i] == logs[1], i
    assert np.isfinite(list(logs[0].values())).all()


def test_run_ahead_caller_trains_on_the_batches_it_sampled():
    """A caller that never waits for the logs enqueues a step in ~1 ms while the GPU needs ~3.4 ms, so it is soon many
    steps ahead; ExperienceReplay hands out batches from a ring of four buffers.  The engine must order the caller's
    next gathers behind the dynamics phase that still has to read a recycled buffer: 14 un-synchronised pipelined steps
    from the device replay end in exactly the weights of the serial schedule (same sampled indices, same device noise
    stream).  (Regression: without that ordering the pipelined run consumed overwritten batches.)"""
    from big_dreamer_amd.engine import DreamerEngine
    from big_dreamer_amd.memory import ExperienceReplay
    d = synth.CONFIG2
    P = synth.make_params(d, 0)
    rep = synth.make_replay(d, rows=2000, seed=0)
    flats = []
    for pipe in (True, False):
        eng = DreamerEngine(d, None, "cuda", params=P)
        eng.pipeline = pipe
        buf = ExperienceReplay(2000, d.A, 5, False, d.O, torch.device("cuda"))
        for k, v in rep.items():
            getattr(buf, k)[:] = v
        buf.idx, buf.full = 0, True
        buf.sync_device()
        np.random.seed(5)
        torch.manual_seed(5)
        torch.cuda.synchronize()
        for _ in range(14):
            o, a, r, n = buf.sample(d.B, d.L)
            eng.train_step({"observations": o, "actions": a, "rewards": r, "nonterminals": n}, None, sync_logs=False)
        eng.join()
        torch.cuda.synchronize()
        flats.append({g: eng.groups[g].flat.clone() for g in ("model", "actor", "critic")})
    for g in ("model", "actor", "critic"):
        assert torch.equal(flats[0][g], flats[1][g]), g


def test_replay_sample_on_device_matches_reference_golden():
    """R0 through bd_replay_gather: same draws -> the reference's batches (bit exact, pure copies)."""
    from big_dreamer_amd.memory import ExperienceReplay
    g = load_golden("replay")
    d = synth.TINY
    rep = synth.make_replay(d, rows=64, seed=3)
    for case, (idx, full) in {"partial": (40, False), "wrapped": (17, True)}.items():
        buf = ExperienceReplay(64, d.A, 5, False, d.O, "cuda")
        for k, v in rep.items():
            getattr(buf, k)[:] = v
        buf.idx, buf.full = idx, full
        np.random.seed(11)
        o, a, r, n = buf.sample(6, 7)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(o.cpu().numpy(), g[f"{case}.observations"])
        np.testing.assert_array_equal(a.cpu().numpy(), g[f"{case}.actions"])
        np.testing.assert_array_equal(r.cpu().numpy(), g[f"{case}.rewards"])
        np.testing.assert_array_equal(n.cpu().numpy(), g[f"{case}.nonterminals"])


def test_pixel_replay_gather_dequantise_matches_reference():
    """R0 (pixels): bd_replay_gather_pixels == preprocess_observation_ of the reference (golden, injected noise)."""
    from big_dreamer_amd import _cabi as cabi
    g = load_golden("pixel_preprocess")
    u8 = torch.as_tensor(g["u8"]).cuda().contiguous()
    noise = torch.as_tensor(g["noise"]).cuda().contiguous()
    idx = torch.arange(u8.shape[0], dtype=torch.int64, device="cuda")
    for bits in (5, 8, 3):
        out = torch.empty(u8.shape, dtype=torch.float32, device="cuda")
        cabi.check(cabi.lib.bd_replay_gather_pixels(u8.data_ptr(), idx.data_ptr(), u8.shape[0], 3 * 64 * 64, bits,
                                                    noise.data_ptr(), out.data_ptr(), cabi.stream()))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), g[f"out{bits}"])     # bit exact
    # permuted gather
    perm = torch.tensor([3, 0, 5, 5, 1], dtype=torch.int64, device="cuda")
    out = torch.empty(5, 3, 64, 64, dtype=torch.float32, device="cuda")
    cabi.check(cabi.lib.bd_replay_gather_pixels(u8.data_ptr(), perm.data_ptr(), 5, 3 * 64 * 64, 5, noise.data_ptr(),
                                                out.data_ptr(), cabi.stream()))
    torch.cuda.synchronize()
    want = np.floor(g["u8"][[3, 0, 5, 5, 1]].astype(np.float32) / 8) / 32 - 0.5 + g["noise"][:5] / 32
    np.testing.assert_array_equal(out.cpu().numpy(), want.astype(np.float32))
