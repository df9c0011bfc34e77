"""The frozen imagined heads' fused forward + dgrad (csrc/heads.hip, bd_img_heads_fwd_bwd) against the separate
mlp.hip forward / backward pair it replaces, whole train steps with BD_HEADS_FUSED on and off, and the host-side shape
checks (the last test needs no GPU)."""
import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests.helpers import CASES


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("dims,extra", [
    (synth.CONFIG2, 0),                                                                   # configs[1]: M = 34 300
    (synth.CONFIG2, 7),                                                                   # ragged last tile
    (synth.Dims(B=5, L=4, H=4, Be=42, S=10, Hd=30, E=64, A=3, O=6), 5),                   # widths not multiples of 4
    (synth.SMALL, 3),                                                                     # Hd = 36: 16-row tiles
])
def test_fused_heads_match_the_separate_chains(dims, extra):
    from big_dreamer_amd.engine import DreamerEngine
    d = dims
    eng = DreamerEngine(d, None, "cuda", params=synth.make_params(d, 7))
    Mi, F = d.Hm * d.N + extra, d.Be + d.S
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(Mi, F, device="cuda", generator=g)
    d_r = torch.randn(Mi, device="cuda", generator=g)
    d_v = torch.randn(Mi, device="cuda", generator=g)
    # the separate chains (what BD_HEADS_FUSED=0 runs)
    r_ref, r_acts, r_layers = eng.dense_forward("reward_model", "rew", "tr", x, F, Mi, 1)
    v_ref, v_acts, v_layers = eng.dense_forward("critic_target", "tgt", "tv", x, F, Mi, 1)
    dx_ref = torch.zeros(Mi, F, device="cuda")
    eng.mlp_backward(Mi, d_r, 1, r_layers, r_acts + [None], None, din0=dx_ref, ld0=F, w0=F)
    eng.mlp_backward(Mi, d_v, 1, v_layers, v_acts + [None], None, din0=dx_ref, ld0=F, w0=F, accumulate=True)
    # fused, into poisoned outputs (every element must be written)
    r_out = torch.full((Mi,), float("nan"), device="cuda")
    v_out = torch.full((Mi,), float("nan"), device="cuda")
    dx = torch.full((Mi, F), float("nan"), device="cuda")
    eng.img_heads_fused(Mi, x, d_r, d_v, r_out, v_out, dx)
    torch.cuda.synchronize()
    for name, got, want, tol in (("r_out", r_out, r_ref.view(Mi), 1e-6), ("v_out", v_out, v_ref.view(Mi), 1e-6),
                                 ("dx", dx, dx_ref, 2e-6)):
        assert torch.isfinite(got).all(), name
        scale = float(want.abs().max())
        err = float((got - want).abs().max())
        assert scale > 0 and err <= tol * scale, (name, err, scale)
    # deterministic: a second launch gives the same bits
    r2, v2, dx2 = torch.empty_like(r_out), torch.empty_like(v_out), torch.empty_like(dx)
    eng.img_heads_fused(Mi, x, d_r, d_v, r2, v2, dx2)
    torch.cuda.synchronize()
    assert torch.equal(r2, r_out) and torch.equal(v2, v_out) and torch.equal(dx2, dx)


@pytest.mark.gpu
@pytest.mark.parametrize("name,rho", [("small", -1), ("small", 0.5), ("tiny_discount", -1), ("tiny_discount", 0.5),
                                      ("config2", -1)])
def test_train_steps_fused_against_separate_heads(name, rho):
    """Two train steps in fresh engines, fused heads on and off: logs and post-Adam weights within the tolerances
    test_hip_parity.py holds the engine to against the oracle (only summation orders differ)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = CASES[name]
    hp = dict(hp, gradient_mixing=rho)
    P = synth.make_params(d, seed)
    runs = []
    for fused in (True, False):
        eng = DreamerEngine(d, hp, "cuda", params=P)
        assert eng.heads_fused
        eng.heads_fused = fused
        eng.enable_timers(True)
        logs = []
        for step in range(2):
            logs.append(eng.train_step(_dev(synth.make_batch(d, seed + step)), _dev(synth.make_noise(d, seed + step))))
            if step == 0:
                eng.update_critic()
        torch.cuda.synchronize()
        spans = set(eng.timer_summary())
        assert "img_heads_bwd" in spans and ("img_heads_fwd" in spans) != fused, spans
        runs.append((logs, {g: eng.groups[g].flat.detach().cpu().numpy() for g in ("model", "actor", "critic")}))
    (lf, wf), (ls, ws) = runs
    for step in range(2):
        for k, v in ls[step].items():
            tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
            assert abs(lf[step][k] - v) <= tol[0] + tol[1] * abs(v), (step, k, lf[step][k], v)
    for g in wf:
        np.testing.assert_allclose(wf[g], ws[g], atol=2e-5, rtol=1e-5, err_msg=g)


@pytest.mark.gpu
def test_pipelined_schedule_stays_bit_identical_with_fused_heads():
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = CASES["small"]
    P = synth.make_params(d, seed)
    engs = []
    for pipe in (True, False):
        eng = DreamerEngine(d, hp, "cuda", params=P)
        assert eng.heads_fused
        eng.pipeline = pipe
        engs.append(eng)
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(3)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(3)]
    logs = []
    for eng in engs:
        for i in range(3):
            eng.train_step(batches[i], noises[i], sync_logs=False)
        logs.append(eng.logs())
        torch.cuda.synchronize()
    for i, e in enumerate(engs):
        for grp in ("model", "actor", "critic", "critic_target"):
            assert torch.equal(e.groups[grp].flat, engs[1].groups[grp].flat), (i, grp)
        assert logs[i] == logs[1], i


def test_host_checks_reject_uncovered_shapes():
    """No GPU needed: the checks run before any launch and return -1 with a message."""
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    assert lib.bd_img_heads_supported(230, 200) == 1
    assert lib.bd_img_heads_supported(52, 30) == 1 and lib.bd_img_heads_supported(58, 36) == 1
    assert lib.bd_img_heads_supported(230, 256) == 0          # 16 column blocks: more than the waves' pairs hold
    assert lib.bd_img_heads_supported(230, 0) == 0 and lib.bd_img_heads_supported(0, 200) == 0
    assert lib.bd_img_heads_supported(40000, 200) == 0        # LDS image beyond the workgroup's 160 KiB

    def args(M, F, Hd):
        a = cabi.ImgHeadsArgs()
        a.M, a.F, a.Hd, a.x, a.dx = M, F, Hd, 256, 256       # never dereferenced: the checks fail first
        for h in range(2):
            H = a.head[h]
            for l in range(cabi.BD_HEAD_HIDDEN):
                H.w[l] = H.wt[l] = H.b[l] = 256
            H.w_out = H.b_out = H.dout = H.out = 256
        return a
    import ctypes as C
    for M, F, Hd in ((100, 230, 256), (0, 230, 200), (100, 230, 0), (20_000_000, 230, 200)):
        assert lib.bd_img_heads_fwd_bwd(C.byref(args(M, F, Hd)), None) == -1, (M, F, Hd)
        assert b"bd_img_heads_fwd_bwd" in lib.bd_last_error()
    a = args(100, 230, 200)
    a.head[1].wt[2] = None
    assert lib.bd_img_heads_fwd_bwd(C.byref(a), None) == -1 and b"head 1" in lib.bd_last_error()
