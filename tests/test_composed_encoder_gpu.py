"""Composed encoder tail: the product descriptors of bd_pack_weights, the chain record of
bd_wgrad_grouped and the whole dynamics step in the composed form, each against float64 / the oracle.

Bounds are derived, not tuned.  A dot product of L fp32 terms summed in any fixed order is within L * 2^-24 * sum|a b| of
the exact value (first order), so
  * product pack: E * 2^-24 * (|A| |B|) per element;
  * chained weight gradients: (N + Hd + 2) * 2^-24 * (the same products of absolute values): N for the row sums of the
    slab GEMM and its reduce, Hd + 1 for the weight-space product and the bias term, 1 for the fp32 operand in between.
The whole-step comparison uses the tolerances tests/test_hip_parity.py applies to the direct form (its _rel calls in
test_train_steps_vs_oracle_and_golden), through its own helpers."""
import numpy as np
import pytest
import torch

from big_dreamer_amd import synth
from tests import dense_ref as R
from tests.conv_ref import unpack_ref
from tests.helpers import CASES, CAT_CASES
from tests.test_hip_parity import _dev, _rel

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def _within(name, got, ref, bound):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"COMPOSED_WORST {name}: max err / bound = {worst:.3f}  max|err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{name}: {int((err > bound).sum())} elements above the bound (worst ratio {worst:.3f})"


# ---- product pack ------------------------------------------------------------------------------------------------------
# (Hd, E, K, Be): Be = 22 puts the strided A view off 16-byte alignment (scalar loads), the others take the float4 loads
@pytest.mark.parametrize("Hd,E,K,Be", [(24, 40, 24, 22), (24, 40, 24, 24), (16, 16, 16, 16), (200, 1024, 200, 200)])
def test_product_pack_against_float64(cabi, Hd, E, K, Be):
    g = torch.Generator(device="cuda").manual_seed(Hd + E + Be)
    Wq1 = torch.randn(Hd, Be + E, device="cuda", generator=g)
    A = Wq1[:, Be:]                                         # strided view, as belief_posterior.model.0.weight[:, Be:]
    B = torch.randn(E, K, device="cuda", generator=g)
    b = torch.randn(E, device="cuda", generator=g)
    nf = int(cabi.packed_floats(Hd, K))
    out = torch.full((2 * nf + Hd + 4,), float("nan"), device="cuda")
    fwd, tr, vec = out[:nf], out[nf:2 * nf], out[2 * nf:2 * nf + Hd]
    descs = (cabi.PackDesc * 3)(
        cabi.PackDesc(A.data_ptr(), fwd.data_ptr(), A.stride(0), Hd, K, 0, cabi.PACK_PRODUCT, B.data_ptr(), B.stride(0), E),
        cabi.PackDesc(A.data_ptr(), tr.data_ptr(), A.stride(0), Hd, K, 1, cabi.PACK_PRODUCT, B.data_ptr(), B.stride(0), E),
        cabi.PackDesc(A.data_ptr(), vec.data_ptr(), A.stride(0), Hd, 1, 0, cabi.PACK_PRODUCT_VEC, b.data_ptr(), 1, E))
    table = R.device_table(descs)
    cabi.check(cabi.lib.bd_pack_weights(table.data_ptr(), 3 + 3 * cabi.PACK_PRODUCTS, cabi.stream()))
    torch.cuda.synchronize()
    A64, B64, b64 = A.double(), B.double(), b.double()
    ref, bound = A64 @ B64, E * U * (A64.abs() @ B64.abs())
    _within("encq", unpack_ref(fwd, Hd, K), ref, bound)
    _within("encq.T", unpack_ref(tr, K, Hd), ref.t(), bound.t())
    _within("encq_b", vec, A64 @ b64, E * U * (A64.abs() @ b64.abs()))
    # the padding of the packed blocks is zero, and nothing behind the outputs was written
    for p, (n, k) in ((fwd, (Hd, K)), (tr, (K, Hd))):
        full = p.reshape(-(-n // 16), -(-k // 16), 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(-(-n // 16) * 16, -1)
        assert float(full[n:].abs().sum()) == 0.0 and float(full[:, k:].abs().sum()) == 0.0
    assert bool(torch.isnan(out[2 * nf + Hd:]).all())


# ---- chained weight gradients ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Hd,E", [(1, 24, 40), (37, 24, 40), (50, 24, 40), (50, 200, 1024)])
def test_chained_wgrads_against_float64(cabi, N, Hd, E):
    Be, pad = Hd, 5                                       # target rows: [Be | E | pad] columns
    g = torch.Generator(device="cuda").manual_seed(N + Hd)
    d_q1 = torch.randn(N, Hd, device="cuda", generator=g)
    act3 = torch.randn(N, Hd, device="cuda", generator=g)
    Wq1 = torch.randn(Hd, Be + E, device="cuda", generator=g)
    W4 = torch.randn(E, Hd, device="cuda", generator=g)
    b4 = torch.randn(E, device="cuda", generator=g)
    Wq1e = Wq1[:, Be:]
    # float64 of the direct formulas, with the sums of absolute values
    q64, a64, W64, W464, b464 = d_q1.double(), act3.double(), Wq1e.double(), W4.double(), b4.double()
    emb = a64 @ W464.t() + b464
    emb_abs = a64.abs() @ W464.abs().t() + b464.abs()
    d_emb = q64 @ W64
    d_emb_abs = q64.abs() @ W64.abs()
    want = {"dW_q1e": (q64.t() @ emb, q64.abs().t() @ emb_abs), "dW_enc4": (d_emb.t() @ a64, d_emb_abs.t() @ a64.abs()),
            "db_enc4": (d_emb.sum(0), d_emb_abs.sum(0))}
    c = (N + Hd + 2) * U

    def targets():
        return (torch.full((Hd, Be + E + pad), float("nan"), device="cuda"), torch.full((E, Hd), float("nan"), device="cuda"),
                torch.full((E,), float("nan"), device="cuda"))

    def check(tag, gWq1, gW4, gb4):
        _within(f"{tag} dW_q1e", gWq1[:, Be:Be + E], want["dW_q1e"][0], c * want["dW_q1e"][1])
        _within(f"{tag} dW_enc4", gW4, want["dW_enc4"][0], c * want["dW_enc4"][1])
        _within(f"{tag} db_enc4", gb4, want["db_enc4"][0], c * want["db_enc4"][1])
        assert bool(torch.isnan(gWq1[:, :Be]).all()) and bool(torch.isnan(gWq1[:, Be + E:]).all()), \
            f"{tag}: wrote outside the [Be, Be + E) columns of the target view"

    def run(descs):
        rc, tb, tr, wsf = R.wgrad_plan(cabi, descs)
        cabi.check(rc)
        table = R.device_table(descs)
        ws = torch.full((max(1, wsf),), float("nan"), device="cuda")
        cabi.check(cabi.lib.bd_wgrad_grouped(table.data_ptr(), len(descs), tb, tr, ws.data_ptr(), cabi.stream()))
        torch.cuda.synchronize()
        return tr

    # composed: one Hd x Hd GEMM into scratch + the chain record
    gWq1, gW4, gb4 = targets()
    dWc = torch.full((Hd, Hd), float("nan"), device="cuda")
    dbc = torch.full((Hd,), float("nan"), device="cuda")
    descs = (cabi.WgradDesc * 2)()
    descs[0] = cabi.WgradDesc(d_q1.data_ptr(), Hd, act3.data_ptr(), Hd, N, None, 0, N, Hd, Hd, dWc.data_ptr(), Hd, dbc.data_ptr())
    ch = descs[1]
    ch.kind, ch.N, ch.K, ch.c_E = cabi.WGRAD_CHAIN, Hd, Hd, E
    ch.dW, ch.ldw, ch.db = dWc.data_ptr(), Hd, dbc.data_ptr()
    ch.c_A, ch.c_lda, ch.c_B, ch.c_ldb, ch.c_b = Wq1e.data_ptr(), Wq1.stride(0), W4.data_ptr(), Hd, b4.data_ptr()
    ch.c_dA, ch.c_ldda = gWq1[:, Be:].data_ptr(), gWq1.stride(0)
    ch.c_dB, ch.c_lddb, ch.c_db = gW4.data_ptr(), Hd, gb4.data_ptr()
    assert run(descs) >> 24 == 1, "the plan word carries the chain record"
    check("chained", gWq1, gW4, gb4)
    first = [t.clone() for t in (gWq1[:, Be:Be + E], gW4, gb4)]
    run(descs)
    assert all(torch.equal(a, b) for a, b in zip(first, (gWq1[:, Be:Be + E], gW4, gb4))), "the same launch twice differs"

    # the direct kernels on the same inputs meet the same bound (guards this test's reference and bound)
    gWq1, gW4, gb4 = targets()
    emb32, d_emb32 = emb.float().contiguous(), d_emb.float().contiguous()
    direct = (cabi.WgradDesc * 2)()
    direct[0] = cabi.WgradDesc(d_q1.data_ptr(), Hd, emb32.data_ptr(), E, N, None, 0, N, Hd, E, gWq1[:, Be:].data_ptr(),
                               gWq1.stride(0), None)
    direct[1] = cabi.WgradDesc(d_emb32.data_ptr(), E, act3.data_ptr(), Hd, N, None, 0, N, E, Hd, gW4.data_ptr(), Hd,
                               gb4.data_ptr())
    assert run(direct) >> 24 == 0
    check("direct", gWq1, gW4, gb4)


def test_chain_records_must_close_the_table_and_name_a_result(cabi):
    x = torch.zeros(64, 16, device="cuda")
    descs = (cabi.WgradDesc * 2)()
    descs[1] = cabi.WgradDesc(x.data_ptr(), 16, x.data_ptr(), 16, 64, None, 0, 64, 16, 16, x.data_ptr(), 16, None)
    descs[0].kind = cabi.WGRAD_CHAIN
    assert R.wgrad_plan(cabi, descs)[0] != 0              # a chain record in front of a GEMM descriptor
    descs[0], descs[1] = descs[1], cabi.WgradDesc()
    ch = descs[1]
    ch.kind, ch.N, ch.K, ch.c_E, ch.ldw = cabi.WGRAD_CHAIN, 16, 16, 16, 16
    for f in ("dW", "db", "c_A", "c_B", "c_b", "c_dA", "c_dB", "c_db"):
        setattr(ch, f, x.data_ptr() + 4096)
    ch.c_lda = ch.c_ldb = ch.c_ldda = ch.c_lddb = 16
    assert R.wgrad_plan(cabi, descs)[0] != 0              # its (dW, db) is no descriptor's output


# ---- whole dynamics step: composed against direct, both against the oracle -----------------------------------------------
def _case(name):
    from oracle import dreamer_oracle as O
    cat = name in CAT_CASES
    d, seed, hp, _ = (CAT_CASES if cat else CASES)[name]
    P, batch, noise = synth.make_params(d, seed), synth.make_batch(d, seed), synth.make_noise(d, seed)
    od = O.OracleDreamer(P, dict(hp, planning_horizon=d.H, **({"categorical": (d.cat_D, d.cat_C)} if cat else {})))
    ologs = od.train_step(batch, noise)
    return d, hp, P, batch, noise, od, ologs, getattr(od, "model_modules", O.MODEL_MODULES)


@pytest.fixture(scope="module", params=["small", "cat_tiny"])
def case(request):
    return _case(request.param)


@pytest.mark.parametrize("composed", [False, True])
def test_dynamics_step_against_oracle(case, composed):
    """One train step from the same parameters, batch and explicit noise: losses, grad_norm_model and every model
    gradient tensor at the tolerances of tests/test_hip_parity.py (post-Adam weights of a first step are not compared:
    g / (|g| + eps) amplifies last-bit differences)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, hp, P, batch, noise, od, ologs, mods = case
    assert not d.pixel
    eng = DreamerEngine(d, hp, "cuda", params=P)
    eng.encoder_composed = composed
    assert eng.composed_encoder_tail(d.N) is composed
    logs = eng.train_step(_dev(batch), _dev(noise))
    torch.cuda.synchronize()
    rep = []
    try:
        for k in ("observation_loss", "reward_loss", "kl_loss"):
            _rel(k, logs[k], ologs[k], 2e-5, 5e-5, rep)
        gn = od.last["grad_norms"]["model"]
        _rel("grad_norm_model", [logs["grad_norm_model"]], [gn], 1e-6, 1e-3, rep)
        coef = min(1.0, od.hp["grad_clip_norm"] / (gn + 1e-6))
        i = 0
        for mod in mods:
            for k in od.P[mod]:
                want = od.last["model_grads"][i].numpy() * coef
                scale = float(np.abs(want).max()) + 1e-12
                _rel(f"grad.{mod}.{k}", eng.G(mod, k).detach().cpu().numpy(), want, 2e-3 * scale + 1e-9, 2e-3, rep)
                i += 1
    finally:
        print("\n".join(rep))


def test_default_rule_selects_by_rows_and_never_for_pixels():
    from big_dreamer_amd.engine import DreamerEngine
    eng = DreamerEngine(synth.TINY, None, "cuda", params=synth.make_params(synth.TINY, 0))
    Hd = synth.TINY.Hd
    assert eng.encoder_composed is None
    assert eng.composed_encoder_tail(4 * Hd) and not eng.composed_encoder_tail(4 * Hd - 1)
    eng.pixel = True
    eng.encoder_composed = True
    assert not eng.composed_encoder_tail(1 << 20)


def test_composed_serial_and_pipelined_schedules_are_bit_identical():
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = CASES["small"]
    P = synth.make_params(d, seed)
    steps = 3
    batches = [_dev(synth.make_batch(d, seed + 10 * i)) for i in range(steps)]
    noises = [_dev(synth.make_noise(d, seed + 10 * i)) for i in range(steps)]
    engs, logs = [], []
    for pipe in (True, False):
        eng = DreamerEngine(d, hp, "cuda", params=P)
        eng.pipeline, eng.encoder_composed = pipe, True
        for i in range(steps):
            eng.train_step(batches[i], noises[i], sync_logs=False)
        logs.append(eng.logs())
        torch.cuda.synchronize()
        engs.append(eng)
    a, b = engs
    for grp in ("model", "actor", "critic"):
        ga, gb = a.groups[grp], b.groups[grp]
        assert torch.equal(ga.flat, gb.flat) and torch.equal(ga.grad, gb.grad), grp
        assert torch.equal(ga.m, gb.m) and torch.equal(ga.v, gb.v), grp
    assert logs[0] == logs[1] and np.isfinite(list(logs[0].values())).all()
