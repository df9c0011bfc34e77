"""Is the fused imagined-heads test itself sharp?  (no GPU)

tests/heads_ref.py accepts the kernel when |got - ref| <= HEADS_C_TOL * S on the last contraction of each output.  Here a
float32 restatement of the chain (torch, CPU) must pass HeadsCase.check, and every planted fault that drops, doubles or
misplaces work in the same restatement must fail it, each at a shape and window where it applies.  The restated host
dispatch must agree with bd_img_heads_supported (which launches nothing), and the GPU shape tables of
tests/test_heads_kernels_gpu.py must reach every dispatch class the kernel has."""
import pytest
import torch

from tests import heads_ref as R
from tests import test_heads_kernels_gpu as G

SHAPES = [(37, 230, 200), (33, 52, 30), (19, 39, 20), (40, 20, 64), (33, 600, 200), (5, 17, 240), (33, 1072, 200),
          (17, 7, 3), (50, 100, 112)]


def _elu(x):
    return torch.where(x > 0, x, torch.expm1(x))


def _elu_grad(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1.0)


def emulate(case: R.HeadsCase, fault=None):
    """The kernel's operation in float32; `fault` plants one error."""
    M, F, Hd = case.M, case.F, case.Hd
    x = case.x.view.clone()
    if fault == "drop_x_col":
        x[:, F - 1] = 0.0
    douts = [H["dout"].clone() for H in case.heads]
    if fault == "drop_last_row_dout":
        for d in douts:
            d[M - 1] = 0.0
    if fault == "swap_dout":
        douts.reverse()
    outs, g0 = [], []
    for h, H in enumerate(case.heads):
        a = [x]
        for l in range(R.HIDDEN):
            inp = a[-1]
            if fault == "drop_hidden_block" and h == 1 and l == 2:
                inp = inp.clone()
                inp[:, 16 * (R.cdiv(Hd, 16) - 1):] = 0.0
            pre = inp @ H["W"][l].t()
            if not (fault == "omit_bias" and h == 0 and l == 1):
                pre = pre + H["b"][l]
            a.append(_elu(pre))
        out = a[R.HIDDEN] @ H["w_out"]
        if not (fault == "omit_b_out" and h == 1):
            out = out + H["b_out"]
        outs.append(out)
        g = douts[h].view(M, 1) * H["w_out"] * _elu_grad(a[R.HIDDEN])
        for l in range(R.HIDDEN - 1, 0, -1):
            save = a[l + 1] if (fault == "wrong_save" and h == 0 and l == 2) else a[l]
            g = (g @ H["W"][l]) * _elu_grad(save)
        g0.append(g)
    dx = g0[0] @ case.heads[0]["W"][0]
    if fault != "missing_head":
        dx = dx + g0[1] @ case.heads[1]["W"][0]
    if fault == "double_dx":
        dx = dx + dx
    return outs[0], outs[1], dx


def _check(case, got):
    case.out_r.view[:, 0] = got[0]
    case.out_v.view[:, 0] = got[1]
    case.dx.view.copy_(got[2])
    return case.check(f"emulation {case.M, case.F, case.Hd, case.window}")


@pytest.mark.parametrize("window", [None, "cols", "rows", "hidden", "head_r", "head_v"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_passes_the_tolerance(shape, window):
    case = R.HeadsCase(*shape, seed=sum(shape), window=window, device="cpu")
    worst = _check(case, emulate(case))
    print(f"HEADS_WORST emulation:{shape},{window} {worst:.3e}")
    if window == "rows":
        assert not case.dx.view[:-1].any()


FAULTS = [("drop_x_col", (33, 52, 30), "cols"), ("drop_x_col", (19, 39, 20), None), ("drop_x_col", (37, 230, 200), None),
          ("drop_hidden_block", (37, 230, 200), "hidden"), ("drop_hidden_block", (33, 52, 30), None),
          ("omit_bias", (37, 230, 200), None), ("omit_bias", (17, 7, 3), "hidden"),
          ("omit_b_out", (50, 100, 112), None), ("omit_b_out", (33, 52, 30), "cols"),
          ("drop_last_row_dout", (37, 230, 200), "rows"), ("drop_last_row_dout", (5, 17, 240), None),
          ("wrong_save", (37, 230, 200), None), ("wrong_save", (40, 20, 64), "hidden"),
          ("swap_dout", (33, 52, 30), None), ("swap_dout", (37, 230, 200), "head_r"),
          ("missing_head", (50, 100, 112), None), ("missing_head", (33, 52, 30), "head_r"),
          ("double_dx", (19, 39, 20), None), ("double_dx", (37, 230, 200), "rows")]


@pytest.mark.parametrize("fault,shape,window", FAULTS)
def test_planted_fault_fails_the_tolerance(fault, shape, window):
    case = R.HeadsCase(*shape, seed=1 + sum(shape), window=window, device="cpu")
    with pytest.raises(AssertionError, match="out of tolerance"):
        _check(case, emulate(case, fault))


def test_write_outside_an_output_is_caught():
    case = R.HeadsCase(17, 7, 3, seed=0, device="cpu")
    got = emulate(case)
    case.dx.full[case.M, 0] = 0.0            # the row behind dx[M*F]
    with pytest.raises(AssertionError, match="wrote outside dx"):
        _check(case, got)


def test_pack_restatement_is_the_documented_layout():
    """pack_ref element by element against cabi.hip:12-14, on a shape with ragged n and k."""
    N, K = 19, 37
    W = torch.arange(1, N * K + 1, dtype=torch.float32).view(N, K)
    for tr in (False, True):
        Wo = W.t() if tr else W
        No, Ki = Wo.shape
        Kb = R.cdiv(Ki, 16)
        p = R.pack_ref(W, tr)
        assert p.numel() == R.cdiv(N, 16) * R.cdiv(K, 16) * 256
        for e in range(p.numel() // 4):
            lane, blk = e & 63, e >> 6
            nb, kb = divmod(blk, Kb)
            n, k0 = nb * 16 + (lane & 15), kb * 16 + 4 * (lane >> 4)
            for i in range(4):
                want = float(Wo[n, k0 + i]) if n < No and k0 + i < Ki else 0.0
                assert float(p[4 * e + i]) == want, (tr, e, i)


def test_support_rule_agrees_with_the_library():
    from big_dreamer_amd import _cabi as cabi
    for F in (1, 16, 52, 230, 600, 1072, 1073, 2320, 2321):
        for Hd in range(1, 261):
            assert bool(cabi.lib.bd_img_heads_supported(F, Hd)) == R.heads_supported(F, Hd), (F, Hd)
    assert R.heads_lds(2, 1072, 200) == R.MAX_LDS and R.heads_lds(1, 2320, 240) == R.MAX_LDS
    assert not R.heads_supported(1073, 200) and not R.heads_supported(2321, 240)
    assert R.heads_rt(200) == 2 and R.heads_rt(36) == 1 and R.heads_rt(256) == 0


def test_gpu_shape_tables_reach_every_dispatch_class():
    """All fifteen (per, left) classes with Nb <= 15 at the RT heads_rt picks, both loaders, F < Hd, and a large-LDS
    launch for each of RT = 1 and RT = 2."""
    shapes = G.all_shapes()
    classes = [R.heads_class(F, Hd, off) for _, F, Hd, off in shapes]
    want = {(per, left) for per in range(4) for left in range(4)} - {(0, 0)}
    assert len(want) == 15
    assert {(per, left) for _, per, left, _, _, _ in classes} == want
    for per, left in want:          # the RT is a function of `left` alone: two leftover pairs per block need 2*left <= 4
        assert {rt for rt, p, l, _, _, _ in classes if (p, l) == (per, left)} == {1 if left == 3 else 2}
    assert {ld for _, _, _, ld, _, _ in classes} == {"pairs", "scalar"}
    for rt in (1, 2):
        assert any(c[0] == rt and c[3] == "scalar" for c in classes), rt
        assert any(c[0] == rt and c[4] for c in classes), ("F < Hd", rt)
        assert any(c[0] == rt and c[5] for c in classes), ("large LDS", rt)
    assert any(R.heads_lds(R.heads_rt(Hd), F, Hd) == R.MAX_LDS for _, F, Hd, _ in shapes)
    # the misaligned even-F base and the widths the forms of tall_sweep split at
    assert any(F % 2 == 0 and off == 1 for _, F, _, off in shapes)
    assert {1, 16, 17, 112, 176, 240} <= {Hd for _, _, Hd, _ in shapes}
