"""CPU tests: the host checks of bd_imagine_backward's window of time steps (t_begin, t_end, d_carry_in, d_carry_out)
reject a bad window before any launch, and the default chunk plan of the behaviour chain follows its stated rule."""
import ctypes as C
import types

import pytest


def _args(**kw):
    """Arguments that pass every check up to the window (fake non-NULL pointers: nothing is launched on rejection)."""
    from big_dreamer_amd import _cabi as cabi
    g = cabi.ImagineBwdArgs()
    for name, typ in g._fields_:
        if typ is C.c_void_p and name not in ("d_carry_in", "d_carry_out"):
            setattr(g, name, 4096)
    for i in range(3):
        g.wt_a[i] = 4096
    g.N, g.Hm, g.Be, g.S, g.A, g.Hd = 17, 5, 40, 10, 3, 32
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("window, text", [
    (dict(t_begin=2, t_end=2, d_carry_in=4096, d_carry_out=4096), b"bad window"),          # t_begin >= t_end
    (dict(t_begin=3, t_end=2, d_carry_in=4096, d_carry_out=4096), b"bad window"),
    (dict(t_begin=3, t_end=0, d_carry_out=4096), b"bad window"),                             # (0 / 0 alone is the rollout)
    (dict(t_begin=-1, t_end=5), b"bad window"),
    (dict(t_begin=0, t_end=6), b"bad window"),                                               # t_end > Hm
    (dict(t_begin=4, t_end=6, d_carry_out=4096), b"bad window"),
    (dict(t_begin=0, t_end=3), b"d_carry_in"),                                               # missing where needed
    (dict(t_begin=2, t_end=4, d_carry_out=4096), b"d_carry_in"),
    (dict(t_begin=2, t_end=5), b"d_carry_out"),
    (dict(t_begin=2, t_end=4, d_carry_in=4096), b"d_carry_out"),
    (dict(t_begin=0, t_end=5, d_carry_in=4096), b"d_carry_in"),                              # present where not needed
    (dict(t_begin=0, t_end=0, d_carry_in=4096), b"d_carry_in"),
    (dict(t_begin=0, t_end=5, d_carry_out=4096), b"d_carry_out"),
    (dict(t_begin=0, t_end=0, d_carry_out=4096), b"d_carry_out"),
])
def test_bad_windows_are_rejected_without_a_launch(window, text):
    from big_dreamer_amd import _cabi as cabi
    assert cabi.lib.bd_imagine_backward(C.byref(_args(**window)), None) != 0, window
    err = cabi.lib.bd_last_error()
    assert b"bd_imagine_backward" in err and text in err, (window, err)


def test_mlp_backward_rejects_a_negative_form_M():
    from big_dreamer_amd import _cabi as cabi
    m = cabi.MlpBwdArgs()
    m.M, m.dout, m.lddo, m.dout_scale, m.n_layers, m.form_M = 16, 4096, 8, 1.0, 1, -1
    m.layer[0] = cabi.LayerBwd(None, None, 8, 8, cabi.ACT_NONE, 4096)
    assert cabi.lib.bd_mlp_backward(C.byref(m), None) != 0 and b"form_M" in cabi.lib.bd_last_error()


def test_chunk_plan_rule():
    """behaviour_plan: explicit plans, near-equal K chunks, the default rule and the configurations that never chunk."""
    from big_dreamer_amd import engine as E

    def eng(bh_chunks, fused=True, categorical=False, rho=-1, use_discount=False, pixel=False):
        return types.SimpleNamespace(bh_chunks=bh_chunks, heads_fused=fused, pixel=pixel,
                                     _mix=None if rho in (-1, 1) else float(rho),
                                     d=types.SimpleNamespace(categorical=categorical, use_discount=use_discount))

    plan = E.DreamerEngine.behaviour_plan
    assert E._parse_bh_chunks("") is None and E._parse_bh_chunks("1") == 1 and E._parse_bh_chunks("5, 5,4") == (5, 5, 4)
    with pytest.raises(ValueError):
        E._parse_bh_chunks("5,0")
    assert plan(eng(1), 14, 2450) == (14,)
    assert plan(eng(3), 14, 2450) == (5, 5, 4) and plan(eng(4), 14, 2450) == (4, 4, 3, 3)
    assert plan(eng((8, 6)), 14, 2450) == (8, 6) and plan(eng(9), 5, 37) == (1, 1, 1, 1, 1)
    with pytest.raises(ValueError):
        plan(eng((8, 5)), 14, 2450)
    for off in (dict(fused=False), dict(categorical=True), dict(rho=0.5), dict(rho=0.0), dict(use_discount=True)):
        assert plan(eng((5, 5, 4), **off), 14, 2450) == (14,), off
    # the default rule: chunks only for a big state-observation rollout whose scans leave CUs idle
    default = plan(eng(None), 14, 2450)
    assert default in ((14,), plan(eng(E.BH_DEFAULT_CHUNKS), 14, 2450))
    assert plan(eng(None), 5, 37) == (5,) and plan(eng(None), 14, 16 * 193) == (14,) and plan(eng(None), 5, 2450) == (5,)
    assert plan(eng(None, pixel=True), 14, 2450) == (14,)
