"""CPU test: the default chunk plan of the behaviour chain follows its stated rule."""
import types

import pytest


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
