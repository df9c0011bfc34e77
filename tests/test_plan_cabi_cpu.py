"""CPU tests: the C ABI of the CEM planner's rollout (csrc/planner.hip) without a launch.  bd_plan_rollout and
bd_plan_rollout_cat are two entry points over one argument block, one validator and one kernel body: which latent kind
each takes, what each refuses and in whose name, and the LDS carve (PlanDims) against the two formulas the launchers
computed by hand when each latent kind had a kernel file of its own."""
import ctypes as C
import itertools
import re

import pytest

from tests.helpers import split_scratch_floats

MAX_LDS = 160 * 1024
GAUSS, CAT = "bd_plan_rollout", "bd_plan_rollout_cat"
ENTRIES = {GAUSS: 0, CAT: 1}        # entry point -> the latent_cat it takes


def _block(entry, **over):
    """A block that `entry` would launch: its latent kind, small sizes, every pointer a fake non-NULL one (nothing is
    launched on a refusal).  `over` then sets the defect."""
    from big_dreamer_amd import _cabi as cabi
    a = cabi.PlanArgs()
    for name, typ in a._fields_:
        if typ is cabi.P:
            setattr(a, name, 4096)
        elif name in ("w_r", "b_r"):
            for i in range(5):
                getattr(a, name)[i] = 4096
    a.rows, a.H, a.cand, a.Be, a.A, a.Hd = 32, 3, 16, 24, 2, 20
    a.latent_cat = ENTRIES[entry]
    a.D, a.C, a.S = (3, 4, 12) if a.latent_cat else (0, 0, 6)
    for k, v in over.items():
        if k in ("w_r", "b_r"):
            for i in range(5):
                getattr(a, k)[i] = v
        else:
            setattr(a, k, v)
    return a


def _refused(entry, a):
    from big_dreamer_amd import _cabi as cabi
    assert getattr(cabi.lib, entry)(None if a is None else C.byref(a), None) != 0, entry
    err = cabi.lib.bd_last_error().decode()
    assert err.startswith(entry + ":"), (entry, err)
    return err


def test_one_struct():
    from big_dreamer_amd import _cabi as cabi
    assert cabi.PlanCatArgs is cabi.PlanArgs


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_block_and_wrong_kind(entry):
    """The block is complete otherwise, so the kind is its only defect."""
    assert "null argument block" in _refused(entry, None)
    other = CAT if entry == GAUSS else GAUSS
    a = _block(other)       # the other entry point's block: latent_cat and the matching dims
    err = _refused(entry, a)
    assert "latent_cat" in err and err.rstrip().endswith(other), err


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_dims_and_latent_rule(entry):
    from big_dreamer_amd import _cabi as cabi
    assert "bad dims" in _refused(entry, cabi.PlanArgs())        # a zeroed block, at either entry point
    assert "bad dims" in _refused(entry, _block(entry, rows=33))    # rows % cand != 0
    if entry == GAUSS:
        assert "state_size 65 > 64" in _refused(entry, _block(entry, S=65))
        assert "missing inputs" in _refused(entry, _block(entry, eps_state=None))
    else:
        assert "C <= 256" in _refused(entry, _block(entry, D=2, C=300, S=600))
        assert "256 % C == 0" in _refused(entry, _block(entry, D=6, C=48, S=288))     # S > 256 and 256 % 48 != 0
        assert "S = D*C" in _refused(entry, _block(entry, S=13))
        assert "% 4 == 0" in _refused(entry, _block(entry, D=3, C=5, S=15, eps_state=None))


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_outputs_and_reward_weights(entry):
    """Reward weights are asked for only when the rollout runs the reward model (returns given), at both entry points."""
    assert "missing outputs" in _refused(entry, _block(entry, returns=None, feat=None))
    if entry == CAT:
        assert "sidx" in _refused(entry, _block(entry, returns=None, sidx=None))
    a = _block(entry)
    a.b_r[4] = None
    assert "missing reward weights (layer 4)" in _refused(entry, a)
    none = dict(w_r=None, b_r=None, w_r0h=None, w_r0sT=None)
    assert "missing reward weights (layer 0)" in _refused(entry, _block(entry, **none))
    if entry == CAT:        # layer 0 is w_r0h / w_r0sT there, and w_r[0] is not looked at
        a = _block(entry)
        a.w_r[0] = None
        a.w_r0sT = None
        assert "missing reward weights (layer 0)" in _refused(entry, a)
    # only feat given: accepted without them.  Nothing may launch, so the block carries a later defect: no `actions`
    # (the outputs are checked after the weights), and -- over-limit sizes -- the LDS rule
    assert "missing outputs" in _refused(entry, _block(entry, returns=None, actions=None, **none))
    assert "B of LDS" in _refused(entry, _block(entry, returns=None, Be=4096, **none))
    assert "missing transition weights" in _refused(entry, _block(entry, returns=None, w_p1=None, **none))


def _kb(x):
    return -(-x // 16)


def _gauss_bytes(Be, S, A, Hd, scratch):
    return 4 * ((3 * _kb(Be) + 2 * _kb(Hd) + _kb(S) + _kb(A) + _kb(Be + S)) * 256 + 16 + scratch)


def _cat_bytes(Be, D, C, A, Hd, scratch):
    S = D * C
    return 4 * ((3 * _kb(Be) + 2 * _kb(Hd) + _kb(A)) * 256 + 16 * max(Be, Hd) + 32 * D + 16
                + max(scratch, 16 * (_kb(S) * 16 + 8)))


def test_lds_carve_is_the_two_former_formulas():
    """Over-limit sizes only (the in-limit carve runs in the GPU suites): the refusal states the bytes PlanDims asks for."""
    scratch = split_scratch_floats()
    assert scratch == 10240
    n = {GAUSS: 0, CAT: 0}
    for Be, Hd, A in itertools.product((24, 200, 4096), (20, 200, 1 << 16), (1, 17, 65)):
        cases = [(GAUSS, dict(S=S), _gauss_bytes(Be, S, A, Hd, scratch)) for S in (6, 30, 64)]
        cases += [(CAT, dict(D=D, C=Cc, S=D * Cc), _cat_bytes(Be, D, Cc, A, Hd, scratch)) for D, Cc in ((3, 5), (32, 32), (8, 32))]
        for entry, lat, want in cases:
            if want <= MAX_LDS:
                continue
            n[entry] += 1
            err = _refused(entry, _block(entry, Be=Be, Hd=Hd, A=A, **lat))
            m = re.search(r"needs (\d+) B of LDS \(limit (\d+)\)", err)
            assert m, err
            assert (int(m.group(1)), int(m.group(2))) == (want, MAX_LDS), (entry, Be, Hd, A, lat, err)
    assert n[GAUSS] and n[CAT], n
    # the reference's default sizes fit, with the figures csrc/planner.hip states
    assert _gauss_bytes(200, 30, 1, 200, scratch) == 126016 and _cat_bytes(200, 32, 32, 1, 200, scratch) == 150592
