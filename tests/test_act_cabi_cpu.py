"""CPU tests: the C ABI of the acting step (csrc/act.hip) without a launch.  bd_act_step and bd_act_step_cat are two entry
points over one argument block, one validator and one kernel body: the sizes each accepts, which of the four
(latent_cat, actor_cat) configurations each takes, and that a refusal names the entry point that was called."""
import ctypes as C
import itertools

import pytest

from tests.helpers import split_scratch_floats

MAX_LDS = 160 * 1024
GRID = list(itertools.product((24, 200), (6, 30, 64, 65), (0, 1, 2, 64, 65), (20, 200, 1 << 16, (1 << 20) + 1), (40, 1024),
                              (-1, 0, 3, 5)))        # Be, S, A, Hd, E, O


def _rule(Be, S, A, Hd, E, O, scratch):
    """What bd_act_step_supported answered when the Gaussian step had a kernel and a launcher of its own."""
    if min(Be, S, A, Hd, E) <= 0 or O < 0 or max(Be, Hd, E, O) > 1 << 20 or S > 64 or A > 64:
        return 0
    kb = lambda x: -(-x // 16)
    floats = (3 * max(kb(Be), kb(Hd)) + max(kb(E), kb(O)) + kb(S) + kb(A)) * 256 + scratch
    return int(floats * 4 <= MAX_LDS)


def test_supported_sizes():
    from big_dreamer_amd import _cabi as cabi
    lib = cabi.lib
    scratch = split_scratch_floats()
    assert scratch == 10240
    assert (200, 30, 1, 200, 1024, 3) in GRID and _rule(200, 30, 1, 200, 1024, 3, scratch) == 1      # the reference's default
    got = {1: 0, 0: 0}
    for Be, S, A, Hd, E, O in GRID:
        want = _rule(Be, S, A, Hd, E, O, scratch)
        got[want] += 1
        assert lib.bd_act_step_supported(Be, S, A, Hd, E, O) == want, (Be, S, A, Hd, E, O)
        # Gaussian latents under the Categorical actor: the same LDS arithmetic
        if A <= 64:
            assert lib.bd_act_step_cat_supported(Be, 0, 0, S, A, Hd, E, O, 0, 1) == want, (Be, S, A, Hd, E, O)
        # (0, 0) is bd_act_step's, whatever the sizes
        assert lib.bd_act_step_cat_supported(Be, 0, 0, S, A, Hd, E, O, 0, 0) == 0, (Be, S, A, Hd, E, O)
    assert got[0] and got[1]
    assert _rule(24, 6, 2, 1 << 16, 40, 5, scratch) == 0 and _rule(24, 64, 64, 20, 40, 0, scratch) == 1       # LDS; O = 0


@pytest.mark.parametrize("entry, over", [("bd_act_step", dict(latent_cat=1)), ("bd_act_step", dict(actor_cat=1)),
                                         ("bd_act_step", dict(latent_cat=1, actor_cat=1)), ("bd_act_step_cat", dict()),
                                         ("bd_act_step", None), ("bd_act_step_cat", None)])
def test_rejection_names_the_entry_point(entry, over):
    """The wrong configuration for an entry point, or a NULL block (over = None): refused in the refusal's own words,
    nothing launched.  The block is complete otherwise, so the configuration is its only defect."""
    from big_dreamer_amd import _cabi as cabi
    a = None
    if over is not None:
        a = cabi.ActArgs()
        for name, typ in a._fields_:        # fake non-NULL pointers: nothing is launched on rejection
            if typ is cabi.P:
                setattr(a, name, 4096)
            elif name in ("w_enc", "b_enc", "w_a", "b_a"):
                for i in range(len(getattr(a, name))):
                    getattr(a, name)[i] = 4096
        a.embedding = None
        a.belief_out, a.state_out, a.action_out = 8192, 12288, 16384
        a.B, a.Be, a.D, a.C, a.S, a.A, a.Hd, a.E, a.O = 1, 24, 2, 3, 6, 2, 20, 40, 5
        for k, v in over.items():
            setattr(a, k, v)
        a = C.byref(a)
    assert getattr(cabi.lib, entry)(a, None) != 0, (entry, over)
    err = cabi.lib.bd_last_error().decode()
    assert err.startswith(entry + ":"), (entry, over, err)
    if over is None:
        assert "null argument block" in err, err
    elif entry == "bd_act_step":
        assert "latent_cat = 0 and actor_cat = 0" in err, err
    else:
        assert "that configuration is bd_act_step" in err, err


def test_one_struct():
    from big_dreamer_amd import _cabi as cabi
    assert cabi.ActCatArgs is cabi.ActArgs
