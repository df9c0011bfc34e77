"""The chunked behaviour chain ("Chunked behaviour chain"): the forward imagination scan launched over segments
of time steps, and whole train steps under a chunk plan, against the single launches -- bit for bit.  Splitting in time
changes no arithmetic, so every comparison is torch.equal."""
import ctypes as C

import pytest
import torch

from big_dreamer_amd import synth
from tests import scan_ref as R
from tests.helpers import CASES, CAT_CASES
from tests.test_scan_kernels_gpu import ImagineCase, cabi, pout, same_bits, sync

pytestmark = pytest.mark.gpu

# N = 37: three row tiles, the last with 5 rows; no width is a multiple of 16
DIMS = R.Dims(T=5, B=37, Be=40, S=6, A=2, Hd=40)
PLANS = ((5,), (3, 2), (2, 2, 1), (1, 1, 1, 1, 1))


def _bounds(plan):
    return [(sum(plan[:i]), sum(plan[:i + 1])) for i in range(len(plan))]


class SegmentCase(ImagineCase):
    """ImagineCase with the forward in any number of time segments."""

    def forward_plan(self, plan):
        c, d, pk, p = cabi(), self.d, self.pk, self.pin
        M = d.T * d.B
        out = {k: pout(M, w) for k, w in self.widths().items()}
        out["sv_actor"] = pout(4 * M, d.Hd)
        for t0, t1 in _bounds(plan):
            a = c.ImagineFwdArgs()
            a.N, a.Hm, a.Be, a.S, a.A, a.Hd, a.n_samples = d.B, t1 - t0, d.Be, d.S, d.A, d.Hd, 1
            a.w_embed_s, a.w_embed_a, a.b_embed = pk["embed_s"].data_ptr(), pk["embed_a"].data_ptr(), self.W["b_e"].data_ptr()
            a.w_ir, a.w_iz, a.w_in = (pk[k].data_ptr() for k in ("ir", "iz", "in"))
            a.w_hr, a.w_hz, a.w_hn = (pk[k].data_ptr() for k in ("hr", "hz", "hn"))
            a.b_ih, a.b_hh = self.W["b_ih"].data_ptr(), self.W["b_hh"].data_ptr()
            a.w_p1, a.b_p1 = pk["p1"].data_ptr(), self.W["b_1"].data_ptr()
            a.w_p2m, a.w_p2s, a.b_p2 = pk["p2m"].data_ptr(), pk["p2s"].data_ptr(), self.W["b_2"].data_ptr()
            a.w_a0h, a.w_a0s = pk["a0h"].data_ptr(), pk["a0s"].data_ptr()
            for l in range(3):
                a.w_a[l] = pk[f"a{l + 1}"].data_ptr()
            for l in range(4):
                a.b_a[l] = self.W["b_a"][l].data_ptr()
            a.w_a4m, a.w_a4s, a.b_a4 = pk["a4m"].data_ptr(), pk["a4s"].data_ptr(), self.W["b_a4"].data_ptr()
            shift = lambda pl, w: pl.ptr + 4 * t0 * d.B * w
            a.start_feat = p["start_feat"].ptr if t0 == 0 else shift(out["feat"], d.Be + d.S) - 4 * d.B * (d.Be + d.S)
            a.eps_action, a.eps_prior, a.eps_entropy = shift(p["eps_action"], d.A), shift(p["eps_prior"], d.S), None
            a.min_std, a.act_raw_init_std, a.act_min_std, a.act_mean_scale = (self.min_std, R.ACT_RAW_INIT_STD, R.ACT_MIN_STD,
                                                                              R.ACT_MEAN_SCALE)
            for k, w in self.widths().items():
                setattr(a, k, shift(out[k], w))
            a.sv_actor, a.sv_actor_stride = shift(out["sv_actor"], d.Hd), (M * d.Hd if len(plan) > 1 else 0)
            c.check(c.lib.bd_imagine_forward_scan(C.byref(a), c.stream()))
            sync()
        for k, v in out.items():
            assert v.outside_unchanged(), f"imagine forward {plan}: {k} written outside its rows"
        return out


@pytest.fixture(scope="module")
def case():
    c = SegmentCase(DIMS, 31)
    c.fwd = c.forward_plan((DIMS.T,))
    return c


def test_forward_segments_give_the_bits_of_the_single_launch(case):
    """ifeat, actions, prior statistics and every save, for every plan; the single launch is the one the float64 suite
    checks (ImagineCase.forward)."""
    same_bits(case.forward(), case.fwd, "forward through forward_plan((5,))")
    for plan in PLANS[1:]:
        same_bits(case.fwd, case.forward_plan(plan), f"forward in segments {plan}")


# ---- engine ---------------------------------------------------------------------------------------------------------------

def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _run(name, plan, pipeline, hp_extra=None, steps=3):
    """`steps` train steps with perf-mode noise in a fresh engine -> (effective plan, logs per step, state)."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = {**CASES, **CAT_CASES}[name]
    torch.manual_seed(1234)
    eng = DreamerEngine(d, dict(hp, **(hp_extra or {})), "cuda", params=synth.make_params(d, seed))
    eng.pipeline, eng.bh_chunks = pipeline, plan
    logs = [eng.train_step(_dev(synth.make_batch(d, seed + i))) for i in range(steps)]
    eng.join()
    torch.cuda.synchronize()
    state = {}
    for g in ("model", "actor", "critic"):
        grp = eng.groups[g]
        state.update({g + ".p": grp.flat.clone(), g + ".m": grp.m.clone(), g + ".v": grp.v.clone()})
    return eng._bh_plan_used, logs, state


def _assert_same(a, b, what):
    assert a[1] == b[1], (what, a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), (what, k)


@pytest.mark.parametrize("pipeline", [True, False], ids=["pipelined", "serial"])
def test_train_steps_under_a_chunk_plan_are_bit_identical(pipeline):
    """SMALL (H = 6: five imagined steps): every parameter, every Adam moment and every logged scalar after three steps."""
    ref = _run("small", 1, pipeline)
    assert ref[0] == (5,) and all(torch.isfinite(v).all() for v in ref[2].values())
    for plan in ((2, 2, 1), (1, 1, 1, 1, 1)):
        got = _run("small", plan, pipeline)
        assert got[0] == plan
        _assert_same(ref, got, plan)


@pytest.mark.parametrize("name, hp_extra, plan", [
    ("cat_tiny", None, (1, 1, 1)),
    ("small", dict(gradient_mixing=0.5), (2, 2, 1)),
    ("tiny_discount", None, (1, 1, 1)),
], ids=["categorical", "gradient_mixing", "use_discount"])
def test_other_configurations_keep_the_single_launches(name, hp_extra, plan):
    ref = _run(name, 1, True, hp_extra, steps=2)
    got = _run(name, plan, True, hp_extra, steps=2)
    assert len(ref[0]) == 1 and got[0] == ref[0], (ref[0], got[0])
    _assert_same(ref, got, name)


def test_chunk_spans_report_the_sum_over_chunks():
    """A span key keeps its meaning under a plan: one entry per step, all chunks' launches in it."""
    from big_dreamer_amd.engine import DreamerEngine
    d, seed, hp, _ = CASES["small"]
    eng = DreamerEngine(d, hp, "cuda", params=synth.make_params(d, seed))
    eng.bh_chunks = (2, 2, 1)
    eng.enable_timers(True)
    for i in range(2):
        eng.train_step(_dev(synth.make_batch(d, seed + i)), sync_logs=False)
    eng.join()
    torch.cuda.synchronize()
    summary = eng.timer_summary()
    for k in ("imagine_fwd", "img_heads_bwd", "imagine_bwd", "actor_hidden_bwd", "wgrad_actor"):
        assert summary[k][1] == 2 and summary[k][0] > 0, (k, summary[k])
    assert len(eng._timer_more["img_heads_bwd"]) == 4 and "actor_hidden_bwd" not in eng._timer_more
