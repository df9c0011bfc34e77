"""GPU tests of the CEM planner kernels (csrc/planner.hip: bd_plan_rollout, bd_plan_rollout_cat, bd_cem_refit) against
tests/plan_ref.py, through the C ABI on engines built at the case's dims: every step recomputed in float64 from the
kernel's own outputs of the step before, every Categorical draw against the margin of the float64 ratios, the refit's
selection exactly and its statistics against the two-pass bound.  Every case launches the rollout in its three forms
(feat and returns, feat only, returns only) and asserts that the first writes the bits of the other two: that is what
licenses checking `returns` against `feat`.  Every launch is followed by a synchronise (which raises on a device error);
nothing retries.  Each test prints the worst err / bound per quantity and the ambiguous-draw count as PLAN_RATIOS lines
(run with -s to see them)."""
import ctypes as C
import json

import pytest
import torch

from tests import plan_ref as PR
from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.dense_ref import SENTINEL

pytestmark = pytest.mark.gpu
BYTE_FILL = 0xEE
GUARD = 64
RNG = (0x5eed1234, 3, 7)


def _cabi():
    from big_dreamer_amd import _cabi as cabi
    return cabi


class Out:
    """A SENTINEL-filled output with GUARD elements behind it that must stay untouched."""

    def __init__(self, n, byte=False):
        self.n = n
        self.buf = torch.full((n + GUARD,), BYTE_FILL if byte else SENTINEL, dtype=torch.uint8 if byte else torch.float32, device="cuda")
        self.fill = BYTE_FILL if byte else SENTINEL

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def take(self, tag):
        assert bool((self.buf[self.n:] == self.fill).all()), f"{tag}: written behind its end"
        return self.buf[:self.n].clone()


class Case:
    """One engine at the case's dims with the case's weights, the inputs on the device, the float64 side of both."""

    def __init__(self, d, P, I):
        from big_dreamer_amd.engine import DreamerEngine
        self.d, self.P = d, P
        self.eng = DreamerEngine(PR.synth_dims(d), None, "cuda", params=P)
        self.I = {k: v.cuda().contiguous() for k, v in I.items()}
        self.W64, self.I64 = R.to64(PR.weights_of(P, "cuda")), R.to64(self.I)
        self.min_std = 0.0 if d.cat else float(self.eng._plan_args(d.rows, d.H, d.cand).min_std)

    def args(self, **over):
        d = self.d
        a = self.eng._plan_args(d.rows, d.H, d.cand)
        for k in ("init_belief", "init_state", "act_mean", "act_std", "eps_action", "eps_state"):
            setattr(a, k, self.I[k].data_ptr())
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def launch(self, form, eps_state="given"):
        """form: 'both' | 'feat' | 'returns'.  eps_state: 'given', 'kernel' (NULL + the Philox triple RNG) or a device tensor.
        Returns name -> flat device tensor of what the form writes."""
        cabi, d = _cabi(), self.d
        a = self.args()
        if eps_state == "kernel":
            a.eps_state, (a.seed, a.step, a.stream_id) = None, RNG
        elif torch.is_tensor(eps_state):
            a.eps_state = eps_state.data_ptr()
        out = dict(actions=Out(d.H * d.rows * d.A))
        if form != "returns":
            out["feat"] = Out(d.H * d.rows * (d.Be + d.S))
            if d.cat:
                out["sidx"] = Out(d.H * d.rows * d.D, byte=True)
        if form != "feat":
            out["returns"] = Out(d.rows)
        a.returns = a.feat = a.sidx = None
        for k, v in out.items():
            setattr(a, k, v.ptr)
        cabi.check((cabi.lib.bd_plan_rollout_cat if d.cat else cabi.lib.bd_plan_rollout)(C.byref(a), cabi.stream()))
        torch.cuda.synchronize()
        return {k: v.take(f"{form} {k}") for k, v in out.items()}

    def three_forms(self, tag, eps_state="given"):
        """The three launch forms; the combined one must write the bits of the two single-output ones.  Returns it."""
        both, feat, ret = (self.launch(f, eps_state) for f in ("both", "feat", "returns"))
        for k in feat:
            assert torch.equal(both[k], feat[k]), f"{tag}: {k} of the feat + returns launch differs from the feat-only launch"
        assert torch.equal(both["returns"], ret["returns"]), f"{tag}: returns differ between the combined and the returns-only launch"
        assert torch.equal(both["actions"], ret["actions"]), f"{tag}: actions of the returns-only launch"
        return both

    def tensors64(self, out):
        d = self.d
        K = dict(actions=out["actions"].double().view(d.H, d.rows, d.A), feat=out["feat"].double().view(d.H, d.rows, d.Be + d.S),
                 returns=out["returns"].double().view(1, d.rows, 1))
        if d.cat:
            K["sidx"] = out["sidx"].long().view(d.H, d.rows, d.D)
        return K

    def check(self, tag, out, eps_state=None):
        """Every element of every output against the float64 step reference.  Returns (worst err / bound per quantity,
        (ambiguous draws, draws, draws with a class >= 128))."""
        d = self.d
        for k, v in out.items():
            if k == "sidx":
                assert int(v.max()) < d.C, f"{tag}: sidx holds unwritten elements or classes outside [0, {d.C})"
            else:
                assert bool(torch.isfinite(v).all()) and not bool((v == SENTINEL).any()), f"{tag}: {k} holds unwritten elements"
        K = self.tensors64(out)
        I64 = self.I64 if eps_state is None else dict(self.I64, eps_state=eps_state.double())
        rep = {}
        R.check_layers(PR.split_feat(PR.rollout_layers(d, self.W64, I64, K, self.min_std), K, d.Be), K, rep, tag + " ")
        counts = PR.sample_checks(d, self.W64, I64, K, tag=tag + " ") if d.cat else (0, 0, 0)
        return rep, counts


# ---- Gaussian latents ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PR.GAUSS_CASES))
def test_gaussian_rollout_against_float64(name):
    d, P, I = PR.gauss_case(name)
    case = Case(d, P, I)
    out = case.three_forms(name)
    rep, _ = case.check(name, out)
    print("PLAN_RATIOS gaussian", name, json.dumps(rep), PR.dual_head_form(d.S), f"lds {PR.lds_bytes(d.Be, d.S, d.A, d.Hd)}")
    assert rep and max(rep.values()) < 1.0, rep


def test_gaussian_tile_does_not_depend_on_its_neighbour():
    """Rows 0..15 of the 17-row run equal the 16-row run on the same inputs, bit for bit."""
    d17, P, I = PR.gauss_case("rows_1x17_h4")
    d16 = d17._replace(cand=16)
    I16 = dict(I, eps_action=I["eps_action"][:, :16].contiguous(), eps_state=I["eps_state"][:, :16].contiguous())
    o17, o16 = Case(d17, P, I).launch("both"), Case(d16, P, I16).launch("both")
    for k, w in (("actions", d17.A), ("feat", d17.Be + d17.S)):
        assert torch.equal(o17[k].view(d17.H, 17, w)[:, :16], o16[k].view(d16.H, 16, w)), k
    assert torch.equal(o17["returns"][:16], o16["returns"])


def test_gaussian_refusals_come_before_any_launch():
    cabi = _cabi()
    for name, over, text in (("s64", dict(S=65), b"state_size"), ("widest", dict(Be=PR.GAUSS_TOO_WIDE.Be), b"B of LDS")):
        d, P, I = PR.gauss_case(name)
        case = Case(d, P, I)
        outs = [Out(d.H * d.rows * d.A), Out(d.rows), Out(d.H * d.rows * (d.Be + d.S))]
        a = case.args(actions=outs[0].ptr, returns=outs[1].ptr, feat=outs[2].ptr, **over)
        assert cabi.lib.bd_plan_rollout(C.byref(a), cabi.stream()) != 0
        msg = cabi.lib.bd_last_error()
        assert text in msg and (name != "widest" or b"needs" in msg), msg
        torch.cuda.synchronize()
        assert all(bool((o.buf == SENTINEL).all()) for o in outs), f"{name}: a refused call wrote its outputs"


# ---- Categorical latents --------------------------------------------------------------------------------------------------------

def _rng_fill(n):
    cabi = _cabi()
    q = torch.empty(n, device="cuda")
    r = cabi.RngFillArgs()
    r.n, r.seed, r.step = 1, RNG[0], RNG[1]
    r.t[0] = cabi.RngTensor(q.data_ptr(), q.numel(), cabi.BD_RNG_EXPONENTIAL, RNG[2])
    cabi.check(cabi.lib.bd_rng_fill(C.byref(r), cabi.stream()))
    torch.cuda.synchronize()
    return q


@pytest.mark.parametrize("seed", PR.CAT_SEEDS)
@pytest.mark.parametrize("name", list(PR.CAT_CASES))
def test_categorical_rollout_against_float64(name, seed):
    d, P, I = PR.cat_case(name, seed)
    case = Case(d, P, I)
    out = case.three_forms(name)
    rep, (amb, n, high) = case.check(name, out)
    line = f"ambiguous {amb} of {n}"
    assert rep and max(rep.values()) < 1.0, rep
    assert amb <= PR.AMBIGUOUS_CAP * n, (amb, n)
    K = case.tensors64(out)
    if d.C == 256:
        assert high > n // 2 and int(K["sidx"].max()) == 255, f"only {high} of {n} sampled classes are >= 128"
    if name == "dup":      # first maximum wins: the planted pair ties exactly and the higher index is never sampled
        for f in RC.dup_factors(d):
            assert not bool((K["sidx"][..., f] == RC.DUP_HI).any()), f"factor {f}: class {RC.DUP_HI} sampled"
        assert sum(int((K["sidx"][..., f] == RC.DUP_LO).sum()) for f in RC.dup_factors(d)) > 0, "the planted pair never won"
    if d.S % 4 == 0:       # in-kernel noise: the bits of a run fed bd_rng_fill's buffer, which is checked like any other run
        q = _rng_fill(d.H * d.rows * d.S).view(d.H, d.rows, d.S)
        fed, ker = case.three_forms(name + " rng-fed", q), case.three_forms(name + " in-kernel", "kernel")
        for k in fed:
            assert torch.equal(fed[k], ker[k]), f"{name}: {k} with in-kernel noise differs from the run fed bd_rng_fill's buffer"
        rep2, (amb2, n2, _) = case.check(name + " rng-fed", fed, q)
        assert max(rep2.values()) < 1.0 and amb2 <= PR.AMBIGUOUS_CAP * n2, (rep2, amb2, n2)
        line += f", rng {amb2} of {n2}"
    print("PLAN_RATIOS categorical", name, seed, json.dumps(rep), line, RC.sample_path(d.C), f"lds {PR.lds_bytes(d.Be, d.S, d.A, d.Hd, d.D, d.C)}")


# ---- refit ------------------------------------------------------------------------------------------------------------------------

def _refit(ret, act, H, B, cand, top, A):
    cabi = _cabi()
    dr, da = torch.from_numpy(ret).cuda(), torch.from_numpy(act).cuda()
    m, s = Out(H * B * A), Out(H * B * A)
    rc = cabi.lib.bd_cem_refit(dr.data_ptr(), ret.shape[0], da.data_ptr(), H, B, cand, top, A, m.ptr, s.ptr, cabi.stream())
    torch.cuda.synchronize()
    return rc, m, s, da


@pytest.mark.parametrize("case", PR.refit_cases(), ids=lambda c: c[0])
def test_refit_selection_and_statistics(case):
    name, (H, B, cand, top, A), rs, rpat, apat, seed = case
    ret, act = PR.refit_inputs(H, B, cand, top, A, rs, seed, rpat, apat)
    rc, m, s, da = _refit(ret, act, H, B, cand, top, A)
    _cabi().check(rc)
    ref = PR.refit_ref(ret, da, H, B, cand, top, A)
    rep = {}
    PR.check_refit(name, m.take("mean").view(H, B, A), s.take("std").view(H, B, A), ref, top, rep)
    print("PLAN_RATIOS refit", name, json.dumps(rep))


def test_refit_refusals():
    cabi = _cabi()
    ret, act = PR.refit_inputs(1, 1, 8, 4, 1, 1, 0)
    for cand, top, text in ((8, 9, b"top_candidates"), (8, 0, b"top_candidates"), (4097, 4, b"at most 4096"), (4096, 1025, b"at most 4096")):
        rc, m, s, _ = _refit(ret, act, 1, 1, cand, top, 1)
        assert rc != 0 and text in cabi.lib.bd_last_error(), (cand, top, cabi.lib.bd_last_error())
        assert bool((m.buf == SENTINEL).all()) and bool((s.buf == SENTINEL).all())
