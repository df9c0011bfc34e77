"""GPU tests of the Categorical RSSM scan kernels against tests/scan_cat_ref.py: bd_observe_cat_forward / _backward, their
cluster forms at every accepted cluster size, bd_imagine_cat_forward and bd_imagine_cat_backward, called through the C ABI,
every layer of every step checked in float64 from the kernel's own tensors of the layer before, every sampled class
against the margin of the float64 ratios.  Every launch is followed by a synchronise (which raises on a device error) and,
for a cluster launch, by bd_observe_cluster_status; nothing retries.  Each test prints the worst err / bound ratio per
tensor and form and the ambiguous-sample count as SCAN_CAT_RATIOS lines (run with -s to see them)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import scan_cat_ref as RC
from tests import scan_ref as R
from tests.dense_ref import SENTINEL, Placed, pack, placed_input
from tests.test_scan_kernels_gpu import cabi, pin, pout, ptr, same_bits, sync, view64

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV = ("sv_s", "sv_x", "sv_gates", "sv_q")
BYTE_FILL = 0xEE


class PlacedBytes:
    """[rows x cols] uint8 output with two rows of padding behind it (the sidx outputs)."""

    def __init__(self, rows, cols):
        self.rows, self.cols = rows, cols
        self.buf = torch.full(((rows + 2) * cols + 16,), BYTE_FILL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[:rows * cols].view(rows, cols)
        self.ptr = self.buf.data_ptr()

    def outside_unchanged(self):
        return bool((self.buf[self.rows * self.cols:] == BYTE_FILL).all())


def gru_blocks(W, Be):
    out = {}
    for i, g in enumerate("rzn"):
        out["i" + g] = W["W_ih"][i * Be:(i + 1) * Be]
        out["h" + g] = W["W_hh"][i * Be:(i + 1) * Be]
    return out


def forms_of(d):
    return ["single"] + [f"cluster{Cm}" for Cm in RC.cluster_sizes(d.B, d.Be, d.D, d.C, d.Hd)]


# ---- observe ------------------------------------------------------------------------------------------------------------

class ObserveCase:
    def __init__(self, d, seed, nonterm="zeros", init="mixed", dpl=True, bias_high=False, duplicate=False):
        self.d = d
        self.W = W = RC.make_weights(d, seed, "cuda", bias_high=bias_high)
        self.I = I = RC.make_observe_inputs(d, seed, "cuda", nonterm=nonterm, init=init)
        if duplicate:
            RC.plant_duplicate(d, W, I["q_post"])
        self.G = G = RC.make_observe_grads(d, seed, "cuda", dpl=dpl)
        Be, S_ = d.Be, d.S
        blocks = dict(embed_s=W["W_e"][:, :S_], embed_a=W["W_e"][:, S_:], q1h=W["W_1"], q2=W["W_2"], **gru_blocks(W, Be))
        self.pk = {k: pack(v, False) for k, v in blocks.items() if k != "embed_s"}
        self.pkT = {k: pack(v, True) for k, v in blocks.items() if k != "embed_a"}
        self.embed_sT = W["W_e"][:, :S_].t().contiguous()
        self.pin = dict(init_belief=pin(I["init_belief"], Be), init_state=pin(I["init_state"], S_), actions=pin(I["actions"], d.A),
                        nonterm=pin(I["nonterm"], 1), pre_emb=pin(I["pre_emb"], d.Hd), q_post=pin(I["q_post"], S_),
                        dfeat=pin(G["dfeat"], Be + S_), dpost_logits=pin(G["dpost_logits"], S_))
        self.W64, self.I64, self.G64 = R.to64(W), R.to64(I), R.to64(G)
        sync()

    def workspace(self, form):
        if form == "single":
            return None
        d = self.d
        n = int(cabi().lib.bd_observe_cat_cluster_ws_floats(d.B, d.Be, d.Hd, d.D, int(form[7:])))
        return torch.zeros(n, device="cuda")

    def _launch(self, form, single, cluster, args, ws):
        c = cabi()
        if form == "single":
            c.check(single(C.byref(args), c.stream()))
            sync()
            return
        c.check(cluster(C.byref(args), int(form[7:]), ws.data_ptr(), ws.numel(), c.stream()))
        sync()
        c.check(c.lib.bd_observe_cluster_status(ws.data_ptr(), self.d.B, c.stream()))

    def forward(self, form, ws=None, save=SV):
        c, d, pk, p = cabi(), self.d, self.pk, self.pin
        a = c.ObserveCatFwdArgs()
        a.T, a.B, a.Be, a.D, a.C, a.A, a.Hd = d
        a.w_embed_sT, a.w_embed_a, a.b_embed = self.embed_sT.data_ptr(), pk["embed_a"].data_ptr(), self.W["b_e"].data_ptr()
        a.w_ir, a.w_iz, a.w_in = (pk[k].data_ptr() for k in ("ir", "iz", "in"))
        a.w_hr, a.w_hz, a.w_hn = (pk[k].data_ptr() for k in ("hr", "hz", "hn"))
        a.b_ih, a.b_hh = self.W["b_ih"].data_ptr(), self.W["b_hh"].data_ptr()
        a.w_q1h, a.b_q1, a.w_q2, a.b_q2 = pk["q1h"].data_ptr(), self.W["b_1"].data_ptr(), pk["q2"].data_ptr(), self.W["b_2"].data_ptr()
        for k in ("init_belief", "init_state", "actions", "nonterm", "pre_emb", "q_post"):
            setattr(a, k, ptr(p[k]))
        M = d.T * d.B
        out = {k: (pout(M, w(d)) if (k in save or not k.startswith("sv_")) else None) for k, w in RC.OBS_FWD_TENSORS.items()}
        out["sidx"] = PlacedBytes(M, d.D)
        for k, v in out.items():
            setattr(a, k, ptr(v))
        self._launch(form, c.lib.bd_observe_cat_forward, c.lib.bd_observe_cat_forward_cluster, a, ws)
        for k, v in out.items():
            assert v is None or v.outside_unchanged(), f"{form}: {k} written outside its rows"
        return out

    def backward(self, form, fwd, ws=None):
        c, d, pkT, p = cabi(), self.d, self.pkT, self.pin
        b = c.ObserveCatBwdArgs()
        b.T, b.B, b.Be, b.D, b.C, b.A, b.Hd = d
        b.wt_embed_s = pkT["embed_s"].data_ptr()
        b.wt_ir, b.wt_iz, b.wt_in = (pkT[k].data_ptr() for k in ("ir", "iz", "in"))
        b.wt_hr, b.wt_hz, b.wt_hn = (pkT[k].data_ptr() for k in ("hr", "hz", "hn"))
        b.wt_q1h, b.wt_q2 = pkT["q1h"].data_ptr(), pkT["q2"].data_ptr()
        keep = {k: placed_input(fwd[k].view.clone(), fwd[k].cols) for k in ("feat", "post_logits", "sv_x", "sv_gates", "sv_q")}
        for k, v in keep.items():
            setattr(b, k, v.ptr)
        for k in ("init_belief", "nonterm", "dfeat", "dpost_logits"):
            setattr(b, k, ptr(p[k]))
        out = {k: pout(d.T * d.B, w(d)) for k, w in RC.OBS_BWD_TENSORS.items()}
        for k, v in out.items():
            setattr(b, k, v.ptr)
        self._launch(form, c.lib.bd_observe_cat_backward, c.lib.bd_observe_cat_backward_cluster, b, ws)
        for k, v in out.items():
            assert v.outside_unchanged(), f"{form}: {k} written outside its rows"
        return out

    def tensors64(self, fwd):
        d = self.d
        K = {k: (view64(v, d, v.cols) if v is not None else None) for k, v in fwd.items() if k != "sidx"}
        K["sidx"] = fwd["sidx"].view.reshape(d.T, d.B, d.D).long()
        return K

    def check(self, form, fwd, bwd, AL=R.HW, exact=False, report=None):
        """Returns (ambiguous factors, factors, factors with a class >= 128)."""
        d = self.d
        Kf = self.tensors64(fwd)
        R.check_layers(RC.observe_fwd_layers(d, self.W64, self.I64, Kf, AL), Kf, report, f"{form} ")
        counts = [0, 0, 0]
        for t in range(d.T):
            res = RC.sample_check(Kf["post_logits"][t], self.I64["q_post"][t], Kf["sidx"][t], d.D, d.C, RC.sample_path(d.C, exact),
                                  f"{form} t={t} ")
            counts = [x + y for x, y in zip(counts, res)]
        Kb = {k: view64(v, d, v.cols) for k, v in bwd.items()}
        I = dict(self.I64, **{k: Kf[k] for k in ("feat", "post_logits", "sv_x", "sv_gates", "sv_q")})
        R.check_layers(RC.observe_bwd_layers(d, self.W64, I, Kb, self.G64, AL), Kb, report, f"{form} ")
        return counts


def run_observe_shape(name, AL=R.HW, exact=False, repeats=True):
    """Every form that accepts the shape, against the same reference; returns ({form: {tensor: worst err / bound}}, counts)."""
    d = RC.OBSERVE_SHAPES[name][0]
    nonterm, init, dpl = RC.observe_variant(name)
    case = ObserveCase(d, RC.SEEDS[0], nonterm, init, dpl, bias_high=name == "c256_d2")
    reports, counts, first = {}, [0, 0, 0], None
    for form in forms_of(d):
        ws = case.workspace(form)
        fwd = case.forward(form, ws)
        bwd = case.backward(form, fwd, ws)
        reports[form] = {}
        counts = [x + y for x, y in zip(counts, case.check(form, fwd, bwd, AL, exact, reports[form]))]      # summed over the forms
        if first is None:
            first = fwd
        assert torch.equal(first["sidx"].buf, fwd["sidx"].buf), f"{name}: sampled classes differ between single and {form}"
        assert torch.equal(first["feat"].view[:, d.Be:], fwd["feat"].view[:, d.Be:]), f"{name}: one-hot states differ, {form}"
        if d.C == 1:        # degenerate single class: the state is all ones, the logit gradient exactly dpost_logits
            assert bool((fwd["feat"].view[:, d.Be:] == 1).all())
            assert torch.equal(bwd["d_q2_out"].view, case.G["dpost_logits"].reshape(-1, d.S)), f"{name} {form}: d_q2_out"
        if repeats:
            same_bits(fwd, case.forward(form, ws), f"{name} {form} forward, second run")
            same_bits(bwd, case.backward(form, fwd, ws), f"{name} {form} backward, second run")
            if ws is not None:
                same_bits(fwd, case.forward(form, case.workspace(form)), f"{name} {form} forward, fresh workspace")
                same_bits(bwd, case.backward(form, fwd, case.workspace(form)), f"{name} {form} backward, fresh workspace")
    return reports, counts


@pytest.mark.parametrize("name", list(RC.OBSERVE_SHAPES))
def test_observe_forms_against_float64(name):
    d, Cm = RC.OBSERVE_SHAPES[name][:2]
    reports, (amb, n, high) = run_observe_shape(name)
    print("SCAN_CAT_RATIOS observe", name, json.dumps(reports), f"ambiguous {amb} of {n}")
    assert list(reports)[1:2] == ([f"cluster{Cm}"] if Cm else []), list(reports)
    for form, rep in reports.items():
        assert rep and max(rep.values()) < 1.0, (form, rep)
    assert amb <= 1e-3 * n, (amb, n)
    if name == "c256_d2":
        assert high > n // 2, f"only {high} of {n} sampled classes are >= 128"


@pytest.mark.parametrize("name", ["c32_d12", "c16_d20", "c5_d3"])
def test_observe_inference_and_partial_saves_are_bit_identical(name):
    """Every sv_* NULL (inference), and each sv_* pointer NULL on its own: the outputs, the sampled classes and the
    remaining saves keep their bits, in every form."""
    d = RC.OBSERVE_SHAPES[name][0]
    case = ObserveCase(d, RC.SEEDS[1])
    for form in forms_of(d):
        ws = case.workspace(form)
        full = case.forward(form, ws)
        same_bits(full, case.forward(form, ws, save=()), f"{name} {form} inference")
        for drop in SV:
            same_bits(full, case.forward(form, ws, save=tuple(k for k in SV if k != drop)), f"{name} {form} without {drop}")


@pytest.mark.parametrize("name", ["c16_d20", "c32_d12"])
def test_first_maximum_wins_between_identical_classes(name):
    """Class 11 of two factors is a copy of class 3 (W_2 row, bias, draws): the kernel's two logits are bit-equal (asserted
    first), so the ratios tie and the lower index must be the one sampled wherever the pair wins, in every form."""
    d = RC.OBSERVE_SHAPES[name][0]
    case = ObserveCase(d, RC.SEEDS[0], duplicate=True)
    for form in forms_of(d):
        fwd = case.forward(form, case.workspace(form), save=())
        won = RC.duplicate_check(d, fwd["post_logits"].view.reshape(d.T, d.B, d.S), fwd["sidx"].view.reshape(d.T, d.B, d.D))
        print("SCAN_CAT_RATIOS duplicate", name, form, f"pair won {won} of {d.T * d.B * 2}")
        assert won > 0, "the planted pair never won: the case checks nothing"


# ---- imagination --------------------------------------------------------------------------------------------------------

N_SAMPLES = 3


class ImagineCase:
    def __init__(self, d, seed, ent_weight=True, start="mixed", dentropy=-0.37, bias_high=False, discrete=False, variant=None):
        """variant: one of the Categorical actor's variants (scan_ref.make_discrete_case; implies discrete)."""
        self.d, self.dentropy, self.discrete, self.sat, self.dup = d, dentropy, discrete or variant is not None, None, None
        if variant is not None:
            self.W, self.I, self.sat, self.dup = RC.make_discrete_case(d, seed, variant, "cuda")
        else:
            self.W = RC.make_weights(d, seed, "cuda", imagine=True, bias_high=bias_high)
            self.I = RC.make_imagine_inputs(d, seed, "cuda", start=start, discrete=discrete)
        W, I = self.W, self.I
        self.G = G = RC.make_imagine_grads(d, seed, "cuda", ent_weight=ent_weight)
        g = torch.Generator().manual_seed(seed + 6000)
        self.eps_entropy = torch.randn(d.T, N_SAMPLES, d.B, d.A, generator=g).cuda()
        Be, S_, A = d.Be, d.S, d.A
        blocks = dict(embed_s=W["W_e"][:, :S_], embed_a=W["W_e"][:, S_:], p1=W["W_1"], p2=W["W_2"], a0h=W["W_a0"][:, :Be],
                      a1=W["W_a"][0], a2=W["W_a"][1], a3=W["W_a"][2], a4m=W["W_a4"][:A], a4s=W["W_a4"][A:], a4=W["W_a4"],
                      **gru_blocks(W, Be))
        self.pk = {k: pack(v, False) for k, v in blocks.items()}
        self.pkT = {k: pack(v, True) for k, v in blocks.items()}
        self.embed_sT = W["W_e"][:, :S_].t().contiguous()
        self.a0sT = W["W_a0"][:, Be:].t().contiguous()
        self.pin = dict(start_feat=pin(I["start_feat"], Be + S_), eps_action=pin(I["eps_action"], A), q_prior=pin(I["q_prior"], S_),
                        dfeat=pin(G["dfeat"], Be + S_), ent_weight=pin(G["ent_weight"], 1),
                        eps_entropy=pin(self.eps_entropy, A))
        self.W64, self.I64, self.G64 = R.to64(W), R.to64(I), R.to64(G)
        sync()

    def widths(self):
        d = self.d
        if self.discrete:
            return dict(feat=d.Be + d.S, prior_logits=d.S, action=d.A, sv_act_stats=d.A, sv_x=d.Be, sv_gates=4 * d.Be, sv_p=d.Hd,
                        entropy=1)
        return dict(feat=d.Be + d.S, prior_logits=d.S, action=d.A, sv_act_stats=4 * d.A, sv_x=d.Be, sv_gates=4 * d.Be, sv_p=d.Hd,
                    sv_act_us=2 * d.A, entropy=1)

    def forward(self, with_us=True, start_sidx=None, start_feat=None, entropy=False, eps_entropy=None, n_samples=N_SAMPLES,
                stats=True):
        """entropy: eps_entropy given (the call runs bd_actor_entropy itself); otherwise the scan alone.  eps_entropy
        (a Placed [Hm * n_samples * N x A]) with stats = False: the in-scan estimate (test_entropy_kernels_gpu.py)."""
        c, d, pk, p = cabi(), self.d, self.pk, self.pin
        M = d.T * d.B
        out = {k: pout(M, w) for k, w in self.widths().items()}
        out["sv_actor"] = pout(4 * M, d.Hd)
        out["sidx"] = PlacedBytes(M, d.D)
        if not with_us or self.discrete:
            out["sv_act_us"] = None
        if not stats:
            out["sv_act_stats"] = None
        a = c.ImagineCatFwdArgs()
        a.N, a.Hm, a.Be, a.D, a.C, a.A, a.Hd, a.n_samples = d.B, d.T, d.Be, d.D, d.C, d.A, d.Hd, n_samples
        a.w_embed_sT, a.w_embed_a, a.b_embed = self.embed_sT.data_ptr(), pk["embed_a"].data_ptr(), self.W["b_e"].data_ptr()
        a.w_ir, a.w_iz, a.w_in = (pk[k].data_ptr() for k in ("ir", "iz", "in"))
        a.w_hr, a.w_hz, a.w_hn = (pk[k].data_ptr() for k in ("hr", "hz", "hn"))
        a.b_ih, a.b_hh = self.W["b_ih"].data_ptr(), self.W["b_hh"].data_ptr()
        a.w_p1, a.b_p1, a.w_p2, a.b_p2 = pk["p1"].data_ptr(), self.W["b_1"].data_ptr(), pk["p2"].data_ptr(), self.W["b_2"].data_ptr()
        a.w_a0h, a.w_a0sT = pk["a0h"].data_ptr(), self.a0sT.data_ptr()
        for l in range(3):
            a.w_a[l] = pk[f"a{l + 1}"].data_ptr()
        for l in range(4):
            a.b_a[l] = self.W["b_a"][l].data_ptr()
        a.w_a4m, a.w_a4s, a.b_a4 = pk["a4m"].data_ptr(), pk["a4s"].data_ptr(), self.W["b_a4"].data_ptr()
        a.start_feat = (start_feat if start_feat is not None else p["start_feat"]).ptr
        if start_sidx is not None:      # [N x D] bytes with two rows of 0xEE behind them, as the float inputs carry NaN
            sx = PlacedBytes(d.B, d.D)
            sx.view.copy_(start_sidx)
        a.start_sidx = sx.ptr if start_sidx is not None else None
        a.eps_action, a.q_prior = p["eps_action"].ptr, p["q_prior"].ptr
        a.eps_entropy = eps_entropy.ptr if eps_entropy is not None else (p["eps_entropy"].ptr if entropy else None)
        a.act_raw_init_std, a.act_min_std, a.act_mean_scale = R.ACT_RAW_INIT_STD, R.ACT_MIN_STD, R.ACT_MEAN_SCALE
        for k, v in out.items():
            setattr(a, k, ptr(v))
        a.discrete_actions = int(self.discrete)
        c.check(c.lib.bd_imagine_cat_forward(C.byref(a), c.stream()))
        sync()
        for k, v in out.items():
            assert v is None or v.outside_unchanged(), f"imagine forward: {k} written outside its rows"
        if not entropy and not self.discrete and stats:
            assert bool((out["entropy"].buf == SENTINEL).all()), "the scan wrote an entropy although sv_act_stats was given"
        return out

    def actor_entropy(self, out):
        """bd_actor_entropy on the scan's statistics, as the caller of the scan-alone form runs it."""
        c, d = cabi(), self.d
        c.check(c.lib.bd_actor_entropy(self.pin["eps_entropy"].ptr, out["sv_act_stats"].ptr, out["entropy"].ptr, d.T, d.B, d.A,
                                       N_SAMPLES, c.stream()))
        sync()
        assert out["sv_act_stats"].outside_unchanged() and out["entropy"].outside_unchanged()

    def tensors64(self, out):
        d = self.d
        skip = ("sv_actor", "sidx") if self.discrete else ("sv_actor", "entropy", "sidx")
        K = {k: (view64(v, d, v.cols) if v is not None else None) for k, v in out.items() if k not in skip}
        sa = out["sv_actor"].view.reshape(4, d.T, d.B, d.Hd).double()
        K.update({f"sv_actor{l}": sa[l] for l in range(4)})
        K["sidx"] = out["sidx"].view.reshape(d.T, d.B, d.D).long()
        return K

    def backward(self, fwd, actor_pre=True, chain=False, ent_weight=True):
        """chain: the scan with d_actor_pre = NULL followed by the caller's bd_mlp_backward over all rows, bound as the engine
        binds it (the Categorical actor: lddo = A and the transposed pack of W_a4's A logit rows as the last layer)."""
        c, d, pkT, p = cabi(), self.d, self.pkT, self.pin
        M, A = d.T * d.B, d.A
        Ao = A if self.discrete else 2 * A
        b = c.ImagineCatBwdArgs()
        b.N, b.Hm, b.Be, b.D, b.C, b.A, b.Hd = d.B, d.T, d.Be, d.D, d.C, d.A, d.Hd
        b.wt_embed_s, b.wt_embed_a = pkT["embed_s"].data_ptr(), pkT["embed_a"].data_ptr()
        b.wt_ir, b.wt_iz, b.wt_in = (pkT[k].data_ptr() for k in ("ir", "iz", "in"))
        b.wt_hr, b.wt_hz, b.wt_hn = (pkT[k].data_ptr() for k in ("hr", "hz", "hn"))
        b.wt_p1, b.wt_p2 = pkT["p1"].data_ptr(), pkT["p2"].data_ptr()
        for l in range(3):
            b.wt_a[l] = pkT[f"a{l + 1}"].data_ptr()
        b.wt_a4m, b.wt_a4s = pkT["a4m"].data_ptr(), (None if self.discrete else pkT["a4s"].data_ptr())
        stats = fwd["sv_act_stats"].view.clone()
        if not self.discrete:
            stats[:, 2 * A:3 * A], stats[:, 3 * A:] = self.G["slot2"].reshape(M, A), self.G["slot3"].reshape(M, A)
        keep = {k: placed_input(fwd[k].view.clone(), fwd[k].cols) for k in ("feat", "prior_logits", "action", "sv_actor", "sv_x", "sv_gates", "sv_p")}
        keep["sv_act_stats"] = placed_input(stats, stats.shape[1])
        for k, v in keep.items():
            setattr(b, k, v.ptr)
        b.start_feat, b.eps_action = p["start_feat"].ptr, p["eps_action"].ptr
        b.dfeat, b.dentropy, b.ent_weight = p["dfeat"].ptr, self.dentropy, (ptr(p["ent_weight"]) if ent_weight else None)
        out = dict(d_actor_out=pout(M, Ao), d_actor_pre=pout(4 * M, d.Hd) if (actor_pre or chain) else None)
        b.d_actor_out, b.d_actor_pre = out["d_actor_out"].ptr, (out["d_actor_pre"].ptr if actor_pre else None)
        b.discrete_actions = int(self.discrete)
        c.check(c.lib.bd_imagine_cat_backward(C.byref(b), c.stream()))
        sync()
        if chain:       # the actor's hidden layers as the caller's dense chain over all rows (d_actor_pre = NULL form)
            m = c.MlpBwdArgs()
            m.M, m.dout, m.lddo, m.dout_scale, m.n_layers = M, out["d_actor_out"].ptr, Ao, 1.0, 5
            for l in range(4):
                m.layer[l] = c.LayerBwd(pkT[f"a{l}"].data_ptr() if l else None, keep["sv_actor"].ptr + 4 * l * M * d.Hd, d.Hd,
                                        d.Hd if l else d.Be + d.S, c.ACT_ELU, out["d_actor_pre"].ptr + 4 * l * M * d.Hd)
            m.layer[4] = c.LayerBwd(pkT["a4m" if self.discrete else "a4"].data_ptr(), None, Ao, d.Hd, c.ACT_NONE, None)
            c.check(c.lib.bd_mlp_backward(C.byref(m), c.stream()))
            sync()
        for k, v in out.items():
            assert v is None or v.outside_unchanged(), f"imagine backward: {k} written outside its rows"
        return out, stats.reshape(d.T, d.B, -1).double()

    def check_forward(self, out, AL=R.HW, exact=False, report=None, I64=None):
        """Returns the float64 views and (ambiguous, draws, draws of a class >= 128): the prior's factors and, with the
        Categorical actor, the actor's draws, counted together.  self.pair_won: how often the planted pair won (or None)."""
        d, I64 = self.d, I64 or self.I64
        K = self.tensors64(out)
        R.check_layers(RC.imagine_fwd_layers(d, self.W64, I64, K, AL, discrete=self.discrete, sat=self.sat), K, report, "imagine ")
        counts = [0, 0, 0]
        if self.discrete:           # the actor's sampled class, read from the action, against the margin on the kernel's norm
            amb, n, self.pair_won = RC.actor_checks(d, K["sv_act_stats"], I64["eps_action"], K["action"], self.sat, self.dup, "imagine ")
            counts = [amb, n, 0]
        for t in range(d.T):
            res = RC.sample_check(K["prior_logits"][t], I64["q_prior"][t], K["sidx"][t], d.D, d.C, RC.sample_path(d.C, exact),
                                  f"imagine t={t} ")
            counts = [x + y for x, y in zip(counts, res)]
        return K, counts

    def check_backward(self, Kf, bwd, stats64, AL=R.HW, report=None, ent_weight=True):
        d = self.d
        K = dict(d_actor_out=view64(bwd["d_actor_out"], d, bwd["d_actor_out"].cols))
        if bwd["d_actor_pre"] is not None:
            ap = bwd["d_actor_pre"].view.reshape(4, d.T, d.B, d.Hd).double()
            K.update({f"d_actor_pre{l}": ap[l] for l in range(4)})
        I = dict(self.I64, **{k: v for k, v in Kf.items() if v is not None})
        I["sv_act_stats"] = stats64
        G = self.G64 if ent_weight else dict(self.G64, ent_weight=None)
        R.check_layers(RC.imagine_bwd_layers(d, self.W64, I, K, G, self.dentropy, AL, actor_pre=bwd["d_actor_pre"] is not None,
                                             discrete=self.discrete, sat=self.sat), K, report, "imagine ")
        return K


def run_imagine_shape(name, AL=R.HW, exact=False, extras=False):
    d = RC.IMAGINE_SHAPES[name]
    disc = name == "discrete"
    case = ImagineCase(d, RC.SEEDS[2], bias_high=name == "c256_d2", discrete=disc)
    rep = {}
    fwd = case.forward()                                  # start_sidx NULL: zero rows and one-hot rows from start_feat
    Kf, counts = case.check_forward(fwd, AL, exact, rep)
    bwd, stats = case.backward(fwd, actor_pre=not disc)
    case.check_backward(Kf, bwd, stats, AL, rep)
    same_bits(fwd, case.forward(), f"{name} forward, second run")
    if disc:
        bwd_nw, stats_nw = case.backward(fwd, actor_pre=False, ent_weight=False)
        case.check_backward(Kf, bwd_nw, stats_nw, AL, rep, ent_weight=False)
    if extras or name == "c256_d2":
        # start_sidx given: the zero rows become the LAST class of every factor (C = 256: an index above 127); the one-hot
        # (odd) rows keep their bits
        sf = case.I["start_feat"].clone()
        sf[0::2, d.Be + d.C - 1::d.C] = 1.0
        sidx0 = sf[:, d.Be:].reshape(d.B, d.D, d.C).argmax(-1).to(torch.uint8).contiguous()
        given = case.forward(start_sidx=sidx0, start_feat=pin(sf, d.Be + d.S))
        case.check_forward(given, AL, exact, rep, dict(case.I64, start_feat=sf.double()))
        for k in ("feat", "prior_logits", "action", "sv_x", "sv_p"):
            a, b = (o[k].view.reshape(d.T, d.B, -1)[:, 1::2] for o in (fwd, given))
            assert torch.equal(a, b), f"{name}: {k} of the one-hot rows differs between start_sidx given and NULL"
        assert torch.equal(fwd["sidx"].view.reshape(d.T, d.B, d.D)[:, 1::2], given["sidx"].view.reshape(d.T, d.B, d.D)[:, 1::2])
    if extras:
        same_bits(fwd, case.forward(with_us=False), f"{name} forward without sv_act_us")
        # eps_entropy NULL (the scan alone) followed by bd_actor_entropy == the call with eps_entropy
        whole = case.forward(entropy=True)
        alone = case.forward()
        case.actor_entropy(alone)
        same_bits(whole, alone, f"{name} scan + bd_actor_entropy against the call with eps_entropy")
        assert bool(torch.isfinite(whole["entropy"].view).all())
        # ent_weight NULL; d_actor_pre NULL: the same d_actor_out; NULL followed by the caller's bd_mlp_backward
        bwd_nw, stats_nw = case.backward(fwd, actor_pre=True, ent_weight=False)
        case.check_backward(Kf, bwd_nw, stats_nw, AL, rep, ent_weight=False)
        bwd2, _ = case.backward(fwd, actor_pre=False)
        same_bits(dict(d_actor_out=bwd["d_actor_out"]), bwd2, f"{name} backward without d_actor_pre")
        bwd3, _ = case.backward(fwd, actor_pre=False, chain=True)
        case.check_backward(Kf, bwd3, stats, AL, rep)
    return rep, counts


@pytest.mark.parametrize("name", list(RC.IMAGINE_SHAPES))
def test_imagine_scan_against_float64(name):
    d = RC.IMAGINE_SHAPES[name]
    if name == "tile_loop":
        assert RC.cdiv(d.B, 16) == 257 and RC.cat_grid(d.B) == 129     # workgroups walk two tiles, the last walks one
    rep, (amb, n, high) = run_imagine_shape(name, extras=name in ("c32_d12", "c16_d20"))
    print("SCAN_CAT_RATIOS imagine", name, json.dumps(rep), f"ambiguous {amb} of {n}")
    assert rep and max(rep.values()) < 1.0, rep
    assert amb <= 1e-3 * n, (amb, n)
    if name == "c256_d2":
        assert high > n // 2


# ---- imagination with the Categorical actor at its own shapes and variants ------------------------------------------------------

def run_discrete_case(name, variant, AL=R.HW, exact=False, extras=True):
    """One case of scan_cat_ref.DISCRETE_SHAPES, as test_scan_kernels_gpu.run_discrete_case runs the Gaussian-latent ones:
    forward and backward layer by layer, the backward as the engine runs it (the scan with d_actor_pre = NULL, then
    bd_mlp_backward), ent_weight given and NULL, the draws of the actor and of the prior against their margins, the exact
    statements of the saturated rows, second runs bit for bit.  Returns (worst ratios, (ambiguous, draws), pair wins)."""
    d = RC.DISCRETE_SHAPES[name]
    case = ImagineCase(d, RC.SEEDS[2], variant=variant)
    rep = {}
    fwd = case.forward()
    Kf, (amb, n, _) = case.check_forward(fwd, AL, exact, rep)
    bwd, stats = case.backward(fwd, actor_pre=False, chain=True)
    Kb = case.check_backward(Kf, bwd, stats, AL, rep)
    assert all(f"d_actor_pre{l}" in Kb for l in range(4))
    bwd_nw, _ = case.backward(fwd, actor_pre=False, ent_weight=False)
    Kb_nw = case.check_backward(Kf, bwd_nw, stats, AL, rep, ent_weight=False)
    if case.sat is not None:
        assert R.saturated_exact(d, Kf, Kb, case.sat, f"{name} ") > 0 and R.saturated_exact(d, Kf, Kb_nw, case.sat, f"{name} ") > 0
    if d.A == 1:        # one class: norm = 0, p = 1, H = 0 and no gradient, exactly
        assert bool((Kf["sv_act_stats"] == 0).all() and (Kf["action"] == 1).all() and (Kf["entropy"].abs() == 0).all())
        assert bool((Kb["d_actor_out"] == 0).all())
    if extras:
        same_bits(fwd, case.forward(), f"{name} {variant} forward, second run")
        bwd2, _ = case.backward(fwd, actor_pre=False, chain=True)
        same_bits(bwd, bwd2, f"{name} {variant} backward and actor chain, second run")
    return rep, (amb, n), case.pair_won


@pytest.mark.parametrize("name,variant", R.discrete_cases(RC.DISCRETE_SHAPES))
def test_imagine_scan_with_the_categorical_actor_against_float64(name, variant):
    d = RC.DISCRETE_SHAPES[name]
    if name == "tile_loop_a17":
        assert RC.cdiv(d.B, 16) == 257 and RC.cat_grid(d.B) == 129     # workgroups walk two tiles, the last walks one
    rep, (amb, n), won = run_discrete_case(name, variant)
    print("SCAN_CAT_RATIOS imagine discrete", name, variant, json.dumps(rep), f"ambiguous {amb} of {n}" + (f", pair won {won}" if won is not None else ""))
    assert rep and max(rep.values()) < 1.0, rep
    assert amb <= 1e-3 * n, (amb, n)
    assert won is None or won > 0, "the planted pair never won: the case checks nothing"


# ---- the -DBD_EXACT_MATH twin, in a fresh process ------------------------------------------------------------------------

def test_exact_math_twin_against_float64():
    """c32_d12 and c16_d20, observe in every form and imagine, and the Categorical actor's cases scan_ref.DISCRETE_EXACT, on
    libbigdreamer_hip_exact.so with the libm-grade allowances and the libm sampler margin."""
    lib = os.path.join(ROOT, "big_dreamer_amd", "libbigdreamer_hip_exact.so")
    assert os.path.exists(lib), "build() makes the exact-math twin"
    env = dict(os.environ, BD_LIB=lib)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_cat_exact_worker.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("SCAN_CAT_EXACT_RESULT ")]
    assert line, res.stdout[-2000:]
    rep = json.loads(line[-1][len("SCAN_CAT_EXACT_RESULT "):])
    print("SCAN_CAT_RATIOS exact", json.dumps(rep))
    for name in ("c32_d12", "c16_d20"):
        assert set(rep["observe"][name]) == {"single", "cluster4"}
        for group in list(rep["observe"][name].values()) + [rep["imagine"][name]]:
            assert group and max(group.values()) < 1.0, rep
    assert set(rep["discrete"]) == {f"{n}:{v}" for n, v in R.DISCRETE_EXACT}
    for group in rep["discrete"].values():
        assert group and max(group.values()) < 1.0, rep
    assert rep["ambiguous"] <= 1e-3 * rep["factors"], rep
