"""GPU tests of the Gaussian RSSM scan kernels against tests/scan_ref.py: bd_observe_forward / bd_observe_backward, the
cluster calls in their K-split and round-1 forms, bd_imagine_forward_scan and bd_imagine_backward (with the tanh-Normal actor
and with the Categorical one, discrete_actions = 1), called through the C ABI, every layer of every step checked in float64 from the kernel's own tensors of the layer before.  Every launch is
followed by a synchronise (which raises on a device error) before the next one; nothing retries.  Each test prints the
worst err / bound ratio per tensor and form (run with -s to see them)."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV = ("sv_s", "sv_x", "sv_gates", "sv_q")
# (nonterm, dpost_mean, dpost_std, min_std), cycled over the shape table
VARIANTS = (("zeros", True, True, 0.1), ("none", False, False, 0.1), ("ones", True, False, 0.25), ("zeros", False, True, 0.1))


def cabi():
    from big_dreamer_amd import _cabi
    return _cabi


def sync():
    torch.cuda.synchronize()


def pin(x, w):
    """An input as [rows x w] with NaN behind its last valid row."""
    return None if x is None else placed_input(x.reshape(-1, w).float().contiguous(), w)


def pout(rows, w):
    return Placed(rows, w, w)


def ptr(p):
    return None if p is None else p.ptr


def view64(p, d, w):
    return p.view.reshape(d.T, d.B, w).double()


def same_bits(a, b, what):
    for k in a:
        if a[k] is not None and b.get(k) is not None:
            assert torch.equal(a[k].buf, b[k].buf), f"{what}: {k} differs"


# ---- observe ------------------------------------------------------------------------------------------------------------

class ObserveCase:
    def __init__(self, d, seed, nonterm="zeros", dpm=True, dps=True, min_std=0.1):
        self.d, self.min_std = d, min_std
        self.W = W = R.make_weights(d, seed, "cuda")
        self.I = I = R.make_observe_inputs(d, seed, "cuda", nonterm=nonterm)
        self.G = G = R.make_observe_grads(d, seed, "cuda", dpm=dpm, dps=dps)
        Be, S_ = d.Be, d.S
        blocks = dict(embed_s=W["W_e"][:, :S_], embed_a=W["W_e"][:, S_:], q1h=W["W_1"], q2m=W["W_2"][:S_], q2s=W["W_2"][S_:])
        for i, g in enumerate("rzn"):
            blocks["i" + g] = W["W_ih"][i * Be:(i + 1) * Be]
            blocks["h" + g] = W["W_hh"][i * Be:(i + 1) * Be]
        self.pk = {k: pack(v, False) for k, v in blocks.items()}
        self.pkT = {k: pack(v, True) for k, v in blocks.items() if k != "embed_a"}
        self.pin = dict(init_belief=pin(I["init_belief"], Be), init_state=pin(I["init_state"], S_), actions=pin(I["actions"], d.A),
                        nonterm=pin(I["nonterm"], 1), pre_emb=pin(I["pre_emb"], d.Hd), eps_post=pin(I["eps_post"], S_),
                        dfeat=pin(G["dfeat"], Be + S_), dpost_mean=pin(G["dpost_mean"], S_), dpost_std=pin(G["dpost_std"], S_))
        self.W64, self.I64, self.G64 = R.to64(W), R.to64(I), R.to64(G)
        sync()

    def workspace(self):
        lib = cabi().lib
        return torch.zeros(max(1, int(lib.bd_observe_cluster_ws_floats(self.d.B, self.d.Be))), device="cuda")

    def _launch(self, form, single, cluster, args, ws):
        c = cabi()
        if form == "single":
            c.check(single(C.byref(args), c.stream()))
            sync()
            return
        assert c.lib.bd_observe_cluster_set_ksplit(0 if form == "round1" else -1) == 0
        try:
            c.check(cluster(C.byref(args), ws.data_ptr(), ws.numel(), c.stream()))
            sync()
            c.check(c.lib.bd_observe_cluster_status(ws.data_ptr(), self.d.B, c.stream()))
        finally:
            c.lib.bd_observe_cluster_set_ksplit(-1)

    def forward(self, form, ws=None, save=SV):
        c, d, pk, p = cabi(), self.d, self.pk, self.pin
        a = c.ObserveFwdArgs()
        a.T, a.B, a.Be, a.S, a.A, a.Hd = d
        a.w_embed_s, a.w_embed_a, a.b_embed = pk["embed_s"].data_ptr(), pk["embed_a"].data_ptr(), self.W["b_e"].data_ptr()
        a.w_ir, a.w_iz, a.w_in = (pk[k].data_ptr() for k in ("ir", "iz", "in"))
        a.w_hr, a.w_hz, a.w_hn = (pk[k].data_ptr() for k in ("hr", "hz", "hn"))
        a.b_ih, a.b_hh = self.W["b_ih"].data_ptr(), self.W["b_hh"].data_ptr()
        a.w_q1h, a.b_q1 = pk["q1h"].data_ptr(), self.W["b_1"].data_ptr()
        a.w_q2m, a.w_q2s, a.b_q2 = pk["q2m"].data_ptr(), pk["q2s"].data_ptr(), self.W["b_2"].data_ptr()
        for k in ("init_belief", "init_state", "actions", "nonterm", "pre_emb", "eps_post"):
            setattr(a, k, ptr(p[k]))
        a.min_std = self.min_std
        M = d.T * d.B
        out = {k: (pout(M, w(d)) if (k in save or not k.startswith("sv_")) else None) for k, w in R.OBS_FWD_TENSORS.items()}
        for k, v in out.items():
            setattr(a, k, ptr(v))
        self._launch(form, c.lib.bd_observe_forward, c.lib.bd_observe_forward_cluster, a, ws)
        for k, v in out.items():
            assert v is None or v.outside_unchanged(), f"{form}: {k} written outside its rows"
        return out

    def backward(self, form, fwd, ws=None):
        c, d, pkT, p = cabi(), self.d, self.pkT, self.pin
        b = c.ObserveBwdArgs()
        b.T, b.B, b.Be, b.S, b.A, b.Hd = d
        b.wt_embed_s = pkT["embed_s"].data_ptr()
        b.wt_ir, b.wt_iz, b.wt_in = (pkT[k].data_ptr() for k in ("ir", "iz", "in"))
        b.wt_hr, b.wt_hz, b.wt_hn = (pkT[k].data_ptr() for k in ("hr", "hz", "hn"))
        b.wt_q1h, b.wt_q2m, b.wt_q2s = pkT["q1h"].data_ptr(), pkT["q2m"].data_ptr(), pkT["q2s"].data_ptr()
        keep = {k: placed_input(fwd[k].view.clone(), fwd[k].cols) for k in ("feat", "post_std", "sv_x", "sv_gates", "sv_q")}
        for k, v in keep.items():
            setattr(b, k, v.ptr)
        for k in ("init_belief", "nonterm", "eps_post", "dfeat", "dpost_mean", "dpost_std"):
            setattr(b, k, ptr(p[k]))
        b.min_std = self.min_std
        out = {k: pout(d.T * d.B, w(d)) for k, w in R.OBS_BWD_TENSORS.items()}
        for k, v in out.items():
            setattr(b, k, v.ptr)
        self._launch(form, c.lib.bd_observe_backward, c.lib.bd_observe_backward_cluster, b, ws)
        for k, v in out.items():
            assert v.outside_unchanged(), f"{form}: {k} written outside its rows"
        return out

    def check(self, form, fwd, bwd, AL=R.HW, report=None):
        d = self.d
        Kf = {k: view64(v, d, v.cols) for k, v in fwd.items()}
        R.check_layers(R.observe_fwd_layers(d, self.W64, self.I64, Kf, self.min_std, AL), Kf, report, f"{form} ")
        Kb = {k: view64(v, d, v.cols) for k, v in bwd.items()}
        I = dict(self.I64, **{k: Kf[k] for k in ("feat", "post_std", "sv_x", "sv_gates", "sv_q")})
        R.check_layers(R.observe_bwd_layers(d, self.W64, I, Kb, self.G64, self.min_std, AL), Kb, report, f"{form} ")


def run_observe_shape(name, AL=R.HW, repeats=True):
    """Every form that accepts the shape, against the same reference; returns {form: {tensor: worst err / bound}}."""
    d, _C, _form = R.OBSERVE_SHAPES[name]
    nonterm, dpm, dps, ms = VARIANTS[list(R.OBSERVE_SHAPES).index(name) % len(VARIANTS)]
    case = ObserveCase(d, 11, nonterm, dpm, dps, ms)
    reports = {}
    for form in R.observe_forms(d.B, d.Be, d.S, d.A, d.Hd):
        ws = case.workspace() if form != "single" else None
        fwd = case.forward(form, ws)
        bwd = case.backward(form, fwd, ws)
        reports[form] = {}
        case.check(form, fwd, bwd, AL, reports[form])
        if repeats:
            fwd2 = case.forward(form, ws)                 # the same bits twice in a row (reused workspace) ...
            same_bits(fwd, fwd2, f"{name} {form} forward, second run")
            bwd2 = case.backward(form, fwd, ws)
            same_bits(bwd, bwd2, f"{name} {form} backward, second run")
            if ws is not None:                            # ... and with a fresh zeroed workspace
                same_bits(fwd, case.forward(form, case.workspace()), f"{name} {form} forward, fresh workspace")
                same_bits(bwd, case.backward(form, fwd, case.workspace()), f"{name} {form} backward, fresh workspace")
    return reports


@pytest.mark.parametrize("name", list(R.OBSERVE_SHAPES))
def test_observe_forms_against_float64(name):
    reports = run_observe_shape(name)
    print("SCAN_RATIOS observe", name, json.dumps(reports))
    for form, rep in reports.items():
        assert rep and max(rep.values()) < 1.0, (form, rep)


@pytest.mark.parametrize("name", ["b17_T7", "ragged42", "configs1", "s64"])
def test_observe_inference_and_partial_saves_are_bit_identical(name):
    """Every sv_* NULL (inference), and each sv_* pointer NULL on its own: the outputs and the remaining saves keep
    their bits, in every form."""
    d = R.OBSERVE_SHAPES[name][0]
    case = ObserveCase(d, 12)
    for form in R.observe_forms(d.B, d.Be, d.S, d.A, d.Hd):
        ws = case.workspace() if form != "single" else None
        full = case.forward(form, ws)
        same_bits(full, case.forward(form, ws, save=()), f"{name} {form} inference")
        for drop in SV:
            same_bits(full, case.forward(form, ws, save=tuple(k for k in SV if k != drop)), f"{name} {form} without {drop}")


# ---- imagination --------------------------------------------------------------------------------------------------------

class ImagineCase:
    """discrete: the Categorical actor (discrete_actions = 1) in one of its variants (scan_ref.make_discrete_case):
    w_a4s and sv_act_us NULL, sv_act_stats A wide, the entropy written by the scan, the backward with d_actor_pre = NULL."""

    def __init__(self, d, seed, ent_weight=True, min_std=0.1, dentropy=-0.37, discrete=False, variant="regular"):
        self.d, self.min_std, self.dentropy, self.discrete, self.sat, self.dup = d, min_std, dentropy, discrete, None, None
        if discrete:
            self.W, self.I, self.sat, self.dup = R.make_discrete_case(d, seed, variant, "cuda")
        else:
            self.W, self.I = R.make_weights(d, seed, "cuda", imagine=True), R.make_imagine_inputs(d, seed, "cuda")
        W, I = self.W, self.I
        self.G = G = R.make_imagine_grads(d, seed, "cuda", ent_weight=ent_weight)
        Be, S_, A = d.Be, d.S, d.A
        blocks = dict(embed_s=W["W_e"][:, :S_], embed_a=W["W_e"][:, S_:], p1=W["W_1"], p2m=W["W_2"][:S_], p2s=W["W_2"][S_:],
                      a0h=W["W_a0"][:, :Be], a0s=W["W_a0"][:, Be:], a1=W["W_a"][0], a2=W["W_a"][1], a3=W["W_a"][2],
                      a4m=W["W_a4"][:A], a4s=W["W_a4"][A:], a4=W["W_a4"])
        for i, g in enumerate("rzn"):
            blocks["i" + g] = W["W_ih"][i * Be:(i + 1) * Be]
            blocks["h" + g] = W["W_hh"][i * Be:(i + 1) * Be]
        self.pk = {k: pack(v, False) for k, v in blocks.items()}
        self.pkT = {k: pack(v, True) for k, v in blocks.items()}
        self.pin = dict(start_feat=pin(I["start_feat"], Be + S_), eps_action=pin(I["eps_action"], A), eps_prior=pin(I["eps_prior"], S_),
                        dfeat=pin(G["dfeat"], Be + S_), ent_weight=pin(G["ent_weight"], 1))
        self.W64, self.I64, self.G64 = R.to64(W), R.to64(I), R.to64(G)
        sync()

    def widths(self):
        d = self.d
        if self.discrete:
            return dict(feat=d.Be + d.S, prior_mean=d.S, prior_std=d.S, action=d.A, sv_act_stats=d.A, sv_x=d.Be, sv_gates=4 * d.Be,
                        sv_p=d.Hd, entropy=1)
        return dict(feat=d.Be + d.S, prior_mean=d.S, prior_std=d.S, action=d.A, sv_act_stats=4 * d.A, sv_x=d.Be, sv_gates=4 * d.Be,
                    sv_p=d.Hd, sv_act_us=2 * d.A, entropy=1)

    def forward(self, with_us=True, with_mean=True, split=0, eps_entropy=None, n_samples=1, stats=True, wrapper=False):
        """One launch, or two time segments [0, split) and [split, Hm) through sv_actor_stride.  eps_entropy (a Placed
        [Hm * n_samples * N x A]) with stats = False: the in-scan entropy estimate; with wrapper = True:
        bd_imagine_forward, which follows the scan with bd_actor_entropy (test_entropy_kernels_gpu.py)."""
        c, d, pk, p = cabi(), self.d, self.pk, self.pin
        M = d.T * d.B
        out = {k: pout(M, w) for k, w in self.widths().items()}
        out["sv_actor"] = pout(4 * M, d.Hd)
        if not with_us and not self.discrete:
            out["sv_act_us"] = None
        if not with_mean:
            out["prior_mean"] = None
        if not stats:
            out["sv_act_stats"] = None
        for t0, t1 in (((0, split), (split, d.T)) if split else ((0, d.T),)):
            a = c.ImagineFwdArgs()
            a.N, a.Hm, a.Be, a.S, a.A, a.Hd, a.n_samples = d.B, t1 - t0, d.Be, d.S, d.A, d.Hd, n_samples
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
            a.w_a4m, a.w_a4s, a.b_a4 = pk["a4m"].data_ptr(), (None if self.discrete else pk["a4s"].data_ptr()), self.W["b_a4"].data_ptr()
            shift = lambda pl, w: None if pl is None else pl.ptr + 4 * t0 * d.B * w
            a.start_feat = p["start_feat"].ptr if t0 == 0 else shift(out["feat"], d.Be + d.S) - 4 * d.B * (d.Be + d.S)
            a.eps_action, a.eps_prior = shift(p["eps_action"], d.A), shift(p["eps_prior"], d.S)
            a.eps_entropy = shift(eps_entropy, n_samples * d.A)
            a.min_std, a.act_raw_init_std, a.act_min_std, a.act_mean_scale = self.min_std, R.ACT_RAW_INIT_STD, R.ACT_MIN_STD, R.ACT_MEAN_SCALE
            for k, w in self.widths().items():
                setattr(a, k, shift(out[k], w))
            a.sv_actor, a.sv_actor_stride = shift(out["sv_actor"], d.Hd), M * d.Hd
            a.discrete_actions = int(self.discrete)
            c.check((c.lib.bd_imagine_forward if wrapper else c.lib.bd_imagine_forward_scan)(C.byref(a), c.stream()))
            sync()
        for k, v in out.items():
            assert v is None or v.outside_unchanged(), f"imagine forward: {k} written outside its rows"
        if stats and not self.discrete and not (wrapper and eps_entropy is not None):
            assert bool((out["entropy"].buf == SENTINEL).all()), "the scan wrote an entropy although sv_act_stats was given"
        return out

    def tensors64(self, out):
        d = self.d
        skip = ("sv_actor",) if self.discrete else ("sv_actor", "entropy")
        K = {k: (view64(v, d, v.cols) if v is not None else None) for k, v in out.items() if k not in skip}
        sa = out["sv_actor"].view.reshape(4, d.T, d.B, d.Hd).double()
        K.update({f"sv_actor{l}": sa[l] for l in range(4)})
        return K

    def backward(self, fwd, actor_pre=True, chain=False, ent_weight=True):
        """chain: the scan with d_actor_pre = NULL followed by the caller's bd_mlp_backward over all rows, bound as the engine
        binds it (the Categorical actor: lddo = A and the transposed pack of W_a4's A logit rows as the last layer)."""
        c, d, pkT, p = cabi(), self.d, self.pkT, self.pin
        M, A = d.T * d.B, d.A
        Ao = A if self.discrete else 2 * A
        b = c.ImagineBwdArgs()
        b.N, b.Hm, b.Be, b.S, b.A, b.Hd = d.B, d.T, d.Be, d.S, d.A, d.Hd
        b.wt_embed_s, b.wt_embed_a = pkT["embed_s"].data_ptr(), pkT["embed_a"].data_ptr()
        b.wt_ir, b.wt_iz, b.wt_in = (pkT[k].data_ptr() for k in ("ir", "iz", "in"))
        b.wt_hr, b.wt_hz, b.wt_hn = (pkT[k].data_ptr() for k in ("hr", "hz", "hn"))
        b.wt_p1, b.wt_p2m, b.wt_p2s = pkT["p1"].data_ptr(), pkT["p2m"].data_ptr(), pkT["p2s"].data_ptr()
        for l in range(3):
            b.wt_a[l] = pkT[f"a{l + 1}"].data_ptr()
        b.wt_a4m, b.wt_a4s = pkT["a4m"].data_ptr(), (None if self.discrete else pkT["a4s"].data_ptr())
        stats = fwd["sv_act_stats"].view.clone()
        if not self.discrete:
            stats[:, 2 * A:3 * A], stats[:, 3 * A:] = self.G["slot2"].reshape(M, A), self.G["slot3"].reshape(M, A)
        keep = {k: placed_input(fwd[k].view.clone(), fwd[k].cols) for k in ("feat", "prior_std", "action", "sv_actor", "sv_x", "sv_gates", "sv_p")}
        keep["sv_act_stats"] = placed_input(stats, stats.shape[1])
        for k, v in keep.items():
            setattr(b, k, v.ptr)
        b.start_feat, b.eps_action, b.eps_prior = p["start_feat"].ptr, p["eps_action"].ptr, p["eps_prior"].ptr
        b.min_std, b.dfeat, b.dentropy = self.min_std, p["dfeat"].ptr, self.dentropy
        b.ent_weight = ptr(p["ent_weight"]) if ent_weight else None
        out = dict(d_actor_out=pout(M, Ao), d_actor_pre=pout(4 * M, d.Hd) if (actor_pre or chain) else None)
        b.d_actor_out, b.d_actor_pre = out["d_actor_out"].ptr, (out["d_actor_pre"].ptr if actor_pre else None)
        b.discrete_actions = int(self.discrete)
        c.check(c.lib.bd_imagine_backward(C.byref(b), c.stream()))
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
        stats64 = stats.reshape(d.T, d.B, -1).double()
        return out, stats64

    def check_forward(self, out, AL=R.HW, report=None):
        K = self.tensors64(out)
        R.check_layers(R.imagine_fwd_layers(self.d, self.W64, self.I64, K, self.min_std, AL, discrete=self.discrete, sat=self.sat),
                       K, report, "imagine ")
        return K

    def check_actor(self, K):
        """The Categorical actor's sampled classes against the margin on the kernel's own norm (and the planted pair):
        (ambiguous draws, draws, times the pair won or None)."""
        return RC.actor_checks(self.d, K["sv_act_stats"], self.I64["eps_action"], K["action"], self.sat, self.dup, "imagine ")

    def check_backward(self, Kf, bwd, stats64, AL=R.HW, report=None, ent_weight=True):
        d = self.d
        K = dict(d_actor_out=view64(bwd["d_actor_out"], d, bwd["d_actor_out"].cols))
        if bwd["d_actor_pre"] is not None:
            ap = bwd["d_actor_pre"].view.reshape(4, d.T, d.B, d.Hd).double()
            K.update({f"d_actor_pre{l}": ap[l] for l in range(4)})
        I = dict(self.I64, **{k: v for k, v in Kf.items() if v is not None})
        I["sv_act_stats"] = stats64
        G = self.G64 if ent_weight else dict(self.G64, ent_weight=None)
        R.check_layers(R.imagine_bwd_layers(d, self.W64, I, K, G, self.dentropy, self.min_std, AL, actor_pre=bwd["d_actor_pre"] is not None,
                                            discrete=self.discrete, sat=self.sat), K, report, "imagine ")
        return K


def run_imagine_shape(name, AL=R.HW, ent_weight=True, extras=True):
    d = R.IMAGINE_SHAPES[name]
    case = ImagineCase(d, 21, ent_weight=ent_weight)
    rep = {}
    fwd = case.forward()
    Kf = case.check_forward(fwd, AL, rep)
    bwd, stats = case.backward(fwd, actor_pre=True)
    case.check_backward(Kf, bwd, stats, AL, rep)
    if extras:
        same_bits(fwd, case.forward(), f"{name} forward, second run")
        bare = case.forward(with_us=False, with_mean=False)             # sv_act_us and prior_mean NULL
        same_bits(fwd, bare, f"{name} forward without sv_act_us / prior_mean")
        case.check_forward(bare, AL)
        if d.T >= 2:
            same_bits(fwd, case.forward(split=d.T // 2), f"{name} forward in two time segments")
        bwd2, _ = case.backward(fwd, actor_pre=False)                   # d_actor_pre NULL: the same d_actor_out
        same_bits(dict(d_actor_out=bwd["d_actor_out"]), bwd2, f"{name} backward without d_actor_pre")
        bwd3, _ = case.backward(fwd, actor_pre=False, chain=True)       # ... followed by the caller's bd_mlp_backward
        case.check_backward(Kf, bwd3, stats, AL, rep)
    return rep


@pytest.mark.parametrize("name", list(R.IMAGINE_SHAPES))
def test_imagine_scan_against_float64(name):
    for ew in (True, False):
        rep = run_imagine_shape(name, ent_weight=ew, extras=ew)
        print("SCAN_RATIOS imagine", name, "ent_weight" if ew else "no_ent_weight", json.dumps(rep))
        assert rep and max(rep.values()) < 1.0, rep


# ---- imagination with the Categorical actor (discrete_actions = 1) -------------------------------------------------------------

def run_discrete_case(name, variant, AL=R.HW, extras=True):
    """One case of scan_ref.DISCRETE_SHAPES: forward and backward layer by layer, the backward as the engine runs it (the scan
    with d_actor_pre = NULL, then bd_mlp_backward: d_actor_pre0..3 against the float64 chain), ent_weight given and NULL,
    the actor's draws against the margin, the exact statements of the saturated rows; with extras the second runs and the
    forward in two time segments, bit for bit.  Returns (worst err / bound per tensor, (ambiguous, draws, pair wins))."""
    d = R.DISCRETE_SHAPES[name]
    case = ImagineCase(d, R.SEEDS[2], discrete=True, variant=variant)
    rep = {}
    fwd = case.forward()
    Kf = case.check_forward(fwd, AL, rep)
    counts = case.check_actor(Kf)
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
        if d.T >= 2:        # the chunked behaviour chain: two time segments through sv_actor_stride
            same_bits(fwd, case.forward(split=d.T // 2), f"{name} {variant} forward in two time segments")
    return rep, counts


@pytest.mark.parametrize("name,variant", R.discrete_cases(R.DISCRETE_SHAPES))
def test_imagine_scan_with_the_categorical_actor_against_float64(name, variant):
    rep, (amb, n, won) = run_discrete_case(name, variant)
    print("SCAN_RATIOS imagine discrete", name, variant, json.dumps(rep), f"ambiguous {amb} of {n}" + (f", pair won {won}" if won is not None else ""))
    assert rep and max(rep.values()) < 1.0, rep
    assert amb <= 1e-3 * n, (amb, n)
    assert won is None or won > 0, "the planted pair never won: the case checks nothing"


# ---- the -DBD_EXACT_MATH twin, in a fresh process ------------------------------------------------------------------------

def test_exact_math_twin_against_float64():
    """One observe case per form, one imagine case and the two cases of scan_ref.DISCRETE_EXACT (the Categorical actor) on
    libbigdreamer_hip_exact.so with the libm-grade allowances."""
    lib = os.path.join(ROOT, "big_dreamer_amd", "libbigdreamer_hip_exact.so")
    assert os.path.exists(lib), "build() makes the exact-math twin"
    env = dict(os.environ, BD_LIB=lib)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "scan_exact_worker.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("SCAN_EXACT_RESULT ")]
    assert line, res.stdout[-2000:]
    rep = json.loads(line[-1][len("SCAN_EXACT_RESULT "):])
    print("SCAN_RATIOS exact", json.dumps(rep))
    assert set(rep["observe"]) == {"single", "ksplit", "round1"}
    assert set(rep["discrete"]) == {f"{n}:{v}" for n, v in R.DISCRETE_EXACT}
    for group in list(rep["observe"].values()) + [rep["imagine"]] + list(rep["discrete"].values()):
        assert group and max(group.values()) < 1.0, rep
    assert rep["ambiguous"] <= 1e-3 * rep["draws"], rep
