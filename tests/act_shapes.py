"""The shape table of the acting-step tests (tests/test_act_shapes_cpu.py, tests/test_act_shapes_gpu.py): one row per
branch of csrc/act.hip and of the bd_device.h / bd_categorical.h helpers it calls that the one-point tests
(tests/test_act_step_gpu.py, tests/test_act_step_cat_gpu.py, tests/test_act_mode_gpu.py: Be = 24, Hd = 20, E = 40, O = 5)
do not select.  Dims are dataclasses.replace of synth.TINY / synth.CAT_TINY, parameters synth.make_params(d, PARAM_SEED),
data act_cat_ref.make_data(d, seed); the float64 reference of every row is act_cat_ref.act_step_cat, which with Gaussian
latents and the tanh-Normal actor is act_ref.act_step (the CPU test pins that).

A data seed is CHOSEN on the CPU (tests/test_act_shapes_cpu.py asserts it): every Categorical sampler call of the row is
decided by more than the row's derived gap, and every width's last input column moves an output.

Launches above 64 KiB of LDS (allow_big_lds, set per instantiation act_step_kernel<LC, AC, EV>): before this table only
<Gaussian, tanh-Normal, sampling> had one (tests/test_act_step_gpu.py::test_act_step_matches_the_reference, CONFIG2).  The
seven others -- <Gaussian, Categorical>, <Categorical, tanh-Normal>, <Categorical, Categorical> sampling, and all four
evaluation instantiations -- get theirs from the four big_* rows (Be = Hd = 200, E = 1024, embedding form, B = 3), which
tests/test_act_shapes_gpu.py runs both as the sampling step and with an evaluation policy."""
import contextlib
import dataclasses
from collections import namedtuple

import numpy as np

from big_dreamer_amd import synth
from tests import act_cat_ref as R
from tests import act_ref

PARAM_SEED = R.PARAM_SEED
TOL = 2e-5                  # the project's fp32 forward tolerance, abs + rel (bd_device.h, tests/test_act_step_gpu.TOL)
EMB_ROWS = 17               # rows of the embedding form; the obs form has act_cat_ref.ROWS = 33
BIG_B = 3                   # rows of the big-LDS rows (embedding form only)
WIDTHS = ("Be", "S", "A", "Hd", "E", "O")

# dims, data seed, the branch the row selects, big = launched above 64 KiB (embedding form, B = 3 on the GPU)
Row = namedtuple("Row", "dims seed branch big", defaults=(False,))


def _gauss(Be, S, A, Hd, E, O, disc=False):
    return dataclasses.replace(synth.TINY, Be=Be, S=S, A=A, Hd=Hd, E=E, O=O, discrete_actions=disc)


def _cat(D, C, A=2, disc=False, Be=24, Hd=20, E=40, O=5):
    return dataclasses.replace(synth.CAT_TINY, Be=Be, S=D * C, A=A, Hd=Hd, E=E, O=O, cat_D=D, cat_C=C, discrete_actions=disc)


ROWS = {
    # ---- Gaussian latents, tanh-Normal actor: act_step_kernel<0, 0, *> -------------------------------------------------
    "mult16": Row(_gauss(32, 16, 16, 32, 48, 16), 0,
                  "every width a multiple of 16: `col0 + r < width` / `col < a.A` never cut a block, no zero-filled tail"),
    "plus1": Row(_gauss(33, 17, 17, 33, 49, 17), 0,
                 "every width one past a multiple of 16: the last block of every layer holds one valid column"),
    "head32": Row(_gauss(24, 32, 32, 20, 40, 5), 0,
                  "S = A = 32: Nb = 2 = kSplitPairs, the widest head still in tile_dual_head_elem's split-K form"),
    "head33": Row(_gauss(24, 33, 33, 20, 40, 5), 0,
                  "S = A = 33: Nb = 3 > kSplitPairs, both dual heads leave the split-K form (scratch = nullptr)"),
    "head64": Row(_gauss(24, 64, 64, 20, 40, 5), 0,
                  "S = A = 64 = kHeadMaxN: the plain [2][16][64] area behind the partials is full"),
    "hd_gt_be": Row(_gauss(24, 6, 2, 80, 40, 5), 0, "Kb_g = Kb_hd (Hd > Be): t0 / t1 / t2 sized by the hidden width"),
    "be_gt_hd": Row(_gauss(80, 6, 2, 20, 40, 5), 0, "Kb_g = Kb_h (Be > Hd): t0 / t1 / t2 sized by the belief width"),
    "o_gt_e": Row(_gauss(24, 6, 2, 20, 24, 70), 0, "Kb_io = Kb_o (O > E): the ef region sized by the observation"),
    "ones": Row(_gauss(24, 1, 1, 20, 40, 1), 0, "S = A = O = 1: one valid column in the only block of state, action, obs"),
    # ---- Gaussian latents, Categorical actor: act_step_kernel<0, 1, *> -------------------------------------------------
    "disc1": Row(_gauss(24, 6, 1, 20, 40, 5, True), 0, "A = 1: one class, one valid lane in disc_norm / disc_sample"),
    "disc33": Row(_gauss(24, 6, 33, 20, 40, 5, True), 0,
                  "A = 33: Nb = 3 > kSplitPairs, the actor logits leave tile_linear_seg's split-K form"),
    "disc64": Row(_gauss(24, 6, 64, 20, 40, 5, True), 0, "A = 64 = kHeadMaxN: every lane of the row's wave holds a class"),
    "gru13_disc": Row(_gauss(200, 30, 6, 32, 40, 5, True), 1,
                      "Be = 200: gru_tile's Nb == 13 form (scratch partials) in <0, 1, *>"),
    # ---- Categorical latents: act_step_kernel<1, *, *> ------------------------------------------------------------------
    "gru13_cat": Row(_cat(4, 32, 6, True, Be=200, Hd=32), 3, "Be = 200: gru_tile's Nb == 13 form in <1, 1, *>"),
    "c32_d3": Row(_cat(3, 32), 6, "C = 32, S = 96: cat_sample_reg<32> with three factors, image ld = 104"),
    "c9_d7": Row(_cat(7, 9, 3, True, Be=40, Hd=32), 3,
                 "7 x 9, S = 63: cat_sample_any, S no multiple of 16 (one dead image column), Categorical actor"),
    "c16_d16": Row(_cat(16, 16, 2, Be=32, Hd=24), 1, "S = 256: the last width CatGeo keeps in one chunk"),
    "c16_d17": Row(_cat(17, 16, 1, Be=48, Hd=16), 1, "S = 272 > 256: CatGeo in two chunks (nF = 16), the second 16 columns wide"),
    "c16_d20": Row(_cat(20, 16, 3, True), 1, "S = 320: two chunks, Categorical actor"),
    "c64_d16": Row(_cat(16, 64, 2, Be=32, Hd=24), 0, "C = 64, S = 1024: cat_sample_any over four chunks of four factors"),
    "c256_d2": Row(_cat(2, 256, 2), 17, "C = 256: one factor per chunk, the widest class count"),
    "c2_d136": Row(_cat(136, 2, 3, Be=40), 2, "136 x 2, S = 272: the `256 % C == 0 && S % 16 == 0` branch of CatGeo::ok"),
    "c1_d16": Row(_cat(16, 1, 2), 0, "C = 1: every factor has its one class; the rotation `f % C` is 0"),
    # ---- above 64 KiB: Be = Hd = 200, E = 1024, embedding form, B = 3 ------------------------------------------------------
    "big_gauss_tanh": Row(_gauss(200, 30, 2, 200, 1024, 5), 0, "allow_big_lds of <0, 0, EV> (sampling: CONFIG2's)", True),
    "big_gauss_disc": Row(_gauss(200, 30, 6, 200, 1024, 5, True), 0, "allow_big_lds of <0, 1, *>", True),
    "big_cat_tanh": Row(_cat(64, 2, 2, Be=200, Hd=200, E=1024), 0, "allow_big_lds of <1, 0, *>", True),
    "big_cat_disc": Row(_cat(32, 4, 6, True, Be=200, Hd=200, E=1024), 3, "allow_big_lds of <1, 1, *>", True),
}

# Rows of a form: the reference of a form is computed on all of them, and a B-row run is held to its first B rows (a
# decision's rows do not depend on each other).  The big rows keep BIG_B rows in both forms; the GPU runs their embedding
# form only (what they are for, the launch above 64 KiB, does not depend on the form: E = 1024 alone fills 64 KiB).
EDGE_B = ("mult16", "plus1", "ones", "c9_d7", "disc33")      # rows that also run B = 1 and 16


def form_rows(name, form):
    return BIG_B if ROWS[name].big else (R.ROWS if form == "obs" else EMB_ROWS)


def obs_B(name):
    """Row counts of the observation form on the GPU."""
    if ROWS[name].big:
        return ()
    return (1, 16, 17, 33) if name in EDGE_B else (17, 33)


# rows run with an evaluation policy (action_mode "mean" / "mode", state_mean) and rows run on in-kernel noise
EVAL_ROWS = ("head33", "head64", "ones", "gru13_disc", "c9_d7", "c16_d17") + tuple(k for k, r in ROWS.items() if r.big)
NOISE_ROWS = ("plus1", "head33", "disc33", "c9_d7")


def eval_runs(name):
    """(B, form) of the evaluation runs of a row."""
    return ((BIG_B, "emb"),) if ROWS[name].big else ((EMB_ROWS, "obs"), (EMB_ROWS, "emb"))


def sharp_form(name):
    """The form whose chain shows that a tail column matters: the one the GPU runs at the most rows."""
    return "emb" if ROWS[name].big else "obs"


def exempt(name, width):
    """Widths whose last column CANNOT move an output of the row, whatever the data, with the reason; None otherwise."""
    r = ROWS[name]
    if r.big and width == "O":
        return "the GPU runs the embedding form only: the encoder, the one reader of the observation, is not evaluated"
    if r.dims.cat_C == 1 and width in ("E", "O"):
        return "C = 1: embedding and observation reach the outputs through the posterior logits alone, and one class always wins"
    return None


_made = {}


def inputs(name):
    """(dims, parameters, data) of a row, made once per process and never written to."""
    if name not in _made:
        r = ROWS[name]
        _made[name] = (r.dims, synth.make_params(r.dims, PARAM_SEED), R.make_data(r.dims, r.seed))
    return _made[name]


_chains = {}


def chain(name, form, explore, P=None, data=None):
    """The float64 chain of three decisions on all rows of the form (form_rows), computed once per (row, form, explore);
    with other parameters or data: computed afresh."""
    d, P0, data0 = inputs(name)
    n = form_rows(name, form)
    if P is not None or data is not None:
        return R.chain(P or P0, d, data or data0, n, explore, form)
    key = (name, form, explore)
    if key not in _chains:
        _chains[key] = R.chain(P0, d, data0, n, explore, form)
    return _chains[key]


def first_rows(ch, B):
    """The first B rows of a chain (arrays of `info` included)."""
    cut = lambda v: v[:B] if isinstance(v, np.ndarray) else v
    return [(b[:B], s[:B], a[:B], {k: cut(v) for k, v in info.items()}) for b, s, a, info in ch]


@contextlib.contextmanager
def float32_restatement():
    """act_ref / act_cat_ref cast every operand with `_f64`; under this context they cast to float32, and numpy evaluates
    every product, sum and activation of the restatement in float32."""
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    saved = act_ref._f64, R._f64
    act_ref._f64 = R._f64 = f32
    try:
        yield
    finally:
        act_ref._f64, R._f64 = saved


# ---- the logit error the forward tolerance allows, and the gap a row must show ------------------------------------------------
def _layer_bound(W, b, x):
    """A linear layer on activations held to TOL (abs + rel, |x| <= 1 after ELU / one-hot / tanh cells up to the relative
    part, which sum|a*b| carries): TOL * max_j sum_k |W_jk| for the operand's error, plus 2^-23 * max sum_k |x_k W_jk|
    (+ |b_j|) for the fp32 accumulation of the layer itself."""
    W, x = np.abs(np.asarray(W, np.float64)), np.abs(np.asarray(x, np.float64))
    return TOL * float(W.sum(1).max()) + 2.0 ** -23 * float((x @ W.T + np.abs(np.asarray(b, np.float64))).max())


def actor_hidden(P, x):
    """The operand of the actor's output layer: four (Linear + ELU) on [h'; s'], float64."""
    for l in range(4):
        x = act_ref._elu(x @ act_ref._f64(P["actor"][f"model.{2 * l}.weight"]).T + act_ref._f64(P["actor"][f"model.{2 * l}.bias"]))
    return x


def logit_bound(P, d, info):
    """Largest logit error of the decision's Categorical samplers that a kernel within the forward tolerance can show."""
    bound = 0.0
    if d.categorical:
        tm = P["transition_model"]
        bound = _layer_bound(tm["belief_posterior.model.2.weight"], tm["belief_posterior.model.2.bias"], info["post_hidden"])
    if d.discrete_actions:
        bound = max(bound, _layer_bound(P["actor"]["model.8.weight"], P["actor"]["model.8.bias"],
                                        actor_hidden(P, info["actor_in"])))
    return bound


def required_gap(bound):
    """A relative gap g of two ratios is a difference g of two logits, each off by at most `bound`."""
    return max(R.MIN_GAP, 2.0 * bound)


def samplers(d):
    return d.categorical or d.discrete_actions


# ---- the tail columns ---------------------------------------------------------------------------------------------------------
def drop_last_column(P, d, width):
    """A copy of P in which every weight that reads the LAST input column of the given width is zero: what a kernel
    computes that drops the ragged tail of that width."""
    Q = {m: dict(sd) for m, sd in P.items()}

    def zero(mod, key, col):
        w = Q[mod][key].copy()
        w[:, col] = 0.0
        Q[mod][key] = w

    tm, hidden = "transition_model", [f"model.{2 * l}.weight" for l in range(1, 5)]
    if width == "Be":
        zero(tm, "rnn.weight_ih", d.Be - 1)
        zero(tm, "rnn.weight_hh", d.Be - 1)
        zero(tm, "belief_posterior.model.0.weight", d.Be - 1)
        zero("actor", "model.0.weight", d.Be - 1)
    elif width == "S":
        zero(tm, "fc_embed_state_action.0.weight", d.S - 1)
        zero("actor", "model.0.weight", d.Be + d.S - 1)
    elif width == "A":
        zero(tm, "fc_embed_state_action.0.weight", d.S + d.A - 1)
    elif width == "Hd":
        for key in hidden:
            zero("encoder", key, d.Hd - 1)
            zero("actor", key, d.Hd - 1)
        zero(tm, "belief_posterior.model.2.weight", d.Hd - 1)
    elif width == "E":
        zero(tm, "belief_posterior.model.0.weight", d.Be + d.E - 1)
    elif width == "O":
        zero("encoder", "model.0.weight", d.O - 1)
    else:
        raise ValueError(width)
    return Q


def moved(d, got, want):
    """(largest |got - want| / (TOL + TOL |want|) over belief', Gaussian state', tanh-Normal action' of the chains; whether
    a sampled class differs)."""
    ratio, flipped = 0.0, False
    for (gb, gs, ga, gi), (wb, ws, wa, wi) in zip(got, want):
        pairs = [(gb, wb)]
        if d.categorical:
            flipped = flipped or not np.array_equal(gi["post_idx"], wi["post_idx"])
        else:
            pairs.append((gs, ws))
        if d.discrete_actions:
            flipped = flipped or not np.array_equal(ga.argmax(1), wa.argmax(1))
        else:
            pairs.append((ga, wa))
        for g, w in pairs:
            g, w = np.asarray(g, np.float64), np.asarray(w, np.float64)
            ratio = max(ratio, float((np.abs(g - w) / (TOL + TOL * np.abs(w))).max()))
    return ratio, flipped
