"""ctypes binding of ``libbigdreamer_hip.so`` (C ABI declared in ``include/bigdreamer_hip.h``).

The product path has no CPU fallback: importing this module without the built HIP library raises.
Build it with ``python -c "import __graft_entry__ as g; g.build()"`` (or ``make -C big_dreamer_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# BD_LIB selects an alternative build of the same library (kernel tuning experiments only)
LIB_PATH = os.environ.get("BD_LIB") or os.path.join(_HERE, "libbigdreamer_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: the MI355X HIP extension has not been built "
        "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")

lib = C.CDLL(LIB_PATH)

BD_MAX_LAYERS = 6
ACT_NONE, ACT_ELU, ACT_ELU_GRAD = 0, 1, 2
ACT_RELU, ACT_RELU_GRAD, ACT_TANH, ACT_TANH_GRAD = 3, 4, 5, 6
# cnn_activation_function (the torch.nn class names the reference resolves) -> (forward code, "times f' of the saved output")
CNN_ACTS = {"ELU": (ACT_ELU, ACT_ELU_GRAD), "ReLU": (ACT_RELU, ACT_RELU_GRAD), "Tanh": (ACT_TANH, ACT_TANH_GRAD)}
GRAD_ACTS = (ACT_ELU_GRAD, ACT_RELU_GRAD, ACT_TANH_GRAD)
P = C.c_void_p
F32 = C.c_float
I32 = C.c_int


class PackDesc(C.Structure):
    _fields_ = [("src", P), ("dst", P), ("ld", I32), ("N", I32), ("K", I32), ("transpose", I32),
                ("kind", I32), ("src2", P), ("ld2", I32), ("E", I32)]


PACK_COPY, PACK_PRODUCT, PACK_PRODUCT_VEC = 0, 1, 2
PACK_PRODUCTS = 65536        # bd_pack_weights: n = descriptors + PACK_PRODUCTS * (trailing product descriptors)
WGRAD_GEMM, WGRAD_CHAIN = 0, 1


class Layer(C.Structure):
    _fields_ = [("w", P), ("bias", P), ("N", I32), ("K", I32), ("act", I32), ("save", P)]


class MlpFwdArgs(C.Structure):
    _fields_ = [("M", I32), ("in0", P), ("ld0", I32), ("w0", I32), ("in1", P), ("ld1", I32), ("w1", I32),
                ("n_layers", I32), ("layer", Layer * BD_MAX_LAYERS), ("out", P), ("ldo", I32),
                ("gidx", P), ("gWT", P), ("gD", I32), ("gC", I32)]


class LayerBwd(C.Structure):
    _fields_ = [("wt", P), ("saved", P), ("N", I32), ("K", I32), ("act", I32), ("dpre", P)]


class MlpBwdArgs(C.Structure):
    _fields_ = [("M", I32), ("dout", P), ("lddo", I32), ("dout_scale", F32), ("n_layers", I32),
                ("layer", LayerBwd * BD_MAX_LAYERS), ("din0", P), ("ld0", I32), ("w0", I32),
                ("din1", P), ("ld1", I32), ("w1", I32), ("accumulate", I32)]


BD_HEAD_HIDDEN = 4


class ImgHead(C.Structure):
    _fields_ = [("w", P * BD_HEAD_HIDDEN), ("wt", P * BD_HEAD_HIDDEN), ("b", P * BD_HEAD_HIDDEN),
                ("w_out", P), ("b_out", P), ("dout", P), ("out", P)]


class ImgHeadsArgs(C.Structure):
    _fields_ = [("M", I32), ("F", I32), ("Hd", I32), ("x", P), ("head", ImgHead * 2), ("dx", P)]


BD_RNG_MAX_TENSORS = 6
BD_RNG_NORMAL, BD_RNG_EXPONENTIAL, BD_RNG_UNIFORM = 0, 1, 2


class RngTensor(C.Structure):
    _fields_ = [("p", P), ("count", C.c_size_t), ("kind", I32), ("stream_id", C.c_uint)]


class RngFillArgs(C.Structure):
    _fields_ = [("n", I32), ("seed", C.c_ulonglong), ("step", C.c_ulonglong), ("t", RngTensor * BD_RNG_MAX_TENSORS)]


class WgradDesc(C.Structure):
    _fields_ = [("dpre", P), ("ldp", I32), ("act1", P), ("lda1", I32), ("M1", I32), ("act2", P), ("lda2", I32),
                ("M", I32), ("N", I32), ("K", I32), ("dW", P), ("ldw", I32), ("db", P),
                ("splits", I32), ("rows_per", I32), ("tiles_n", I32), ("tiles_k", I32), ("block_begin", I32),
                ("red_begin", I32), ("ws_off", C.c_ulonglong),
                ("g_nseg", I32), ("g_seglen", I32), ("g_gh", I32), ("g_gw", I32), ("g_IH", I32), ("g_IW", I32), ("g_C", I32),
                ("g_pad", I32),
                ("kind", I32), ("c_E", I32), ("c_A", P), ("c_lda", I32), ("c_B", P), ("c_ldb", I32), ("c_b", P),
                ("c_dA", P), ("c_ldda", I32), ("c_dB", P), ("c_lddb", I32), ("c_db", P)]


def _ptr_fields(names):
    return [(n, P) for n in names]


class ObserveFwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("T", "B", "Be", "S", "A", "Hd")] + _ptr_fields(
        ["w_embed_s", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh",
         "w_q1h", "b_q1", "w_q2m", "w_q2s", "b_q2", "init_belief", "init_state", "actions", "nonterm", "pre_emb",
         "eps_post"]) + [("min_std", F32)] + _ptr_fields(
        ["feat", "post_mean", "post_std", "sv_s", "sv_x", "sv_gates", "sv_q"]))


class ObserveBwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("T", "B", "Be", "S", "A", "Hd")] + _ptr_fields(
        ["wt_embed_s", "wt_ir", "wt_iz", "wt_in", "wt_hr", "wt_hz", "wt_hn", "wt_q1h", "wt_q2m", "wt_q2s",
         "init_belief", "nonterm", "eps_post", "feat", "post_std", "sv_x", "sv_gates", "sv_q", "dfeat", "dpost_mean",
         "dpost_std"]) + [("min_std", F32)] + _ptr_fields(
        ["d_embed_pre", "d_gi", "d_gh", "d_q1_pre", "d_q2_out"]))


class ImagineFwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("N", "Hm", "Be", "S", "A", "Hd", "n_samples")] + _ptr_fields(
        ["w_embed_s", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh", "w_p1",
         "b_p1", "w_p2m", "w_p2s", "b_p2", "w_a0h", "w_a0s"]) + [("w_a", P * 3), ("b_a", P * 4)] + _ptr_fields(
        ["w_a4m", "w_a4s", "b_a4", "start_feat", "eps_action", "eps_entropy", "eps_prior"]) + [
        ("min_std", F32), ("act_raw_init_std", F32), ("act_min_std", F32), ("act_mean_scale", F32)] + _ptr_fields(
        ["feat", "prior_mean", "prior_std", "entropy", "action", "sv_actor", "sv_act_stats", "sv_x", "sv_gates",
         "sv_p"]) + [("sv_actor_stride", C.c_size_t)] + _ptr_fields(["sv_act_us"]) + [("discrete_actions", I32)])


class ImagineBwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("N", "Hm", "Be", "S", "A", "Hd")] + _ptr_fields(
        ["wt_embed_s", "wt_embed_a", "wt_ir", "wt_iz", "wt_in", "wt_hr", "wt_hz", "wt_hn", "wt_p1", "wt_p2m",
         "wt_p2s"]) + [("wt_a", P * 3)] + _ptr_fields(
        ["wt_a4m", "wt_a4s", "start_feat", "feat", "prior_std", "action", "eps_action", "eps_prior", "sv_actor",
         "sv_act_stats", "sv_x", "sv_gates", "sv_p"]) + [("min_std", F32)] + _ptr_fields(["dfeat"]) + [
        ("dentropy", F32)] + _ptr_fields(["d_actor_pre", "d_actor_out", "ent_weight"]) + [("discrete_actions", I32)])


U8P = C.c_void_p


class ObserveCatFwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("T", "B", "Be", "D", "C", "A", "Hd")] + _ptr_fields(
        ["w_embed_sT", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh",
         "w_q1h", "b_q1", "w_q2", "b_q2", "init_belief", "init_state", "actions", "nonterm", "pre_emb", "q_post",
         "feat", "post_logits", "sidx", "sv_s", "sv_x", "sv_gates", "sv_q"]))


class ObserveCatBwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("T", "B", "Be", "D", "C", "A", "Hd")] + _ptr_fields(
        ["wt_embed_s", "wt_ir", "wt_iz", "wt_in", "wt_hr", "wt_hz", "wt_hn", "wt_q1h", "wt_q2", "init_belief", "nonterm",
         "feat", "post_logits", "sv_x", "sv_gates", "sv_q", "dfeat", "dpost_logits", "d_embed_pre", "d_gi", "d_gh",
         "d_q1_pre", "d_q2_out"]))


class ImagineCatFwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("N", "Hm", "Be", "D", "C", "A", "Hd", "n_samples")] + _ptr_fields(
        ["w_embed_sT", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh", "w_p1",
         "b_p1", "w_p2", "b_p2", "w_a0h", "w_a0sT"]) + [("w_a", P * 3), ("b_a", P * 4)] + _ptr_fields(
        ["w_a4m", "w_a4s", "b_a4", "start_feat", "start_sidx", "eps_action", "eps_entropy", "q_prior"]) + [
        ("act_raw_init_std", F32), ("act_min_std", F32), ("act_mean_scale", F32)] + _ptr_fields(
        ["feat", "sidx", "prior_logits", "entropy", "action", "sv_actor", "sv_act_stats", "sv_x", "sv_gates", "sv_p",
         "sv_act_us"]) + [("discrete_actions", I32)])


class ImagineCatBwdArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("N", "Hm", "Be", "D", "C", "A", "Hd")] + _ptr_fields(
        ["wt_embed_s", "wt_embed_a", "wt_ir", "wt_iz", "wt_in", "wt_hr", "wt_hz", "wt_hn", "wt_p1", "wt_p2"]) + [
        ("wt_a", P * 3)] + _ptr_fields(
        ["wt_a4m", "wt_a4s", "start_feat", "feat", "prior_logits", "action", "eps_action", "sv_actor", "sv_act_stats",
         "sv_x", "sv_gates", "sv_p", "dfeat"]) + [("dentropy", F32)] + _ptr_fields(["d_actor_pre", "d_actor_out", "ent_weight"]) + [
        ("discrete_actions", I32)])


class PlanArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("rows", "H", "cand", "Be", "D", "C", "S", "A", "Hd", "latent_cat")] + _ptr_fields(
        ["w_embed_s", "w_embed_sT", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh",
         "w_p1", "b_p1", "w_p2m", "w_p2s", "w_p2", "b_p2"]) + [("w_r", P * 5)] + _ptr_fields(["w_r0h", "w_r0sT"]) + [
        ("b_r", P * 5), ("min_std", F32)] + _ptr_fields(
        ["init_belief", "init_state", "act_mean", "act_std", "eps_action", "eps_state"]) + [
        ("seed", C.c_ulonglong), ("step", C.c_ulonglong), ("stream_id", C.c_uint)] + _ptr_fields(
        ["actions", "returns", "feat", "sidx"]))


PlanCatArgs = PlanArgs     # bd_plan_cat_args is a typedef of bd_plan_args


class ActArgs(C.Structure):
    _fields_ = ([(n, I32) for n in ("B", "Be", "D", "C", "S", "A", "Hd", "E", "O", "latent_cat", "actor_cat")] + [
        ("w_enc", P * 5), ("b_enc", P * 5)] + _ptr_fields(
        ["w_embed_s", "w_embed_sT", "w_embed_a", "b_embed", "w_ir", "w_iz", "w_in", "w_hr", "w_hz", "w_hn", "b_ih", "b_hh",
         "w_q1h", "w_q1e", "b_q1", "w_q2m", "w_q2s", "w_q2", "b_q2", "w_a0h", "w_a0s", "w_a0sT"]) + [
        ("w_a", P * 3), ("b_a", P * 4)] + _ptr_fields(
        ["w_a4m", "w_a4s", "b_a4", "belief", "state", "action", "obs", "embedding", "eps_post", "eps_action",
         "eps_explore"]) + [("seed", C.c_ulonglong), ("step", C.c_ulonglong), ("stream_post", C.c_uint),
                            ("stream_action", C.c_uint), ("stream_explore", C.c_uint),
                            ("min_std", F32), ("act_raw_init_std", F32), ("act_min_std", F32), ("act_mean_scale", F32),
                            ("action_noise", F32), ("explore", I32)] + _ptr_fields(
        ["belief_out", "state_out", "action_out"]) + [
        # the evaluation policy: appended, a zeroed tail is the sampling step
        ("action_mode", I32), ("latent_mean", I32), ("n_mode", I32), ("eps_mode", P), ("stream_mode", C.c_uint),
        ("act_stats_out", P), ("mode_index_out", P)])


ActCatArgs = ActArgs       # bd_act_cat_args is a typedef of bd_act_args
# bd_scan_lds_bytes: kernel ids in the order of bigdreamer_hip.h (BD_SCAN_*)
SCAN_KERNELS = {name: i for i, name in enumerate((
    "observe_fwd", "observe_bwd", "observe_cfwd", "observe_cbwd", "observe_kfwd", "observe_kbwd", "imagine_fwd", "imagine_bwd",
    "observe_cat_fwd", "observe_cat_bwd", "imagine_cat_fwd", "imagine_cat_bwd", "observe_cat_cfwd", "observe_cat_cbwd"))}
BD_POLICY_SAMPLE, BD_POLICY_MODE, BD_POLICY_MEAN = 0, 1, 2
ACTION_MODES = {"sample": BD_POLICY_SAMPLE, "mode": BD_POLICY_MODE, "mean": BD_POLICY_MEAN}


class ConvArgs(C.Structure):
    _fields_ = [("in_", P), ("out", P), ("w", P), ("bias", P),
                ("imgs", I32), ("gh", I32), ("gw", I32), ("N", I32), ("K", I32),
                ("nseg", I32), ("seglen", I32), ("C", I32), ("IH", I32), ("IW", I32), ("sy", I32), ("y0", I32),
                ("ss", I32), ("sx", I32), ("x0", I32), ("mask", I32), ("cshift", I32), ("vec4", I32),
                ("OH", I32), ("OW", I32), ("osy", I32), ("oy0", I32), ("osx", I32), ("ox0", I32), ("ldo", I32),
                ("act", I32), ("fuse_cq", I32), ("aux", P)]


class ReplayAppendArgs(C.Structure):
    _fields_ = [("n", I32), ("size", I32), ("rows", P), ("obs", P), ("obs_width", I32), ("bit_depth", I32),
                ("dst_obs", P), ("act", P), ("A", I32), ("dst_act", P), ("reward", P), ("nonterminal", P),
                ("dst_reward", P), ("dst_nonterminal", P)]


class ReplaySampleArgs(C.Structure):
    _fields_ = (_ptr_fields(["obs", "act", "reward", "nonterminal"]) + [(n, I32) for n in (
        "obs_width", "A", "size", "lanes", "lane_size", "idx", "full", "n", "L", "bit_depth")] + [
        (n, C.c_ulonglong) for n in ("seed", "step", "pix_seed", "pix_step")] + _ptr_fields(
        ["dst_obs", "dst_act", "dst_reward", "dst_nonterminal", "idx_out"]))


BD_FP_MAX_BUFFERS = 16


class FingerprintBuf(C.Structure):
    _fields_ = [("p", P), ("n", C.c_size_t)]


class FingerprintArgs(C.Structure):
    _fields_ = [("n_buf", I32), ("buf", FingerprintBuf * BD_FP_MAX_BUFFERS)]


BD_MOMENTS_MAX_BUFFERS, BD_MOMENTS_WORDS = 16, 6
BD_LATENT_WORDS, BD_LATENT_CAT_WORDS, BD_SEGMENTS_MAX = 15, 5, 32


class MomentsBuf(C.Structure):
    _fields_ = [("p", P), ("q", P), ("n", C.c_size_t)]


class MomentsArgs(C.Structure):
    _fields_ = [("n_buf", I32), ("buf", MomentsBuf * BD_MOMENTS_MAX_BUFFERS)]


# every symbol include/bigdreamer_hip.h declares, with its signature
_SIGS = {
    "bd_last_error": (C.c_char_p, []),
    "bd_version": (I32, []),
    "bd_packed_floats": (C.c_size_t, [I32, I32]),
    "bd_pack_weights": (I32, [P, I32, P]),
    "bd_mlp_forward": (I32, [C.POINTER(MlpFwdArgs), P]),
    "bd_mlp_backward": (I32, [C.POINTER(MlpBwdArgs), P]),
    "bd_mlp_set_tall": (I32, [I32]),
    "bd_wgrad_ws_floats": (C.c_size_t, [I32, I32, I32]),
    "bd_wgrad": (I32, [P, I32, P, I32, I32, I32, I32, P, I32, P, I32, P, C.c_size_t, P]),
    "bd_wgrad_plan": (I32, [C.POINTER(WgradDesc), I32, C.POINTER(I32), C.POINTER(I32), C.POINTER(C.c_size_t)]),
    "bd_wgrad_grouped": (I32, [P, I32, I32, I32, P, P]),
    "bd_wgrad_grouped_phase": (I32, [P, I32, I32, I32, P, I32, P]),
    "bd_observe_forward": (I32, [C.POINTER(ObserveFwdArgs), P]),
    "bd_observe_backward": (I32, [C.POINTER(ObserveBwdArgs), P]),
    "bd_observe_cluster_size": (I32, [I32, I32]),
    "bd_observe_cluster_ws_floats": (C.c_size_t, [I32, I32]),
    "bd_observe_forward_cluster": (I32, [C.POINTER(ObserveFwdArgs), P, C.c_size_t, P]),
    "bd_observe_backward_cluster": (I32, [C.POINTER(ObserveBwdArgs), P, C.c_size_t, P]),
    "bd_observe_cluster_status": (I32, [P, I32, P]),
    "bd_observe_cluster_err_offset": (C.c_size_t, [I32]),
    "bd_scan_lds_bytes": (C.c_size_t, [I32] * 8),
    "bd_observe_cluster_set_spin_limit": (I32, [C.c_uint]),
    "bd_observe_cluster_set_ksplit": (I32, [I32]),
    "bd_gauss_head_forward": (I32, [P, P, I32, I32, F32, P, P, P, P]),
    "bd_gauss_head_backward": (I32, [P, P, P, P, P, I32, I32, P, P]),
    "bd_observe_cat_forward": (I32, [C.POINTER(ObserveCatFwdArgs), P]),
    "bd_observe_cat_backward": (I32, [C.POINTER(ObserveCatBwdArgs), P]),
    "bd_observe_cat_cluster_size": (I32, [I32, I32, I32, I32, I32]),
    "bd_observe_cat_cluster_ws_floats": (C.c_size_t, [I32, I32, I32, I32, I32]),
    "bd_observe_cat_forward_cluster": (I32, [C.POINTER(ObserveCatFwdArgs), I32, P, C.c_size_t, P]),
    "bd_observe_cat_backward_cluster": (I32, [C.POINTER(ObserveCatBwdArgs), I32, P, C.c_size_t, P]),
    "bd_imagine_cat_forward": (I32, [C.POINTER(ImagineCatFwdArgs), P]),
    "bd_imagine_cat_backward": (I32, [C.POINTER(ImagineCatBwdArgs), P]),
    "bd_imagine_forward": (I32, [C.POINTER(ImagineFwdArgs), P]),
    "bd_imagine_forward_scan": (I32, [C.POINTER(ImagineFwdArgs), P]),
    "bd_actor_entropy": (I32, [P, P, P, I32, I32, I32, I32, P]),
    "bd_imagine_backward": (I32, [C.POINTER(ImagineBwdArgs), P]),
    "bd_lambda_return_forward": (I32, [P, P, I32, I32, F32, F32, P, P]),
    "bd_rng_fill": (I32, [C.POINTER(RngFillArgs), P]),
    "bd_philox4x32_10": (I32, [C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]),
    "bd_actor_entropy_rng": (I32, [C.c_ulonglong, C.c_ulonglong, C.c_uint, P, P, I32, I32, I32, I32, P]),
    "bd_gemm_nt": (I32, [P, I32, P, I32, P, I32, I32, I32, I32, I32, P]),
    "bd_categorical_head_forward": (I32, [P, P, I32, I32, I32, P, P, P]),
    "bd_categorical_head_backward": (I32, [P, P, I32, I32, I32, P, P]),
    "bd_kl_categorical_forward": (I32, [P, P, I32, I32, I32, F32, I32, P, I32, P, P]),
    "bd_kl_categorical_backward": (I32, [P, P, I32, I32, I32, F32, F32, F32, F32, P, I32, P, P, P]),
    "bd_plan_rollout": (I32, [C.POINTER(PlanArgs), P]),
    "bd_cem_refit": (I32, [P, I32, P, I32, I32, I32, I32, I32, P, P, P]),
    "bd_plan_rollout_cat": (I32, [C.POINTER(PlanCatArgs), P]),
    "bd_act_step_supported": (I32, [I32, I32, I32, I32, I32, I32]),
    "bd_act_step": (I32, [C.POINTER(ActArgs), P]),
    "bd_act_step_cat_supported": (I32, [I32] * 10),
    "bd_act_step_cat": (I32, [C.POINTER(ActCatArgs), P]),
    "bd_tanh_normal_mode": (I32, [P, P, P, C.c_ulonglong, C.c_ulonglong, C.c_uint, I32, I32, I32, P, P, P]),
    "bd_lambda_return_backward": (I32, [P, F32, I32, I32, F32, F32, P, P, P]),
    "bd_img_heads_supported": (I32, [I32, I32]),
    "bd_img_heads_fwd_bwd": (I32, [C.POINTER(ImgHeadsArgs), P]),
    "bd_actor_reinforce": (I32, [P, P, P, P, P, P, P, I32, I32, I32, F32, F32, F32, I32, P, P, I32, P, P]),
    "bd_actor_reinforce_cat": (I32, [P, P, P, P, P, P, I32, I32, I32, F32, F32, F32, I32, P, P, I32, P, P]),
    "bd_normal_nll": (I32, [P, I32, P, I32, I32, I32, F32, P, I32, P, I32, P, P]),
    "bd_bernoulli_nll": (I32, [P, P, C.c_size_t, F32, P, P, I32, P, P]),
    "bd_kl_forward": (I32, [P, P, P, P, I32, I32, F32, I32, P, I32, P, P]),
    "bd_kl_backward": (I32, [P, P, P, P, I32, I32, F32, F32, F32, F32, P, I32, P, P, P, P, P]),
    "bd_sum": (I32, [P, C.c_size_t, P, I32, P, P]),
    "bd_sumsq": (I32, [P, C.c_size_t, P, I32, P, P]),
    "bd_adam_step": (I32, [P, P, P, P, C.c_size_t, F32, F32, F32, F32, F32, I32, F32, P, I32, P]),
    "bd_polyak": (I32, [P, P, C.c_size_t, F32, P]),
    "bd_replay_gather": (I32, [P, P, I32, I32, P, P]),
    "bd_replay_gather_pixels": (I32, [P, P, I32, I32, I32, P, P, P]),
    "bd_replay_gather_pixels_rng": (I32, [P, P, I32, I32, I32, C.c_ulonglong, C.c_ulonglong, P, P]),
    "bd_replay_append": (I32, [C.POINTER(ReplayAppendArgs), P]),
    "bd_replay_sample_gather": (I32, [C.POINTER(ReplaySampleArgs), P]),
    "bd_reduce_ws_floats": (C.c_size_t, []),
    "bd_conv_gemm": (I32, [C.POINTER(ConvArgs), P]),
    "bd_conv_thin_forward": (I32, [P, I32, I32, I32, I32, I32, P, I32, P, I32, P, P, P]),
    "bd_conv_pack_class": (I32, [P, P, I32, I32, I32, I32, I32, I32, I32, P]),
    "bd_conv_pack_fused": (I32, [P, P, I32, I32, I32, P]),
    "bd_act_backward": (I32, [P, P, C.c_size_t, I32, P]),
    "bd_elu_backward": (I32, [P, P, C.c_size_t, P]),
    "bd_image_layout": (I32, [P, P, I32, I32, I32, I32, P]),
    "bd_eval_frame": (I32, [P, P, I32, U8P, I32, I32, P]),
    "bd_openl_video": (I32, [P, P, I32, I32, U8P, P]),
    "bd_openl_error": (I32, [P, P, I32, I32, I32, I32, P, P]),
    "bd_colsum_ws_floats": (C.c_size_t, [I32]),
    "bd_colsum": (I32, [P, C.c_size_t, I32, P, P, P]),
    "bd_fingerprint": (I32, [C.POINTER(FingerprintArgs), P, P]),
    "bd_diag_ws_floats": (C.c_size_t, []),
    "bd_moments": (I32, [C.POINTER(MomentsArgs), P, P, P]),
    "bd_latent_stats": (I32, [P, P, P, P, I32, I32, P, P, P, P]),
    "bd_latent_stats_categorical": (I32, [P, P, I32, I32, I32, P, P, P, P, P]),
    "bd_segment_sumsq": (I32, [P, I32, C.POINTER(C.c_size_t), P, P, P]),
    "bd_return_range": (I32, [P, I32, I32, I32, C.c_double, C.c_double, P, P, P]),
    "bd_return_seed": (I32, [P, F32, P, C.c_size_t, P, P, I32, P]),
    "bd_actor_reinforce_norm": (I32, [P, P, P, P, P, P, P, P, I32, I32, I32, F32, F32, F32, I32, P, P, I32, P, P]),
    "bd_actor_reinforce_cat_norm": (I32, [P, P, P, P, P, P, P, I32, I32, I32, F32, F32, F32, I32, P, P, I32, P, P]),
    "bd_twohot_decode": (I32, [P, I32, I32, I32, F32, P, P, P]),
    "bd_twohot_decode_backward": (I32, [P, I32, P, I32, I32, F32, P, I32, P]),
    "bd_twohot_nll": (I32, [P, I32, P, P, I32, I32, F32, F32, P, I32, P, P, P]),
    "bd_symlog": (I32, [P, C.c_size_t, P, P]),
    "bd_symexp": (I32, [P, C.c_size_t, P, P]),
}

for _name, (_res, _args) in _SIGS.items():
    _fn = getattr(lib, _name)          # AttributeError here = header/library mismatch
    _fn.restype = _res
    _fn.argtypes = _args

EXPORTED = tuple(_SIGS)


def check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("bigdreamer_hip: " + lib.bd_last_error().decode())


def ptr(t) -> int:
    """Device pointer of a tensor (None -> NULL).  The kernels read every operand as dense row-major with the leading
    dimension the caller states, so a tensor must be contiguous or a row-strided 2-D view of one (unit inner stride,
    e.g. ``W[:, :S]`` or ``feat[:, :Be]``): a permuted or column-strided view would be read with the wrong strides."""
    if t is None:
        return None
    if not (t.dtype in (torch.float32, torch.int64, torch.uint8) and t.is_cuda):
        raise TypeError("expected a CUDA fp32/int64/uint8 tensor")
    if not (t.is_contiguous() or (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1])):
        raise ValueError(f"non-contiguous tensor (shape {tuple(t.shape)}, strides {t.stride()}) passed to a HIP kernel: "
                         "call .contiguous() first")
    return t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def packed_floats(N: int, K: int) -> int:
    return ((N + 15) // 16) * ((K + 15) // 16) * 256
