"""cnn_activation_function on the host side (no GPU): validation order, Dims, and the ReLU decision margin of the golden
case that the GPU tests compare against without exempting any element."""
import dataclasses

import numpy as np
import pytest

from big_dreamer_amd import synth
from tests.cnn_act_ref import CNN_ACT_CASES, conv_margins
from tests.helpers import abssum, compare_tensor, load_golden, sample_of


class _Env:
    action_size, observation_size = 2, 5


def _params(**over):
    return dict({"ActorCritic": {"gradient_mixing": -1}, "disable_cuda": True}, **over)


def test_dims_default_and_validation():
    assert synth.Dims().cnn_act == "ELU" and synth.TINY_PIXEL.cnn_act == "ELU"
    assert dataclasses.replace(synth.TINY_PIXEL, cnn_act="ReLU").cnn_act == "ReLU"
    with pytest.raises(ValueError, match="ELU.*ReLU.*Tanh"):
        synth.Dims(cnn_act="GELU")


@pytest.mark.parametrize("bad", ["GELU", "relu", "", None])
def test_unknown_cnn_activation_raises_before_the_device_check(bad):
    from big_dreamer_amd.dreamer import Dreamer
    with pytest.raises(ValueError, match="ELU.*ReLU.*Tanh"):       # disable_cuda=True would otherwise raise RuntimeError
        Dreamer(_params(cnn_activation_function=bad), _Env())


@pytest.mark.parametrize("algo", ["dreamer", "planet"])
def test_dense_activation_other_than_elu_raises_before_the_device_check(algo):
    from big_dreamer_amd.dreamer import Dreamer
    from big_dreamer_amd.planet import Planet
    cls = Planet if algo == "planet" else Dreamer
    with pytest.raises(NotImplementedError, match="reference default activation \\(ELU\\)"):
        cls(_params(dense_activation_function="ReLU", algorithm=algo), _Env())


@pytest.mark.parametrize("act", ["ELU", "ReLU", "Tanh"])
def test_known_cnn_activation_passes_validation(act):
    """Accepted with pixel_observation False too (no effect there, as in the reference): the next error is the device's."""
    from big_dreamer_amd.dreamer import Dreamer
    with pytest.raises(RuntimeError, match="no CPU path"):
        Dreamer(_params(cnn_activation_function=act, dense_activation_function="ELU", pixel_observation=False), _Env())


def test_kernel_codes_match_the_header():
    """_cabi's codes are the header's: a _GRAD code is its forward code + 1."""
    import os
    import re
    from big_dreamer_amd import _cabi as cabi
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bigdreamer_hip.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define BD_ACT_(\w+) (\d+)", hdr)}
    assert codes == {"NONE": 0, "ELU": 1, "ELU_GRAD": 2, "RELU": 3, "RELU_GRAD": 4, "TANH": 5, "TANH_GRAD": 6}
    assert cabi.CNN_ACTS == {"ELU": (codes["ELU"], codes["ELU_GRAD"]), "ReLU": (codes["RELU"], codes["RELU_GRAD"]),
                             "Tanh": (codes["TANH"], codes["TANH_GRAD"])}
    assert "int bd_act_backward(float* g, const float* y, size_t n, int act, void* stream);" in hdr


@pytest.fixture(scope="module")
def margins():
    """The float64 oracle's two train steps per activation, run once: (count, min ratio, total, logs)."""
    return {act: conv_margins(act, CNN_ACT_CASES[act][0], CNN_ACT_CASES[act][1]) for act in ("ReLU", "Tanh")}


def test_relu_decision_margin(margins):
    """ReLU' jumps at 0: an fp32 implementation that rounds a conv pre-activation to the other side of 0 changes that
    element's gradient by its full size.  Every conv pre-activation of the two golden train steps (8 encoder + 6 decoder
    layer passes, 1 100 928 values) is recomputed in float64 with plain F.conv2d / F.conv_transpose2d calls
    (tests/cnn_act_ref.py); m = C_TOL * sum|a*b| is the fp32 bound of its contraction (tests/dense_ref.py).  The number with
    |pre| <= m must be 0, so no element is exempt in any GPU comparison of tiny_pixel_relu.npz.

    Generator seed 91 (tests/gen_golden_cnn_act.py --search: the first of 20, 21, ... with a count of 0; the others had
    1 to 12); smallest |pre| / m = 1.241."""
    count, ratio, total, _ = margins["ReLU"]
    print(f"ReLU: {count} of {total} conv pre-activations within the fp32 bound of 0; smallest |pre|/m = {ratio:.4f}")
    assert total == 2 * 6 * (31 * 31 * 32 + 14 * 14 * 64 + 6 * 6 * 128 + 2 * 2 * 256 + 25 * 128 + 13 * 13 * 64 + 30 * 30 * 32)
    assert count == 0
    assert ratio > 1.0


@pytest.mark.parametrize("act", ["ReLU", "Tanh"])
def test_float64_oracle_with_swapped_stacks_matches_the_reference_golden(act, margins):
    """The conv stacks written in tests/cnn_act_ref.py compute what the reference computes with that
    cnn_activation_function: the world-model losses of both train steps against the reference's own run (fp32, so the
    fp32 tolerances of tests/test_hip_parity.py).  The behaviour-learning logs are left to the fp32 comparisons of the GPU
    test: the policy entropy is a 100-sample mean of a tanh-Normal log-density clamped near saturation, which float64 and
    fp32 evaluate differently whatever the conv stacks do."""
    d, seed, name = CNN_ACT_CASES[act]
    g = load_golden(name)
    P = synth.make_params(d, seed)
    assert np.isclose(abssum(v for sd in P.values() for v in sd.values()), float(g["fingerprint.params"]), rtol=1e-12)
    assert np.isclose(abssum(synth.make_batch(d, seed).values()), float(g["fingerprint.batch"]), rtol=1e-12)
    logs = margins[act][3]
    for step in range(2):
        for k in ("observation_loss", "reward_loss", "kl_loss", "model_loss"):
            v, atol, rtol = logs[step][k], 2e-5, 5e-5
            want = float(g[f"step{step}.log.{k}"])
            assert abs(v - want) <= atol + rtol * abs(want), (act, step, k, v, want)
        # post-Adam weights of both conv stacks: an Adam step moves a weight by <= lr (2e-4), agreement must be far below it
        for k, v in logs[step].items():
            if k.startswith("param."):
                compare_tensor(g, f"step{step}.{k}", v, False, atol=2e-5, rtol=1e-5)


def test_golden_relu_file_is_not_an_elu_run():
    """A generator that dropped the key would have written an ELU run: the same seed on ELU stacks moves the first conv
    layer's weights elsewhere (the losses alone barely tell: the pixel NLL is dominated by its constant)."""
    d, seed, name = CNN_ACT_CASES["ReLU"]
    g = load_golden(name)
    got = conv_margins("ELU", d, seed)[3][0]["param.encoder.model.0.weight"]
    err = np.abs(sample_of(got) - g["step0.param.encoder.model.0.weight.sample"])
    assert (err > 1e-4).sum() > 10, err.max()
