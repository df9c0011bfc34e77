"""Golden vectors for cnn_activation_function = ReLU / Tanh, produced by the reference itself through
oracle/gen_golden.py's ``run_config`` (its ``**over`` reaches the reference's parameter dict).  TEST INFRASTRUCTURE; runs
where the reference is installed (see oracle/gen_golden.py), never on the GPU box.

    python tests/gen_golden_cnn_act.py            # writes tests/golden/tiny_pixel_relu.npz, tiny_pixel_tanh.npz
    python tests/gen_golden_cnn_act.py --search   # prints, per candidate seed, the ReLU decision margin (no reference needed)

The ReLU seed is the first one at which no conv pre-activation of the two train steps lies within its fp32 bound of 0
(tests/test_cnn_activation_cpu.py::test_relu_decision_margin), so no fp32 implementation can take ReLU's other branch
anywhere and no element is exempt in any comparison against the file.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests.cnn_act_ref import CNN_ACT_CASES, conv_margins  # noqa: E402


def search(first: int = 20, last: int = 200) -> None:
    d = CNN_ACT_CASES["ReLU"][0]
    for seed in range(first, last):
        count, ratio, total, _ = conv_margins("ReLU", d, seed)
        print(f"seed {seed}: {count} of {total} conv pre-activations within the fp32 bound of 0; min |pre|/m = {ratio:.3f}",
              flush=True)
        if count == 0:
            break


def main() -> None:
    from oracle import gen_golden
    torch.manual_seed(0)
    torch.set_num_threads(8)
    dreamer_mod, _ = gen_golden._import_reference()
    for act in ("ReLU", "Tanh"):
        d, seed, name = CNN_ACT_CASES[act]
        # the reference's stacks are built from the key; Dims.cnn_act only tells OUR engine which epilogue to run
        gen_golden.run_config(dreamer_mod, name, d, full=False, seed=seed, cnn_activation_function=act)


if __name__ == "__main__":
    search() if "--search" in sys.argv else main()
