"""Child process of tests/test_cnn_activation_gpu.py::test_two_train_steps_vs_reference_golden: two whole train steps of a
``Dreamer`` built with ``cnn_activation_function = argv[1]`` on TINY_PIXEL, against the golden file the reference wrote
for that activation and against the CPU oracle with its conv stacks on the same activation.  A child because
BD_CONV_FUSE_ELU is read when big_dreamer_amd.conv_stack is imported.  Prints every figure, then CNN_ACT_RESULT ok."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from big_dreamer_amd import synth  # noqa: E402
from tests.cnn_act_ref import CNN_ACT_CASES, oracle_cnn_act  # noqa: E402
from tests.helpers import assert_close, check_fingerprints, compare_tensor, load_golden  # noqa: E402


class _Env:
    def __init__(self, d):
        self.action_size, self.observation_size = d.A, (3, 64, 64)


def _params(d, act):
    """The reference's parameter dict (conf/config.yaml defaults) at the golden case's sizes."""
    from big_dreamer_amd.config import load_config
    p = load_config()
    p.update(pixel_observation=True, belief_size=d.Be, state_size=d.S, hidden_size=d.Hd, embedding_size=d.E,
             batch_size=d.B, seq_len=d.L, planning_horizon=d.H, experience_size=64, cnn_activation_function=act)
    return p


def _dev(dct):
    return {k: torch.as_tensor(v).cuda().contiguous() for k, v in dct.items()}


def _rel(name, got, want, atol, rtol, rep):
    got = np.asarray(got, dtype=np.float64).reshape(np.asarray(want).shape)
    want = np.asarray(want, dtype=np.float64)
    rep.append(f"{name:44s} max|err|={np.abs(got - want).max():.3e}  max|ref|={np.abs(want).max():.3e}")
    assert_close(name, got, want, atol, rtol)


def run(act: str) -> None:
    from big_dreamer_amd import _cabi as cabi, conv_stack
    from big_dreamer_amd.dreamer import Dreamer
    d, seed, name = CNN_ACT_CASES[act]
    g = load_golden(name)
    P = synth.make_params(d, seed)
    batch = synth.make_batch(d, seed)
    check_fingerprints(g, P, batch, synth.make_noise(d, seed))
    agent = Dreamer(_params(d, act), _Env(d))
    eng = agent.engine
    assert eng.d == d, (eng.d, d)
    assert isinstance(eng.conv, conv_stack.ConvStacks) and (eng.conv.act, eng.conv.act_grad) == cabi.CNN_ACTS[act]
    assert type(agent.encoder.model[1]).__name__ == act and type(agent.observation_model.decoder[3]).__name__ == act
    assert [k for k in agent.encoder.state_dict()] == [f"model.{i}.{w}" for i in (0, 2, 4, 6) for w in ("weight", "bias")]
    eng.load_params(P)
    for grp in ("model", "actor", "critic", "critic_target"):
        eng.pack(grp)
    db = _dev(batch)
    rep = [f"cnn_activation_function={act} BD_CONV_FUSE_ELU={os.environ.get('BD_CONV_FUSE_ELU', '0')} "
           f"FUSE_ELU={conv_stack.FUSE_ELU}"]
    try:
        with oracle_cnn_act(act) as O:
            od = O.OracleDreamer(P, dict(planning_horizon=d.H))
            for step in range(2):
                nz = synth.make_noise(d, seed + step)
                ologs = od.train_step(batch, nz)
                logs = eng.train_step(db, _dev(nz))
                if step == 0:
                    od.update_critic()
                    eng.update_critic()
                torch.cuda.synchronize()
                # the tolerances of tests/test_hip_parity.py::test_train_steps_vs_oracle_and_golden
                for k, v in ologs.items():
                    tol = (2e-4, 2e-4) if k in ("policy_entropy", "actor_loss") else (2e-5, 5e-5)
                    _rel(f"s{step}.{k}", logs[k], v, tol[0], tol[1], rep)
                    _rel(f"s{step}.{k}(golden)", logs[k], g[f"step{step}.log.{k}"], tol[0], tol[1], rep)
                gn = od.last["grad_norms"]
                _rel(f"s{step}.grad_norms", [logs["grad_norm_model"], logs["grad_norm_actor"], logs["grad_norm_critic"]],
                     [gn["model"], gn["actor"], gn["critic"]], 1e-6, 1e-3, rep)
                _rel(f"s{step}.grad_norms(golden)", [logs["grad_norm_model"], logs["grad_norm_actor"], logs["grad_norm_critic"]],
                     g[f"step{step}.grad_norms"], 1e-6, 1e-3, rep)
                coef = {k: min(1.0, od.hp["grad_clip_norm"] / (gn[k] + 1e-6)) for k in gn}
                groups = {"model": (od.model_modules, od.last["model_grads"]), "actor": (("actor",), od.last["actor_grads"]),
                          "critic": (("critic",), od.last["critic_grads"])}
                for grp, (mods, grads) in groups.items():
                    i = 0
                    for mod in mods:
                        for k in od.P[mod]:
                            want = grads[i].numpy() * coef[grp]
                            got = eng.G(mod, k).detach().cpu().numpy()
                            scale = float(np.abs(want).max()) + 1e-12
                            _rel(f"s{step}.grad.{mod}.{k}", got, want, 2e-3 * scale + 1e-9, 2e-3, rep)
                            # the reference's own clipped gradient (stored in full, or as sums + a strided sample)
                            compare_tensor(g, f"step{step}.grad.{mod}.{k}", got, False, atol=2e-3 * scale + 1e-9, rtol=2e-3)
                            i += 1
                for mod in list(od.model_modules) + ["actor", "critic", "critic_target"]:
                    for k, p in od.P[mod].items():
                        got = eng.W(mod, k).detach().cpu().numpy()
                        _rel(f"s{step}.param.{mod}.{k}", got, p.detach().numpy(), 2e-5, 1e-5, rep)
                        compare_tensor(g, f"step{step}.param.{mod}.{k}", got, False, atol=2e-5, rtol=1e-5)
    finally:
        print("\n".join(rep))
    print("CNN_ACT_RESULT ok")


if __name__ == "__main__":
    run(sys.argv[1])
