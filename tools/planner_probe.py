#!/usr/bin/env python3
"""Time MPCPlanner.forward (reference defaults: H=15, 10 iterations, 1000 candidates, top 100) at the config-2 model size:
fused HIP path vs the same planner composed from the agent's own modules (one launch per piece) vs the CPU oracle.

    planner_probe.py [B] [--latent categorical]

--latent categorical: 32 x 32 Categorical latents (otherwise the same defaults).  Times bd_plan_rollout_cat in both
BD_PLAN_FUSE forms and the default, with in-kernel sampler noise and with an explicit draw buffer, against the composed
baseline (TransitionModel.forward(embeddings=None) + reward_model + torch.topk, which uses none of the planner kernels).
Every figure is reported as the median and the range of REPS repetitions of the timed loop."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from big_dreamer_amd import synth  # noqa: E402
from big_dreamer_amd.config import load_config  # noqa: E402
from big_dreamer_amd.dreamer import Dreamer  # noqa: E402
from big_dreamer_amd.env import SyntheticEnv  # noqa: E402
from big_dreamer_amd.planner import MPCPlanner  # noqa: E402


REPS = 5


def main():
    args = sys.argv[1:]
    cat = False
    if "--latent" in args:
        i = args.index("--latent")
        cat = args[i + 1] == "categorical"
        del args[i:i + 2]
    B = int(args[0]) if args else 1
    d = synth.CONFIG5_STATE if cat else synth.CONFIG2
    H, iters, cand, top = 15, 10, 1000, 100
    over = ["experience_size=400"]
    if cat:
        over += ["latent_distribution=Categorical", f"discrete_latent_dimensions={d.cat_D}",
                 f"discrete_latent_classes={d.cat_C}"]
    params = load_config(over)
    agent = Dreamer(params, SyntheticEnv(d.O, d.A, 40, 2, 0))
    mpc = MPCPlanner(d.A, H, iters, cand, top, agent.transition_model, agent.reward_model)
    belief, state = 0.5 * torch.randn(B, d.Be, device="cuda"), torch.randn(B, d.S, device="cuda")
    if cat:
        idx = torch.randint(0, d.cat_C, (B, d.cat_D), device="cuda")
        state = torch.nn.functional.one_hot(idx, d.cat_C).float().view(B, d.S)

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def spread(fn, n):
        ts = sorted(timed(fn, n) for _ in range(REPS))
        return ts[REPS // 2], ts[0], ts[-1]

    if cat:
        return categorical(B, d, H, iters, cand, top, agent, mpc, belief, state, spread)
    fused, lo, hi = spread(lambda: mpc(belief, state), 20)
    print(f"B={B}: fused HIP {fused:.2f} ms/plan (range {lo:.2f}-{hi:.2f} over {REPS} x 20 plans)", flush=True)

    def unfused():
        xb = belief.unsqueeze(1).expand(B, cand, d.Be).reshape(-1, d.Be)
        xs = state.unsqueeze(1).expand(B, cand, d.S).reshape(-1, d.S)
        mean = torch.zeros(H, B, 1, d.A, device="cuda")
        std = torch.ones(H, B, 1, d.A, device="cuda")
        for _ in range(iters):
            actions = (mean + std * torch.randn(H, B, cand, d.A, device="cuda")).view(H, B * cand, d.A)
            beliefs, states, _, _, _ = agent.transition_model(xs, actions, xb)
            ret = agent.reward_model(beliefs.view(-1, d.Be), states.view(-1, d.S)).view(H, -1).sum(dim=0)
            _, topk = ret.reshape(B, cand).topk(top, dim=1, largest=True, sorted=False)
            topk = topk + cand * torch.arange(0, B, device="cuda").unsqueeze(1)
            best = actions[:, topk.view(-1)].reshape(H, B, top, d.A)
            mean, std = best.mean(dim=2, keepdim=True), best.std(dim=2, unbiased=False, keepdim=True)
        return mean[0].squeeze(1)

    unf = timed(unfused, 5)
    print(f"B={B}: per-module HIP {unf:.2f} ms/plan", flush=True)
    from oracle import dreamer_oracle as O
    P = {m: {k: v.detach().cpu() for k, v in getattr(agent, m).state_dict().items()}
         for m in ("transition_model", "reward_model")}
    nz = synth.make_planner_noise(d, B, H, iters, cand, 0)
    n = len(os.sched_getaffinity(0))
    try:                                                  # a GPU box exposes the whole host but grants a share
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    torch.set_num_threads(n)
    t0 = time.perf_counter()
    with torch.no_grad():
        O.mpc_planner(P, belief.cpu(), state.cpu(), d.A, H, iters, cand, top, torch.as_tensor(nz["action"]),
                      torch.as_tensor(nz["state"]))
    cpu = (time.perf_counter() - t0) * 1e3
    steps = iters * H * B * cand
    print(f"B={B}: fused HIP {fused:.2f} ms/plan ({steps / fused / 1e3:.2f} M candidate steps/s) | per-module HIP {unf:.2f} ms | "
          f"CPU oracle {cpu:.0f} ms ({torch.get_num_threads()} threads)")


def categorical(B, d, H, iters, cand, top, agent, mpc, belief, state, spread):
    fmt = lambda t: f"{t[0]:.2f} ms/plan (range {t[1]:.2f}-{t[2]:.2f} over {REPS} x 10 plans)"
    eps_a = torch.randn(iters, H, B, cand, d.A, device="cuda")
    q = torch.empty(iters, H, B * cand, d.S, device="cuda").exponential_()
    for fuse in ("", "1", "0"):
        if fuse:
            os.environ["BD_PLAN_FUSE"] = fuse
        else:
            os.environ.pop("BD_PLAN_FUSE", None)
        name = {"": "default", "1": "BD_PLAN_FUSE=1", "0": "BD_PLAN_FUSE=0"}[fuse]
        print(f"B={B} categorical {name}: in-kernel noise {fmt(spread(lambda: mpc(belief, state), 10))}", flush=True)
        print(f"B={B} categorical {name}: explicit buffer {fmt(spread(lambda: mpc(belief, state, _noise={'action': eps_a, 'state': q}), 10))}",
              flush=True)
    os.environ.pop("BD_PLAN_FUSE", None)
    del q

    def composed():
        xb = belief.unsqueeze(1).expand(B, cand, d.Be).reshape(-1, d.Be)
        xs = state.unsqueeze(1).expand(B, cand, d.S).reshape(-1, d.S)
        mean = torch.zeros(H, B, 1, d.A, device="cuda")
        std = torch.ones(H, B, 1, d.A, device="cuda")
        for _ in range(iters):
            actions = (mean + std * torch.randn(H, B, cand, d.A, device="cuda")).view(H, B * cand, d.A)
            beliefs, states, _, _, _ = agent.transition_model(xs, actions, xb)
            # (reward_model(beliefs, states) itself refuses a dense 1224-wide input at this size -- bd_mlp_forward's launch
            # fails -- so the baseline takes the engine's own one-hot form of the chain, as the training step does)
            feat = torch.cat([beliefs, states], dim=-1).view(-1, d.Be + d.S)
            sidx = states.view(-1, d.cat_D, d.cat_C).argmax(dim=-1).to(torch.uint8)
            ret, _, _ = agent.engine.dense_forward("reward_model", "rew", "probe_rew", feat, d.Be + d.S, feat.shape[0], 1, sidx=sidx)
            ret = ret.view(H, -1).sum(dim=0)
            _, topk = ret.reshape(B, cand).topk(top, dim=1, largest=True, sorted=False)
            topk = topk + cand * torch.arange(0, B, device="cuda").unsqueeze(1)
            best = actions[:, topk.view(-1)].reshape(H, B, top, d.A)
            mean, std = best.mean(dim=2, keepdim=True), best.std(dim=2, unbiased=False, keepdim=True)
        return mean[0].squeeze(1)

    print(f"B={B} categorical composed baseline (per-module HIP): {fmt(spread(composed, 10))}", flush=True)


if __name__ == "__main__":
    main()
