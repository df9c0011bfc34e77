"""Dreamer agent with the reference's call surface (src/dreamer.py, src/planet.py) on the HIP engine.

Kept surface: ``Dreamer(params, env)``, ``train_step() -> Dict[str, float]``,
``imagine_ahead``, ``get_action``, ``update_critic``, ``update_belief_and_act``, ``buffer.append/sample``,
``eval()/train()``, ``observation_model(h, s)``, module attributes with reference ``state_dict`` names, ``load``
of the reference's checkpoint dict (src/planet.py:103-114), and the module function ``lambda_return``.
Added: ``act_step`` -- the decision of ``update_belief_and_act`` (src/planet.py:370-403, src/dreamer.py:429-444) without the
environment, one kernel launch (bd_act_step); ``evaluate`` -- the test loop of the reference's src/main.py:191-283; ``open_loop`` -- the
open-loop prediction video and error curve of DreamerV1 / DreamerV2 (openloop.py).
"""
from __future__ import annotations

import os
from typing import Any, Dict, Optional, Tuple

import torch
from torch import Tensor

from . import _cabi as cabi
from .collect import check_collect_envs
from .config import (ACTION_MODES, CRITIC_HEAD_DEFAULTS, CRITIC_HEAD_KEYS, RETURN_NORM_KEYS, REWARD_HEAD_DEFAULTS,
                     REWARD_HEAD_KEYS, check_action_distribution, check_cnn_activation, check_critic_head,
                     check_dense_activation, check_gradient_mixing, check_return_normalization, check_reward_head,
                     check_symlog_observations)
from .engine import DEFAULT_HP, DreamerEngine
from .memory import ExperienceReplay
from .models import ActorModel, CnnImageEncoder, DenseModel, ObservationModel, TransitionModel, encoder_for
from .synth import Dims


def _hp_from_params(params: Dict[str, Any]) -> Dict[str, float]:
    ac = params["ActorCritic"]
    return dict(
        kl_balance=params["kl_balance"], kl_loss_weight=params["kl_loss_weight"], free_nats=params["free_nats"],
        grad_clip_norm=params["grad_clip_norm"], discount=params["discount"], disclam=params["disclam"],
        model_learning_rate=params["model_learning_rate"], actor_learning_rate=ac["actor_learning_rate"],
        value_learning_rate=ac["value_learning_rate"], adam_epsilon=params["adam_epsilon"],
        weight_decay=params["weight_decay"], entropy_weight=ac["entropy_weight"], polyak_avg=ac["polyak_avg"],
        discount_weight=params.get("discount_weight", 5.0), gradient_mixing=ac.get("gradient_mixing", -1),
        **{k: ac[k] for k in RETURN_NORM_KEYS if k in ac})


class Dreamer:
    """Drop-in for the reference's ``Dreamer``: state or 64x64 pixel observations, Gaussian or Categorical latents
    (``latent_distribution``; Categorical: state_size = dimensions * classes, src/planet.py:56-57)."""

    def __init__(self, params: Dict[str, Any], env, device: Optional[str] = None, world_size: int = 1,
                 process_group=None):
        self.latent_distribution = params.get("latent_distribution", "Gaussian")
        if self.latent_distribution not in ("Gaussian", "Categorical"):
            raise NotImplementedError(f"{self.latent_distribution}  is yet yet implemented")     # as src/dreamer.py:108
        # -1: the reference's dynamics-backprop actor gradient; rho in [0, 1]: DreamerV2's REINFORCE / dynamics mix
        # (the reference raises for anything but -1, src/dreamer.py:336-339)
        check_gradient_mixing(params["ActorCritic"].get("gradient_mixing", -1))
        # percentile return normalisation of the actor objective (DreamerV3); "none": the reference's objective
        check_return_normalization(*(params["ActorCritic"].get(k, DEFAULT_HP[k]) for k in RETURN_NORM_KEYS),
                                   algorithm=params.get("algorithm"))
        # "normal": the reference's width-1 critic; "twohot" (DreamerV3): K logits over symlog bins ("Two-hot critic")
        self.critic_head, self.critic_bins, self.critic_bin_range = check_critic_head(
            *(params["ActorCritic"].get(k, CRITIC_HEAD_DEFAULTS[k]) for k in CRITIC_HEAD_KEYS), algorithm=params.get("algorithm"))
        # the world model's heads ("World-model heads on any scale"): "twohot" reward logits over symlog bins,
        # symlog on vector observations; both off: the reference's world model
        self.reward_head, self.reward_bins, self.reward_bin_range = check_reward_head(
            *(params.get(k, REWARD_HEAD_DEFAULTS[k]) for k in REWARD_HEAD_KEYS), algorithm=params.get("algorithm"))
        self.symlog_observations = check_symlog_observations(
            params.get("symlog_observations", False), bool(params.get("pixel_observation", False)), params.get("algorithm"))
        # the pixel conv stacks take ELU / ReLU / Tanh (no effect on state observations, as in the reference); the dense
        # chains and scans are ELU only, and say so instead of ignoring the key
        self.cnn_activation_function = check_cnn_activation(params.get("cnn_activation_function", "ELU"))
        check_dense_activation(params.get("dense_activation_function", "ELU"))
        self.action_distribution = check_action_distribution(params.get("action_distribution", "Gaussian"))
        if self.action_distribution == "Categorical" and params.get("algorithm") == "planet":
            raise ValueError("action_distribution=Categorical: PlaNet's CEM planner searches a continuous action space")
        self.use_discount = bool(params.get("use_discount", False))
        self.collect_envs = check_collect_envs(params)     # replay lanes (collect.py); 1: the reference's single ring
        if params.get("disable_cuda", False) or not torch.cuda.is_available():
            raise RuntimeError("big_dreamer_amd runs on MI355X only: there is no CPU path (disable_cuda=True is the "
                               "reference's own CPU mode)")
        self.env = env
        self.params = params
        self.device = torch.device(device or f"cuda:{torch.cuda.current_device()}")
        self.belief_size, self.state_size = params["belief_size"], params["state_size"]
        cat_D = cat_C = 0
        if self.latent_distribution == "Categorical":
            cat_D, cat_C = int(params["discrete_latent_dimensions"]), int(params["discrete_latent_classes"])
            self.state_size = cat_D * cat_C                                                    # src/planet.py:56-57
        self.action_size, self.hidden_size = env.action_size, params["hidden_size"]
        self.embedding_size = params["embedding_size"]
        self.batch_size, self.seq_len = params["batch_size"], params["seq_len"]
        self.planning_horizon = params["planning_horizon"]
        self.action_noise = params["action_noise"]
        self.action_repeat = params["action_repeat"]
        self.seed_steps = params["seed_steps"]
        self.pixel_observation = bool(params.get("pixel_observation", False))
        obs_size = 3 * 64 * 64 if self.pixel_observation else env.observation_size
        self.dims = Dims(B=self.batch_size, L=self.seq_len, H=self.planning_horizon, Be=self.belief_size,
                         S=self.state_size, Hd=self.hidden_size, E=self.embedding_size, A=self.action_size,
                         O=obs_size, pixel=self.pixel_observation, cat_D=cat_D, cat_C=cat_C,
                         use_discount=self.use_discount, discrete_actions=self.action_distribution == "Categorical",
                         cnn_act=self.cnn_activation_function, critic_head=self.critic_head, critic_bins=self.critic_bins,
                         critic_bin_range=self.critic_bin_range, reward_head=self.reward_head, reward_bins=self.reward_bins,
                         reward_bin_range=self.reward_bin_range, symlog_obs=self.symlog_observations)
        self.engine = DreamerEngine(self.dims, _hp_from_params(params), self.device, world_size=world_size,
                                    process_group=process_group,
                                    replica_check_interval=params.get("replica_check_interval", 0),
                                    replica_on_mismatch=params.get("replica_on_mismatch", "raise"),
                                    diagnostics_interval=params.get("diagnostics_interval", 0))
        e = self.engine
        # PyTorch-default initialisation happens in the nn.Modules below (their parameters alias the engine's
        # flat buffers), so seeding torch before construction reproduces a run (src/main.py:56-58).
        init = {}
        feat = self.belief_size + self.state_size
        px, E = self.pixel_observation, self.embedding_size
        for mod, build in (
            ("transition_model", lambda: _ref_init_transition(self.dims)),
            ("observation_model", (lambda: _ref_init_decoder(feat, E)) if px else
             (lambda: _ref_init_dense(feat, self.hidden_size, env.observation_size))),
            ("reward_model", lambda: _ref_init_dense(feat, self.hidden_size, self.dims.reward_out)),
            ("encoder", (lambda: _ref_init_cnn(E)) if px else
             (lambda: _ref_init_dense(env.observation_size, self.hidden_size, self.embedding_size))),
            ("actor", lambda: _ref_init_dense(feat, self.hidden_size, self.dims.actor_out)),
            ("critic", lambda: _ref_init_dense(feat, self.hidden_size, self.dims.critic_out)),
        ) + ((("discount_model", lambda: _ref_init_dense(feat, self.hidden_size, 1)),) if self.use_discount else ()):
            init[mod] = {k: v.detach().numpy() for k, v in build().state_dict().items()}
        init["critic_target"] = init["critic"]                # copy.deepcopy(self.critic), src/dreamer.py:50
        e.load_params(init)
        for g in ("model", "actor", "critic", "critic_target"):
            e.pack(g)
        self.transition_model = TransitionModel(self.belief_size, self.state_size, self.action_size, self.hidden_size,
                                                self.embedding_size, latent_distribution=self.latent_distribution,
                                                discrete_latent_dimensions=cat_D or 32, discrete_latent_classes=cat_C or 32,
                                                engine=e)
        if px:
            self.observation_model = ObservationModel(self.belief_size, self.state_size, E,
                                                      activation=self.cnn_activation_function, engine=e)
            self.encoder = CnnImageEncoder(E, activation=self.cnn_activation_function, engine=e)
        else:
            self.observation_model = DenseModel(feat, self.hidden_size, env.observation_size, engine=e,
                                                module="observation_model", prefix="obs")
            self.encoder = encoder_for(e, env.observation_size, self.hidden_size, self.embedding_size)
        self.reward_model = DenseModel(feat, self.hidden_size, self.dims.reward_out, engine=e, module="reward_model",
                                       prefix="rew")
        self.actor = ActorModel(self.belief_size, self.state_size, self.hidden_size, self.action_size,
                                action_distribution=self.action_distribution, engine=e)
        self.critic = DenseModel(feat, self.hidden_size, self.dims.critic_out, engine=e, module="critic", prefix="cri")
        self.critic_target = DenseModel(feat, self.hidden_size, self.dims.critic_out, engine=e, module="critic_target",
                                        prefix="tgt")
        if self.use_discount:       # src/dreamer.py:80-85
            self.discount_model = DenseModel(feat, self.hidden_size, 1, engine=e, module="discount_model", prefix="dsc")
        self.buffer = ExperienceReplay(params["experience_size"], env.action_size, params["bit_depth"], px,
                                       env.observation_size, self.device, lanes=self.collect_envs,
                                       device_sampler=bool(params.get("sample_on_device", False)))
        self.load(params)

    # ---------------------------------------------------------------------------------------- checkpoints
    def load(self, params: Dict[str, Any]) -> None:
        """src/planet.py:103-114: load the reference's checkpoint dict -- the four world-model state dicts AND
        ``model_optimizer`` (Adam moments and step count, so a resumed run continues the reference's bias correction) --
        with a loader that executes nothing from the file.  Checkpoints written by ``save`` below also restore the
        actor, the critic and its target and their optimisers (the reference never saves those)."""
        path = params.get("models", "")
        if path and os.path.exists(path):
            d = torch.load(path, map_location="cpu", weights_only=True)
            self._check_checkpoint_head(d)          # before anything is copied
            self._check_checkpoint_world_model(d)
            for key in ("transition_model", "observation_model", "reward_model", "encoder"):
                getattr(self, key).load_state_dict(d[key])
            if "model_optimizer" in d:
                self.engine.load_optimizer_state_dict("model", d["model_optimizer"])
            for key in ("actor", "critic", "critic_target") + (("discount_model",) if self.use_discount else ()):
                if key in d:
                    getattr(self, key).load_state_dict(d[key])
            if self.use_discount and "discount_model" not in d and "model_optimizer" in d and d["model_optimizer"]["state"]:
                import warnings      # (a checkpoint in the reference's five-key layout: that is what the reference does too)
                warnings.warn("use_discount=True: the checkpoint carries Adam moments for the discount head (it is part of "
                              "the world-model optimiser, src/dreamer.py:167-169) but not its weights, which stay freshly "
                              "initialised")
            for key, group in (("actor_optimizer", "actor"), ("value_optimizer", "critic")):
                if key in d:
                    self.engine.load_optimizer_state_dict(group, d[key])

    def _critic_head_record(self) -> Dict[str, Any]:
        if self.critic_head == "normal":
            return {"kind": "normal"}
        return {"kind": self.critic_head, "bins": int(self.critic_bins), "range": float(self.critic_bin_range)}

    def _check_checkpoint_head(self, d: Dict[str, Any]) -> None:
        """ValueError unless the checkpoint's critic head is this agent's in kind, K and Z (a checkpoint without the record
        holds the width-1 critic; one without a critic at all -- the reference's files -- has nothing to compare)."""
        if "critic" not in d and "critic_target" not in d:
            return
        theirs = (d.get("run_state") or {}).get("critic_head") or {"kind": "normal"}
        mine = self._critic_head_record()
        if dict(theirs) != mine:
            raise ValueError(f"checkpoint critic head {dict(theirs)} does not match the agent's {mine} "
                             "(ActorCritic.critic_head / critic_bins / critic_bin_range)")

    def _reward_head_record(self) -> Dict[str, Any]:
        if self.reward_head == "normal":
            return {"kind": "normal"}
        return {"kind": self.reward_head, "bins": int(self.reward_bins), "range": float(self.reward_bin_range)}

    def _check_checkpoint_world_model(self, d: Dict[str, Any]) -> None:
        """ValueError unless the checkpoint's reward head is this agent's in kind, K and Z and its world model was trained
        on the same observation transform (a checkpoint without the records -- the reference's files among them -- holds
        the width-1 reward model on raw observations)."""
        rs = d.get("run_state") or {}
        theirs, mine = dict(rs.get("reward_head") or {"kind": "normal"}), self._reward_head_record()
        if theirs != mine:
            raise ValueError(f"checkpoint reward head {theirs} does not match the agent's {mine} "
                             "(reward_head / reward_bins / reward_bin_range)")
        theirs, mine = bool(rs.get("symlog_observations", False)), bool(self.symlog_observations)
        if theirs != mine:
            raise ValueError(f"checkpoint symlog_observations={theirs} does not match the agent's symlog_observations={mine}")

    def save(self, path: str, extra: Optional[Dict[str, Any]] = None) -> None:
        """Checkpoint in the layout ``Planet.load`` reads (src/planet.py:109-114: transition_model, observation_model,
        reward_model, encoder, model_optimizer -- the reference can resume from it), plus actor / critic /
        critic_target, the discount head when ``use_discount`` is set (its parameters are the tail of the world-model
        optimiser, src/dreamer.py:167-169) and the actor / value optimisers (src/dreamer.py:56-67 names) so that this
        framework resumes exactly.
        One more key, ``run_state``, holds what decides the NEXT draws (``load`` ignores it, ``load_run_state`` restores it):
        the engine's noise state (engine.noise_state), the torch CPU and device, numpy and Python generator states
        (checkpoint.capture_generators) and `extra`, a flat dict of ints, floats and strings that belongs to the caller (the
        CLI keeps its step there).  The whole file loads with ``weights_only=True``, and it is written atomically.
        The replay buffer is saved apart (``buffer.save``); the episode in flight -- environment, belief, state, previous
        action -- is the caller's and is not saved: a resumed run starts fresh episodes.
        Data-parallel runs: a COLLECTIVE (it issues the held-back optimiser steps): every rank calls it at the same point.
        The reference declares ``save`` (src/base_agent.py:29-34) but never implements it (src/main.py:274 TODO)."""
        from .checkpoint import atomic_write, capture_generators, check_extra
        e = self.engine
        extra = check_extra(extra)
        # first: noise_state() issues the held-back optimiser steps and orders the pipeline streams before this one, so the
        # weights copied below are those the saved moments and step counts belong to
        noise = e.noise_state()
        d = {key: {k: v.detach().cpu().clone().contiguous() for k, v in getattr(self, key).state_dict().items()}
             for key in ("transition_model", "observation_model", "reward_model", "encoder", "actor", "critic",
                         "critic_target") + (("discount_model",) if self.use_discount else ())}
        d["model_optimizer"] = e.optimizer_state_dict("model")
        d["actor_optimizer"] = e.optimizer_state_dict("actor")
        d["value_optimizer"] = e.optimizer_state_dict("critic")
        d["run_state"] = {"format": 1, "noise": noise, "generators": capture_generators(self.device),
                          "extra": extra}
        if e.hp["return_normalization"] != "none":      # (checkpoints of default runs stay what they were)
            d["run_state"]["return_norm"] = e.return_norm_state()
        if self.critic_head != "normal":
            d["run_state"]["critic_head"] = self._critic_head_record()
        if self.reward_head != "normal":
            d["run_state"]["reward_head"] = self._reward_head_record()
        if self.symlog_observations:
            d["run_state"]["symlog_observations"] = True
        atomic_write(path, lambda fh: torch.save(d, fh))

    def load_run_state(self, path: str) -> Dict[str, Any]:
        """Restore the ``run_state`` of a checkpoint ``save`` wrote -- the four generators and the engine's noise state,
        exactly as saved -- and return its ``extra``.  Weights and optimisers are ``load``'s (``models=<file>``), the replay
        is ``buffer.load``'s; call this last, after everything that draws random numbers while the agent is set up.
        ValueError for a checkpoint without ``run_state`` (the reference's files, and files older than this key).
        Data-parallel runs: a COLLECTIVE, as ``save`` is."""
        from .checkpoint import read_run_state, restore_generators
        rs = read_run_state(path)
        self.engine.load_noise_state(rs["noise"])
        if self.engine.hp["return_normalization"] != "none":     # a checkpoint without the key: the empty state
            self.engine.load_return_norm_state(rs.get("return_norm") or dict(lo=0.0, hi=0.0, count=0.0, skipped=0.0))
        restore_generators(rs["generators"], self.device)
        return dict(rs["extra"])

    # ---------------------------------------------------------------------------------------- replicas
    def fingerprint(self) -> Dict[str, Tuple[int, int]]:
        """{"actor.flat": (hash, nonfinite), ...}: a 64-bit fingerprint of the bit patterns and the number of non-finite
        elements of every flat buffer the agent owns (weights and Adam moments of the three optimisers, the critic target),
        computed on the device in one launch (bd_fingerprint).  Two agents with equal dicts are bit-identical.  Synchronises;
        data-parallel: a COLLECTIVE, as ``save`` is (it issues the held-back optimiser steps)."""
        words, names = self.engine.fingerprint()
        w = words.cpu().numpy().view("uint64")
        return {f"{g}.{b}": (int(w[i, 0]), int(w[i, 1])) for i, (g, b) in enumerate(names)}

    def check_replicas(self) -> Dict[str, Any]:
        """Do all ranks hold the same weights, Adam moments and step counts?  {"agree", "mismatch", "nonfinite"}, the same
        on every rank; a synchronous COLLECTIVE.  One rank: the non-finite counts only."""
        return self.engine.check_replicas()

    def sync_replicas(self, src: int = 0) -> None:
        """Make every rank a bit-identical copy of rank `src` (weights, optimiser state, everything packed from them).
        A synchronous COLLECTIVE."""
        self.engine.sync_replicas(src)

    def return_norm_state(self) -> Dict[str, float]:
        """The running range of ``ActorCritic.return_normalization=percentile``: {"lo", "hi", "count", "skipped"}."""
        return self.engine.return_norm_state()

    def load_return_norm_state(self, state: Dict[str, float]) -> None:
        self.engine.load_return_norm_state(state)

    def eval(self) -> None:      # no dropout / batch-norm anywhere on the path
        pass

    def train(self) -> None:
        pass

    # ---------------------------------------------------------------------------------------- replay
    def randomly_initialize_replay_buffer(self) -> Tuple[int, int]:
        """src/planet.py:136-159."""
        total_steps, s = 0, 0
        while total_steps < self.seed_steps:
            done, t = False, 0
            observation = self.env.reset()
            while not done:
                action = self.env.sample_random_action()
                next_observation, reward, done = self.env.step(action)
                self.buffer.append(observation, action, reward, done)
                observation = next_observation
                t += 1
            s += 1
            total_steps += t * self.action_repeat
        self.env.close()
        return total_steps, s

    # ---------------------------------------------------------------------------------------- training
    def train_step(self) -> Dict[str, float]:
        """src/dreamer.py:253-393.  Returns the reference's log dict."""
        obs, actions, rewards, nonterminals = self.buffer.sample(self.batch_size, self.seq_len)
        batch = {"observations": obs, "actions": actions, "rewards": rewards, "nonterminals": nonterminals}
        if os.environ.get("BD_LAZY_LOGS", "1") == "0":       # eager: every call waits for the GPU, like the reference's .item()
            logs = self.engine.train_step(batch)
            return {k: v for k, v in logs.items() if not k.startswith("grad_norm_")}
        # Lazy mapping with the reference's keys: values are fetched when a key is first read, so the collect loop's burst
        # `for _ in range(collect_interval): logs = model.train_step()` (src/main.py:105-108) keeps the cross-step
        # pipeline full and only the dict it actually reads waits for the device.
        logs = self.engine.train_step(batch, sync_logs="lazy")
        logs._drop = ("grad_norm_",)        # the optimisers' totals; the per-module "grad_norm/<module>" of a diagnosed step stay
        return logs

    def set_diagnostics(self, interval: int = 0) -> None:
        """Training diagnostics in the log dict of every `interval`-th train step (0 = off; diagnostics.py has the keys)."""
        self.engine.set_diagnostics(interval)

    @property
    def diagnostics_interval(self) -> int:
        return self.engine.diagnostics_interval

    def update_critic(self) -> None:
        self.engine.update_critic()

    @torch.no_grad()
    def value(self, belief: Tensor, state: Tensor, target: bool = False) -> Tensor:
        """The critic's (target=True: the target critic's) value of (belief, state), (..., 1): what the module returns
        with critic_head="normal", the decoded logits -- symexp of the softmax mean over the bins, bd_twohot_decode --
        with "twohot", where ``critic`` / ``critic_target`` themselves return the logits (..., K)."""
        out = (self.critic_target if target else self.critic)(belief, state)
        if self.critic_head == "normal":
            return out
        lead, K = out.shape[:-1], self.critic_bins
        logits = out.reshape(-1, K).contiguous()
        val = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
        return self.engine.twohot_decode(logits, logits.shape[0], val).view(*lead, 1)

    @torch.no_grad()
    def reward(self, belief: Tensor, state: Tensor) -> Tensor:
        """The reward model's prediction for (belief, state), (..., 1): what the module returns with reward_head="normal",
        the decoded logits -- symexp of the softmax mean over the bins, bd_twohot_decode -- with "twohot", where
        ``reward_model`` itself returns the logits (..., K)."""
        out = self.reward_model(belief, state)
        if self.reward_head == "normal":
            return out
        lead, K = out.shape[:-1], self.reward_bins
        logits = out.reshape(-1, K).contiguous()
        val = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
        return self.engine.twohot_decode(logits, logits.shape[0], val, head="reward").view(*lead, 1)

    def encoder_input(self, observation: Tensor) -> Tensor:
        """What the encoder reads for `observation` (on the device): the observation itself, or -- symlog_observations --
        symlog of it in a fresh tensor (bd_symlog); the caller's tensor is never modified."""
        obs = observation.to(self.device)
        if not self.symlog_observations:
            return obs
        obs = obs.float().contiguous()
        self.engine.join()
        return self.engine.symlog(obs, torch.empty_like(obs))

    # ---------------------------------------------------------------------------------------- acting / imagination
    @torch.no_grad()
    def imagine_ahead(self, prev_state: Tensor, prev_belief: Tensor, _noise: Optional[Dict[str, Tensor]] = None):
        """src/dreamer.py:179-237: (seq,batch,S), (seq,batch,Be) -> beliefs (H-1,N,Be), prior_states (H-1,N,S),
        (prior_means, prior_stds), action_entropy (H-1,N)."""
        e, d = self.engine, self.dims
        e.join()
        N = prev_state.shape[0] * prev_state.shape[1]
        start = torch.cat([prev_belief.reshape(N, d.Be), prev_state.reshape(N, d.S)], dim=1).contiguous().float()
        Hm = self.planning_horizon - 1
        noise = _noise or dict(self._action_draw(Hm, N), img_prior=self._state_draw(Hm, N))
        ifeat, ent, _ = e.imagine(start, N, Hm, noise, save=False, tag="api_")
        f = ifeat.view(Hm, N, d.Be + d.S)
        if d.categorical:
            params = (e._buf["api_iprior_logits"].view(Hm, N, d.cat_D, d.cat_C).clone(),)
        else:
            params = (e._buf["api_iprior_mean"].view(Hm, N, d.S).clone(), e._buf["api_iprior_std"].view(Hm, N, d.S).clone())
        return f[..., :d.Be].clone(), f[..., d.Be:].clone(), params, ent.view(Hm, N).clone()

    def _state_draw(self, steps: int, rows: int) -> Tensor:
        """Noise of one state sample per row: standard normals (Gaussian latents) or the sampler's Exp(1) variates per
        class (Categorical; the one-step get_action path never looks at them)."""
        t = torch.empty(steps, rows, self.dims.S, device=self.engine.dev)
        return t.exponential_() if self.dims.categorical else t.normal_()

    def _action_draw(self, steps: int, rows: int) -> Dict[str, Tensor]:
        """Noise of the actor's samples: standard normals and the entropy estimator's draws (tanh-Normal), or the
        sampler's Exp(1) variates per class (Categorical: the entropy is exact)."""
        e, d = self.engine, self.dims
        if d.discrete_actions:
            return {"action": torch.empty(steps, rows, d.A, device=e.dev).exponential_()}
        return {"action": torch.randn(steps, rows, d.A, device=e.dev),
                "entropy": torch.randn(steps, d.n_entropy, rows, d.A, device=e.dev)}

    @torch.no_grad()
    def get_action(self, belief: Tensor, state: Tensor, deterministic: bool = False,
                   _noise: Optional[Dict[str, Tensor]] = None) -> Tuple[Tensor, Tensor]:
        """src/dreamer.py:429-444: tanh-Normal sample and its 100-sample entropy estimate.  Categorical actor: the
        straight-through one-hot sample (src/models.py:518-522) and the exact entropy; deterministic: the one-hot mode."""
        e, d = self.engine, self.dims
        e.join()
        N = belief.shape[0]
        if d.discrete_actions:
            start = torch.cat([belief, state], dim=1).contiguous().float()
            if deterministic:       # q = 1 for every class: argmax(p / q) is argmax p, the first maximum winning
                noise = {"action": torch.ones(1, N, d.A, device=e.dev)}
            else:
                noise = {"action": _noise["action"].to(e.dev).float().reshape(1, N, d.A).contiguous()} if _noise \
                    else self._action_draw(1, N)
            noise["img_prior"] = torch.ones(1, N, d.S, device=e.dev)
            _, ent, act = e.imagine(start, N, 1, noise, save=False, tag="act_")
            act = act.view(N, d.A)
            if deterministic:
                act = torch.nn.functional.one_hot(act.argmax(-1), d.A).float()
            return act.clone(), ent.view(N).clone()
        if deterministic:
            # SampleDist.mode (src/models.py:709-723): of n_samples draws, the one with the highest log-density per row;
            # then the entropy estimate on fresh draws (RNG order: mode, entropy).  Never used by the reference loop --
            # a few elementwise torch ops on the actor's (mean, std), entropy from the same kernel as below.
            mean, std = self.actor(belief, state)
            nz = _noise or {}
            eps = nz["mode"].to(e.dev).float() if "mode" in nz else torch.randn(d.n_entropy, N, d.A, device=e.dev)
            sample = torch.tanh(mean.unsqueeze(0) + std.unsqueeze(0) * eps)
            idx = torch.argmax(_tanh_normal_log_prob(sample, mean.unsqueeze(0), std.unsqueeze(0)), dim=0)
            action = torch.gather(sample, 0, idx.reshape(1, N, 1).expand(1, N, d.A)).squeeze(0)
            start = torch.cat([belief, state], dim=1).contiguous().float()
            noise = {"action": torch.zeros(1, N, d.A, device=e.dev),
                     "entropy": (nz["entropy"].to(e.dev).float().reshape(1, d.n_entropy, N, d.A) if "entropy" in nz
                                 else torch.randn(1, d.n_entropy, N, d.A, device=e.dev)),
                     "img_prior": torch.ones(1, N, d.S, device=e.dev)}
            _, ent, _ = e.imagine(start, N, 1, noise, save=False, tag="act_")
            return action, ent.view(N).clone()
        start = torch.cat([belief, state], dim=1).contiguous().float()
        noise = _noise or {"action": torch.randn(1, N, d.A, device=e.dev),
                           "entropy": torch.randn(1, d.n_entropy, N, d.A, device=e.dev),
                           "img_prior": torch.ones(1, N, d.S, device=e.dev)}       # the unused prior sample's draws
        _, ent, act = e.imagine(start, N, 1, noise, save=False, tag="act_")   # one step: actor + sample (+ unused prior)
        return act.view(N, d.A).clone(), ent.view(N).clone()

    @property
    def act_fused(self) -> bool:
        """Whether update_belief_and_act goes through act_step: the configuration is one bd_act_step takes and the switch
        BD_ACT_FUSED (default 1, README) is not 0."""
        return os.environ.get("BD_ACT_FUSED", "1") != "0" and self.engine.act_step_supported

    @torch.no_grad()
    def act_step(self, belief: Tensor, posterior_state: Tensor, action: Tensor, observation: Tensor, explore: bool = False,
                 _noise: Optional[Dict[str, Tensor]] = None, action_mode: str = "sample",
                 state_mean: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """The decision of update_belief_and_act (src/planet.py:370-403 with get_action, src/dreamer.py:429-444) without
        the environment, in one kernel launch (bd_act_step): (belief, posterior state, previous action, observation) ->
        (belief, posterior state, action), all on the device.  Pixel observations go through the conv encoder first.
        `_noise`: the composed path's keys "post" (B,S), "action" (B,A) and, with explore, "explore" (B,A); "prior" and
        "entropy" are accepted and ignored (their draws feed nothing that is returned).  Without it the draws come from
        the engine's Philox streams.  The results are engine buffers, valid until the call after the next one.
        `action_mode`, `state_mean`: the evaluation policy (update_belief_and_act); "mode" reads `_noise`'s "mode"
        (n_entropy,B,A), the layout of get_action's."""
        _check_action_mode(action_mode)
        obs, emb = self._act_inputs(self.engine.act_step_supported, observation,
                                    "act_step: the fused acting kernel takes Gaussian latents and the tanh-Normal actor at sizes "
                                    "bd_act_step_supported accepts ({config}); use update_belief_and_act, which composes the "
                                    "step from the scan kernels")
        return self.engine.act_step(belief, posterior_state, action, obs=obs, embedding=emb, explore=bool(explore),
                                    action_noise=self.action_noise, noise=_noise, action_mode=action_mode,
                                    state_mean=bool(state_mean))

    def _act_inputs(self, supported: bool, observation: Tensor, refusal: str):
        """The preamble of act_step / act_step_cat: refuse an unsupported configuration (`refusal`, its {config} filled in
        here), then the observation on the device as (obs, None), or -- pixels -- (None, its conv embedding)."""
        if not supported:
            d = self.dims
            raise NotImplementedError(refusal.format(
                config=f"latent_distribution={self.latent_distribution}, action_distribution={self.action_distribution}, "
                       f"dims {d.Be}/{d.S}/{d.A}/{d.Hd}/{d.E}"))
        obs = observation.to(self.device)
        return (None, self.encoder(obs)) if self.pixel_observation else (obs, None)

    @property
    def act_fused_cat(self) -> bool:
        """Whether update_belief_and_act goes through act_step_cat: Categorical latents and / or the Categorical actor at
        sizes bd_act_step_cat takes, and the switch BD_ACT_FUSED_CAT (default 0, README; read at every call) is 1."""
        return os.environ.get("BD_ACT_FUSED_CAT", "0") == "1" and self.engine.act_step_cat_supported

    @torch.no_grad()
    def act_step_cat(self, belief: Tensor, posterior_state: Tensor, action: Tensor, observation: Tensor, explore: bool = False,
                     _noise: Optional[Dict[str, Tensor]] = None, action_mode: str = "sample",
                     state_mean: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """act_step for latent_distribution=Categorical and / or action_distribution=Categorical (bd_act_step_cat): the
        decision of update_belief_and_act without the environment, in one kernel launch.  Pixel observations go through the
        conv encoder first.  `_noise`: the composed path's keys "post" (B,S), "action" (B,A) and, with explore, "explore"
        (B,A) (tanh-Normal actor) or "explore_u" (B,) uniforms and "explore_k" (B,) classes (Categorical actor; the kernel
        gets v = (k + 0.5) / A, whose class is k); "prior" and "entropy" are accepted and ignored.  Without it the draws come
        from the engine's Philox streams.  The results are engine buffers, valid until the call after the next one.
        `action_mode`, `state_mean`: the evaluation policy, as act_step."""
        _check_action_mode(action_mode)
        d = self.dims
        obs, emb = self._act_inputs(self.engine.act_step_cat_supported, observation,
                                    "act_step_cat: the fused acting kernel takes Categorical latents and / or the Categorical "
                                    "actor at sizes bd_act_step_cat_supported accepts ({config}); Gaussian latents with the "
                                    "tanh-Normal actor use act_step, everything else update_belief_and_act, which composes "
                                    "the step from the scan kernels")
        nz = _noise
        if nz is not None:
            nz = {k: nz[k] for k in ("post", "action", "mode") if k in nz}
            if explore and d.discrete_actions:
                u, k = _noise["explore_u"].to(self.device).float(), _noise["explore_k"].to(self.device).float()
                nz["explore"] = torch.stack([u, (k + 0.5) / d.A], dim=1)
            elif explore:
                nz["explore"] = _noise["explore"]
        return self.engine.act_step_cat(belief, posterior_state, action, obs=obs, embedding=emb, explore=bool(explore),
                                        action_noise=self.action_noise, noise=nz, action_mode=action_mode,
                                        state_mean=bool(state_mean))

    @torch.no_grad()
    def update_belief_and_act(self, env, belief, posterior_state, action, observation, explore=False,
                              _noise: Optional[Dict[str, Tensor]] = None, action_mode: str = "sample",
                              state_mean: bool = False):
        """src/planet.py:370-403.  (Data-parallel runs: issues any held-back actor update first -- a collective, call on
        every rank, as the collect loop does.)  Where act_fused holds the decision is one launch (act_step), and so it is
        where act_fused_cat holds (act_step_cat; BD_ACT_FUSED_CAT=1, off by default); the code below composes it from the
        encoder chain, a one-step observe scan and a one-step imagination otherwise.
        The evaluation policy (Dreamer v1 / v2 evaluate with the actor's mode, v2 optionally with the posterior mean):
        `action_mode` "sample" (the reference's loop), "mode" -- tanh-Normal actor: SampleDist.mode, of n_entropy draws
        (`_noise`'s "mode" (n_entropy,B,A)) the one with the largest log-density, the first maximum winning; Categorical
        actor: the exact one-hot of argmax p -- or "mean" -- tanh(mean), no draw; Categorical actor: as "mode".
        `state_mean`: the posterior's mean (Gaussian latents) or per-factor argmax (Categorical) instead of a sample.
        Exploration, where asked for, is applied on top as before.  Every route honours them; another `action_mode` is a
        ValueError."""
        _check_action_mode(action_mode)
        if self.act_fused or self.act_fused_cat:
            step = self.act_step if self.act_fused else self.act_step_cat
            belief, posterior_state, action = step(belief, posterior_state, action, observation, explore=explore, _noise=_noise,
                                                   action_mode=action_mode, state_mean=state_mean)
            batched = hasattr(env, "n") and hasattr(env, "envs")          # EnvBatcher (src/env.py:343)
            next_observation, reward, done = env.step(action.cpu() if batched else action[0].cpu())
            return belief, posterior_state, action, next_observation, reward, done
        self.engine.flush_optimizers()
        # `_noise` (parity tests): the reference's draws in its RNG order -- "prior" (B,S), "post" (B,S), "action" (B,A),
        # "entropy" (100,B,A), and with explore "explore" (B,A)
        nz = _noise
        embedding = self.encoder(self.encoder_input(observation)).unsqueeze(dim=0)
        B = belief.shape[0]
        if state_mean:
            # the mean of the posterior: its sample at zero normal noise, or -- Categorical -- at q = 1 for every class
            fixed = (torch.ones if self.dims.categorical else torch.zeros)(1, B, self.state_size, device=self.device)
            state_noise = (fixed if nz is None or "prior" not in nz else nz["prior"].unsqueeze(0), fixed)
        else:
            state_noise = None if nz is None else (nz["prior"].unsqueeze(0), nz["post"].unsqueeze(0))
        belief, _, _, posterior_state, _ = self.transition_model(
            posterior_state, action.unsqueeze(dim=0), belief, embedding, _noise=state_noise)
        belief, posterior_state = belief.squeeze(dim=0), posterior_state.squeeze(dim=0)
        if action_mode == "sample":
            action, _ = self.get_action(belief, posterior_state, _noise=None if nz is None else dict(
                {k: nz[k].unsqueeze(0).contiguous() for k in ("action", "entropy") if k in nz},
                img_prior=torch.ones(1, B, self.state_size, device=self.device)))
        elif self.dims.discrete_actions:
            action, _ = self.get_action(belief, posterior_state, deterministic=True)      # the exact one-hot of argmax p
        else:
            mean, std = self.actor(belief, posterior_state)
            if action_mode == "mode":
                action, _ = self.engine.tanh_normal_mode(mean, std, None if nz is None else nz["mode"])
            else:       # tanh(mean) as the sampling kernels form it: zero action noise (one draw for the unread entropy)
                action, _ = self.get_action(belief, posterior_state, _noise={
                    "action": torch.zeros(1, B, self.action_size, device=self.device),
                    "entropy": torch.zeros(1, 1, B, self.action_size, device=self.device).expand(
                        1, self.dims.n_entropy, B, self.action_size).contiguous(),
                    "img_prior": torch.ones(1, B, self.state_size, device=self.device)})
        if explore and self.dims.discrete_actions:
            # epsilon-greedy: with probability action_noise a uniformly random one-hot (Gaussian noise would leave the
            # simplex); `_noise`: "explore_u" (B,) uniforms, "explore_k" (B,) classes
            B, A = action.shape
            u = torch.rand(B, device=action.device) if nz is None else nz["explore_u"].to(action.device)
            k = torch.randint(A, (B,), device=action.device) if nz is None else nz["explore_k"].to(action.device)
            rnd = torch.nn.functional.one_hot(k.long(), A).to(action.dtype)
            action = torch.where((u < self.action_noise).unsqueeze(1), rnd, action)
        elif explore:
            eps = torch.randn_like(action) if nz is None else nz["explore"]
            action = torch.clamp(action + self.action_noise * eps, -1, 1)
        batched = hasattr(env, "n") and hasattr(env, "envs")          # EnvBatcher (src/env.py:343)
        next_observation, reward, done = env.step(action.cpu() if batched else action[0].cpu())
        return belief, posterior_state, action, next_observation, reward, done

    # ---------------------------------------------------------------------------------------- evaluation
    def evaluate(self, envs=None, episodes: Optional[int] = None, video: bool = False, _noise=None,
                 action_mode: Optional[str] = None, state_mean: Optional[bool] = None) -> Dict[str, Any]:
        """The reference's test loop (src/main.py:191-283; evaluate.run_evaluation): `episodes` (default
        ``test_episodes``) environments side by side for at most max_episode_length // action_repeat decisions without
        exploration noise.  Returns Eval_{min,avg,max,std}_return, ``returns``, ``steps`` and ``video`` -- uint8 (steps, 3,
        GH, GW) real-vs-predicted frames, pixel observations only, else None.  `envs`: an EnvBatcher to use instead of a
        fresh one.  Data-parallel runs: update_belief_and_act carries collectives, so every rank calls this.
        `action_mode` / `state_mean`: the evaluation policy of update_belief_and_act; None takes the config's
        ``eval_action`` ('sample') / ``eval_state_mean`` (false).  With "mean" (or a Categorical actor's "mode") and
        state_mean the decisions draw nothing: two evaluations of one agent on the same environments return the same."""
        from .env import Env, EnvBatcher
        from .evaluate import run_evaluation
        action_mode = self.params.get("eval_action", "sample") if action_mode is None else action_mode
        state_mean = bool(self.params.get("eval_state_mean", False)) if state_mean is None else bool(state_mean)
        _check_action_mode(action_mode)
        if envs is None:
            envs = EnvBatcher(Env, self.params, int(episodes or self.params["test_episodes"]))
        max_steps = int(self.params["max_episode_length"]) // int(self.action_repeat)
        return run_evaluation(self, envs, max_steps, video=bool(video) and self.pixel_observation, _noise=_noise,
                              action_mode=action_mode, state_mean=state_mean)

    # ---------------------------------------------------------------------------------------- open-loop prediction
    def open_loop(self, batch=None, sequences: int = 6, context: int = 5, video: Optional[bool] = None,
                  _noise=None) -> Dict[str, Any]:
        """The open-loop prediction diagnostic (DreamerV1's image_summaries, DreamerV2's video_pred; openloop.run_open_loop):
        `sequences` replay sequences of ``seq_len`` records are filtered on their first `context` steps, then the prior runs
        on on the recorded actions alone, and every step is decoded.  Returns ``openl_obs_mse`` -- (T,) float32, T =
        seq_len - 1: per step the mean of (model - truth)^2 --, ``openl_mse_context`` and ``openl_mse_open`` (floats, its
        means over steps < context and >= context), ``context``, ``video`` -- uint8 (T, 3, 192, 64 sequences): truth over
        model over error per sequence, pixel observations only (`video=None`: yes for those), else None -- and the decoded
        ``beliefs`` / ``states`` (device tensors).  `batch`: a time-major batch as ``buffer.sample(n, L)`` returns it; None
        draws ``buffer.sample(sequences, seq_len)``, which advances the replay's index RNG and the pixel dequantisation
        counter as any sample does (a training run that calls this samples different batches afterwards than one that does
        not).  No collectives: in a data-parallel run rank 0 alone may call it."""
        from .openloop import check_open_loop, run_open_loop
        if batch is None:
            check_open_loop(int(self.seq_len), int(sequences), int(context))
            batch = self.buffer.sample(int(sequences), int(self.seq_len))
        return run_open_loop(self, batch, int(context), video=video, _noise=_noise)


class DreamerV2(Dreamer):
    """src/dreamerV2.py:13-25: Dreamer with the V2 KL settings (balanced KL; kl_loss_weight 1.0 is replaced by 0.1);
    ``latent_distribution=Categorical`` selects the 32 x 32 discrete latents (BASELINE configs[4])."""

    def __init__(self, params: Dict[str, Any], env, **kw):
        p = dict(params)
        if p.get("kl_loss_weight") == 1.0:
            p["kl_loss_weight"] = 0.1
        super().__init__(p, env, **kw)
        self.kl_balance = p["kl_balance"]


def _check_action_mode(action_mode) -> None:
    if action_mode not in ACTION_MODES:
        raise ValueError(f"action_mode {action_mode!r} is none of {ACTION_MODES}")


def _tanh_normal_log_prob(y: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """Independent(TransformedDistribution(Normal(mean, std), TanhBijector()), 1).log_prob(y) (src/models.py:630-673)."""
    import math
    yc = torch.where(torch.abs(y) <= 1.0, torch.clamp(y, -0.99999997, 0.99999997), y)
    x = 0.5 * torch.log((1 + yc) / (1 - yc))
    ladj = 2.0 * (math.log(2) - x - torch.nn.functional.softplus(-2.0 * x))
    base = -((x - mean) ** 2) / (2 * std ** 2) - torch.log(std) - math.log(math.sqrt(2 * math.pi))
    return (base - ladj).sum(-1)


def lambda_return(imged_reward: Tensor, value_pred: Tensor, bootstrap: Tensor, discount: float = 0.99,
                  lambda_: float = 0.95) -> Tensor:
    """src/dreamer.py:447-471 on the GPU (bd_lambda_return_forward).  The kernel takes the bootstrap from the
    last value row, as the only call site does (``bootstrap=value_pred[-1]``, src/dreamer.py:332)."""
    if not torch.equal(bootstrap, value_pred[-1]):
        raise NotImplementedError("bootstrap must be value_pred[-1] (the reference's only use)")
    Hm = imged_reward.shape[0]
    N = imged_reward[0].numel()
    r, v = imged_reward.contiguous().float(), value_pred.contiguous().float()
    out = torch.empty_like(r)
    cabi.check(cabi.lib.bd_lambda_return_forward(r.data_ptr(), v.data_ptr(), Hm, N, discount, lambda_, out.data_ptr(),
                                                 cabi.stream()))
    return out


# -------------------------------------------------------------------------------------------------
# PyTorch-default initialisation of the reference's modules (shapes: src/models.py, src/utils.py:368-404)
def _ref_init_dense(i: int, h: int, o: int) -> torch.nn.Module:
    from torch import nn
    layers, k = [], i
    for _ in range(4):
        layers += [nn.Linear(k, h), nn.ELU()]
        k = h
    layers += [nn.Linear(k, o), nn.Identity()]
    m = nn.Module()
    m.model = nn.Sequential(*layers)
    return m


def _ref_init_cnn(E: int) -> torch.nn.Module:
    from torch import nn
    m = nn.Module()
    m.model = nn.Sequential(nn.Conv2d(3, 32, 4, 2), nn.ELU(), nn.Conv2d(32, 64, 4, 2), nn.ELU(), nn.Conv2d(64, 128, 4, 2),
                            nn.ELU(), nn.Conv2d(128, 256, 4, 2), nn.ELU(), nn.Flatten(),
                            nn.Identity() if E == 1024 else nn.Linear(1024, E))
    return m


def _ref_init_decoder(feat: int, E: int) -> torch.nn.Module:
    from torch import nn
    m = nn.Module()
    m.decoder = nn.Sequential(nn.Linear(feat, E), nn.Identity(), nn.ConvTranspose2d(E, 128, 5, 2), nn.ELU(),
                              nn.ConvTranspose2d(128, 64, 5, 2), nn.ELU(), nn.ConvTranspose2d(64, 32, 6, 2), nn.ELU(),
                              nn.ConvTranspose2d(32, 3, 6, 2))
    return m


def _ref_init_transition(d: Dims) -> torch.nn.Module:
    from torch import nn
    from .models import CategoricalBeliefHolder, GaussianBeliefHolder
    m = nn.Module()
    m.rnn = nn.GRUCell(d.Be, d.Be)
    m.fc_embed_state_action = nn.Sequential(nn.Linear(d.S + d.A, d.Be), nn.ELU())
    if d.categorical:
        m.belief_prior = CategoricalBeliefHolder(d.Be, d.Hd, d.cat_D, d.cat_C)
        m.belief_posterior = CategoricalBeliefHolder(d.Be + d.E, d.Hd, d.cat_D, d.cat_C)
    else:
        m.belief_prior = GaussianBeliefHolder(d.Be, d.Hd, d.S, 0.1)
        m.belief_posterior = GaussianBeliefHolder(d.Be + d.E, d.Hd, d.S, 0.1)
    return m
