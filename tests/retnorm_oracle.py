"""TEST INFRASTRUCTURE: CPU restatement of the actor objective with percentile return normalisation
(``ActorCritic.return_normalization = percentile``; DESIGN.md, "Return normalisation") on top of
tests/mixing_oracle.py (tanh-Normal actor) and tests/discrete_oracle.py (Categorical actor).  Plain torch fp32 with
autograd; the running range is tests/retnorm_ref.py.

With rho, w, l, b, eta as in tests/mixing_oracle.py and S = max(floor, hi - lo) of the range as it stands BEFORE the step
(fp32):

    obj[k, n]  = w * (rho * R / S + (1 - rho) * l * sg(R - b) / S + eta * ent)
    actor_loss = -mean obj

Only the actor changes: the critic's target, value_loss and the world model read the raw R.  After the step's returns
exist they update the range (retnorm_ref.update).  hp: return_norm_low / high / decay / floor (defaults 0.05, 0.95, 0.99, 1).
"""
from __future__ import annotations

import torch

from oracle import dreamer_oracle as O
from tests import retnorm_ref
from tests.discrete_oracle import DiscreteOracleDreamer, discrete_imagine_ahead
from tests.mixing_oracle import MixingOracleDreamer, mixing_rho, tanh_normal_log_density

RN_DEFAULTS = dict(return_norm_low=0.05, return_norm_high=0.95, return_norm_decay=0.99, return_norm_floor=1.0)


class _RangeMixin:
    """The running range and what both restatements do with it."""

    def _rn_hp(self, key):
        return self.hp.get(key, RN_DEFAULTS[key])

    def rn_begin(self):
        """(S as a Python float of the fp32 scale, log entries) of the step about to run."""
        if not hasattr(self, "rn_state"):
            self.rn_state = retnorm_ref.empty_state()
        S = retnorm_ref.scale(self.rn_state, self._rn_hp("return_norm_floor"))
        return float(S), dict(return_scale=float(S), return_p_low=float(self.rn_state["lo"]),
                              return_p_high=float(self.rn_state["hi"]))

    def rn_end(self, returns):
        x = returns.detach().numpy().reshape(-1)
        k_lo, k_hi = retnorm_ref.ranks(x.size, self._rn_hp("return_norm_low"), self._rn_hp("return_norm_high"))
        self.rn_state = retnorm_ref.update(self.rn_state, x, k_lo, k_hi, self._rn_hp("return_norm_decay"))

    def _world_model_update(self, batch, noise, logs, keep):
        hp = self.hp
        model_loss, obs_loss, rew_loss, kl, inter = self.world_model_forward(batch, noise)
        logs.update(observation_loss=obs_loss.item(), reward_loss=rew_loss.item(), kl_loss=kl.item(),
                    model_loss=model_loss.item())
        if self._discount_loss is not None:
            logs["discount_loss"] = self._discount_loss.item()
        grads = torch.autograd.grad(model_loss, self.model_params, allow_unused=True)
        grads = [torch.zeros_like(p) if g is None else g.clone() for g, p in zip(grads, self.model_params)]
        model_grads = [g.clone() for g in grads] if keep else None
        gn_model = O.clip_grad_norm_(grads, hp["grad_clip_norm"])
        O.adam_step(self.model_params, grads, self.opt["model"], hp["model_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        return inter, model_grads, gn_model

    def _discount_weights(self, Pf, img_b, img_s):
        if not self.use_discount:
            return None
        with torch.no_grad():
            dl = O.dense_on_features(img_b, img_s, Pf["discount_model"])
            arr = self.hp["discount"] * torch.round(torch.sigmoid(dl))
            arr[:, 0, 0] = 1.0
            return torch.cumprod(arr, 0)

    def _actor_and_critic_updates(self, actor_loss, img_b, img_s, returns, wts, logs, keep):
        hp, P = self.hp, self.P
        agrads = [g.clone() for g in torch.autograd.grad(actor_loss, self.actor_params)]
        actor_grads = [g.clone() for g in agrads] if keep else None
        gn_actor = O.clip_grad_norm_(agrads, hp["grad_clip_norm"])
        O.adam_step(self.actor_params, agrads, self.opt["actor"], hp["actor_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        v = O.dense_on_features(img_b.detach(), img_s.detach(), P["critic"])
        nll = 0.5 * (returns.detach() - v) ** 2 + O.HALF_LOG_2PI          # the raw returns
        value_loss = (wts * nll).mean() if wts is not None else nll.mean()
        logs.update(value_loss=value_loss.item())
        cgrads = [g.clone() for g in torch.autograd.grad(value_loss, self.critic_params)]
        critic_grads = [g.clone() for g in cgrads] if keep else None
        gn_critic = O.clip_grad_norm_(cgrads, hp["grad_clip_norm"])
        O.adam_step(self.critic_params, cgrads, self.opt["critic"], hp["value_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        return actor_grads, critic_grads, gn_actor, gn_critic

    def _frozen(self):
        Pf = dict(self.P)
        for mod in self.model_modules + ("critic_target",):
            Pf[mod] = {k: v.detach() for k, v in self.P[mod].items()}
        return Pf


class RetnormOracleDreamer(_RangeMixin, MixingOracleDreamer):
    """MixingOracleDreamer with the returns of the actor objective divided by the running range's scale."""

    def train_step(self, batch_np, noise_np, keep: bool = True):
        hp, P = self.hp, self.P
        rho = mixing_rho(hp)
        batch = {k: torch.as_tensor(v) for k, v in batch_np.items()}
        noise = {k: torch.as_tensor(v) for k, v in noise_np.items()}
        logs = {}
        S, rn_logs = self.rn_begin()
        inter, model_grads, gn_model = self._world_model_update(batch, noise, logs, keep)
        beliefs, post_states = inter["beliefs"].detach(), inter["posterior_states"].detach()
        Pf = self._frozen()
        img_b, img_s, _, ent = O.imagine_ahead(Pf, post_states, beliefs, hp["planning_horizon"], noise["action"],
                                               noise["entropy"], noise["img_prior"], self.cat)
        img_reward = O.dense_on_features(img_b, img_s, Pf["reward_model"])
        value_pred = O.dense_on_features(img_b, img_s, Pf["critic_target"])
        returns = O.lambda_return(img_reward, value_pred, value_pred[-1], hp["discount"], hp["disclam"])
        Hm, N = img_b.shape[0], img_b.shape[1]
        start_b, start_s = beliefs.reshape(N, -1), post_states.reshape(N, -1)
        fb = torch.cat([start_b[None], img_b[:-1]], 0).reshape(Hm * N, -1).detach()
        fs = torch.cat([start_s[None], img_s[:-1]], 0).reshape(Hm * N, -1).detach()
        mean, std = O.actor_forward(fb, fs, P["actor"])
        u = (mean + std * noise["action"].reshape(Hm * N, -1)).detach()
        logp = tanh_normal_log_density(u, mean, std).reshape(Hm, N, 1)
        b0 = O.dense_on_features(start_b, start_s, Pf["critic_target"]).reshape(1, N, 1)
        adv = (returns - torch.cat([b0, value_pred[:-1]], 0)).detach()
        objective = rho * returns / S + (1 - rho) * logp * adv / S + hp["entropy_weight"] * ent.unsqueeze(-1)
        wts = self._discount_weights(Pf, img_b, img_s)
        if wts is not None:
            objective = wts * objective
        actor_loss = -objective.mean()
        logs.update(actor_loss=actor_loss.item(), policy_entropy=ent.mean().item(), **rn_logs)
        actor_grads, critic_grads, gn_actor, gn_critic = self._actor_and_critic_updates(actor_loss, img_b, img_s, returns,
                                                                                        wts, logs, keep)
        self.rn_end(returns)
        if keep:
            self.last = dict(returns=returns.detach(), advantage=adv, log_prob=logp.detach(), action_entropy=ent.detach(),
                             model_grads=model_grads, actor_grads=actor_grads, critic_grads=critic_grads,
                             grad_norms=dict(model=gn_model.item(), actor=gn_actor.item(), critic=gn_critic.item()))
        return logs


class RetnormDiscreteOracleDreamer(_RangeMixin, DiscreteOracleDreamer):
    """The same on the Categorical actor (tests/discrete_oracle.py): l = norm[k], the exact entropy."""

    def train_step(self, batch_np, noise_np, keep: bool = True):
        hp = self.hp
        rho = mixing_rho(hp)
        batch = {k: torch.as_tensor(v) for k, v in batch_np.items()}
        noise = {k: torch.as_tensor(v) for k, v in noise_np.items()}
        logs = {}
        S, rn_logs = self.rn_begin()
        inter, model_grads, gn_model = self._world_model_update(batch, noise, logs, keep)
        beliefs, post_states = inter["beliefs"].detach(), inter["posterior_states"].detach()
        Pf = self._frozen()
        img_b, img_s, ent, logp, _ = discrete_imagine_ahead(Pf, post_states, beliefs, hp["planning_horizon"],
                                                            noise["action"], noise["img_prior"], self.cat)
        img_reward = O.dense_on_features(img_b, img_s, Pf["reward_model"])
        value_pred = O.dense_on_features(img_b, img_s, Pf["critic_target"])
        returns = O.lambda_return(img_reward, value_pred, value_pred[-1], hp["discount"], hp["disclam"])
        N = img_b.shape[1]
        b0 = O.dense_on_features(beliefs.reshape(N, -1), post_states.reshape(N, -1), Pf["critic_target"]).reshape(1, N, 1)
        adv = (returns - torch.cat([b0, value_pred[:-1]], 0)).detach()
        objective = rho * returns / S + (1 - rho) * logp.unsqueeze(-1) * adv / S + hp["entropy_weight"] * ent.unsqueeze(-1)
        wts = self._discount_weights(Pf, img_b, img_s)
        if wts is not None:
            objective = wts * objective
        actor_loss = -objective.mean()
        logs.update(actor_loss=actor_loss.item(), policy_entropy=ent.mean().item(), **rn_logs)
        actor_grads, critic_grads, gn_actor, gn_critic = self._actor_and_critic_updates(actor_loss, img_b, img_s, returns,
                                                                                        wts, logs, keep)
        self.rn_end(returns)
        if keep:
            self.last = dict(returns=returns.detach(), action_entropy=ent.detach(), model_grads=model_grads,
                             actor_grads=actor_grads, critic_grads=critic_grads,
                             grad_norms=dict(model=gn_model.item(), actor=gn_actor.item(), critic=gn_critic.item()))
        return logs
