"""TEST INFRASTRUCTURE: CPU restatement of the mixed actor gradient (``ActorCritic.gradient_mixing`` = rho; DreamerV2,
eq. 6, its ``actor_grad_mix``) on top of ``oracle.dreamer_oracle.OracleDreamer``.  Plain torch fp32 with autograd.

Slots k = 0 .. Hm-1 over the N = T*B start rows; slot k took a_k = tanh(u_k), u_k = mu_k + sigma_k * eps_k with
(mu_k, sigma_k) = actor(sg f_{k-1}) (f_{-1} = the detached start features), and led to f_k.  With the lambda-return
R_k, the 100-sample entropy ent_k and the cumulative discount weight w_k (use_discount; else 1):

    obj[k, n]  = w_k * (rho * R_k + (1 - rho) * l_k * sg(R_k - b_k) + eta * ent_k)
    l_k        = sum_a [log N(sg u_k; mu_k, sigma_k) - log(1 - tanh^2(sg u_k))]
    b_k        = critic_target(f_{k-1})
    actor_loss = -mean obj

rho = -1 is the reference's objective and equals rho = 1.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import dreamer_oracle as O


def mixing_rho(hp) -> float:
    rho = float(hp.get("gradient_mixing", -1))
    return 1.0 if rho == -1 else rho


def tanh_normal_log_density(u, mean, std):
    """log-density of the tanh-Normal action tanh(u) at the exact pre-tanh sample u, summed over the action dims; the
    Jacobian term in tanh_normal_log_prob's stable form 2 (log 2 - u - softplus(-2u))."""
    base = -((u - mean) ** 2) / (2 * std ** 2) - torch.log(std) - math.log(math.sqrt(2 * math.pi))
    ladj = 2.0 * (math.log(2) - u - F.softplus(-2.0 * u))
    return (base - ladj).sum(-1)


def actor_head(out):
    """ActorModel's head (src/models.py:506-517) on the raw output [rows x 2A] -> mean, std."""
    m, r = torch.chunk(out, 2, dim=-1)
    return O.ACT_MEAN_SCALE * torch.tanh(m / O.ACT_MEAN_SCALE), F.softplus(r + O.RAW_INIT_STD) + O.ACT_MIN_STD


class MixingOracleDreamer(O.OracleDreamer):
    """OracleDreamer with the mixed actor objective; everything else is the parent's step, line by line."""

    def train_step(self, batch_np, noise_np, keep: bool = True):
        hp, P = self.hp, self.P
        rho = mixing_rho(hp)
        batch = {k: torch.as_tensor(v) for k, v in batch_np.items()}
        noise = {k: torch.as_tensor(v) for k, v in noise_np.items()}
        logs = {}
        # ---------------- dynamics learning (as OracleDreamer.train_step) ----------------
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
        # ---------------- behaviour learning ----------------
        beliefs = inter["beliefs"].detach()
        post_states = inter["posterior_states"].detach()
        Pf = dict(P)
        for mod in self.model_modules + ("critic_target",):
            Pf[mod] = {k: v.detach() for k, v in P[mod].items()}
        img_b, img_s, _, ent = O.imagine_ahead(Pf, post_states, beliefs, hp["planning_horizon"], noise["action"],
                                               noise["entropy"], noise["img_prior"], self.cat)
        img_reward = O.dense_on_features(img_b, img_s, Pf["reward_model"])
        value_pred = O.dense_on_features(img_b, img_s, Pf["critic_target"])
        returns = O.lambda_return(img_reward, value_pred, value_pred[-1], hp["discount"], hp["disclam"])
        # REINFORCE: the actor re-run on the detached features each action was taken at, the exact pre-tanh samples
        Hm, N = img_b.shape[0], img_b.shape[1]
        start_b, start_s = beliefs.reshape(N, -1), post_states.reshape(N, -1)
        fb = torch.cat([start_b[None], img_b[:-1]], 0).reshape(Hm * N, -1).detach()
        fs = torch.cat([start_s[None], img_s[:-1]], 0).reshape(Hm * N, -1).detach()
        mean, std = O.actor_forward(fb, fs, P["actor"])
        u = (mean + std * noise["action"].reshape(Hm * N, -1)).detach()
        logp = tanh_normal_log_density(u, mean, std).reshape(Hm, N, 1)
        b0 = O.dense_on_features(start_b, start_s, Pf["critic_target"]).reshape(1, N, 1)
        adv = (returns - torch.cat([b0, value_pred[:-1]], 0)).detach()
        objective = rho * returns + (1 - rho) * logp * adv + hp["entropy_weight"] * ent.unsqueeze(-1)
        wts = None
        if self.use_discount:
            with torch.no_grad():
                dl = O.dense_on_features(img_b, img_s, Pf["discount_model"])
                arr = hp["discount"] * torch.round(torch.sigmoid(dl))
                arr[:, 0, 0] = 1.0
                wts = torch.cumprod(arr, 0)
            objective = wts * objective
        actor_loss = -objective.mean()
        logs.update(actor_loss=actor_loss.item(), policy_entropy=ent.mean().item())
        agrads = [g.clone() for g in torch.autograd.grad(actor_loss, self.actor_params)]
        actor_grads = [g.clone() for g in agrads] if keep else None
        gn_actor = O.clip_grad_norm_(agrads, hp["grad_clip_norm"])
        O.adam_step(self.actor_params, agrads, self.opt["actor"], hp["actor_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        # critic (unchanged)
        v = O.dense_on_features(img_b.detach(), img_s.detach(), P["critic"])
        target = returns.detach()
        nll = 0.5 * (target - v) ** 2 + O.HALF_LOG_2PI
        value_loss = (wts * nll).mean() if wts is not None else nll.mean()
        logs.update(value_loss=value_loss.item())
        cgrads = [g.clone() for g in torch.autograd.grad(value_loss, self.critic_params)]
        critic_grads = [g.clone() for g in cgrads] if keep else None
        gn_critic = O.clip_grad_norm_(cgrads, hp["grad_clip_norm"])
        O.adam_step(self.critic_params, cgrads, self.opt["critic"], hp["value_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        if keep:
            self.last = dict(inter={k: t.detach() for k, t in inter.items()}, imged_beliefs=img_b.detach(),
                             imged_states=img_s.detach(), action_entropy=ent.detach(),
                             imged_reward=img_reward.detach(), value_pred=value_pred.detach(),
                             returns=returns.detach(), critic_value=v.detach(), advantage=adv, log_prob=logp.detach(),
                             model_grads=model_grads, actor_grads=actor_grads, critic_grads=critic_grads,
                             grad_norms=dict(model=gn_model.item(), actor=gn_actor.item(), critic=gn_critic.item()))
        return logs
