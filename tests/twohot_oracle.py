"""TEST INFRASTRUCTURE: CPU restatement of a train step with the two-hot critic (``ActorCritic.critic_head = twohot``;
DESIGN.md, "Two-hot critic") on top of tests/retnorm_oracle.py, hence tests/mixing_oracle.py (tanh-Normal actor) and
tests/discrete_oracle.py (Categorical actor).  Plain torch fp32 with autograd; the head itself is tests/twohot_ref.py
restated in torch so that autograd differentiates it.

critic and critic_target end in K logits.  Wherever the step reads a target value it decodes target logits
(v = symexp(softmax(l) . z)): the imagined values, the REINFORCE baseline.  The dynamics gradient flows through the
decode.  The critic loss is the mean over the Hm x N rows of w_r (logsumexp(l) - (1 - w) l_k - w l_{k+1}) against the
detached lambda-returns, w_r the cumulative discount weights under use_discount.  lambda-returns, the actor objective,
return normalisation (hp return_normalization = "percentile", else the scale is 1 and no range is kept) and the world
model read the decoded values as they read the width-1 critic's.  hp: critic_bins, critic_bin_range.
"""
from __future__ import annotations

import torch

from oracle import dreamer_oracle as O
from tests.discrete_oracle import discrete_imagine_ahead
from tests.mixing_oracle import mixing_rho, tanh_normal_log_density
from tests.retnorm_oracle import RetnormDiscreteOracleDreamer, RetnormOracleDreamer


def bins(K: int, Z: float) -> torch.Tensor:
    return (2 * torch.arange(K) - (K - 1)).to(torch.float32) * (Z / (K - 1))


def symexp(m: torch.Tensor) -> torch.Tensor:
    return torch.sign(m) * torch.expm1(torch.abs(m))


def decode(logits: torch.Tensor, Z: float) -> torch.Tensor:
    """[..., K] -> [..., 1]"""
    z = bins(logits.shape[-1], Z)
    return symexp((torch.softmax(logits, -1) * z).sum(-1, keepdim=True))


def row_loss(logits: torch.Tensor, y: torch.Tensor, Z: float) -> torch.Tensor:
    """[..., K], [..., 1] -> [..., 1]: the cross-entropy against the two-hot encoding of symlog(y)."""
    K = logits.shape[-1]
    t = torch.clamp(torch.sign(y) * torch.log1p(torch.abs(y)), -Z, Z)
    u = (t + Z) / (2 * (Z / (K - 1)))
    k = torch.clamp(torch.floor(u), max=K - 2)
    w = u - k
    k = k.long()
    lk, lk1 = torch.gather(logits, -1, k), torch.gather(logits, -1, k + 1)
    return torch.logsumexp(logits, -1, keepdim=True) - (1 - w) * lk - w * lk1


class _TwohotStep:
    """The train step both restatements share; `discrete` selects the actor."""

    discrete = False

    def value(self, b, s, sd):
        return decode(O.dense_on_features(b, s, sd), self.hp.get("critic_bin_range", 20.0))

    def train_step(self, batch_np, noise_np, keep: bool = True):
        hp, P = self.hp, self.P
        rho = mixing_rho(hp)
        Z = hp.get("critic_bin_range", 20.0)
        batch = {k: torch.as_tensor(v) for k, v in batch_np.items()}
        noise = {k: torch.as_tensor(v) for k, v in noise_np.items()}
        logs = {}
        norm = hp.get("return_normalization", "none") == "percentile"
        S, rn_logs = self.rn_begin() if norm else (1.0, {})
        inter, model_grads, gn_model = self._world_model_update(batch, noise, logs, keep)
        beliefs, post_states = inter["beliefs"].detach(), inter["posterior_states"].detach()
        Pf = self._frozen()
        if self.discrete:
            img_b, img_s, ent, logp, _ = discrete_imagine_ahead(Pf, post_states, beliefs, hp["planning_horizon"],
                                                                noise["action"], noise["img_prior"], self.cat)
            logp = logp.unsqueeze(-1)
        else:
            img_b, img_s, _, ent = O.imagine_ahead(Pf, post_states, beliefs, hp["planning_horizon"], noise["action"],
                                                   noise["entropy"], noise["img_prior"], self.cat)
        img_reward = O.dense_on_features(img_b, img_s, Pf["reward_model"])
        value_pred = self.value(img_b, img_s, Pf["critic_target"])
        returns = O.lambda_return(img_reward, value_pred, value_pred[-1], hp["discount"], hp["disclam"])
        Hm, N = img_b.shape[0], img_b.shape[1]
        start_b, start_s = beliefs.reshape(N, -1), post_states.reshape(N, -1)
        if not self.discrete:
            fb = torch.cat([start_b[None], img_b[:-1]], 0).reshape(Hm * N, -1).detach()
            fs = torch.cat([start_s[None], img_s[:-1]], 0).reshape(Hm * N, -1).detach()
            mean, std = O.actor_forward(fb, fs, P["actor"])
            u = (mean + std * noise["action"].reshape(Hm * N, -1)).detach()
            logp = tanh_normal_log_density(u, mean, std).reshape(Hm, N, 1)
        b0 = self.value(start_b, start_s, Pf["critic_target"]).reshape(1, N, 1)
        adv = (returns - torch.cat([b0, value_pred[:-1]], 0)).detach()
        objective = rho * returns / S + (1 - rho) * logp * adv / S + hp["entropy_weight"] * ent.unsqueeze(-1)
        wts = self._discount_weights(Pf, img_b, img_s)
        if wts is not None:
            objective = wts * objective
        actor_loss = -objective.mean()
        logs.update(actor_loss=actor_loss.item(), policy_entropy=ent.mean().item(), **rn_logs)
        agrads = [g.clone() for g in torch.autograd.grad(actor_loss, self.actor_params)]
        actor_grads = [g.clone() for g in agrads] if keep else None
        gn_actor = O.clip_grad_norm_(agrads, hp["grad_clip_norm"])
        O.adam_step(self.actor_params, agrads, self.opt["actor"], hp["actor_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        c_logits = O.dense_on_features(img_b.detach(), img_s.detach(), P["critic"])
        ce = row_loss(c_logits, returns.detach(), Z)
        value_loss = (wts * ce).mean() if wts is not None else ce.mean()
        logs.update(value_loss=value_loss.item())
        cgrads = [g.clone() for g in torch.autograd.grad(value_loss, self.critic_params)]
        critic_grads = [g.clone() for g in cgrads] if keep else None
        gn_critic = O.clip_grad_norm_(cgrads, hp["grad_clip_norm"])
        O.adam_step(self.critic_params, cgrads, self.opt["critic"], hp["value_learning_rate"], hp["adam_epsilon"],
                    hp["weight_decay"])
        if norm:
            self.rn_end(returns)
        if keep:
            self.last = dict(returns=returns.detach(), value_pred=value_pred.detach(), action_entropy=ent.detach(),
                             critic_value=decode(c_logits.detach(), Z), model_grads=model_grads, actor_grads=actor_grads,
                             critic_grads=critic_grads,
                             grad_norms=dict(model=gn_model.item(), actor=gn_actor.item(), critic=gn_critic.item()))
        return logs


class TwohotOracleDreamer(_TwohotStep, RetnormOracleDreamer):
    """RetnormOracleDreamer with the two-hot critic."""


class TwohotDiscreteOracleDreamer(_TwohotStep, RetnormDiscreteOracleDreamer):
    """The same on the Categorical actor."""

    discrete = True
