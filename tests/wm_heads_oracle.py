"""TEST INFRASTRUCTURE: CPU restatement of a train step with the world-model heads of DESIGN.md, "World-model heads on
any scale" (``reward_head = twohot``, ``symlog_observations = true``), on top of tests/twohot_oracle.py's classes.  Plain
torch fp32 with autograd; the two-hot head is ``row_loss`` / ``decode`` of tests/twohot_oracle.py, symlog is restated in
torch here (tests/symlog_ref.py is its numpy specification).

hp: ``reward_head`` ("normal"), ``reward_bins``, ``reward_bin_range`` (20), ``symlog_observations`` (False), and
``critic_head`` -- "twohot", what the classes this file derives from implement, or "normal" for the width-1 critic under
Normal(v, 1).  With the first four at their defaults a step is the step of the class derived from, bit for bit.

world_model_forward: the encoder reads symlog(obs[1:]) and observation_loss is the Normal(., 1) loss against it;
reward_model ends in K logits and reward_loss is the mean over rows of the cross-entropy against the two-hot encoding
of symlog(reward).  Behaviour: the imagined reward is the decoded logits, so autograd differentiates through the decode.
"""
from __future__ import annotations

import torch

from oracle import dreamer_oracle as O
from tests.discrete_oracle import discrete_imagine_ahead
from tests.mixing_oracle import mixing_rho, tanh_normal_log_density
from tests.twohot_oracle import TwohotDiscreteOracleDreamer, TwohotOracleDreamer, decode, row_loss


def symlog(x: torch.Tensor) -> torch.Tensor:
    return torch.sign(x) * torch.log1p(torch.abs(x))


class _WmHeadsStep:
    """The train step both restatements share; `discrete` selects the actor."""

    def _reward_twohot(self) -> bool:
        return self.hp.get("reward_head", "normal") == "twohot"

    def _critic_twohot(self) -> bool:
        return self.hp.get("critic_head", "twohot") == "twohot"

    def reward(self, b, s, sd):
        out = O.dense_on_features(b, s, sd)
        return decode(out, self.hp.get("reward_bin_range", 20.0)) if self._reward_twohot() else out

    def value(self, b, s, sd):
        out = O.dense_on_features(b, s, sd)
        return decode(out, self.hp.get("critic_bin_range", 20.0)) if self._critic_twohot() else out

    def world_model_forward(self, batch, noise):
        hp, P = self.hp, self.P
        obs, actions, rewards, nonterm = (batch[k] for k in ("observations", "actions", "rewards", "nonterminals"))
        B = obs.size(1)
        Be = P["transition_model"]["rnn.weight_hh"].size(1)
        S = P["transition_model"]["belief_prior.model.2.weight"].size(0) // (1 if self.cat else 2)
        init_belief = torch.zeros(B, Be)
        init_state = torch.zeros(B, S)
        pixel = obs.dim() == 5
        obs_t = obs[1:]
        if hp.get("symlog_observations", False):
            assert not pixel
            obs_t = symlog(obs_t)           # encoder input and decoder target
        emb = O.cnn_encoder(obs_t, P["encoder"]) if pixel else O.mlp(obs_t, P["encoder"])
        beliefs, prior_states, prior_params, post_states, post_params = O.transition_forward(
            P["transition_model"], init_state, actions[:-1], init_belief, emb, nonterm[:-1],
            noise["obs_prior"], noise["obs_post"], self.cat)
        if pixel:
            obs_loss = O.normal_nll_mean(O.cnn_decoder(beliefs, post_states, P["observation_model"]), obs_t, event_dims=3)
        else:
            obs_loss = O.normal_nll_mean(O.dense_on_features(beliefs, post_states, P["observation_model"]), obs_t)
        rew_out = O.dense_on_features(beliefs, post_states, P["reward_model"])
        if self._reward_twohot():
            Z = hp.get("reward_bin_range", 20.0)
            rew_loss = row_loss(rew_out, rewards[:-1].unsqueeze(-1), Z).mean()
            rew_pred = decode(rew_out, Z)
        else:
            rew_loss = O.normal_nll_mean(rew_out, rewards[:-1].unsqueeze(-1))
            rew_pred = rew_out
        self._discount_loss = None
        if self.use_discount:
            logits = O.dense_on_features(beliefs, post_states, P["discount_model"])
            self._discount_loss = torch.nn.functional.binary_cross_entropy_with_logits(
                logits, nonterm[:-1].float(), reduction="none").sum(-1).mean()
        if self.cat:
            kl = O.kl_loss_categorical(post_params[0], prior_params[0], hp["kl_balance"], hp["free_nats"])
            model_loss = obs_loss + rew_loss + kl * hp["kl_loss_weight"]
            if self._discount_loss is not None:
                model_loss = model_loss + self._discount_loss * hp["discount_weight"]
            inter = dict(embeddings=emb, beliefs=beliefs, prior_states=prior_states, prior_logits=prior_params[0],
                         posterior_states=post_states, posterior_logits=post_params[0], reward_pred=rew_pred)
            return model_loss, obs_loss, rew_loss, kl, inter
        kl = O.kl_loss(post_params, prior_params, hp["kl_balance"], hp["free_nats"])
        model_loss = obs_loss + rew_loss + kl * hp["kl_loss_weight"]
        if self._discount_loss is not None:
            model_loss = model_loss + self._discount_loss * hp["discount_weight"]
        inter = dict(embeddings=emb, beliefs=beliefs, prior_states=prior_states, prior_means=prior_params[0],
                     prior_stds=prior_params[1], posterior_states=post_states, posterior_means=post_params[0],
                     posterior_stds=post_params[1], reward_pred=rew_pred)
        return model_loss, obs_loss, rew_loss, kl, inter

    def train_step(self, batch_np, noise_np, keep: bool = True):
        """tests/twohot_oracle._TwohotStep.train_step with the imagined reward decoded and the critic head selectable."""
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
        img_reward = self.reward(img_b, img_s, Pf["reward_model"])
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
        c_out = O.dense_on_features(img_b.detach(), img_s.detach(), P["critic"])
        if self._critic_twohot():
            ce = row_loss(c_out, returns.detach(), Z)
            c_val = decode(c_out.detach(), Z)
        else:
            ce = 0.5 * (returns.detach() - c_out) ** 2 + O.HALF_LOG_2PI
            c_val = c_out.detach()
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
                             imged_reward=img_reward.detach(), reward_pred=inter["reward_pred"].detach(),
                             critic_value=c_val, model_grads=model_grads, actor_grads=actor_grads,
                             critic_grads=critic_grads,
                             grad_norms=dict(model=gn_model.item(), actor=gn_actor.item(), critic=gn_critic.item()))
        return logs


class WmHeadsOracleDreamer(_WmHeadsStep, TwohotOracleDreamer):
    """TwohotOracleDreamer with the two-hot reward head and symlog observations."""

    discrete = False


class WmHeadsDiscreteOracleDreamer(_WmHeadsStep, TwohotDiscreteOracleDreamer):
    """The same on the Categorical actor."""

    discrete = True
