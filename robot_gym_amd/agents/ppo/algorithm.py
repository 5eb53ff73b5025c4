"""The KL-penalised PPO update of the reference (agents/ppo/algorithm.py) in torch, full batch, on the parameter tensors the
act kernel reads: autograd and Adam are plumbing, the optimisers step in place."""
import math

import torch

LOG_2PI = math.log(2.0 * math.pi)


def diag_normal_kl(mean0, logstd0, mean1, logstd1):
    """KL(N0 || N1) of two diagonal normals, summed over the last axis (utility.diag_normal_kl)."""
    l0, l1 = 2.0 * logstd0, 2.0 * logstd1
    return 0.5 * (torch.exp(l0 - l1).expand_as(mean0).sum(-1) + ((mean1 - mean0) ** 2 / torch.exp(l1)).sum(-1) + l1.sum(-1) - l0.sum(-1)
                  - mean0.shape[-1])


def diag_normal_logpdf(mean, logstd, loc, conv="exact"):
    """Log density of a diagonal normal, summed over the last axis.  conv="exact": the density, -logstd per component (what
    tfp gives the reference's `perform`, and rg_policy_act).  conv="reference": utility.diag_normal_logpdf as written, which
    carries -0.5 * logstd."""
    if conv not in ("exact", "reference"):
        raise ValueError(f"conv_logpdf must be 'exact' or 'reference', got {conv!r}")
    const = -0.5 * LOG_2PI - (logstd if conv == "exact" else 0.5 * logstd)
    return (const - 0.5 * ((loc - mean) / torch.exp(logstd)) ** 2).sum(-1)


class PPO:
    """update(rollout) runs epochs_policy full-batch Adam steps on policy.policy_params (networks and logstd), epochs_value on
    policy.value_params, then moves the KL penalty.  Ticks with rollout.mask == 0 count as 0 in every mean over time, as the
    reference's length mask does; the advantage is normalised by the mean and std + 1e-8 of the unmasked ticks."""

    def __init__(self, policy, policy_lr=1e-4, value_lr=3e-4, epochs_policy=50, epochs_value=50, kl_target=1e-2, kl_cutoff_factor=2,
                 kl_cutoff_coef=1000, kl_init_penalty=1, conv_logpdf="exact"):
        if conv_logpdf not in ("exact", "reference"):
            raise ValueError(f"conv_logpdf must be 'exact' or 'reference', got {conv_logpdf!r}")
        self.policy = policy
        self.epochs_policy, self.epochs_value = int(epochs_policy), int(epochs_value)
        self.kl_target, self.kl_cutoff_factor, self.kl_cutoff_coef = float(kl_target), float(kl_cutoff_factor), float(kl_cutoff_coef)
        self.penalty = float(kl_init_penalty)
        self.conv_logpdf = conv_logpdf
        self.policy_opt = torch.optim.Adam([policy.policy_params], lr=policy_lr)
        self.value_opt = torch.optim.Adam([policy.value_params], lr=value_lr)

    def batch(self, rollout):
        """The tensors of an update from a rollout: normalised observations [T, B, obs_dim], the normalised advantage, the
        mask as the parameters' dtype."""
        p = self.policy
        with torch.no_grad():
            x = p.normalize_obs(rollout.obs.permute(0, 2, 1))
            valid = (rollout.mask != 0).to(p.dtype)
            adv = rollout.adv.to(p.dtype)
            n = valid.sum().clamp_min(1.0)
            m = (adv * valid).sum() / n
            var = ((adv - m) ** 2 * valid).sum() / n
            adv = (adv - m) / (torch.sqrt(var) + 1e-8)
        return dict(x=x, valid=valid, adv=adv, action=rollout.action.to(p.dtype), old_mean=rollout.mean.to(p.dtype),
                    old_logstd=rollout.logstd.to(p.dtype), ret=rollout.ret.to(p.dtype))

    def _evaluate(self, b):
        """(mean, value) of the batch under the current parameters; a recurrent policy's update overrides it."""
        return self.policy.evaluate(b["x"])

    def kl(self, b):
        """KL(behaviour || current) per robot [B], averaged over time."""
        mean, _ = self._evaluate(b)
        return (diag_normal_kl(b["old_mean"], b["old_logstd"], mean, self.policy.logstd) * b["valid"]).mean(0)

    def policy_loss(self, b):
        mean, _ = self._evaluate(b)
        logstd = self.policy.logstd
        kl = (diag_normal_kl(b["old_mean"], b["old_logstd"], mean, logstd) * b["valid"]).mean(0)
        ratio = torch.exp(diag_normal_logpdf(mean, logstd, b["action"], self.conv_logpdf)
                          - diag_normal_logpdf(b["old_mean"], b["old_logstd"], b["action"], self.conv_logpdf))
        surrogate = -(ratio * b["adv"] * b["valid"]).mean(0)
        threshold = self.kl_target * self.kl_cutoff_factor
        cutoff = self.kl_cutoff_coef * (kl > threshold).to(kl.dtype) * (kl - threshold) ** 2
        return (surrogate + self.penalty * kl + cutoff).mean()

    def value_loss(self, b):
        _, value = self._evaluate(b)
        return (0.5 * (b["ret"] - value) ** 2 * b["valid"]).mean()

    def adjust_penalty(self, kl_change):
        """x 1.5 above 1.3 x the target, / 1.5 below 0.7 x, else unchanged."""
        if kl_change > 1.3 * self.kl_target:
            self.penalty *= 1.5
        elif kl_change < 0.7 * self.kl_target:
            self.penalty /= 1.5
        return self.penalty

    def update(self, rollout):
        b = self.batch(rollout)
        first = last = None
        for _ in range(self.epochs_policy):
            self.policy_opt.zero_grad(set_to_none=True)
            loss = self.policy_loss(b)
            loss.backward()
            self.policy_opt.step()
            first = loss.detach() if first is None else first
            last = loss.detach()
        vfirst = vlast = None
        for _ in range(self.epochs_value):
            self.value_opt.zero_grad(set_to_none=True)
            loss = self.value_loss(b)
            loss.backward()
            self.value_opt.step()
            vfirst = loss.detach() if vfirst is None else vfirst
            vlast = loss.detach()
        with torch.no_grad():
            kl_change = float(self.kl(b).mean())
        self.adjust_penalty(kl_change)
        f = lambda t: None if t is None else float(t)
        return dict(policy_loss_first=f(first), policy_loss_last=f(last), value_loss_first=f(vfirst), value_loss_last=f(vlast), kl_change=kl_change,
                    penalty=self.penalty)
