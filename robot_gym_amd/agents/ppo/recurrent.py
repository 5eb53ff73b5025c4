"""The recurrent Gaussian policy of the PPO agent for B robots (include/rg_rnn.h): dense relu layers, a GRU block cell and the
tanh mean head, with the feed-forward value network beside it.  Acting and sequence evaluation run in the HIP kernels; the
update is torch autograd (back-propagation through time over a rollout, truncated at its first tick) on the parameter
memory the kernels read.  The reference: agents/ppo/scripts/networks.py (RecurrentGaussianPolicy)."""
import math

import torch

from robot_gym_amd.agents.ppo.algorithm import PPO
from robot_gym_amd.agents.ppo.policy import BatchedGaussianPolicy
from robot_gym_amd.agents.ppo.rollout import RolloutBuffer
from robot_gym_amd.core import goto_abi, policy_abi, rnn_abi


class RecurrentGaussianPolicy(BatchedGaussianPolicy):
    """Owns an rg_rnn handle (act, unroll), an rg_policy handle of the same obs_dim (record, returns) and the tensors the
    kernels read and write.  Beside those of BatchedGaussianPolicy:

        policy_params  float32 [policy_count]   dense layers, W_ru, b_ru, W_c, b_c, the head, logstd (rg_rnn.h, Parameters)
        hidden         float32 [B, H]           the cell's state; act() advances it in place
        pending_reset  int32 [B]                robots whose next act() reads a zero state; all ones after construction and after
                                                begin_episodes(); act() consumes it

    dense_layers, cell, head, value_layers and logstd are views of the two parameter tensors.  device="cpu" makes a host-only
    policy (evaluate_sequence, normalize_*, state_dict work; act and unroll raise NO_DEVICE)."""

    def __init__(self, batch, obs_dim=16, act_dim=2, policy_layers=(200,), gru_units=100, value_layers=(200, 100), seed=0, device=None, dtype=None,
                 obs_clip=5.0, reward_clip=10.0, discount=0.985, gae_lambda=1.0):
        self.batch = B = int(batch)
        rnn = dict(obs_dim=obs_dim, act_dim=act_dim, policy_layers=tuple(policy_layers), gru_units=gru_units, value_layers=tuple(value_layers),
                   seed=seed, obs_clip=obs_clip)
        host_only = device is not None and torch.device(device).type == "cpu"
        none = rnn_abi.DEVICE_NONE if host_only else device
        self._rnn = rnn_abi.RnnHandle(B, none, **rnn)
        # record and returns read obs_dim, the clips and the discounts only; the networks of this handle are not used
        self._handle = policy_abi.PolicyHandle(B, policy_abi.DEVICE_NONE if host_only else device, obs_dim=obs_dim, act_dim=act_dim, policy_layers=(),
                                               value_layers=tuple(value_layers), seed=seed, obs_clip=obs_clip, reward_clip=reward_clip,
                                               discount=discount, gae_lambda=gae_lambda)
        self.fields = dict(self._rnn.fields, reward_clip=float(reward_clip), discount=float(discount), gae_lambda=float(gae_lambda))
        self.device = dev = torch.device("cpu") if host_only else self._rnn.device
        self.dtype = dtype = dtype or torch.float32
        if not host_only and dtype != torch.float32:
            raise ValueError("the kernels read float32 parameters")
        self.obs_dim, self.act_dim, self.gru_units = int(obs_dim), int(act_dim), int(gru_units)
        self.obs_clip, self.reward_clip = float(obs_clip), float(reward_clip)
        lay = self.layout = self._rnn.layout
        self.policy_params = torch.zeros(lay["policy_count"], dtype=dtype, device=dev)
        self.value_params = torch.zeros(lay["value_count"], dtype=dtype, device=dev)
        self.act_state = torch.zeros(2, B, dtype=torch.int64, device=dev)
        self.act_state[0] = torch.arange(B, dtype=torch.int64, device=dev)
        self.norm_state = torch.zeros(policy_abi.NORM_ROWS, dtype=torch.float64, device=dev)
        self.hidden = torch.zeros(B, self.gru_units, dtype=torch.float32, device=dev)
        self.pending_reset = torch.ones(B, dtype=torch.int32, device=dev)
        self._scratch_action = torch.zeros(B, self.act_dim, dtype=torch.float32, device=dev)
        self._scratch_hidden = torch.zeros(B, self.gru_units, dtype=torch.float32, device=dev)
        self.policy_params.requires_grad_(True)
        self.value_params.requires_grad_(True)
        self.init_parameters(seed)

    # ---- views ----------------------------------------------------------------------------------------------------------

    @property
    def dense_layers(self):
        """[(W [in, out], b [out]), ...] of the dense relu layers in front of the cell: views of policy_params."""
        return self._views(self.policy_params, self.layout["dense"])

    @property
    def cell(self):
        """((W_ru [n_x + H, 2H], b_ru [2H]), (W_c [n_x + H, H], b_c [H])): the x rows first; columns 0 .. H-1 of W_ru the reset gate."""
        return tuple(self._views(self.policy_params, [self.layout["w_ru"], self.layout["w_c"]]))

    @property
    def head(self):
        return self._views(self.policy_params, [self.layout["head"]])[0]

    @property
    def policy_layers(self):
        """Every (W, b) block of policy_params in the buffer's order: the dense layers, (W_ru, b_ru), (W_c, b_c), the head."""
        return self.dense_layers + list(self.cell) + [self.head]

    def init_parameters(self, seed=0):
        """As BatchedGaussianPolicy: Glorot-uniform weights and zero biases for the dense layers and the value network, the
        truncated normal for the mean head, logstd = -1.  The cell's own initialisers: Glorot-uniform W_ru and W_c (fan-in
        n_x + H), b_ru = 1, b_c = 0."""
        gen = torch.Generator().manual_seed(int(seed))

        def glorot(W):
            fan_in, fan_out = W.shape
            limit = math.sqrt(6.0 / (fan_in + fan_out))
            W.copy_(((torch.rand(fan_in, fan_out, dtype=torch.float64, generator=gen) * 2.0 - 1.0) * limit).to(self.dtype))

        with torch.no_grad():
            for W, b in self.dense_layers:
                glorot(W)
                b.zero_()
            (W_ru, b_ru), (W_c, b_c) = self.cell
            glorot(W_ru)
            b_ru.fill_(1.0)
            glorot(W_c)
            b_c.zero_()
            W, b = self.head
            std = math.sqrt(1.3 * 0.1 / W.shape[0])
            w = torch.empty(*W.shape, dtype=torch.float64)
            torch.nn.init.trunc_normal_(w, mean=0.0, std=std, a=-2.0 * std, b=2.0 * std, generator=gen)
            W.copy_(w.to(self.dtype))
            b.zero_()
            for W, b in self.value_layers:
                glorot(W)
                b.zero_()
            self.logstd.fill_(-1.0)

    # ---- the kernels ------------------------------------------------------------------------------------------------------

    def begin_episodes(self, mask=None):
        """Robots with mask != 0 (None: all) read a zero state at their next act().  mask: int32 [B] on this device."""
        if mask is None:
            self.pending_reset.fill_(1)
        else:
            self.pending_reset.copy_(torch.where(mask != 0, torch.ones_like(self.pending_reset), self.pending_reset))

    def act(self, obs_cm, sample=True, out=None, advance=True):
        """rg_rnn_act on the current stream.  obs_cm and out as in BatchedGaussianPolicy.act.  advance=True: the tick reads hidden
        (zero where pending_reset != 0), writes the new state over it and clears pending_reset.  advance=False: hidden and
        pending_reset are left as they are (the new state goes to a scratch tensor): a value-only look at an observation."""
        B = self.batch
        if not torch.is_tensor(obs_cm) or tuple(obs_cm.shape) != (self.obs_dim, B) or obs_cm.dtype != torch.float32 or not obs_cm.is_contiguous() \
                or obs_cm.device != self.device:
            raise ValueError(f"act: obs_cm must be a contiguous float32 [{self.obs_dim},{B}] tensor on {self.device}")
        out = dict(out or {})
        out.setdefault("action", self._scratch_action)
        shapes = dict(action=(B, self.act_dim), mean=(B, self.act_dim), value=(B,), logprob=(B,))
        ptr = {}
        for name, t in out.items():
            if name not in shapes:
                raise TypeError(f"act: unknown output {name!r}")
            if tuple(t.shape) != shapes[name] or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"act: out[{name!r}] must be a contiguous float32 {list(shapes[name])} tensor on {self.device}")
            ptr[name] = t.data_ptr()
        hidden_out = self.hidden if advance else self._scratch_hidden
        self._rnn.act(obs_cm.data_ptr(), self.norm_state.data_ptr(), self.policy_params.data_ptr(), self.value_params.data_ptr(),
                      self.act_state.data_ptr(), self.pending_reset.data_ptr(), self.hidden.data_ptr(), hidden_out.data_ptr(),
                      rnn_abi.MODE_SAMPLE if sample else rnn_abi.MODE_MEAN, ptr["action"], ptr.get("mean"), ptr.get("value"), ptr.get("logprob"))
        if advance:
            self.pending_reset.zero_()
        return out

    def unroll(self, rollout, out=None):
        """rg_rnn_unroll over a RecurrentRolloutBuffer of this batch: the means of rollout.obs from rollout.h0 under
        rollout.reset with the current parameters and normaliser.  out: a dict with any of mean [T, B, act_dim], hidden_seq
        [T, B, H], hidden_last [B, H] to write into; a missing mean is allocated.  Returns the dict."""
        T, B, H, f32 = int(rollout.T), self.batch, self.gru_units, torch.float32
        if int(rollout.batch) != B:
            raise ValueError(f"unroll: rollout.batch is {rollout.batch}, the policy's batch is {B}")
        out = dict(out or {})
        if "mean" not in out:
            out["mean"] = torch.zeros(T, B, self.act_dim, dtype=f32, device=self.device)
        unknown = set(out) - {"mean", "hidden_seq", "hidden_last"}
        if unknown:
            raise TypeError(f"unroll: unknown output(s) {sorted(unknown)}")
        obs = self._ptr("unroll", "rollout.obs", rollout.obs, (T, self.obs_dim, B), f32)
        reset = self._ptr("unroll", "rollout.reset", rollout.reset, (T, B), torch.int32)
        h0 = self._ptr("unroll", "rollout.h0", rollout.h0, (B, H), f32)
        mean = self._ptr("unroll", "out['mean']", out["mean"], (T, B, self.act_dim), f32)
        hseq = self._ptr("unroll", "out['hidden_seq']", out.get("hidden_seq"), (T, B, H), f32, optional=True)
        hlast = self._ptr("unroll", "out['hidden_last']", out.get("hidden_last"), (B, H), f32, optional=True)
        self._rnn.unroll(obs, reset, h0, self.norm_state.data_ptr(), self.policy_params.data_ptr(), T, mean, hseq, hlast)
        return out

    # ---- the same arithmetic in torch, for the update -------------------------------------------------------------------

    def evaluate_value(self, obs_norm):
        v, vl = obs_norm, self.value_layers
        for k, (W, b) in enumerate(vl):
            v = v @ W + b
            if k < len(vl) - 1:
                v = torch.relu(v)
        return v[..., 0]

    def evaluate_hidden(self, obs_norm, reset, h0):
        """The cell's state after every tick [T, B, H]: differentiable in the parameters and in obs_norm; h0 enters as a constant."""
        x = obs_norm
        for W, b in self.dense_layers:
            x = torch.relu(x @ W + b)
        (W_ru, b_ru), (W_c, b_c) = self.cell
        n_x, H = self.layout["n_x"], self.gru_units
        gx_ru = x @ W_ru[:n_x] + b_ru            # the x rows of every tick at once
        gx_c = x @ W_c[:n_x] + b_c
        Wh_ru, Wh_c = W_ru[n_x:], W_c[n_x:]
        h = h0.detach().to(x.dtype)
        zero = torch.zeros_like(h)
        states = []
        for t in range(x.shape[0]):
            h = torch.where(reset[t].unsqueeze(-1) != 0, zero, h)
            ru = torch.sigmoid(gx_ru[t] + h @ Wh_ru)
            r, u = ru[..., :H], ru[..., H:]
            c = torch.tanh(gx_c[t] + (r * h) @ Wh_c)
            h = u * h + (1.0 - u) * c
            states.append(h)
        return torch.stack(states)

    def evaluate_sequence(self, obs_norm, reset, h0):
        """(mean [T, B, act_dim], value [T, B]) of normalised observations [T, B, obs_dim] from state h0 [B, H], the state zeroed
        where reset [T, B] != 0 before the tick reads it: differentiable torch ops over the views of the two parameter
        tensors.  No gradient is taken with respect to h0."""
        W, b = self.head
        return torch.tanh(self.evaluate_hidden(obs_norm, reset, h0) @ W + b), self.evaluate_value(obs_norm)

    def evaluate(self, obs_norm):
        raise TypeError("a recurrent policy has no memoryless evaluate(): use evaluate_sequence(obs_norm, reset, h0)")

    # ---- state ------------------------------------------------------------------------------------------------------------

    def clone(self, src, dst):
        """The act state, the hidden row and pending_reset of robot src[k] into robot dst[k]."""
        s = torch.as_tensor(src, dtype=torch.int64, device=self.device).reshape(-1)
        t = torch.as_tensor(dst, dtype=torch.int64, device=self.device).reshape(-1)
        self.act_state.index_copy_(1, t, self.act_state.index_select(1, s))
        self.hidden.index_copy_(0, t, self.hidden.index_select(0, s))
        self.pending_reset.index_copy_(0, t, self.pending_reset.index_select(0, s))

    def state_dict(self):
        return dict(super().state_dict(), hidden=self.hidden.clone(), pending_reset=self.pending_reset.clone())

    def load_state_dict(self, state):
        super().load_state_dict(state)
        self.hidden.copy_(state["hidden"])
        self.pending_reset.copy_(state["pending_reset"])

    def close(self):
        self._rnn.close()
        self._handle.close()


class RecurrentRolloutBuffer(RolloutBuffer):
    """RolloutBuffer and what sequence evaluation needs beside it:

        h0 [B, H]              the cell's state before tick 0
        reset [T, B] int32     reset[t, b] != 0: tick t read a zero state (an episode of robot b began there)"""

    def __init__(self, T, batch, obs_dim=16, act_dim=2, gru_units=100, device=None, dtype=torch.float32):
        super().__init__(T, batch, obs_dim, act_dim, device=device, dtype=dtype)
        self.gru_units = int(gru_units)
        self.h0 = torch.zeros(self.batch, self.gru_units, dtype=dtype, device=device)
        self.reset = torch.zeros(self.T, self.batch, dtype=torch.int32, device=device)


def collect_recurrent(env, policy, rollout, bootstrap=True, update_normalizers=True):
    """collect() for a RecurrentGaussianPolicy and a RecurrentRolloutBuffer.  Beside what collect() does: rollout.h0 is
    policy.hidden before tick 0, rollout.reset[t] is policy.pending_reset as tick t read it, and after every env.step
    pending_reset becomes the step's done.  The bootstrap value is a value-only act that leaves hidden and pending_reset
    alone.  Nothing in the loop reads device data on the host.  Returns rollout.
    update_normalizers=False records the slots and leaves both normalisers as they are (rg_policy_record with an all-zero
    mask): every tick then saw the normaliser policy.unroll(rollout) sees, and rollout.mean is that kernel's to the bit.  With
    the default the normalisers move after every tick, as in collect(), and the two differ by that drift."""
    T = rollout.T
    with torch.no_grad():
        frozen = None if update_normalizers else torch.zeros(policy.batch, dtype=torch.int32, device=policy.device)
        rollout.logstd.copy_(policy.logstd)
        rollout.h0.copy_(policy.hidden)
        if env.auto_reset:
            rollout.mask.fill_(1)
        for t in range(T):
            obs_slot = rollout.obs[t]
            obs_slot.copy_(env.obs.t())
            mask = None
            if not env.auto_reset:
                mask = rollout.mask[t]
                mask.copy_(env.task_state[goto_abi.ROW_DONE] == 0)
            rollout.reset[t].copy_(policy.pending_reset)
            policy.act(obs_slot, sample=True, out=dict(action=rollout.action[t], mean=rollout.mean[t], value=rollout.value[t], logprob=rollout.logprob[t]))
            _, reward, done = env.step(rollout.action[t])
            policy.pending_reset.copy_(done)
            policy.record(obs_slot, reward, done, mask if frozen is None else frozen, ro_reward=rollout.reward[t], ro_done=rollout.done[t])
        policy.act(env.obs.t(), sample=False, out=dict(value=rollout.last_value), advance=False)
        policy.returns(rollout, bootstrap=bootstrap)
    return rollout


def play_recurrent(env, policy, ticks):
    """The deterministic player for a recurrent policy: `ticks` steps of action = mean, the state reset where an episode ended.
    Returns the sum of the rewards per robot, a device tensor [B]."""
    total = torch.zeros(env.batch, dtype=torch.float32, device=env.device)
    with torch.no_grad():
        for _ in range(int(ticks)):
            out = policy.act(env.obs.t(), sample=False)
            _, reward, done = env.step(out["action"])
            policy.pending_reset.copy_(done)
            total += reward
    return total


class RecurrentPPO(PPO):
    """PPO over a RecurrentRolloutBuffer: the same losses, penalty rule and defaults; the means come from
    policy.evaluate_sequence, so a policy step back-propagates through the T ticks of the rollout, truncated at its first
    tick (rollout.h0 is a constant)."""

    def batch(self, rollout):
        b = super().batch(rollout)
        b["reset"], b["h0"] = rollout.reset, rollout.h0.to(self.policy.dtype)
        return b

    def _evaluate(self, b):
        return self.policy.evaluate_sequence(b["x"], b["reset"], b["h0"])

    def value_loss(self, b):
        value = self.policy.evaluate_value(b["x"])   # the value network is feed-forward: no unrolling for its steps
        return (0.5 * (b["ret"] - value) ** 2 * b["valid"]).mean()
