"""RecurrentPPO.update on the device: the policy half is include/rg_bptt.h (the T ticks forward with every intermediate kept, the
float64 head, back-propagation through time through the GRU cell, the weight gradients, Adam, the per-robot KL and the move of
the KL penalty), the value half is include/rg_ppo.h's sweep over the feed-forward value network, all as HIP kernels on the
current stream with no host read.  The same losses, the same Adam, the same penalty rule and the same defaults as RecurrentPPO
(recurrent.py); the arithmetic differs where the two headers say: float32 fixed-order sums instead of rocBLAS, the penalty
in device memory."""
import torch

from robot_gym_amd.core import bptt_abi, ppo_abi

from .device_update import _DeviceUpdate

_SLOTS = ("obs", "action", "mean", "logstd", "adv", "ret", "mask")
_GRAD_SLOTS = ("obs", "action", "mean", "logstd", "adv", "mask")


class DeviceRecurrentPPO(_DeviceUpdate):
    """update(rollout) enqueues rg_ppo_prepare, rg_bptt_update_policy and epochs_value x (rg_ppo_value_grad, rg_ppo_adam) for a
    RecurrentRolloutBuffer of T ticks of policy.batch robots and returns the device tensor `stats` (float64 [6],
    ppo_abi.STAT_NAMES); stats_dict() reads it.  The KL and the penalty read the policy alone, so taking them before the value
    epochs gives RecurrentPPO.update's result.  prepare / policy_grad / value_grad / adam / kl expose the single entries.  It
    steps policy.policy_params and policy.value_params in place: the tensors rg_rnn_act reads, at the same addresses.

        opt_state        float64 [opt_state_bytes / 8], the bytes of rg_bptt.h: step (int64 [1] view), penalty (float64 [1] view),
                         moments (float32 view: m, v of the policy buffer)
        value_opt_state  the opt_state of rg_ppo.h of the value side's handle, of which the value buffer's step and moments are used
        steps            (a method) int64 [2]: the policy's and the value buffer's step counts, gathered on the device
        workspace, value_workspace   scratch of the kernels (what prepare leaves in value_workspace is read by policy_grad)

    The value side is an rg_ppo handle made for policy_layers=() and the policy's value_layers: the value network's layout does not
    depend on the policy network's (rnn_abi.param_layout and policy_abi.param_layout agree on it).
    The keywords are RecurrentPPO's (and Adam's beta1, beta2, adam_eps, which PPO leaves at torch's defaults).  T, the rollout's
    length, sizes the workspaces: given here, or taken from the first rollout an entry sees; after that every rollout must
    have it.  A host-only policy (device="cpu") gives host-only handles: arguments are checked, every entry then raises
    NO_DEVICE."""

    def _alloc(self):
        self._handle = self._value = self.workspace = self.value_workspace = self.value_opt_state = None
        opt_bytes = bptt_abi.OPT_HEADER_BYTES + 4 * 2 * self.policy_count                # rg_bptt.h, opt_state
        self.opt_state = torch.zeros(opt_bytes // 8, dtype=torch.float64, device=self.device)
        self.step = self.opt_state[:1].view(torch.int64)
        self.penalty = self.opt_state[1:2]
        self.moments = self.opt_state[bptt_abi.OPT_HEADER_BYTES // 8:].view(torch.float32)
        self._policy_stats = torch.zeros(bptt_abi.STATS, dtype=torch.float64, device=self.device)

    def _bind(self, T):
        """The two handles, their workspaces and the value side's opt_state for rollouts of T ticks."""
        self.T = int(T)
        p = self.policy
        host_only = self.device.type == "cpu"
        self._handle = bptt_abi.BpttHandle(self.T, self.batch, bptt_abi.DEVICE_NONE if host_only else self.device,
                                           rnn_settings={k: p.fields[k] for k in ("obs_dim", "act_dim", "policy_layers", "gru_units", "value_layers",
                                                                                  "obs_clip", "seed")}, **self._settings)
        if self._handle.opt_state_bytes != self.opt_state.numel() * 8:
            raise RuntimeError("rg_bptt_opt_state_bytes disagrees with the layout of rg_bptt.h")
        value_settings = dict(obs_dim=p.obs_dim, act_dim=p.act_dim, policy_layers=(), value_layers=tuple(p.fields["value_layers"]), obs_clip=p.obs_clip)
        self._value = ppo_abi.PpoHandle(self.T, self.batch, ppo_abi.DEVICE_NONE if host_only else self.device, policy_settings=value_settings,
                                        **self._settings)
        self.workspace = torch.zeros(self._handle.workspace_bytes // 8, dtype=torch.float64, device=self.device)
        self.value_workspace = torch.zeros(self._value.workspace_bytes // 8, dtype=torch.float64, device=self.device)
        self.value_opt_state = torch.zeros(self._value.opt_state_bytes // 8, dtype=torch.float64, device=self.device)
        self._value_policy_count = p.obs_dim * p.act_dim + 2 * p.act_dim     # the policy buffer of the value side's handle: a head and logstd

    @property
    def value_step(self):
        """int64 [1] view: Adam's step count of the value buffer (rg_ppo.h's opt_state, step[1])."""
        return self.value_opt_state[1:2].view(torch.int64)

    @property
    def value_moments(self):
        """float32 view: m, v of the value buffer."""
        first = ppo_abi.OPT_HEADER_BYTES // 4 + 2 * self._value_policy_count
        return self.value_opt_state.view(torch.float32)[first:first + 2 * self.value_count]

    def steps(self):
        """int64 [2] on the device: the step counts of the policy and of the value buffer."""
        return torch.cat([self.step, self.value_step])

    # ---- argument checks ------------------------------------------------------------------------------------------------

    def _rollout(self, call, rollout, slots, recurrent=True):
        """(rg_ppo_rollout over the named slots, reset pointer, h0 pointer) of a RecurrentRolloutBuffer, each tensor checked before
        the library sees its pointer: contiguous, of the shape and dtype the headers give, on this device."""
        ro = super()._rollout(call, rollout, slots)
        if not recurrent:
            return ro
        return (ro, self._check(call, "rollout.reset", getattr(rollout, "reset", None), (self.T, self.batch), torch.int32),
                self._check(call, "rollout.h0", getattr(rollout, "h0", None), (self.batch, self.policy.gru_units), torch.float32))

    def _norm(self, call):
        return self._check(call, "policy.norm_state", self.policy.norm_state, tuple(self.policy.norm_state.shape), torch.float64)

    def _adv_ptr(self):
        return self.value_workspace.data_ptr() + self._value.scalars_offset

    # ---- the entries ----------------------------------------------------------------------------------------------------

    def update(self, rollout):
        """The whole update on the current stream; returns self.stats (a device tensor; nothing is read on the host)."""
        ro, reset, h0 = self._rollout("update", rollout, _SLOTS)
        pp, vp = self._params("update")
        norm = self._norm("update")
        value, ws = self._value, self.value_workspace.data_ptr()
        value.prepare(ro, ws)
        self._handle.update_policy(ro, reset, h0, self._adv_ptr(), norm, pp, self.opt_state.data_ptr(), self.workspace.data_ptr(),
                                   self._policy_stats.data_ptr())
        grad = self._grad[ppo_abi.VALUE].data_ptr()
        for e in range(self.epochs_value):
            value.value_grad(ro, norm, vp, ws, grad, self.stats[3:4].data_ptr())
            if e == 0:
                self.stats[2:3].copy_(self.stats[3:4])
            value.adam(ppo_abi.VALUE, vp, grad, self.value_opt_state.data_ptr())
        if self.epochs_value == 0:
            self.stats[2:4].fill_(float("nan"))
        self.stats[0:2].copy_(self._policy_stats[0:2])
        self.stats[4:6].copy_(self._policy_stats[2:4])
        return self.stats

    def prepare(self, rollout):
        """rg_ppo_prepare: the advantage's n, mean and std for policy_grad."""
        self._value.prepare(self._rollout("prepare", rollout, ("adv", "mask"), recurrent=False), self.value_workspace.data_ptr())

    def adv_stats(self):
        """(n clamped to 1, mean, std + 1e-8, n) as prepare left them: a float64 [4] device tensor."""
        off = self._value.scalars_offset // 8
        return self.value_workspace[off:off + 4]

    def policy_grad(self, rollout, out=None):
        """(grad float32 [policy_count], loss float64 [] view) of RecurrentPPO.policy_loss after prepare(rollout); out: the
        gradient's tensor."""
        ro, reset, h0 = self._rollout("policy_grad", rollout, _GRAD_SLOTS)
        pp, _ = self._params("policy_grad")
        grad = self._out("policy_grad", out, ppo_abi.POLICY)
        self._handle.policy_grad(ro, reset, h0, self._adv_ptr(), self._norm("policy_grad"), pp, self.opt_state.data_ptr(), self.workspace.data_ptr(),
                                 grad.data_ptr(), self._loss[0:1].data_ptr())
        return grad, self._loss[0]

    def value_grad(self, rollout, out=None):
        ro = self._rollout("value_grad", rollout, ("obs", "ret", "mask"), recurrent=False)
        _, vp = self._params("value_grad")
        grad = self._out("value_grad", out, ppo_abi.VALUE)
        self._value.value_grad(ro, self._norm("value_grad"), vp, self.value_workspace.data_ptr(), grad.data_ptr(), self._loss[1:2].data_ptr())
        return grad, self._loss[1]

    def adam(self, which, grad):
        """One Adam step on the policy's buffer `which` ("policy" / "value" or ppo_abi.POLICY / VALUE) with `grad`: rg_bptt_adam or
        rg_ppo_adam."""
        which, grad, (pp, vp) = self._adam_args(which, grad)
        if which == ppo_abi.POLICY:
            self._handle.adam(pp, grad.data_ptr(), self.opt_state.data_ptr())
        else:
            self._value.adam(ppo_abi.VALUE, vp, grad.data_ptr(), self.value_opt_state.data_ptr())

    def kl(self, rollout, out=None):
        """KL(behaviour || current) per robot, float64 [B] on the device."""
        ro, reset, h0 = self._rollout("kl", rollout, ("obs", "mean", "logstd", "mask"))
        pp, _ = self._params("kl")
        out = self._kl_out(out)
        self._handle.kl(ro, reset, h0, self._norm("kl"), pp, self.workspace.data_ptr(), out.data_ptr())
        return out

    def move_penalty(self, kl, out=None):
        """rg_bptt_penalty: moves the penalty by the mean of kl (float64 [B]); returns float64 [2]: kl_change, the new penalty."""
        self._check("move_penalty", "kl", kl, (self.batch,), torch.float64)
        if self._handle is None:
            raise ValueError("move_penalty: no rollout has been seen yet")
        out = self._policy_stats[2:4] if out is None else out
        self._check("move_penalty", "out", out, (2,), torch.float64)
        self._handle.penalty(kl.data_ptr(), self.opt_state.data_ptr(), out.data_ptr())
        return out

    # ---- state ----------------------------------------------------------------------------------------------------------

    def state_dict(self):
        if self.value_opt_state is None:
            raise ValueError("state_dict: no rollout has been seen yet; pass T to DeviceRecurrentPPO")
        return dict(opt_state=self.opt_state.clone(), value_opt_state=self.value_opt_state.clone(), fields=dict(self.fields), T=self.T, batch=self.batch)

    def load_state_dict(self, state):
        """Copies INTO opt_state and value_opt_state (their addresses do not change): Adam's moments and step counts and the
        penalty.  The state must come from the same settings, batch and T."""
        if dict(state["fields"]) != dict(self.fields) or int(state["batch"]) != self.batch:
            raise ValueError("load_state_dict: the state was saved from another configuration")
        if self.T is None:
            self._bind(state["T"])
        if int(state["T"]) != self.T:
            raise ValueError(f"load_state_dict: the state was saved for T = {state['T']}, this update is for T = {self.T}")
        for name in ("opt_state", "value_opt_state"):
            t, own = state[name], getattr(self, name)
            if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != tuple(own.shape):
                raise ValueError(f"load_state_dict: {name} must be a float64 tensor of this configuration's size")
        self.opt_state.copy_(state["opt_state"])
        self.value_opt_state.copy_(state["value_opt_state"])

    def close(self):
        for h in (self._handle, self._value):
            if h is not None:
                h.close()
