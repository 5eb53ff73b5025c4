"""PPO.update on the device (include/rg_ppo.h): the advantage normalisation, the forward and backward passes of both networks,
Adam, the per-robot KL and the move of the KL penalty as HIP kernels on the current stream, with no host read.  The same
losses, the same Adam, the same penalty rule and the same defaults as PPO (algorithm.py); the arithmetic differs where
rg_ppo.h says: float32 fixed-order sums instead of rocBLAS, the penalty in device memory."""
import torch

from robot_gym_amd.core import ppo_abi

_SLOTS = ("obs", "action", "mean", "logstd", "adv", "ret", "mask")


class _DeviceUpdate:
    """What DevicePPO and DeviceRecurrentPPO (device_recurrent.py) have in common: the settings, the tensors an entry writes
    where the caller gives none, and the check of every tensor before its pointer crosses the ABI.  A class adds _alloc (its
    handles as None, its opt_state and the views into it, `penalty` among them), _bind, the entries and the state_dict pair."""

    def __init__(self, policy, T=None, policy_lr=1e-4, value_lr=3e-4, epochs_policy=50, epochs_value=50, kl_target=1e-2, kl_cutoff_factor=2,
                 kl_cutoff_coef=1000, kl_init_penalty=1, conv_logpdf="exact", beta1=0.9, beta2=0.999, adam_eps=1e-8):
        self.policy = policy
        self.T, self.batch = None, int(policy.batch)
        self._settings = dict(policy_lr=policy_lr, value_lr=value_lr, epochs_policy=epochs_policy, epochs_value=epochs_value, kl_target=kl_target,
                              kl_cutoff_factor=kl_cutoff_factor, kl_cutoff_coef=kl_cutoff_coef, conv_logpdf=conv_logpdf, beta1=beta1, beta2=beta2,
                              adam_eps=adam_eps)
        self.fields = ppo_abi.ppo_fields(**self._settings)
        self.device = dev = policy.device
        self.epochs_policy, self.epochs_value = int(epochs_policy), int(epochs_value)
        self.kl_target = float(kl_target)
        self.kl_init_penalty = float(kl_init_penalty)
        lay = policy.layout
        self.policy_count, self.value_count = lay["policy_count"], lay["value_count"]
        self._alloc()
        self.penalty.fill_(self.kl_init_penalty)
        self.stats = torch.zeros(ppo_abi.STATS, dtype=torch.float64, device=dev)
        self._grad = {ppo_abi.POLICY: torch.zeros(self.policy_count, dtype=torch.float32, device=dev),
                      ppo_abi.VALUE: torch.zeros(self.value_count, dtype=torch.float32, device=dev)}
        self._loss = torch.zeros(2, dtype=torch.float64, device=dev)
        self._kl = torch.zeros(self.batch, dtype=torch.float64, device=dev)
        if T is not None:
            self._bind(T)

    # ---- argument checks ------------------------------------------------------------------------------------------------

    def _check(self, call, name, t, shape, dtype):
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            kind = {torch.float32: "float32", torch.int32: "int32", torch.float64: "float64"}[dtype]
            raise ValueError(f"{call}: {name} must be a contiguous {kind} {list(shape)} tensor on {self.device}")
        return t.data_ptr()

    def _rollout(self, call, rollout, slots):
        """rg_ppo_rollout over the named slots of a rollout buffer, each checked before the library sees its pointer: contiguous,
        of the shape and dtype rg_ppo.h gives, on this device."""
        if self.T is None:
            if int(rollout.T) < 1:
                raise ValueError(f"{call}: rollout.T is {rollout.T}, it must be at least 1")
            self._bind(rollout.T)
        p, T, B = self.policy, self.T, self.batch
        if int(rollout.T) != T:
            raise ValueError(f"{call}: rollout.T is {rollout.T}, this update was made for T = {T}")
        if int(rollout.batch) != B:
            raise ValueError(f"{call}: rollout.batch is {rollout.batch}, the policy's batch is {B}")
        f32, i32 = torch.float32, torch.int32
        shapes = dict(obs=((T, p.obs_dim, B), f32), action=((T, B, p.act_dim), f32), mean=((T, B, p.act_dim), f32), logstd=((p.act_dim,), f32),
                      adv=((T, B), f32), ret=((T, B), f32), mask=((T, B), i32))
        return ppo_abi.make_crollout(**{name: self._check(call, "rollout." + name, getattr(rollout, name, None), *shapes[name]) for name in slots})

    def _params(self, call):
        p = self.policy
        return (self._check(call, "policy.policy_params", p.policy_params, (self.policy_count,), torch.float32),
                self._check(call, "policy.value_params", p.value_params, (self.value_count,), torch.float32))

    def _out(self, call, out, which):
        """The gradient's tensor of an entry: the caller's, checked, or this object's own."""
        if out is None:
            return self._grad[which]
        self._check(call, "out", out, (self.policy_count if which == ppo_abi.POLICY else self.value_count,), torch.float32)
        return out

    def _kl_out(self, out):
        if out is None:
            return self._kl
        self._check("kl", "out", out, (self.batch,), torch.float64)
        return out

    def _adam_args(self, which, grad):
        """(ppo_abi.POLICY or VALUE, the gradient's tensor, the two pointers of _params) of adam(which, grad)."""
        which = {"policy": ppo_abi.POLICY, "value": ppo_abi.VALUE}.get(which, which)
        if which not in (ppo_abi.POLICY, ppo_abi.VALUE):
            raise ValueError("adam: which must be 'policy' or 'value'")
        grad = self._out("adam", grad, which)
        if self._handle is None:
            raise ValueError(f"adam: no rollout has been seen yet; pass T to {type(self).__name__} or call an entry that takes the rollout first")
        return which, grad, self._params("adam")

    def stats_dict(self):
        """The dict the host-side update returns, read from the device (this synchronises); a loss of a network with 0 epochs is
        None."""
        return {name: (None if x != x else x) for name, x in zip(ppo_abi.STAT_NAMES, self.stats.tolist())}


class DevicePPO(_DeviceUpdate):
    """update(rollout) enqueues rg_ppo_update for a RolloutBuffer of T ticks of policy.batch robots and returns the device
    tensor `stats` (float64 [6], ppo_abi.STAT_NAMES); stats_dict() reads it.  policy_grad / value_grad / adam / kl expose the
    single entries (update is their composition, after prepare).  It steps policy.policy_params and policy.value_params in
    place: the tensors rg_policy_act reads, at the same addresses.

        opt_state  float64 [opt_state_bytes / 8], the bytes of rg_ppo.h: steps (int64 [2] view), penalty (float64 [1] view),
                   moments (float32 view: m_policy, v_policy, m_value, v_value)
        workspace  scratch of the kernels (what prepare leaves there is read by policy_grad)

    The keywords are PPO's (and Adam's beta1, beta2, adam_eps, which PPO leaves at torch's defaults).  T, the rollout's length,
    sizes the workspace: given here, or taken from the first rollout an entry sees; after that every rollout must have it.
    A host-only policy (device="cpu") gives a host-only handle: arguments are checked, every entry then raises NO_DEVICE."""

    def _alloc(self):
        self._handle = self.workspace = None
        opt_bytes = (ppo_abi.OPT_HEADER_BYTES + 4 * 2 * (self.policy_count + self.value_count) + 7) // 8 * 8     # rg_ppo.h, opt_state
        self.opt_state = torch.zeros(opt_bytes // 8, dtype=torch.float64, device=self.device)
        self.steps = self.opt_state[:2].view(torch.int64)
        self.penalty = self.opt_state[2:3]
        self.moments = self.opt_state[ppo_abi.OPT_HEADER_BYTES // 8:].view(torch.float32)

    def _bind(self, T):
        """The handle and the workspace for rollouts of T ticks."""
        self.T = int(T)
        host_only = self.device.type == "cpu"
        self._handle = ppo_abi.PpoHandle(self.T, self.batch, ppo_abi.DEVICE_NONE if host_only else self.device, policy_settings=self.policy.fields,
                                         **self._settings)
        if self._handle.opt_state_bytes != self.opt_state.numel() * 8:
            raise RuntimeError("rg_ppo_opt_state_bytes disagrees with the layout of rg_ppo.h")
        self.workspace = torch.zeros(self._handle.workspace_bytes // 8, dtype=torch.float64, device=self.device)

    # ---- the entries ----------------------------------------------------------------------------------------------------

    def update(self, rollout):
        """rg_ppo_update on the current stream; returns self.stats (a device tensor; nothing is read on the host)."""
        ro = self._rollout("update", rollout, _SLOTS)
        pp, vp = self._params("update")
        self._handle.update(ro, self.policy.norm_state.data_ptr(), pp, vp, self.opt_state.data_ptr(), self.workspace.data_ptr(), self.stats.data_ptr())
        return self.stats

    def prepare(self, rollout):
        self._handle.prepare(self._rollout("prepare", rollout, ("adv", "mask")), self.workspace.data_ptr())

    def adv_stats(self):
        """(n clamped to 1, mean, std + 1e-8, n) as prepare left them: a float64 [4] device tensor."""
        off = self._handle.scalars_offset // 8
        return self.workspace[off:off + 4]

    def policy_grad(self, rollout, out=None):
        """(grad float32 [policy_count], loss float64 [] view) of PPO.policy_loss after prepare(rollout); out: the gradient's tensor."""
        ro = self._rollout("policy_grad", rollout, ("obs", "action", "mean", "logstd", "adv", "mask"))
        pp, _ = self._params("policy_grad")
        grad = self._out("policy_grad", out, ppo_abi.POLICY)
        self._handle.policy_grad(ro, self.policy.norm_state.data_ptr(), pp, self.opt_state.data_ptr(), self.workspace.data_ptr(), grad.data_ptr(),
                                 self._loss[0:1].data_ptr())
        return grad, self._loss[0]

    def value_grad(self, rollout, out=None):
        ro = self._rollout("value_grad", rollout, ("obs", "ret", "mask"))
        _, vp = self._params("value_grad")
        grad = self._out("value_grad", out, ppo_abi.VALUE)
        self._handle.value_grad(ro, self.policy.norm_state.data_ptr(), vp, self.workspace.data_ptr(), grad.data_ptr(), self._loss[1:2].data_ptr())
        return grad, self._loss[1]

    def adam(self, which, grad):
        """One rg_ppo_adam step on the policy's buffer `which` ("policy" / "value" or ppo_abi.POLICY / VALUE) with `grad`."""
        which, grad, params = self._adam_args(which, grad)
        self._handle.adam(which, params[which], grad.data_ptr(), self.opt_state.data_ptr())

    def kl(self, rollout, out=None):
        """KL(behaviour || current) per robot, float64 [B] on the device."""
        ro = self._rollout("kl", rollout, ("obs", "mean", "logstd", "mask"))
        pp, _ = self._params("kl")
        out = self._kl_out(out)
        self._handle.kl(ro, self.policy.norm_state.data_ptr(), pp, self.workspace.data_ptr(), out.data_ptr())
        return out

    # ---- state ----------------------------------------------------------------------------------------------------------

    def state_dict(self):
        return dict(opt_state=self.opt_state.clone(), fields=dict(self.fields), T=self.T, batch=self.batch)

    def load_state_dict(self, state):
        """Copies INTO opt_state (its address does not change): Adam's moments and step counts and the penalty.  The state must
        come from the same settings, batch and (where both are known) T."""
        t = state["opt_state"]
        if not torch.is_tensor(t) or t.dtype != torch.float64 or tuple(t.shape) != tuple(self.opt_state.shape):
            raise ValueError("load_state_dict: opt_state must be a float64 tensor of this configuration's size")
        if dict(state["fields"]) != dict(self.fields) or int(state["batch"]) != self.batch:
            raise ValueError("load_state_dict: the state was saved from another configuration")
        if state.get("T") is not None and self.T is not None and int(state["T"]) != self.T:
            raise ValueError(f"load_state_dict: the state was saved for T = {state['T']}, this update is for T = {self.T}")
        self.opt_state.copy_(t)

    def close(self):
        if self._handle is not None:
            self._handle.close()
