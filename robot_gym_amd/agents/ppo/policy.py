"""The Gaussian policy and value network of the PPO agent for B robots (include/rg_policy.h): parameters, normaliser and
act state as device tensors, acting through the HIP kernel, and the same arithmetic as differentiable torch ops for the
update.  The reference: agents/ppo/scripts/networks.py (ForwardGaussianPolicy) and agents/ppo/normalize.py."""
import math

import torch

from robot_gym_amd.core import policy_abi


class BatchedGaussianPolicy:
    """Owns the rg_policy handle and the tensors its kernels read and write:

        policy_params  float32 [policy_count]   hidden layers and the mean head, W[in][out] then b[out] each, logstd at the end
        value_params   float32 [value_count]    hidden layers and the scalar head
        act_state      int64 [2, B]             key (arange(B)) and counter of the noise stream
        norm_state     float64 [195]            count / mean / var_sum, 64 observation columns and the reward (policy_abi.NORM_*)

    The views in policy_layers / value_layers ((W [in, out], b [out]) per layer, head last) and logstd alias the two parameter
    tensors: an optimiser stepping on policy_params / value_params in place changes what the next act() reads, with no copy.
    device="cpu" makes a host-only policy (evaluate, normalize_*, state_dict work; act raises NO_DEVICE); dtype is the
    parameters' type there (the kernels read float32 only)."""

    def __init__(self, batch, obs_dim=16, act_dim=2, policy_layers=(200, 100), value_layers=(200, 100), seed=0, device=None, dtype=None,
                 obs_clip=5.0, reward_clip=10.0, discount=0.985, gae_lambda=1.0):
        self.batch = B = int(batch)
        settings = dict(obs_dim=obs_dim, act_dim=act_dim, policy_layers=tuple(policy_layers), value_layers=tuple(value_layers), seed=seed,
                        obs_clip=obs_clip, reward_clip=reward_clip, discount=discount, gae_lambda=gae_lambda)
        host_only = device is not None and torch.device(device).type == "cpu"
        self._handle = policy_abi.PolicyHandle(B, policy_abi.DEVICE_NONE if host_only else device, **settings)
        self.fields = self._handle.fields
        self.device = dev = torch.device("cpu") if host_only else self._handle.device
        self.dtype = dtype = dtype or torch.float32
        if not host_only and dtype != torch.float32:
            raise ValueError("the kernels read float32 parameters")
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.obs_clip, self.reward_clip = float(obs_clip), float(reward_clip)
        lay = self.layout = self._handle.layout
        self.policy_params = torch.zeros(lay["policy_count"], dtype=dtype, device=dev)
        self.value_params = torch.zeros(lay["value_count"], dtype=dtype, device=dev)
        self.act_state = torch.zeros(2, B, dtype=torch.int64, device=dev)
        self.act_state[0] = torch.arange(B, dtype=torch.int64, device=dev)
        self.norm_state = torch.zeros(policy_abi.NORM_ROWS, dtype=torch.float64, device=dev)
        self._scratch_action = torch.zeros(B, self.act_dim, dtype=torch.float32, device=dev)
        self.policy_params.requires_grad_(True)   # leaves: the views below carry gradients back to the two buffers
        self.value_params.requires_grad_(True)
        self.init_parameters(seed)

    @staticmethod
    def _views(buf, layers):
        return [(buf[w:w + i * o].view(i, o), buf[b:b + o]) for i, o, w, b in layers]

    @property
    def policy_layers(self):
        """[(W [in, out], b [out]), ...] of the policy, the mean head last: views of policy_params."""
        return self._views(self.policy_params, self.layout["policy"])

    @property
    def value_layers(self):
        return self._views(self.value_params, self.layout["value"])

    @property
    def logstd(self):
        off = self.layout["logstd_offset"]
        return self.policy_params[off:off + self.act_dim]

    def init_parameters(self, seed=0):
        """The reference's initialisers from a seeded torch generator: Glorot-uniform weights (limit sqrt(6 / (in + out))) for the
        hidden layers and the value head, a truncated normal of variance 1.3 * 0.1 / in (variance scaling with factor 0.1 on
        fan-in, cut at two standard deviations) for the mean head, zero biases, logstd = -1."""
        gen = torch.Generator().manual_seed(int(seed))
        with torch.no_grad():
            for net, layers in ((0, self.policy_layers), (1, self.value_layers)):
                for k, (W, b) in enumerate(layers):
                    fan_in, fan_out = W.shape
                    if net == 0 and k == len(layers) - 1:
                        w = torch.empty(fan_in, fan_out, dtype=torch.float64)
                        torch.nn.init.trunc_normal_(w, mean=0.0, std=math.sqrt(1.3 * 0.1 / fan_in), a=-2.0 * math.sqrt(1.3 * 0.1 / fan_in),
                                                    b=2.0 * math.sqrt(1.3 * 0.1 / fan_in), generator=gen)
                    else:
                        limit = math.sqrt(6.0 / (fan_in + fan_out))
                        w = (torch.rand(fan_in, fan_out, dtype=torch.float64, generator=gen) * 2.0 - 1.0) * limit
                    W.copy_(w.to(self.dtype))
                    b.zero_()
            self.logstd.fill_(-1.0)

    # ---- the kernel ---------------------------------------------------------------------------------------------------

    def act(self, obs_cm, sample=True, out=None):
        """rg_policy_act on the current stream.  obs_cm: contiguous float32 [obs_dim, B] (BatchedGoEnv.obs.t()).  out: a dict with
        any of action [B, act_dim], mean [B, act_dim], value [B], logprob [B] (contiguous float32 tensors on this device) to write
        into; a missing action is written to a tensor of this object.  Returns the dict, action included."""
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
        self._handle.act(obs_cm.data_ptr(), self.norm_state.data_ptr(), self.policy_params.data_ptr(), self.value_params.data_ptr(),
                         self.act_state.data_ptr(), policy_abi.MODE_SAMPLE if sample else policy_abi.MODE_MEAN, ptr["action"], ptr.get("mean"),
                         ptr.get("value"), ptr.get("logprob"))
        return out

    def _ptr(self, call, name, t, shape, dtype, optional=False):
        """data_ptr() of a tensor the kernels may follow: contiguous, of this shape and dtype, on this device.  None gives None
        where the argument is optional.  The kernels check nothing: a pointer that passes here is read or written as it stands."""
        if t is None and optional:
            return None
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            kind = "float32" if dtype == torch.float32 else "int32"
            raise ValueError(f"{call}: {name} must be a contiguous {kind} {list(shape)} tensor on {self.device}" + (" or None" if optional else ""))
        return t.data_ptr()

    def record(self, obs_cm, reward, done, mask=None, ro_obs=None, ro_reward=None, ro_done=None):
        """rg_policy_record: the rollout slot and both normalisers (robots with mask != 0; None: all).  obs_cm, ro_obs: contiguous
        float32 [obs_dim, B]; reward, ro_reward: float32 [B]; done, mask, ro_done: int32 [B]; all on this device."""
        B, f32, i32 = self.batch, torch.float32, torch.int32
        ptrs = [self._ptr("record", "obs_cm", obs_cm, (self.obs_dim, B), f32), self._ptr("record", "reward", reward, (B,), f32),
                self._ptr("record", "done", done, (B,), i32), self._ptr("record", "mask", mask, (B,), i32, True), self.norm_state.data_ptr(),
                self._ptr("record", "ro_obs", ro_obs, (self.obs_dim, B), f32, True), self._ptr("record", "ro_reward", ro_reward, (B,), f32, True),
                self._ptr("record", "ro_done", ro_done, (B,), i32, True)]
        self._handle.record(*ptrs)

    def returns(self, rollout, bootstrap=True):
        """rg_policy_returns over a RolloutBuffer of this batch: fills rollout.ret and rollout.adv.  reward, value, ret, adv:
        contiguous float32 [T, B]; done: int32 [T, B]; last_value: float32 [B] (may be None without bootstrap)."""
        T, B, f32 = int(rollout.T), self.batch, torch.float32
        if int(rollout.batch) != B:
            raise ValueError(f"returns: rollout.batch is {rollout.batch}, the policy's batch is {B}")
        if T < 1:
            raise ValueError(f"returns: rollout.T is {T}, it must be at least 1")
        ptr = {name: self._ptr("returns", "rollout." + name, getattr(rollout, name), (T, B), f32) for name in ("reward", "value", "ret", "adv")}
        done = self._ptr("returns", "rollout.done", rollout.done, (T, B), torch.int32)
        last = self._ptr("returns", "rollout.last_value", rollout.last_value, (B,), f32, optional=not bootstrap)
        self._handle.returns(ptr["reward"], ptr["value"], done, last, self.norm_state.data_ptr(), T, bootstrap, ptr["ret"], ptr["adv"])

    # ---- the same arithmetic in torch, for the update -----------------------------------------------------------------

    def _norm(self, col):
        n = self.norm_state.view(3, policy_abi.NORM_COLS)
        return n[0, col], n[1, col], n[2, col]

    def _scale(self, count, var_sum):
        std = torch.sqrt(var_sum / (count - 1.0).clamp_min(1.0) + 1e-4) + 1e-8
        return torch.where(count > 1.0, std, torch.ones_like(std))

    def normalize_obs(self, obs):
        """StreamingNormalize.transform of observations [..., obs_dim] with the current state, in float64; returned in the
        parameters' dtype."""
        cols = slice(0, self.obs_dim)
        count, mean, var_sum = self._norm(cols)
        v = (obs.to(torch.float64) - mean) / self._scale(count, var_sum)
        if self.obs_clip > 0:
            v = v.clamp(-self.obs_clip, self.obs_clip)
        return v.to(self.dtype)

    def normalize_reward(self, reward):
        """The reward normaliser's transform (scale only) of rewards [...], float64."""
        count, _, var_sum = self._norm(policy_abi.NORM_REWARD)
        v = reward.to(torch.float64) / self._scale(count, var_sum)
        return v.clamp(-self.reward_clip, self.reward_clip) if self.reward_clip > 0 else v

    def evaluate(self, obs_norm):
        """(mean [..., act_dim], value [...]) of normalised observations [..., obs_dim]: differentiable torch ops over the views of
        the two parameter tensors."""
        x, pl = obs_norm, self.policy_layers
        for k, (W, b) in enumerate(pl):
            x = x @ W + b
            x = torch.tanh(x) if k == len(pl) - 1 else torch.relu(x)
        v, vl = obs_norm, self.value_layers
        for k, (W, b) in enumerate(vl):
            v = v @ W + b
            if k < len(vl) - 1:
                v = torch.relu(v)
        return x, v[..., 0]

    # ---- state ------------------------------------------------------------------------------------------------------

    def clone(self, src, dst):
        """The act state (key and counter of the noise stream) of robot src[k] into robot dst[k]: with BatchedGoEnv.clone the
        clone acts as its source does.  Parameters and normalisers are shared by the batch."""
        s = torch.as_tensor(src, dtype=torch.int64, device=self.device).reshape(-1)
        t = torch.as_tensor(dst, dtype=torch.int64, device=self.device).reshape(-1)
        self.act_state.index_copy_(1, t, self.act_state.index_select(1, s))

    def state_dict(self):
        return dict(policy_params=self.policy_params.detach().clone(), value_params=self.value_params.detach().clone(),
                    norm_state=self.norm_state.clone(), act_state=self.act_state.clone(), fields=dict(self.fields))

    def load_state_dict(self, state):
        """Copies INTO the tensors this object owns (their addresses do not change)."""
        if dict(state["fields"], seed=0) != dict(self.fields, seed=0):
            raise ValueError("load_state_dict: the state was saved from another configuration")
        with torch.no_grad():
            for name in ("policy_params", "value_params", "norm_state", "act_state"):
                getattr(self, name).copy_(state[name])

    def close(self):
        self._handle.close()
