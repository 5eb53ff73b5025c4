"""The DDPG agent for B robots on the device (include/rg_ddpg.h): the reference's agents/ddpg/simple_ddpg_agent.py (a keras-rl
DDPGAgent) with every piece -- acting with Ornstein-Uhlenbeck noise, the replay ring with keras-rl's window rule, sampling, both
gradients, clipped Adam and the soft target update -- as HIP kernels on the current stream, with no host read."""
import math

import torch

from robot_gym_amd.core import ddpg_abi

_NETS = ("actor", "critic")


class BatchedDDPGAgent:
    """Owns the rg_ddpg handle and every tensor its kernels read and write:

        actor_params, target_actor_params     float32 [actor_count]    W[in][out] then b[out] per layer, the tanh head last
        critic_params, target_critic_params   float32 [critic_count]   input = the action, then the window
        ring_obs [C, obs_dim, B], ring_action [C, B, act_dim], ring_reward [C, B] float32, ring_done [C, B] int32
        ring_state   int64 [4]                head, count, updates, reserved -- on the device
        ou_state     float32 [B, act_dim]     the Ornstein-Uhlenbeck process of each robot
        act_state    int64 [2, B]             key (arange(B)) and counter of the noise stream
        opt_state    float64 [opt_state_bytes / 8]   the bytes of rg_ddpg.h: steps (int64 [2] view), moments (float32 view)
        workspace, stats (float64 [6], ddpg_abi.STAT_NAMES), idx (int32 [M, 2], the last sample)

    config: the settings of ddpg_abi.DEFAULTS (the reference's).  Initialisation is Keras's Dense default: Glorot-uniform weights,
    zero biases; the targets are hard copies.  device="cpu" makes a host-only agent: arguments are checked, every entry then
    raises NO_DEVICE."""

    def __init__(self, batch, capacity, device=None, **config):
        self.batch = B = int(batch)
        self._config = dict(config, capacity=int(capacity))
        host_only = device is not None and torch.device(device).type == "cpu"
        self._handle = ddpg_abi.DdpgHandle(B, ddpg_abi.DEVICE_NONE if host_only else device, **self._config)
        self.fields = f = self._handle.fields
        self.device = dev = torch.device("cpu") if host_only else self._handle.device
        self.obs_dim, self.act_dim, self.window, self.capacity, self.minibatch = (int(f[k]) for k in ("obs_dim", "act_dim", "window", "capacity", "minibatch"))
        lay = self.layout = self._handle.layout
        self.counts = {ddpg_abi.ACTOR: lay["actor_count"], ddpg_abi.CRITIC: lay["critic_count"]}
        C_, A, M = self.capacity, self.act_dim, self.minibatch
        f32 = dict(dtype=torch.float32, device=dev)
        self.actor_params = torch.zeros(lay["actor_count"], **f32)
        self.critic_params = torch.zeros(lay["critic_count"], **f32)
        self.target_actor_params = torch.zeros_like(self.actor_params)
        self.target_critic_params = torch.zeros_like(self.critic_params)
        self.ring_obs = torch.zeros(C_, self.obs_dim, B, **f32)
        self.ring_action = torch.zeros(C_, B, A, **f32)
        self.ring_reward = torch.zeros(C_, B, **f32)
        self.ring_done = torch.zeros(C_, B, dtype=torch.int32, device=dev)
        self.ring_state = torch.zeros(ddpg_abi.RING_STATE, dtype=torch.int64, device=dev)
        self.ou_state = torch.zeros(B, A, **f32)
        self.act_state = torch.zeros(2, B, dtype=torch.int64, device=dev)
        self.act_state[0] = torch.arange(B, dtype=torch.int64, device=dev)
        if self._handle.opt_state_bytes != (ddpg_abi.OPT_HEADER_BYTES + 8 * (lay["actor_count"] + lay["critic_count"]) + 7) // 8 * 8:
            raise RuntimeError("rg_ddpg_opt_state_bytes disagrees with the layout of rg_ddpg.h")
        self.opt_state = torch.zeros(self._handle.opt_state_bytes // 8, dtype=torch.float64, device=dev)
        self.steps = self.opt_state[:2].view(torch.int64)
        self.moments = self.opt_state[ddpg_abi.OPT_HEADER_BYTES // 8:].view(torch.float32)
        self.workspace = torch.zeros(self._handle.workspace_bytes // 8, dtype=torch.float64, device=dev)
        self.stats = torch.zeros(ddpg_abi.STATS, dtype=torch.float64, device=dev)
        self.idx = torch.zeros(M, 2, dtype=torch.int32, device=dev)
        self._grad = {w: torch.zeros(n, **f32) for w, n in self.counts.items()}
        self._loss = torch.zeros(2, dtype=torch.float64, device=dev)
        self.grad_norm = torch.zeros(1, dtype=torch.float64, device=dev)
        self._action = torch.zeros(B, A, **f32)
        self._obs_slot = torch.zeros(self.obs_dim, B, **f32)
        self.ticks_stored = 0            # host count of store() calls: what collect() compares with its warm-up
        self._ring = ddpg_abi.make_cring(self.ring_obs.data_ptr(), self.ring_action.data_ptr(), self.ring_reward.data_ptr(), self.ring_done.data_ptr(),
                                         self.ring_state.data_ptr())
        self.init_parameters(int(f["seed"]))

    # ---- parameters -----------------------------------------------------------------------------------------------------

    def layers(self, which, target=False):
        """[(W [in, out], b [out]), ...] of a network ("actor" / "critic"), the head last: views of its parameter tensor."""
        buf = getattr(self, ("target_" if target else "") + which + "_params")
        return [(buf[w:w + i * o].view(i, o), buf[b:b + o]) for i, o, w, b in self.layout[which]]

    def init_parameters(self, seed=0):
        """Glorot-uniform weights (limit sqrt(6 / (in + out))) and zero biases from a seeded torch generator, then hard_update()."""
        gen = torch.Generator().manual_seed(int(seed))
        for which in _NETS:
            for W, b in self.layers(which):
                fan_in, fan_out = W.shape
                limit = math.sqrt(6.0 / (fan_in + fan_out))
                W.copy_(((torch.rand(fan_in, fan_out, dtype=torch.float64, generator=gen) * 2.0 - 1.0) * limit).to(torch.float32))
                b.zero_()
        self.hard_update()

    def hard_update(self):
        """The targets become copies of the online networks (in place)."""
        self.target_actor_params.copy_(self.actor_params)
        self.target_critic_params.copy_(self.critic_params)

    # ---- argument checks ------------------------------------------------------------------------------------------------

    def _ptr(self, call, name, t, shape, dtype, optional=False):
        """data_ptr() of a tensor the kernels may follow: contiguous, of this shape and dtype, on this device.  The kernels check
        nothing: a pointer that passes here is read or written as it stands."""
        if t is None and optional:
            return None
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != self.device:
            kind = {torch.float32: "float32", torch.int32: "int32", torch.float64: "float64", torch.int64: "int64"}[dtype]
            raise ValueError(f"{call}: {name} must be a contiguous {kind} {list(shape)} tensor on {self.device}" + (" or None" if optional else ""))
        return t.data_ptr()

    def _own(self, call):
        """The pointers of the tensors this object owns, checked like a caller's: an attribute may have been replaced."""
        f32, B, C_, A = torch.float32, self.batch, self.capacity, self.act_dim
        p = {name: self._ptr(call, name, getattr(self, name), (self.counts[w],), f32)
             for w, names in ((ddpg_abi.ACTOR, ("actor_params", "target_actor_params")), (ddpg_abi.CRITIC, ("critic_params", "target_critic_params")))
             for name in names}
        ring = ddpg_abi.make_cring(self._ptr(call, "ring_obs", self.ring_obs, (C_, self.obs_dim, B), f32),
                                   self._ptr(call, "ring_action", self.ring_action, (C_, B, A), f32),
                                   self._ptr(call, "ring_reward", self.ring_reward, (C_, B), f32),
                                   self._ptr(call, "ring_done", self.ring_done, (C_, B), torch.int32),
                                   self._ptr(call, "ring_state", self.ring_state, (ddpg_abi.RING_STATE,), torch.int64))
        p["opt_state"] = self._ptr(call, "opt_state", self.opt_state, (self._handle.opt_state_bytes // 8,), torch.float64)
        p["workspace"] = self._ptr(call, "workspace", self.workspace, (self._handle.workspace_bytes // 8,), torch.float64)
        p["ou_state"] = self._ptr(call, "ou_state", self.ou_state, (B, A), f32)
        p["act_state"] = self._ptr(call, "act_state", self.act_state, (2, B), torch.int64)
        return ring, p

    def _which(self, call, which):
        which = {"actor": ddpg_abi.ACTOR, "critic": ddpg_abi.CRITIC}.get(which, which)
        if which not in (ddpg_abi.ACTOR, ddpg_abi.CRITIC):
            raise ValueError(f"{call}: which must be 'actor' or 'critic'")
        return which

    def _out(self, call, out, which):
        if out is None:
            return self._grad[which]
        self._ptr(call, "out", out, (self.counts[which],), torch.float32)
        return out

    def _idx(self, call, idx):
        if idx is None:
            return self.idx
        self._ptr(call, "idx", idx, (self.minibatch, 2), torch.int32)
        return idx

    # ---- the entries ----------------------------------------------------------------------------------------------------

    def act(self, obs, noise=True, out=None):
        """rg_ddpg_act on the current stream.  obs: contiguous float32 [obs_dim, B] (BatchedGoEnv.obs.t()), the current
        observation; the rest of the window comes from the ring.  noise=False is the deterministic policy: action = mean, the
        OU state and the counters are left alone.  out: a dict with any of action, mean (contiguous float32 [B, act_dim]); a
        missing action is written to a tensor of this object.  Returns the dict, action included."""
        B, A, f32 = self.batch, self.act_dim, torch.float32
        obs_ptr = self._ptr("act", "obs", obs, (self.obs_dim, B), f32)
        out = dict(out or {})
        out.setdefault("action", self._action)
        for name in out:
            if name not in ("action", "mean"):
                raise TypeError(f"act: unknown output {name!r}")
        ptr = {name: self._ptr("act", f"out[{name!r}]", t, (B, A), f32) for name, t in out.items()}
        ring, p = self._own("act")
        self._handle.act(ring, obs_ptr, p["actor_params"], p["ou_state"], p["act_state"], ddpg_abi.MODE_SAMPLE if noise else ddpg_abi.MODE_MEAN,
                         ptr["action"], ptr.get("mean"))
        return out

    def store(self, obs, action, reward, done):
        """rg_ddpg_store: one tick of all B robots into the ring; the OU rows of the robots with done != 0 are zeroed.  obs: the
        observation that was acted on, contiguous float32 [obs_dim, B]; action float32 [B, act_dim]; reward float32 [B]; done int32 [B]."""
        B, f32 = self.batch, torch.float32
        ptrs = [self._ptr("store", "obs", obs, (self.obs_dim, B), f32), self._ptr("store", "action", action, (B, self.act_dim), f32),
                self._ptr("store", "reward", reward, (B,), f32), self._ptr("store", "done", done, (B,), torch.int32)]
        ring, p = self._own("store")
        self._handle.store(ring, *ptrs, p["ou_state"])
        self.ticks_stored += 1

    def sample(self, out=None):
        """rg_ddpg_sample: (age, robot) of M transitions into out (int32 [M, 2]; None: self.idx).  A short ring writes nothing."""
        idx = self._idx("sample", out)
        ring, _ = self._own("sample")
        self._handle.sample(ring, idx.data_ptr())
        return idx

    def critic_grad(self, idx=None, out=None):
        """(grad float32 [critic_count], loss float64 [] view) of the critic's loss over the transitions idx (None: self.idx)."""
        idx, grad = self._idx("critic_grad", idx), self._out("critic_grad", out, ddpg_abi.CRITIC)
        ring, p = self._own("critic_grad")
        self._handle.critic_grad(ring, idx.data_ptr(), p["critic_params"], p["target_actor_params"], p["target_critic_params"], p["workspace"],
                                 grad.data_ptr(), self._loss[0:1].data_ptr())
        return grad, self._loss[0]

    def actor_grad(self, idx=None, out=None):
        """(grad float32 [actor_count], loss float64 [] view): the deterministic policy gradient through the critic."""
        idx, grad = self._idx("actor_grad", idx), self._out("actor_grad", out, ddpg_abi.ACTOR)
        ring, p = self._own("actor_grad")
        self._handle.actor_grad(ring, idx.data_ptr(), p["actor_params"], p["critic_params"], p["workspace"], grad.data_ptr(), self._loss[1:2].data_ptr())
        return grad, self._loss[1]

    def adam(self, which, grad=None, gated=False):
        """One clipped rg_ddpg_adam step on the network `which` ("actor" / "critic") with grad (None: the tensor the gradient
        entry of that network wrote); the clip scales grad in place; the norm before the clip goes to self.grad_norm.
        gated: do nothing on a short ring, as update() does."""
        which = self._which("adam", which)
        grad = self._out("adam", grad, which)
        _, p = self._own("adam")
        self._handle.adam(which, p["actor_params" if which == ddpg_abi.ACTOR else "critic_params"], grad.data_ptr(), p["opt_state"], p["workspace"],
                          self.grad_norm.data_ptr(), self.ring_state.data_ptr() if gated else None)

    def soft_update(self, which, gated=False):
        """target = (1 - tau) * target + tau * online for the network `which`."""
        which = self._which("soft_update", which)
        _, p = self._own("soft_update")
        name = "actor_params" if which == ddpg_abi.ACTOR else "critic_params"
        self._handle.soft_update(which, p["target_" + name], p[name], self.ring_state.data_ptr() if gated else None)

    def advance(self):
        """updates += 1 in ring_state (nothing on a short ring): the last step of an update."""
        ring, _ = self._own("advance")
        self._handle.advance(ring)

    def update(self, n=1):
        """rg_ddpg_update on the current stream: n whole updates; returns self.stats (a device tensor; nothing is read on the host)."""
        ring, p = self._own("update")
        stats = self._ptr("update", "stats", self.stats, (ddpg_abi.STATS,), torch.float64)
        self._handle.update(ring, p["actor_params"], p["critic_params"], p["target_actor_params"], p["target_critic_params"], p["opt_state"],
                            p["workspace"], int(n), stats)
        return self.stats

    def stats_dict(self):
        """stats read from the device (this synchronises); a figure no update has written is None."""
        return {name: (None if x != x else x) for name, x in zip(ddpg_abi.STAT_NAMES, self.stats.tolist())}

    # ---- state ----------------------------------------------------------------------------------------------------------

    _STATE = ("actor_params", "critic_params", "target_actor_params", "target_critic_params", "ring_obs", "ring_action", "ring_reward", "ring_done",
              "ring_state", "ou_state", "act_state", "opt_state")

    def state_dict(self):
        out = {name: getattr(self, name).clone() for name in self._STATE}
        out.update(fields=dict(self.fields), batch=self.batch, ticks_stored=self.ticks_stored)
        return out

    def load_state_dict(self, state):
        """Copies INTO the tensors this object owns (their addresses do not change).  The state must come from the same
        configuration (the seed aside) and batch."""
        if dict(state["fields"], seed=0) != dict(self.fields, seed=0) or int(state["batch"]) != self.batch:
            raise ValueError("load_state_dict: the state was saved from another configuration")
        for name in self._STATE:
            t, mine = state[name], getattr(self, name)
            if not torch.is_tensor(t) or t.dtype != mine.dtype or tuple(t.shape) != tuple(mine.shape):
                raise ValueError(f"load_state_dict: {name} must be a {mine.dtype} tensor of shape {list(mine.shape)}")
        for name in self._STATE:
            getattr(self, name).copy_(state[name])
        self.ticks_stored = int(state["ticks_stored"])

    def clone(self):
        """A second agent of the same configuration holding a copy of every piece of state: it continues as this one does."""
        twin = BatchedDDPGAgent(self.batch, device=self.device, **self._config)
        twin.load_state_dict(self.state_dict())
        return twin

    def close(self):
        self._handle.close()
