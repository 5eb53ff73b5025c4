"""ctypes shim over the C-ABI of include/rg_ddpg.h (the DDPG agent on the device in librg_mpc.so).

Plumbing only, like ppo_abi: it loads the same library, mirrors rg_ddpg_config, rg_ddpg_layout and rg_ddpg_ring, turns negative
status codes into exceptions and owns one rg_ddpg_handle.  There is NO CPU fallback: without the library or a GPU the handle
raises.  Every buffer is a caller-owned tensor (layouts: rg_ddpg.h).
"""
import ctypes as C

from robot_gym_amd.core.c_abi import Handle, RgError, create_status as _create_status, d, fp, i32, i64, load, merged, resolve_device

ABI_VERSION = 1
MAX_OBS, MAX_ACT, MAX_WINDOW, MAX_INPUT, MAX_LAYERS, MAX_WIDTH = 64, 4, 8, 128, 3, 256
TILE = 16                # RG_DDPG_TILE: samples per tile of a sweep, robots per workgroup of act
MAX_GROUPS = 256         # RG_DDPG_MAX_GROUPS
STATS = 6                # RG_DDPG_STATS
OPT_HEADER_BYTES = 16    # RG_DDPG_OPT_HEADER_BYTES: int64 step[2]
RING_STATE = 4           # RG_DDPG_RING_STATE: head, count, updates, reserved
DEVICE_NONE = -1
MODE_SAMPLE, MODE_MEAN = 0, 1
ACTOR, CRITIC = 0, 1
STAT_NAMES = ("critic_loss_first", "critic_loss_last", "actor_loss_first", "actor_loss_last", "mean_q_last", "critic_grad_norm_last")
STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE"}     # rg_ddpg_status has no ALLOC


class RgDdpgError(RgError):
    unit, names = "rg_ddpg", STATUS


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("obs_dim", i32), ("act_dim", i32), ("window", i32), ("n_actor_layers", i32), ("n_critic_layers", i32),
        ("actor_layers", i32 * MAX_LAYERS), ("critic_layers", i32 * MAX_LAYERS), ("capacity", i32), ("minibatch", i32), ("gamma", d), ("tau", d),
        ("actor_lr", d), ("critic_lr", d), ("beta1", d), ("beta2", d), ("adam_eps", d), ("clipnorm", d), ("ou_theta", d), ("ou_mu", d),
        ("ou_sigma", d), ("ou_dt", d), ("seed", C.c_uint64),
    ]


class CLayout(C.Structure):
    _fields_ = [
        ("actor_count", i32), ("critic_count", i32), ("n_actor", i32), ("n_critic", i32),
        ("actor_in", i32 * 4), ("actor_out", i32 * 4), ("actor_w", i32 * 4), ("actor_b", i32 * 4),
        ("critic_in", i32 * 4), ("critic_out", i32 * 4), ("critic_w", i32 * 4), ("critic_b", i32 * 4),
    ]


class CRing(C.Structure):
    _fields_ = [("obs", fp), ("action", fp), ("reward", fp), ("done", fp), ("state", fp)]


EXPORTS = ("rg_ddpg_create", "rg_ddpg_destroy", "rg_ddpg_last_error", "rg_ddpg_abi_version", "rg_ddpg_config_size", "rg_ddpg_layout_size",
           "rg_ddpg_ring_size", "rg_ddpg_tile", "rg_ddpg_workspace_bytes", "rg_ddpg_opt_state_bytes", "rg_ddpg_groups", "rg_ddpg_lds_bytes",
           "rg_ddpg_param_layout", "rg_ddpg_act", "rg_ddpg_store", "rg_ddpg_sample", "rg_ddpg_critic_grad", "rg_ddpg_actor_grad", "rg_ddpg_adam",
           "rg_ddpg_soft_update", "rg_ddpg_advance", "rg_ddpg_update")

# the reference's agents/ddpg/simple_ddpg_agent.py (Adam's betas and epsilon are torch's and Keras's defaults, 1e-8 for both here);
# the capacity is the caller's choice: a tick holds all B robots
DEFAULTS = dict(obs_dim=16, act_dim=2, window=5, actor_layers=(128, 128, 64), critic_layers=(256, 256, 128), capacity=1024, minibatch=32, gamma=0.99,
                tau=1e-3, actor_lr=1e-3, critic_lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, clipnorm=1.0, ou_theta=0.5, ou_mu=0.4, ou_sigma=0.3,
                ou_dt=1e-2, seed=0)
_FLOATS = ("gamma", "tau", "actor_lr", "critic_lr", "beta1", "beta2", "adam_eps", "clipnorm", "ou_theta", "ou_mu", "ou_sigma", "ou_dt")

_RING = C.POINTER(CRing)
# rg_ddpg.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "workspace_bytes": (i64, [fp]),
    "opt_state_bytes": (i64, [fp]),
    "groups": (i32, [fp]),
    "lds_bytes": (i32, [fp]),
    "param_layout": (i32, [C.POINTER(CConfig), C.POINTER(CLayout)]),
    "act": (i32, [fp, _RING, fp, fp, fp, fp, i32, fp, fp, fp]),
    "store": (i32, [fp, _RING, fp, fp, fp, fp, fp, fp]),
    "sample": (i32, [fp, _RING, fp, fp]),
    "critic_grad": (i32, [fp, _RING, fp, fp, fp, fp, fp, fp, fp, fp]),
    "actor_grad": (i32, [fp, _RING, fp, fp, fp, fp, fp, fp, fp]),
    "adam": (i32, [fp, i32, fp, fp, fp, fp, fp, fp, fp]),
    "soft_update": (i32, [fp, i32, fp, fp, fp, fp]),
    "advance": (i32, [fp, _RING, fp]),
    "update": (i32, [fp, _RING, fp, fp, fp, fp, fp, fp, i32, fp, fp]),
}


def load_library(path=None):
    """The rg_ddpg_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_ddpg", "the DDPG agent has no CPU fallback", SIGNATURES, {"config": CConfig, "layout": CLayout, "ring": CRing},
                {"tile": TILE}, ABI_VERSION, path)


def ddpg_fields(**settings):
    """The value of every rg_ddpg_config setting as a dict: DEFAULTS overridden by `settings`."""
    out = merged(DEFAULTS, settings, "ddpg")
    for name in ("actor_layers", "critic_layers"):
        out[name] = tuple(int(w) for w in out[name])
        if len(out[name]) > MAX_LAYERS:
            raise ValueError(f"{name}: at most {MAX_LAYERS} hidden layers, got {len(out[name])}")
    return out


def make_cconfig(**settings):
    f = ddpg_fields(**settings)
    c = CConfig()
    c.abi_version = ABI_VERSION
    for name in ("obs_dim", "act_dim", "window", "capacity", "minibatch", "seed"):
        setattr(c, name, int(f[name]))
    c.n_actor_layers, c.n_critic_layers = len(f["actor_layers"]), len(f["critic_layers"])
    for k, w in enumerate(f["actor_layers"]):
        c.actor_layers[k] = w
    for k, w in enumerate(f["critic_layers"]):
        c.critic_layers[k] = w
    for name in _FLOATS:
        setattr(c, name, float(f[name]))
    return c


def make_cring(obs=None, action=None, reward=None, done=None, state=None):
    r = CRing()
    r.obs, r.action, r.reward, r.done, r.state = obs, action, reward, done, state
    return r


def param_layout(cconfig=None, **settings):
    """rg_ddpg_param_layout as a dict: actor_count, critic_count and, per network, the layers (head included) as a list of
    (in, out, w_offset, b_offset)."""
    lib = load_library()
    cc = make_cconfig(**settings) if cconfig is None else cconfig
    L = CLayout()
    rc = lib.rg_ddpg_param_layout(C.byref(cc), C.byref(L))
    if rc != 0:
        raise RgDdpgError(rc, lib.rg_ddpg_last_error(None).decode())
    return dict(actor_count=L.actor_count, critic_count=L.critic_count,
                actor=[(L.actor_in[k], L.actor_out[k], L.actor_w[k], L.actor_b[k]) for k in range(L.n_actor)],
                critic=[(L.critic_in[k], L.critic_out[k], L.critic_w[k], L.critic_b[k]) for k in range(L.n_critic)])


def create_status(cconfig=None, batch=1, device=DEVICE_NONE):
    """(status, text) of rg_ddpg_create; destroys the handle when one is made."""
    cc = make_cconfig() if cconfig is None else cconfig
    return _create_status(load_library(), "rg_ddpg", C.byref(cc), int(batch), int(device))


class DdpgHandle(Handle):
    """Owns one rg_ddpg_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_ddpg_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE."""

    unit, error = "rg_ddpg", RgDdpgError

    def __init__(self, batch, device=None, **settings):
        lib = load_library()
        self.batch = int(batch)
        self.fields = ddpg_fields(**settings)
        self.device, index = resolve_device(device, RgDdpgError, "the DDPG kernels have no CPU fallback", DEVICE_NONE)
        cc = make_cconfig(**settings)
        self._create(lib, C.byref(cc), self.batch, index)
        self.layout = param_layout(cc)
        self.workspace_bytes = int(lib.rg_ddpg_workspace_bytes(self._h))
        self.opt_state_bytes = int(lib.rg_ddpg_opt_state_bytes(self._h))
        self.groups = int(lib.rg_ddpg_groups(self._h))
        self.lds_bytes = int(lib.rg_ddpg_lds_bytes(self._h))

    def act(self, ring, obs_ptr, actor_ptr, ou_ptr, act_state_ptr, mode, action_ptr, mean_ptr=None):
        self._check(self._lib.rg_ddpg_act(self._h, C.byref(ring), obs_ptr, actor_ptr, ou_ptr, act_state_ptr, int(mode), action_ptr, mean_ptr, self._s()))

    def store(self, ring, obs_ptr, action_ptr, reward_ptr, done_ptr, ou_ptr=None):
        self._check(self._lib.rg_ddpg_store(self._h, C.byref(ring), obs_ptr, action_ptr, reward_ptr, done_ptr, ou_ptr, self._s()))

    def sample(self, ring, idx_ptr):
        self._check(self._lib.rg_ddpg_sample(self._h, C.byref(ring), idx_ptr, self._s()))

    def critic_grad(self, ring, idx_ptr, critic_ptr, target_actor_ptr, target_critic_ptr, workspace_ptr, grad_ptr, loss_ptr):
        self._check(self._lib.rg_ddpg_critic_grad(self._h, C.byref(ring), idx_ptr, critic_ptr, target_actor_ptr, target_critic_ptr, workspace_ptr,
                                                  grad_ptr, loss_ptr, self._s()))

    def actor_grad(self, ring, idx_ptr, actor_ptr, critic_ptr, workspace_ptr, grad_ptr, loss_ptr):
        self._check(self._lib.rg_ddpg_actor_grad(self._h, C.byref(ring), idx_ptr, actor_ptr, critic_ptr, workspace_ptr, grad_ptr, loss_ptr, self._s()))

    def adam(self, which, params_ptr, grad_ptr, opt_state_ptr, workspace_ptr, norm_ptr=None, gate_ptr=None):
        self._check(self._lib.rg_ddpg_adam(self._h, int(which), params_ptr, grad_ptr, opt_state_ptr, workspace_ptr, norm_ptr, gate_ptr, self._s()))

    def soft_update(self, which, target_ptr, online_ptr, gate_ptr=None):
        self._check(self._lib.rg_ddpg_soft_update(self._h, int(which), target_ptr, online_ptr, gate_ptr, self._s()))

    def advance(self, ring):
        self._check(self._lib.rg_ddpg_advance(self._h, C.byref(ring), self._s()))

    def update(self, ring, actor_ptr, critic_ptr, target_actor_ptr, target_critic_ptr, opt_state_ptr, workspace_ptr, n_updates, stats_ptr):
        self._check(self._lib.rg_ddpg_update(self._h, C.byref(ring), actor_ptr, critic_ptr, target_actor_ptr, target_critic_ptr, opt_state_ptr,
                                             workspace_ptr, int(n_updates), stats_ptr, self._s()))
