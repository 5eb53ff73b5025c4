"""ctypes shim over the C-ABI of include/rg_policy.h (the acting and collecting side of the PPO agent in librg_mpc.so).

Plumbing only, like episode_abi: it loads the same library, mirrors rg_policy_config and rg_policy_layout, turns negative
status codes into exceptions and owns one rg_policy_handle.  There is NO CPU fallback: without the library or a GPU the
handle raises.  Every buffer is a caller-owned tensor (layouts: rg_policy.h).
"""
import ctypes as C
import os

from robot_gym_amd.core import goto_abi, mpc_abi

ABI_VERSION = 1
MAX_OBS, MAX_ACT, MAX_LAYERS, MAX_WIDTH = 64, 4, 3, 256
TILE = 8                 # RG_POLICY_TILE: robots per workgroup of the act kernel
NORM_COLS = 65           # RG_POLICY_NORM_COLS
NORM_REWARD = 64         # RG_POLICY_NORM_REWARD: the reward's column
NORM_ROWS = 195          # RG_POLICY_NORM_ROWS = [count, mean, var_sum][NORM_COLS]
DEVICE_NONE = -1         # RG_POLICY_DEVICE_NONE: a host-only handle
MODE_SAMPLE, MODE_MEAN = 0, 1
d = C.c_double
i32 = C.c_int32
fp = C.c_void_p

STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE", -4: "ALLOC"}


class RgPolicyError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"rg_policy status {status} ({STATUS.get(status, '?')}): {text}")
        self.status = status


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("obs_dim", i32), ("act_dim", i32), ("n_policy_layers", i32), ("n_value_layers", i32), ("reserved0", i32),
        ("policy_layers", i32 * MAX_LAYERS), ("value_layers", i32 * MAX_LAYERS), ("obs_clip", d), ("reward_clip", d), ("discount", d),
        ("gae_lambda", d), ("seed", C.c_uint64),
    ]


class CLayout(C.Structure):
    _fields_ = [
        ("policy_count", i32), ("value_count", i32), ("n_policy", i32), ("n_value", i32), ("logstd_offset", i32), ("reserved0", i32),
        ("policy_in", i32 * 4), ("policy_out", i32 * 4), ("policy_w", i32 * 4), ("policy_b", i32 * 4),
        ("value_in", i32 * 4), ("value_out", i32 * 4), ("value_w", i32 * 4), ("value_b", i32 * 4),
    ]


EXPORTS = ("rg_policy_create", "rg_policy_destroy", "rg_policy_last_error", "rg_policy_abi_version", "rg_policy_config_size",
           "rg_policy_layout_size", "rg_policy_norm_rows", "rg_policy_tile", "rg_policy_param_layout", "rg_policy_act", "rg_policy_record",
           "rg_policy_returns")

# the reference's agents/ppo/scripts/configs.py (default) and networks.py
DEFAULTS = dict(obs_dim=16, act_dim=2, policy_layers=(200, 100), value_layers=(200, 100), obs_clip=5.0, reward_clip=10.0, discount=0.985,
                gae_lambda=1.0, seed=0)

_lib = None


def load_library(path=None):
    """The rg_policy_* entries of librg_mpc.so (mpc_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or mpc_abi.LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `make -C robot_gym_amd/csrc` (or __graft_entry__.build()); "
                          "the policy has no CPU fallback")
    L = C.CDLL(p)
    L.rg_policy_create.argtypes = [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]
    L.rg_policy_create.restype = i32
    L.rg_policy_destroy.argtypes = [fp]
    L.rg_policy_destroy.restype = None
    L.rg_policy_last_error.argtypes = [fp]
    L.rg_policy_last_error.restype = C.c_char_p
    for name in ("abi_version", "config_size", "layout_size", "norm_rows", "tile"):
        getattr(L, f"rg_policy_{name}").restype = i32
    L.rg_policy_param_layout.argtypes = [C.POINTER(CConfig), C.POINTER(CLayout)]
    L.rg_policy_param_layout.restype = i32
    L.rg_policy_act.argtypes = [fp, fp, fp, fp, fp, fp, i32, fp, fp, fp, fp, fp]
    L.rg_policy_act.restype = i32
    L.rg_policy_record.argtypes = [fp, fp, fp, fp, fp, fp, fp, fp, fp, fp]
    L.rg_policy_record.restype = i32
    L.rg_policy_returns.argtypes = [fp, fp, fp, fp, fp, fp, i32, i32, fp, fp, fp]
    L.rg_policy_returns.restype = i32
    if L.rg_policy_abi_version() != ABI_VERSION:
        raise ImportError("librg_mpc.so rg_policy ABI version mismatch")
    if L.rg_policy_config_size() != C.sizeof(CConfig):
        raise ImportError(f"rg_policy_config size mismatch: lib {L.rg_policy_config_size()} vs binding {C.sizeof(CConfig)}")
    if L.rg_policy_layout_size() != C.sizeof(CLayout):
        raise ImportError(f"rg_policy_layout size mismatch: lib {L.rg_policy_layout_size()} vs binding {C.sizeof(CLayout)}")
    if L.rg_policy_norm_rows() != NORM_ROWS:
        raise ImportError(f"rg_policy norm rows mismatch: lib {L.rg_policy_norm_rows()} vs binding {NORM_ROWS}")
    if L.rg_policy_tile() != TILE:
        raise ImportError(f"rg_policy tile mismatch: lib {L.rg_policy_tile()} vs binding {TILE}")
    if path is None:
        _lib = L
    return L


def policy_fields(**settings):
    """The value of every rg_policy_config setting as a dict: DEFAULTS overridden by `settings`."""
    unknown = set(settings) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown policy setting(s) {sorted(unknown)}")
    out = dict(DEFAULTS)
    out.update(settings)
    for name in ("policy_layers", "value_layers"):
        out[name] = tuple(int(w) for w in out[name])
        if len(out[name]) > MAX_LAYERS:
            raise ValueError(f"{name}: at most {MAX_LAYERS} hidden layers, got {len(out[name])}")
    return out


def make_cconfig(**settings):
    f = policy_fields(**settings)
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = 0
    c.obs_dim, c.act_dim, c.seed = int(f["obs_dim"]), int(f["act_dim"]), int(f["seed"])
    c.n_policy_layers, c.n_value_layers = len(f["policy_layers"]), len(f["value_layers"])
    for k, w in enumerate(f["policy_layers"]):
        c.policy_layers[k] = w
    for k, w in enumerate(f["value_layers"]):
        c.value_layers[k] = w
    for name in ("obs_clip", "reward_clip", "discount", "gae_lambda"):
        setattr(c, name, float(f[name]))
    return c


def param_layout(cconfig=None, **settings):
    """rg_policy_param_layout as a dict: policy_count, value_count, logstd_offset and, per network, the layers (head included)
    as a list of (in, out, w_offset, b_offset)."""
    lib = load_library()
    cc = make_cconfig(**settings) if cconfig is None else cconfig
    L = CLayout()
    rc = lib.rg_policy_param_layout(C.byref(cc), C.byref(L))
    if rc != 0:
        raise RgPolicyError(rc, lib.rg_policy_last_error(None).decode())
    return dict(policy_count=L.policy_count, value_count=L.value_count, logstd_offset=L.logstd_offset,
                policy=[(L.policy_in[k], L.policy_out[k], L.policy_w[k], L.policy_b[k]) for k in range(L.n_policy)],
                value=[(L.value_in[k], L.value_out[k], L.value_w[k], L.value_b[k]) for k in range(L.n_value)])


def create_status(cconfig=None, batch=1, device=DEVICE_NONE):
    """(status, text) of rg_policy_create; destroys the handle when one is made."""
    lib = load_library()
    cc = make_cconfig() if cconfig is None else cconfig
    h = fp()
    rc = lib.rg_policy_create(C.byref(cc), int(batch), int(device), C.byref(h))
    text = lib.rg_policy_last_error(None).decode() if rc else ""
    if h:
        lib.rg_policy_destroy(h)
    return rc, text


class PolicyHandle:
    """Owns one rg_policy_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_policy_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE."""

    def __init__(self, batch, device=None, **settings):
        self._h = fp()
        self._lib = load_library()
        self.batch = int(batch)
        self.fields = policy_fields(**settings)
        if device == DEVICE_NONE:
            self.device, index = None, DEVICE_NONE
        else:
            import torch
            if not torch.cuda.is_available():
                raise RgPolicyError(-3, "no GPU: the policy kernels have no CPU fallback")
            index = None if device is None else torch.device(device).index
            self.device = torch.device("cuda", torch.cuda.current_device() if index is None else index)
            index = self.device.index
        cc = make_cconfig(**settings)
        rc = self._lib.rg_policy_create(C.byref(cc), self.batch, index, C.byref(self._h))
        if rc != 0:
            msg = self._lib.rg_policy_last_error(None)
            self._h = fp()
            raise RgPolicyError(rc, msg.decode() if msg else "create failed")
        self.layout = param_layout(cc)

    def _check(self, rc):
        if rc != 0:
            raise RgPolicyError(rc, self._lib.rg_policy_last_error(self._h).decode())

    def _s(self):
        return None if self.device is None else goto_abi._stream(self.device)

    def act(self, obs_ptr, norm_ptr, policy_params_ptr, value_params_ptr, act_state_ptr, mode, action_ptr, mean_ptr=None, value_ptr=None,
            logprob_ptr=None):
        self._check(self._lib.rg_policy_act(self._h, obs_ptr, norm_ptr, policy_params_ptr, value_params_ptr, act_state_ptr, int(mode), action_ptr,
                                            mean_ptr, value_ptr, logprob_ptr, self._s()))

    def record(self, obs_ptr, reward_ptr, done_ptr, mask_ptr, norm_ptr, ro_obs_ptr=None, ro_reward_ptr=None, ro_done_ptr=None):
        self._check(self._lib.rg_policy_record(self._h, obs_ptr, reward_ptr, done_ptr, mask_ptr, norm_ptr, ro_obs_ptr, ro_reward_ptr, ro_done_ptr,
                                               self._s()))

    def returns(self, reward_ptr, value_ptr, done_ptr, last_value_ptr, norm_ptr, T, bootstrap, ret_ptr, adv_ptr):
        self._check(self._lib.rg_policy_returns(self._h, reward_ptr, value_ptr, done_ptr, last_value_ptr, norm_ptr, int(T), int(bool(bootstrap)),
                                                ret_ptr, adv_ptr, self._s()))

    def close(self):
        if self._h:
            self._lib.rg_policy_destroy(self._h)
            self._h = fp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
