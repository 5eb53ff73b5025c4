"""ctypes shim over the C-ABI of include/rg_ppo.h (the PPO update on the device in librg_mpc.so).

Plumbing only, like policy_abi: it loads the same library, mirrors rg_ppo_config and rg_ppo_rollout, turns negative status
codes into exceptions and owns one rg_ppo_handle.  There is NO CPU fallback: without the library or a GPU the handle
raises.  Every buffer is a caller-owned tensor (layouts: rg_ppo.h).
"""
import ctypes as C
import os

from robot_gym_amd.core import goto_abi, mpc_abi, policy_abi

ABI_VERSION = 1
TILE = 16                # RG_PPO_TILE: samples per tile of a sweep
MAX_GROUPS = 256         # RG_PPO_MAX_GROUPS
STATS = 6                # RG_PPO_STATS
OPT_HEADER_BYTES = 32    # RG_PPO_OPT_HEADER_BYTES: int64 step[2], float64 penalty, float64 reserved
DEVICE_NONE = -1
LOGPDF = {"exact": 0, "reference": 1}
POLICY, VALUE = 0, 1
STAT_NAMES = ("policy_loss_first", "policy_loss_last", "value_loss_first", "value_loss_last", "kl_change", "penalty")
d = C.c_double
i32 = C.c_int32
fp = C.c_void_p

STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE"}


class RgPpoError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"rg_ppo status {status} ({STATUS.get(status, '?')}): {text}")
        self.status = status


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("epochs_policy", i32), ("epochs_value", i32), ("conv_logpdf", i32), ("policy_lr", d), ("value_lr", d), ("beta1", d),
        ("beta2", d), ("adam_eps", d), ("kl_target", d), ("kl_cutoff_factor", d), ("kl_cutoff_coef", d),
    ]


class CRollout(C.Structure):
    _fields_ = [("obs", fp), ("action", fp), ("mean", fp), ("logstd", fp), ("adv", fp), ("ret", fp), ("mask", fp)]


EXPORTS = ("rg_ppo_create", "rg_ppo_destroy", "rg_ppo_last_error", "rg_ppo_abi_version", "rg_ppo_config_size", "rg_ppo_rollout_size", "rg_ppo_tile",
           "rg_ppo_workspace_bytes", "rg_ppo_opt_state_bytes", "rg_ppo_groups", "rg_ppo_scalars_offset", "rg_ppo_prepare", "rg_ppo_policy_grad", "rg_ppo_value_grad",
           "rg_ppo_adam", "rg_ppo_kl", "rg_ppo_update")

# those of PPO (robot_gym_amd/agents/ppo/algorithm.py) and of torch.optim.Adam
DEFAULTS = dict(policy_lr=1e-4, value_lr=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-8, epochs_policy=50, epochs_value=50, kl_target=1e-2,
                kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0, conv_logpdf="exact")

_lib = None


def load_library(path=None):
    """The rg_ppo_* entries of librg_mpc.so (mpc_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or mpc_abi.LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `make -C robot_gym_amd/csrc` (or __graft_entry__.build()); "
                          "the device update has no CPU fallback")
    L = C.CDLL(p)
    L.rg_ppo_create.argtypes = [C.POINTER(policy_abi.CConfig), C.POINTER(CConfig), i32, i32, i32, C.POINTER(fp)]
    L.rg_ppo_create.restype = i32
    L.rg_ppo_destroy.argtypes = [fp]
    L.rg_ppo_destroy.restype = None
    L.rg_ppo_last_error.argtypes = [fp]
    L.rg_ppo_last_error.restype = C.c_char_p
    for name in ("abi_version", "config_size", "rollout_size", "tile"):
        getattr(L, f"rg_ppo_{name}").argtypes = []
        getattr(L, f"rg_ppo_{name}").restype = i32
    for name in ("workspace_bytes", "opt_state_bytes", "scalars_offset"):
        getattr(L, f"rg_ppo_{name}").argtypes = [fp]
        getattr(L, f"rg_ppo_{name}").restype = C.c_int64
    L.rg_ppo_groups.argtypes = [fp]
    L.rg_ppo_groups.restype = i32
    ro = C.POINTER(CRollout)
    L.rg_ppo_prepare.argtypes = [fp, ro, fp, fp]
    L.rg_ppo_policy_grad.argtypes = [fp, ro, fp, fp, fp, fp, fp, fp, fp]
    L.rg_ppo_value_grad.argtypes = [fp, ro, fp, fp, fp, fp, fp, fp]
    L.rg_ppo_adam.argtypes = [fp, i32, fp, fp, fp, fp]
    L.rg_ppo_kl.argtypes = [fp, ro, fp, fp, fp, fp, fp]
    L.rg_ppo_update.argtypes = [fp, ro, fp, fp, fp, fp, fp, fp, fp]
    for name in ("prepare", "policy_grad", "value_grad", "adam", "kl", "update"):
        getattr(L, f"rg_ppo_{name}").restype = i32
    if L.rg_ppo_abi_version() != ABI_VERSION:
        raise ImportError("librg_mpc.so rg_ppo ABI version mismatch")
    if L.rg_ppo_config_size() != C.sizeof(CConfig):
        raise ImportError(f"rg_ppo_config size mismatch: lib {L.rg_ppo_config_size()} vs binding {C.sizeof(CConfig)}")
    if L.rg_ppo_rollout_size() != C.sizeof(CRollout):
        raise ImportError(f"rg_ppo_rollout size mismatch: lib {L.rg_ppo_rollout_size()} vs binding {C.sizeof(CRollout)}")
    if L.rg_ppo_tile() != TILE:
        raise ImportError(f"rg_ppo tile mismatch: lib {L.rg_ppo_tile()} vs binding {TILE}")
    if path is None:
        _lib = L
    return L


def ppo_fields(**settings):
    """The value of every rg_ppo_config setting as a dict: DEFAULTS overridden by `settings`."""
    unknown = set(settings) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown ppo setting(s) {sorted(unknown)}")
    out = dict(DEFAULTS)
    out.update(settings)
    if out["conv_logpdf"] not in LOGPDF:
        raise ValueError(f"conv_logpdf must be 'exact' or 'reference', got {out['conv_logpdf']!r}")
    return out


def make_cconfig(**settings):
    f = ppo_fields(**settings)
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.epochs_policy, c.epochs_value, c.conv_logpdf = int(f["epochs_policy"]), int(f["epochs_value"]), LOGPDF[f["conv_logpdf"]]
    for name in ("policy_lr", "value_lr", "beta1", "beta2", "adam_eps", "kl_target", "kl_cutoff_factor", "kl_cutoff_coef"):
        setattr(c, name, float(f[name]))
    return c


def make_crollout(obs=None, action=None, mean=None, logstd=None, adv=None, ret=None, mask=None):
    r = CRollout()
    r.obs, r.action, r.mean, r.logstd, r.adv, r.ret, r.mask = obs, action, mean, logstd, adv, ret, mask
    return r


def create_status(policy_cconfig=None, ppo_cconfig=None, T=4, B=4, device=DEVICE_NONE):
    """(status, text) of rg_ppo_create; destroys the handle when one is made."""
    lib = load_library()
    pc = policy_abi.make_cconfig() if policy_cconfig is None else policy_cconfig
    cc = make_cconfig() if ppo_cconfig is None else ppo_cconfig
    h = fp()
    rc = lib.rg_ppo_create(C.byref(pc), C.byref(cc), int(T), int(B), int(device), C.byref(h))
    text = lib.rg_ppo_last_error(None).decode() if rc else ""
    if h:
        lib.rg_ppo_destroy(h)
    return rc, text


class PpoHandle:
    """Owns one rg_ppo_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_ppo_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE.  policy_settings are
    those of policy_abi (the networks' shapes and obs_clip are what the update reads)."""

    def __init__(self, T, B, device=None, policy_settings=None, **settings):
        self._h = fp()
        self._lib = load_library()
        self.T, self.B = int(T), int(B)
        self.fields = ppo_fields(**settings)
        if device == DEVICE_NONE:
            self.device, index = None, DEVICE_NONE
        else:
            import torch
            if not torch.cuda.is_available():
                raise RgPpoError(-3, "no GPU: the device update has no CPU fallback")
            index = None if device is None else torch.device(device).index
            self.device = torch.device("cuda", torch.cuda.current_device() if index is None else index)
            index = self.device.index
        pc = policy_abi.make_cconfig(**(policy_settings or {}))
        cc = make_cconfig(**settings)
        rc = self._lib.rg_ppo_create(C.byref(pc), C.byref(cc), self.T, self.B, index, C.byref(self._h))
        if rc != 0:
            msg = self._lib.rg_ppo_last_error(None)
            self._h = fp()
            raise RgPpoError(rc, msg.decode() if msg else "create failed")
        self.workspace_bytes = int(self._lib.rg_ppo_workspace_bytes(self._h))
        self.opt_state_bytes = int(self._lib.rg_ppo_opt_state_bytes(self._h))
        self.groups = int(self._lib.rg_ppo_groups(self._h))
        self.scalars_offset = int(self._lib.rg_ppo_scalars_offset(self._h))

    def _check(self, rc):
        if rc != 0:
            raise RgPpoError(rc, self._lib.rg_ppo_last_error(self._h).decode())

    def _s(self):
        return None if self.device is None else goto_abi._stream(self.device)

    def prepare(self, ro, workspace_ptr):
        self._check(self._lib.rg_ppo_prepare(self._h, C.byref(ro), workspace_ptr, self._s()))

    def policy_grad(self, ro, norm_ptr, policy_params_ptr, opt_state_ptr, workspace_ptr, grad_ptr, loss_ptr):
        self._check(self._lib.rg_ppo_policy_grad(self._h, C.byref(ro), norm_ptr, policy_params_ptr, opt_state_ptr, workspace_ptr, grad_ptr, loss_ptr,
                                                 self._s()))

    def value_grad(self, ro, norm_ptr, value_params_ptr, workspace_ptr, grad_ptr, loss_ptr):
        self._check(self._lib.rg_ppo_value_grad(self._h, C.byref(ro), norm_ptr, value_params_ptr, workspace_ptr, grad_ptr, loss_ptr, self._s()))

    def adam(self, which, params_ptr, grad_ptr, opt_state_ptr):
        self._check(self._lib.rg_ppo_adam(self._h, int(which), params_ptr, grad_ptr, opt_state_ptr, self._s()))

    def kl(self, ro, norm_ptr, policy_params_ptr, workspace_ptr, kl_ptr):
        self._check(self._lib.rg_ppo_kl(self._h, C.byref(ro), norm_ptr, policy_params_ptr, workspace_ptr, kl_ptr, self._s()))

    def update(self, ro, norm_ptr, policy_params_ptr, value_params_ptr, opt_state_ptr, workspace_ptr, stats_ptr):
        self._check(self._lib.rg_ppo_update(self._h, C.byref(ro), norm_ptr, policy_params_ptr, value_params_ptr, opt_state_ptr, workspace_ptr,
                                            stats_ptr, self._s()))

    def close(self):
        if self._h:
            self._lib.rg_ppo_destroy(self._h)
            self._h = fp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
