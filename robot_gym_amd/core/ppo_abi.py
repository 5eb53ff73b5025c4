"""ctypes shim over the C-ABI of include/rg_ppo.h (the PPO update on the device in librg_mpc.so).

Plumbing only, like policy_abi: it loads the same library, mirrors rg_ppo_config and rg_ppo_rollout, turns negative status
codes into exceptions and owns one rg_ppo_handle.  There is NO CPU fallback: without the library or a GPU the handle
raises.  Every buffer is a caller-owned tensor (layouts: rg_ppo.h).
"""
import ctypes as C

from robot_gym_amd.core import policy_abi
from robot_gym_amd.core.c_abi import Handle, RgError, create_status as _create_status, d, fp, i32, i64, load, merged, resolve_device

ABI_VERSION = 1
TILE = 16                # RG_PPO_TILE: samples per tile of a sweep
MAX_GROUPS = 256         # RG_PPO_MAX_GROUPS
STATS = 6                # RG_PPO_STATS
OPT_HEADER_BYTES = 32    # RG_PPO_OPT_HEADER_BYTES: int64 step[2], float64 penalty, float64 reserved
DEVICE_NONE = -1
LOGPDF = {"exact": 0, "reference": 1}
POLICY, VALUE = 0, 1
STAT_NAMES = ("policy_loss_first", "policy_loss_last", "value_loss_first", "value_loss_last", "kl_change", "penalty")
STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE"}     # rg_ppo_status has no ALLOC


class RgPpoError(RgError):
    unit, names = "rg_ppo", STATUS


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

_ROLLOUT = C.POINTER(CRollout)
# rg_ppo.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(policy_abi.CConfig), C.POINTER(CConfig), i32, i32, i32, C.POINTER(fp)]),
    "workspace_bytes": (i64, [fp]),
    "opt_state_bytes": (i64, [fp]),
    "scalars_offset": (i64, [fp]),
    "groups": (i32, [fp]),
    "prepare": (i32, [fp, _ROLLOUT, fp, fp]),
    "policy_grad": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp, fp]),
    "value_grad": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp]),
    "adam": (i32, [fp, i32, fp, fp, fp, fp]),
    "kl": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp]),
    "update": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp, fp]),
}


def load_library(path=None):
    """The rg_ppo_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_ppo", "the device update has no CPU fallback", SIGNATURES, {"config": CConfig, "rollout": CRollout}, {"tile": TILE},
                ABI_VERSION, path)


def ppo_fields(**settings):
    """The value of every rg_ppo_config setting as a dict: DEFAULTS overridden by `settings`."""
    out = merged(DEFAULTS, settings, "ppo")
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
    pc = policy_abi.make_cconfig() if policy_cconfig is None else policy_cconfig
    cc = make_cconfig() if ppo_cconfig is None else ppo_cconfig
    return _create_status(load_library(), "rg_ppo", C.byref(pc), C.byref(cc), int(T), int(B), int(device))


class PpoHandle(Handle):
    """Owns one rg_ppo_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_ppo_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE.  policy_settings are
    those of policy_abi (the networks' shapes and obs_clip are what the update reads)."""

    unit, error = "rg_ppo", RgPpoError

    def __init__(self, T, B, device=None, policy_settings=None, **settings):
        lib = load_library()
        self.T, self.B = int(T), int(B)
        self.fields = ppo_fields(**settings)
        self.device, index = resolve_device(device, RgPpoError, "the device update has no CPU fallback", DEVICE_NONE)
        pc = policy_abi.make_cconfig(**(policy_settings or {}))
        self._create(lib, C.byref(pc), C.byref(make_cconfig(**settings)), self.T, self.B, index)
        self.workspace_bytes = int(lib.rg_ppo_workspace_bytes(self._h))
        self.opt_state_bytes = int(lib.rg_ppo_opt_state_bytes(self._h))
        self.groups = int(lib.rg_ppo_groups(self._h))
        self.scalars_offset = int(lib.rg_ppo_scalars_offset(self._h))

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
