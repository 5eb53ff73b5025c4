"""ctypes shim over the C-ABI of include/rg_bptt.h (the recurrent PPO policy update on the device in librg_mpc.so).

Plumbing only, like rnn_abi and ppo_abi, whose structures it takes (rg_rnn_config, rg_ppo_config, rg_ppo_rollout): it loads the
same library, turns negative status codes into exceptions and owns one rg_bptt_handle.  There is NO CPU fallback: without
the library or a GPU the handle raises.  Every buffer is a caller-owned tensor (layouts: rg_bptt.h).
"""
import ctypes as C

from robot_gym_amd.core import ppo_abi, rnn_abi
from robot_gym_amd.core.c_abi import Handle, RgError, create_status as _create_status, fp, i32, i64, load, resolve_device

ABI_VERSION = 1
TILE = rnn_abi.TILE      # RG_RNN_TILE: robots per workgroup of the forward and the delta pass
CHUNK = 16               # RG_BPTT_CHUNK: samples per float32 chain of a weight gradient
ROWS = 16                # RG_BPTT_ROWS
MAX_GROUPS = 64          # RG_BPTT_MAX_GROUPS
STATS = 4                # RG_BPTT_STATS
OPT_HEADER_BYTES = 16    # RG_BPTT_OPT_HEADER_BYTES: int64 step, float64 penalty
DEVICE_NONE = -1
MAX_T, MAX_BATCH, MAX_SAMPLES = rnn_abi.MAX_T, 1 << 24, 1 << 30     # RG_RNN_MAX_T, RG_RNN_MAX_BATCH, RG_PPO_MAX_SAMPLES
STAT_NAMES = ("policy_loss_first", "policy_loss_last", "kl_change", "penalty")
STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE"}     # rg_bptt_status has no ALLOC


class RgBpttError(RgError):
    unit, names = "rg_bptt", STATUS


EXPORTS = ("rg_bptt_create", "rg_bptt_destroy", "rg_bptt_last_error", "rg_bptt_abi_version", "rg_bptt_tile", "rg_bptt_workspace_bytes",
           "rg_bptt_opt_state_bytes", "rg_bptt_groups", "rg_bptt_policy_grad", "rg_bptt_kl", "rg_bptt_adam", "rg_bptt_penalty",
           "rg_bptt_update_policy")

_ROLLOUT = C.POINTER(ppo_abi.CRollout)
# rg_bptt.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(rnn_abi.CConfig), C.POINTER(ppo_abi.CConfig), i32, i32, i32, C.POINTER(fp)]),
    "workspace_bytes": (i64, [fp]),
    "opt_state_bytes": (i64, [fp]),
    "groups": (i32, [fp]),
    "policy_grad": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp, fp, fp, fp, fp]),
    "kl": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp, fp]),
    "adam": (i32, [fp, fp, fp, fp, fp]),
    "penalty": (i32, [fp, fp, fp, fp, fp]),
    "update_policy": (i32, [fp, _ROLLOUT, fp, fp, fp, fp, fp, fp, fp, fp, fp]),
}


def load_library(path=None):
    """The rg_bptt_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_bptt", "the recurrent device update has no CPU fallback", SIGNATURES, {}, {"tile": TILE}, ABI_VERSION, path)


def groups(T, B):
    """G of the W phase (rg_bptt.h): the float64 partials per weight for T * B samples."""
    nchunks = -(-int(T) * int(B) // CHUNK)
    per = -(-nchunks // min(nchunks, MAX_GROUPS))
    return -(-nchunks // per)


def create_status(rnn_cconfig=None, ppo_cconfig=None, T=4, B=4, device=DEVICE_NONE):
    """(status, text) of rg_bptt_create; destroys the handle when one is made."""
    rc_ = rnn_abi.make_cconfig() if rnn_cconfig is None else rnn_cconfig
    cc = ppo_abi.make_cconfig() if ppo_cconfig is None else ppo_cconfig
    return _create_status(load_library(), "rg_bptt", C.byref(rc_), C.byref(cc), int(T), int(B), int(device))


class BpttHandle(Handle):
    """Owns one rg_bptt_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_bptt_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE.  rnn_settings are
    those of rnn_abi (the networks' shapes and obs_clip are what the update reads), the keywords those of ppo_abi."""

    unit, error = "rg_bptt", RgBpttError

    def __init__(self, T, B, device=None, rnn_settings=None, **settings):
        lib = load_library()
        self.T, self.B = int(T), int(B)
        self.fields = ppo_abi.ppo_fields(**settings)
        self.device, index = resolve_device(device, RgBpttError, "the recurrent device update has no CPU fallback", DEVICE_NONE)
        rc = rnn_abi.make_cconfig(**(rnn_settings or {}))
        self._create(lib, C.byref(rc), C.byref(ppo_abi.make_cconfig(**settings)), self.T, self.B, index)
        self.workspace_bytes = int(lib.rg_bptt_workspace_bytes(self._h))
        self.opt_state_bytes = int(lib.rg_bptt_opt_state_bytes(self._h))
        self.groups = int(lib.rg_bptt_groups(self._h))

    def policy_grad(self, ro, reset_ptr, h0_ptr, adv_stats_ptr, norm_ptr, policy_params_ptr, opt_state_ptr, workspace_ptr, grad_ptr, loss_ptr):
        self._check(self._lib.rg_bptt_policy_grad(self._h, C.byref(ro), reset_ptr, h0_ptr, adv_stats_ptr, norm_ptr, policy_params_ptr, opt_state_ptr,
                                                  workspace_ptr, grad_ptr, loss_ptr, self._s()))

    def kl(self, ro, reset_ptr, h0_ptr, norm_ptr, policy_params_ptr, workspace_ptr, kl_ptr):
        self._check(self._lib.rg_bptt_kl(self._h, C.byref(ro), reset_ptr, h0_ptr, norm_ptr, policy_params_ptr, workspace_ptr, kl_ptr, self._s()))

    def adam(self, params_ptr, grad_ptr, opt_state_ptr):
        self._check(self._lib.rg_bptt_adam(self._h, params_ptr, grad_ptr, opt_state_ptr, self._s()))

    def penalty(self, kl_ptr, opt_state_ptr, stats_ptr):
        self._check(self._lib.rg_bptt_penalty(self._h, kl_ptr, opt_state_ptr, stats_ptr, self._s()))

    def update_policy(self, ro, reset_ptr, h0_ptr, adv_stats_ptr, norm_ptr, policy_params_ptr, opt_state_ptr, workspace_ptr, stats_ptr):
        self._check(self._lib.rg_bptt_update_policy(self._h, C.byref(ro), reset_ptr, h0_ptr, adv_stats_ptr, norm_ptr, policy_params_ptr, opt_state_ptr,
                                                    workspace_ptr, stats_ptr, self._s()))
