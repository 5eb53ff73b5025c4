"""ctypes shim over the C-ABI of include/rg_rnn.h (the recurrent Gaussian policy of the PPO agent in librg_mpc.so).

Plumbing only, like policy_abi: it loads the same library, mirrors rg_rnn_config and rg_rnn_layout, turns negative status
codes into exceptions and owns one rg_rnn_handle.  There is NO CPU fallback: without the library or a GPU the handle
raises.  Every buffer is a caller-owned tensor (layouts: rg_rnn.h).
"""
import ctypes as C

from robot_gym_amd.core.c_abi import STATUS, Handle, RgError, create_status as _create_status, d, fp, i32, load, merged, resolve_device  # noqa: F401 -- STATUS stays a name of this module

ABI_VERSION = 1
MAX_OBS, MAX_ACT, MAX_DENSE, MAX_VALUE_LAYERS, MAX_WIDTH, MAX_UNITS = 64, 4, 2, 3, 256, 128
TILE = 8                 # RG_RNN_TILE: robots per workgroup of both kernels
MAX_T = 1 << 16          # RG_RNN_MAX_T
DEVICE_NONE = -1         # RG_RNN_DEVICE_NONE: a host-only handle
MODE_SAMPLE, MODE_MEAN = 0, 1


class RgRnnError(RgError):
    unit = "rg_rnn"


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("obs_dim", i32), ("act_dim", i32), ("n_policy_layers", i32), ("gru_units", i32), ("n_value_layers", i32),
        ("policy_layers", i32 * MAX_DENSE), ("value_layers", i32 * MAX_VALUE_LAYERS), ("reserved0", i32), ("obs_clip", d), ("seed", C.c_uint64),
    ]


class CLayout(C.Structure):
    _fields_ = [
        ("policy_count", i32), ("value_count", i32), ("n_dense", i32), ("n_value", i32), ("n_x", i32), ("gru_units", i32),
        ("dense_in", i32 * 2), ("dense_out", i32 * 2), ("dense_w", i32 * 2), ("dense_b", i32 * 2),
        ("w_ru", i32), ("b_ru", i32), ("w_c", i32), ("b_c", i32), ("head_w", i32), ("head_b", i32), ("logstd_offset", i32), ("reserved0", i32),
        ("value_in", i32 * 4), ("value_out", i32 * 4), ("value_w", i32 * 4), ("value_b", i32 * 4),
    ]


EXPORTS = ("rg_rnn_create", "rg_rnn_destroy", "rg_rnn_last_error", "rg_rnn_abi_version", "rg_rnn_config_size", "rg_rnn_layout_size",
           "rg_rnn_tile", "rg_rnn_param_layout", "rg_rnn_act", "rg_rnn_unroll")

# the reference's agents/ppo/scripts/networks.py (RecurrentGaussianPolicy: policy_layers[:-1], GRUBlockCell(100)) and configs.py
DEFAULTS = dict(obs_dim=16, act_dim=2, policy_layers=(200,), gru_units=100, value_layers=(200, 100), obs_clip=5.0, seed=0)

# rg_rnn.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "param_layout": (i32, [C.POINTER(CConfig), C.POINTER(CLayout)]),
    "act": (i32, [fp, fp, fp, fp, fp, fp, fp, fp, fp, i32, fp, fp, fp, fp, fp]),
    "unroll": (i32, [fp, fp, fp, fp, fp, fp, i32, fp, fp, fp, fp]),
}


def load_library(path=None):
    """The rg_rnn_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_rnn", "the recurrent policy has no CPU fallback", SIGNATURES, {"config": CConfig, "layout": CLayout}, {"tile": TILE},
                ABI_VERSION, path)


def rnn_fields(**settings):
    """The value of every rg_rnn_config setting as a dict: DEFAULTS overridden by `settings`."""
    out = merged(DEFAULTS, settings, "recurrent policy")
    for name, most in (("policy_layers", MAX_DENSE), ("value_layers", MAX_VALUE_LAYERS)):
        out[name] = tuple(int(w) for w in out[name])
        if len(out[name]) > most:
            raise ValueError(f"{name}: at most {most} layers, got {len(out[name])}")
    out["gru_units"] = int(out["gru_units"])
    return out


def make_cconfig(**settings):
    f = rnn_fields(**settings)
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = 0
    c.obs_dim, c.act_dim, c.gru_units, c.seed = int(f["obs_dim"]), int(f["act_dim"]), f["gru_units"], int(f["seed"])
    c.n_policy_layers, c.n_value_layers = len(f["policy_layers"]), len(f["value_layers"])
    for k, w in enumerate(f["policy_layers"]):
        c.policy_layers[k] = w
    for k, w in enumerate(f["value_layers"]):
        c.value_layers[k] = w
    c.obs_clip = float(f["obs_clip"])
    return c


def param_layout(cconfig=None, **settings):
    """rg_rnn_param_layout as a dict: policy_count, value_count, logstd_offset, n_x, gru_units, the dense layers and the value
    network's layers (head included) as lists of (in, out, w_offset, b_offset), and the cell's and the head's blocks w_ru, w_c
    and head the same way."""
    lib = load_library()
    cc = make_cconfig(**settings) if cconfig is None else cconfig
    L = CLayout()
    rc = lib.rg_rnn_param_layout(C.byref(cc), C.byref(L))
    if rc != 0:
        raise RgRnnError(rc, lib.rg_rnn_last_error(None).decode())
    H, nx = L.gru_units, L.n_x
    return dict(policy_count=L.policy_count, value_count=L.value_count, logstd_offset=L.logstd_offset, n_x=nx, gru_units=H,
                dense=[(L.dense_in[k], L.dense_out[k], L.dense_w[k], L.dense_b[k]) for k in range(L.n_dense)],
                w_ru=(nx + H, 2 * H, L.w_ru, L.b_ru), w_c=(nx + H, H, L.w_c, L.b_c), head=(H, cc.act_dim, L.head_w, L.head_b),
                value=[(L.value_in[k], L.value_out[k], L.value_w[k], L.value_b[k]) for k in range(L.n_value)])


def create_status(cconfig=None, batch=1, device=DEVICE_NONE):
    """(status, text) of rg_rnn_create; destroys the handle when one is made."""
    cc = make_cconfig() if cconfig is None else cconfig
    return _create_status(load_library(), "rg_rnn", C.byref(cc), int(batch), int(device))


class RnnHandle(Handle):
    """Owns one rg_rnn_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_rnn_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE."""

    unit, error = "rg_rnn", RgRnnError

    def __init__(self, batch, device=None, **settings):
        lib = load_library()
        self.batch = int(batch)
        self.fields = rnn_fields(**settings)
        self.device, index = resolve_device(device, RgRnnError, "the recurrent policy's kernels have no CPU fallback", DEVICE_NONE)
        cc = make_cconfig(**settings)
        self._create(lib, C.byref(cc), self.batch, index)
        self.layout = param_layout(cc)

    def act(self, obs_ptr, norm_ptr, policy_params_ptr, value_params_ptr, act_state_ptr, reset_ptr, hidden_in_ptr, hidden_out_ptr, mode, action_ptr,
            mean_ptr=None, value_ptr=None, logprob_ptr=None):
        self._check(self._lib.rg_rnn_act(self._h, obs_ptr, norm_ptr, policy_params_ptr, value_params_ptr, act_state_ptr, reset_ptr, hidden_in_ptr,
                                         hidden_out_ptr, int(mode), action_ptr, mean_ptr, value_ptr, logprob_ptr, self._s()))

    def unroll(self, obs_ptr, reset_ptr, h0_ptr, norm_ptr, policy_params_ptr, T, mean_ptr, hidden_seq_ptr=None, hidden_last_ptr=None):
        self._check(self._lib.rg_rnn_unroll(self._h, obs_ptr, reset_ptr, h0_ptr, norm_ptr, policy_params_ptr, int(T), mean_ptr, hidden_seq_ptr,
                                            hidden_last_ptr, self._s()))
