"""ctypes shim over the C-ABI of include/rg_goto.h (the batched go-to-target task of librg_mpc.so).

Plumbing only, like srb_abi: it loads the same library, mirrors rg_goto_config and rg_goto_path_ptrs, turns negative
status codes into exceptions and owns one rg_goto_handle.  There is NO CPU fallback: without the library or a GPU the
handle raises.  Task state, path slab and outputs are caller-owned tensors (layouts: rg_goto.h).
"""
import ctypes as C

import numpy as np

from robot_gym_amd.core.c_abi import (STATUS, Handle, RgError, create_status as _create_status, d, fill_config, fp, host_array, host_ptr, i32,  # noqa: F401 -- STATUS stays a name of this module
                                      index_array, load, merged, resolve_device)

ABI_VERSION = 1
STATE_ROWS = 50          # RG_GOTO_STATE_ROWS
(ROW_POS, ROW_PREV, ROW_POT, ROW_PROGRESS, ROW_NEXT_CP, ROW_PATH_DONE, ROW_ENV_STEPS, ROW_DONE, ROW_REASON, ROW_OVERFLOW,
 ROW_VISIBLE, ROW_CHAIN, ROW_LATCHED, ROW_TRACK_ERR, ROW_OBS) = 0, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18
HDR_ROWS = 4
MAX_CAM_PTS, MAX_VISIBLE, MAX_PATH, MAX_CHECKPOINTS = 16, 128, 65536, 65536
LIMIT_REWARD = -100.0
DEVICE_NONE = -1         # RG_GOTO_DEVICE_NONE: a host-only handle
REASONS = ("none", "fallen", "path_done", "on_target", "progress", "track", "time")   # RG_GOTO_REASON_*


class RgGotoError(RgError):
    unit = "rg_goto"


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("reserved0", i32), ("window_height", d), ("window_top_width", d), ("window_bottom_width", d),
        ("window_distance", d), ("max_track_err", d), ("progress_window", d), ("progress_limit", d), ("target_radius", d),
        ("time_penalty", d), ("checkpoint_reward_total", d), ("max_time", d), ("continuity_break", d), ("action_low", d * 2),
        ("action_high", d * 2), ("cmd_offset", d * 3), ("dt_sim", d), ("substeps", i32), ("num_cam_pts", i32),
        ("num_checkpoints", i32), ("n_max", i32), ("max_visible", i32), ("reserved1", i32),
    ]


PATH_FIELDS = ("x", "y", "s", "first_same_x", "hdr")


class CPathPtrs(C.Structure):
    _fields_ = [(name, fp) for name in PATH_FIELDS]


EXPORTS = ("rg_goto_create", "rg_goto_destroy", "rg_goto_last_error", "rg_goto_abi_version", "rg_goto_config_size", "rg_goto_state_rows",
           "rg_goto_set_path", "rg_goto_pre_step", "rg_goto_post_step", "rg_goto_observe")

# the reference's constants: follower.py:19,52-55, go_env.py:79-81,102-103,229,236,299, path.py:23, line_interpolation.py:101,
# core/sim_constants.py; cmd_offset is filled from the MPCConfig
DEFAULTS = dict(window_height=0.160, window_top_width=0.270, window_bottom_width=0.120, window_distance=0.112, max_track_err=0.1,
                progress_window=0.4, progress_limit=0.5, target_radius=0.15, time_penalty=0.15, checkpoint_reward_total=1000.0,
                max_time=90.0, continuity_break=0.030, action_low=(0.0, -0.4), action_high=(0.35, 0.4), cmd_offset=(0.0, 0.0, 0.0),
                dt_sim=0.001, substeps=10, num_cam_pts=8, num_checkpoints=100, n_max=1024, max_visible=128)
INT_FIELDS = ("substeps", "num_cam_pts", "num_checkpoints", "n_max", "max_visible")

# rg_goto.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "set_path": (i32, [fp, fp, i32, fp, fp, fp, fp, fp, fp, fp, C.POINTER(CPathPtrs), fp, fp]),
    "pre_step": (i32, [fp, fp, fp, C.POINTER(CPathPtrs), fp, fp, fp]),
    "post_step": (i32, [fp, fp, fp, C.POINTER(CPathPtrs), fp, fp, fp, fp]),
    "observe": (i32, [fp, fp, fp, C.POINTER(CPathPtrs), fp, fp]),
}


def load_library(path=None):
    """The rg_goto_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_goto", "the go-to-target task has no CPU fallback", SIGNATURES, {"config": CConfig}, {"state_rows": STATE_ROWS},
                ABI_VERSION, path)


def task_fields(mpc_cfg=None, **task):
    """The value of every rg_goto_config field as a dict: DEFAULTS, cmd_offset from the MPCConfig `mpc_cfg` (if given),
    overridden by `task`."""
    out = merged(DEFAULTS, task, "task")
    if mpc_cfg is not None and "cmd_offset" not in task:
        out["cmd_offset"] = (mpc_cfg.vx_offset, mpc_cfg.vy_offset, mpc_cfg.wz_offset)
    return out


def make_cconfig(mpc_cfg=None, **task):
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = c.reserved1 = 0
    return fill_config(c, task_fields(mpc_cfg, **task), INT_FIELDS)


def create_status(cfg=None, batch=1, device=0, **task):
    """(status, text) of rg_goto_create; destroys the handle when one is made.  cfg: a CConfig, an MPCConfig or None."""
    lib = load_library()
    cc = cfg if isinstance(cfg, CConfig) else make_cconfig(cfg, **task)
    return _create_status(lib, "rg_goto", C.byref(cc), int(batch), int(device))


class GotoHandle(Handle):
    """Owns one rg_goto_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_goto_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE."""

    unit, error = "rg_goto", RgGotoError

    def __init__(self, batch, mpc_cfg=None, device=None, **task):
        lib = load_library()
        self.batch = int(batch)
        self.fields = task_fields(mpc_cfg, **task)
        self.n_max = int(self.fields["n_max"])
        self.device, index = resolve_device(device, RgGotoError, "the go-to-target task has no CPU fallback", DEVICE_NONE)
        self._create(lib, C.byref(make_cconfig(mpc_cfg, **task)), self.batch, index)

    def set_path(self, paths: CPathPtrs, task_state_ptr, idx, npts, length, target, x, y, s, first_same_x):
        """Host arrays as rg_goto_set_path takes them (robot_gym_amd.gym.goto_path.pack_paths makes them)."""
        ia = index_array(idx)
        n = self.batch if ia is None else len(ia)
        npts = host_array(npts, np.int32, (n,), "npts")
        length = host_array(length, np.float64, (n,), "length")
        target = host_array(target, np.float64, (2, n), "target")
        x, y, s = (host_array(a, np.float64, (n, self.n_max), k) for a, k in ((x, "x"), (y, "y"), (s, "s")))
        first_same_x = host_array(first_same_x, np.int32, (n, self.n_max), "first_same_x")
        self._check(self._lib.rg_goto_set_path(self._h, host_ptr(ia), n, npts.ctypes.data, length.ctypes.data,
                                               target.ctypes.data, x.ctypes.data, y.ctypes.data, s.ctypes.data, first_same_x.ctypes.data,
                                               C.byref(paths), task_state_ptr, self._s()))

    def pre_step(self, task_state_ptr, sim_state_ptr, paths: CPathPtrs, action_ptr, cmd_ptr):
        self._check(self._lib.rg_goto_pre_step(self._h, task_state_ptr, sim_state_ptr, C.byref(paths), action_ptr, cmd_ptr, self._s()))

    def post_step(self, task_state_ptr, sim_state_ptr, paths: CPathPtrs, obs_ptr, reward_ptr, done_ptr):
        self._check(self._lib.rg_goto_post_step(self._h, task_state_ptr, sim_state_ptr, C.byref(paths), obs_ptr, reward_ptr, done_ptr, self._s()))

    def observe(self, task_state_ptr, sim_state_ptr, paths: CPathPtrs, obs_ptr):
        self._check(self._lib.rg_goto_observe(self._h, task_state_ptr, sim_state_ptr, C.byref(paths), obs_ptr, self._s()))
