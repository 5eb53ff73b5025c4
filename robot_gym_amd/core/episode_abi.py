"""ctypes shim over the C-ABI of include/rg_episode.h (the episode reset on the device of librg_mpc.so).

Plumbing only, like goto_abi: it loads the same library, mirrors rg_episode_config, turns negative status codes into
exceptions and owns one rg_episode_handle.  There is NO CPU fallback: without the library or a GPU the handle raises.
Every buffer is a caller-owned tensor (layouts: rg_episode.h).
"""
import ctypes as C
import os

from robot_gym_amd.core import goto_abi, mpc_abi, srb_abi

ABI_VERSION = 1
ROWS = 12                # RG_EPISODE_ROWS
(ROW_EPISODE, ROW_PLAN_STATUS, ROW_RETURN, ROW_LENGTH, ROW_LAST_RETURN, ROW_LAST_LENGTH, ROW_LAST_REASON, ROW_NPTS, ROW_NWAY, ROW_KEY,
 ROW_ENDED) = range(11)
MAX_WAYPOINTS, MAX_OBSTACLES, MAX_OSCILLATION = 64, 16, 8
DEVICE_NONE = -1         # RG_EPISODE_DEVICE_NONE: a host-only handle
PLAN_STATUS = ("ok", "target", "waypoints", "short", "long")   # RG_EPISODE_PLAN_*
d = C.c_double
i32 = C.c_int32
fp = C.c_void_p

STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE", -4: "ALLOC"}


class RgEpisodeError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"rg_episode status {status} ({STATUS.get(status, '?')}): {text}")
        self.status = status


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("reserved0", i32), ("kp", d), ("eta", d), ("area_width", d), ("grid", d), ("robot_radius", d),
        ("spacing", d), ("seed", C.c_uint64), ("oscillation_length", i32), ("max_waypoints", i32), ("num_obstacles", i32),
        ("reserved1", i32), ("obstacles", (d * 2) * MAX_OBSTACLES),
    ]


EXPORTS = ("rg_episode_create", "rg_episode_destroy", "rg_episode_last_error", "rg_episode_abi_version", "rg_episode_config_size",
           "rg_episode_state_rows", "rg_episode_reset", "rg_episode_accumulate")

# goto_path.py's constants (KP, ETA, AREA_WIDTH, GRID, ROBOT_RADIUS, SPACING, OSCILLATION_LENGTH)
DEFAULTS = dict(kp=5.0, eta=100.0, area_width=5.0, grid=0.5, robot_radius=0.25, spacing=1e-2, seed=0, oscillation_length=3,
                max_waypoints=64)
INT_FIELDS = ("seed", "oscillation_length", "max_waypoints")

_lib = None


def load_library(path=None):
    """The rg_episode_* entries of librg_mpc.so (mpc_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or mpc_abi.LIB_PATH
    if not os.path.exists(p):
        raise ImportError(f"{p} not found: build it with `make -C robot_gym_amd/csrc` (or __graft_entry__.build()); "
                          "the episode reset has no CPU fallback")
    L = C.CDLL(p)
    L.rg_episode_create.argtypes = [C.POINTER(CConfig), C.POINTER(srb_abi.CConfig), C.POINTER(goto_abi.CConfig), i32, i32, C.POINTER(fp)]
    L.rg_episode_create.restype = i32
    L.rg_episode_destroy.argtypes = [fp]
    L.rg_episode_destroy.restype = None
    L.rg_episode_last_error.argtypes = [fp]
    L.rg_episode_last_error.restype = C.c_char_p
    L.rg_episode_abi_version.restype = i32
    L.rg_episode_config_size.restype = i32
    L.rg_episode_state_rows.restype = i32
    L.rg_episode_reset.argtypes = [fp, fp, fp, fp, fp, fp, C.POINTER(srb_abi.CObsPtrs), C.POINTER(goto_abi.CPathPtrs), fp, fp, fp, fp]
    L.rg_episode_reset.restype = i32
    L.rg_episode_accumulate.argtypes = [fp, fp, fp, fp, fp]
    L.rg_episode_accumulate.restype = i32
    if L.rg_episode_abi_version() != ABI_VERSION:
        raise ImportError("librg_mpc.so rg_episode ABI version mismatch")
    if L.rg_episode_config_size() != C.sizeof(CConfig):
        raise ImportError(f"rg_episode_config size mismatch: lib {L.rg_episode_config_size()} vs binding {C.sizeof(CConfig)}")
    if L.rg_episode_state_rows() != ROWS:
        raise ImportError(f"rg_episode state rows mismatch: lib {L.rg_episode_state_rows()} vs binding {ROWS}")
    if path is None:
        _lib = L
    return L


def episode_fields(obstacles=(), **settings):
    """The value of every rg_episode_config field as a dict: DEFAULTS overridden by `settings`, and the obstacles [(x, y), ...]."""
    unknown = set(settings) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown episode setting(s) {sorted(unknown)}")
    out = dict(DEFAULTS)
    out.update(settings)
    obs = [(float(o[0]), float(o[1])) for o in (() if obstacles is None else obstacles)]
    if len(obs) > MAX_OBSTACLES:
        raise ValueError(f"at most {MAX_OBSTACLES} obstacles, got {len(obs)}")
    out["obstacles"] = tuple(obs)
    return out


def make_cconfig(obstacles=(), **settings):
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = c.reserved1 = 0
    f = episode_fields(obstacles, **settings)
    for name, v in f.items():
        if name == "obstacles":
            c.num_obstacles = len(v)
            for k, (x, y) in enumerate(v):
                c.obstacles[k][0], c.obstacles[k][1] = x, y
        elif name in INT_FIELDS:
            setattr(c, name, int(v))
        else:
            setattr(c, name, float(v))
    return c


def create_status(ecfg=None, scfg=None, gcfg=None, batch=1, device=DEVICE_NONE, mpc_cfg=None):
    """(status, text) of rg_episode_create; destroys the handle when one is made.  ecfg / scfg / gcfg: the three CConfig
    structures, each defaulting to the one made from mpc_cfg (an MPCConfig; None: ghost)."""
    lib = load_library()
    if mpc_cfg is None and (scfg is None or gcfg is None):
        from robot_gym_amd.core.config import MPCConfig
        mpc_cfg = MPCConfig.for_robot("ghost")
    ecfg = make_cconfig() if ecfg is None else ecfg
    scfg = srb_abi.make_cconfig(mpc_cfg) if scfg is None else scfg
    gcfg = goto_abi.make_cconfig(mpc_cfg) if gcfg is None else gcfg
    h = fp()
    rc = lib.rg_episode_create(C.byref(ecfg), C.byref(scfg), C.byref(gcfg), int(batch), int(device), C.byref(h))
    text = lib.rg_episode_last_error(None).decode() if rc else ""
    if h:
        lib.rg_episode_destroy(h)
    return rc, text


class EpisodeHandle:
    """Owns one rg_episode_handle and launches on torch's current stream of its device.  sim_settings / task_settings are the
    keyword settings the simulator (srb_abi.make_cconfig) and the task (goto_abi.make_cconfig) were created with.
    device=DEVICE_NONE makes the host-only handle of rg_episode_create: it needs no GPU, every call checks its arguments and
    then raises NO_DEVICE."""

    def __init__(self, batch, mpc_cfg, device=None, obstacles=(), sim_settings=None, task_settings=None, **settings):
        self._h = fp()
        self._lib = load_library()
        self.batch = int(batch)
        self.fields = episode_fields(obstacles, **settings)
        if device == DEVICE_NONE:
            self.device, index = None, DEVICE_NONE
        else:
            import torch
            if not torch.cuda.is_available():
                raise RgEpisodeError(-3, "no GPU: the episode reset has no CPU fallback")
            index = None if device is None else torch.device(device).index
            self.device = torch.device("cuda", torch.cuda.current_device() if index is None else index)
            index = self.device.index
        ec = make_cconfig(obstacles, **settings)
        sc = srb_abi.make_cconfig(mpc_cfg, **(sim_settings or {}))
        gc = goto_abi.make_cconfig(mpc_cfg, **(task_settings or {}))
        rc = self._lib.rg_episode_create(C.byref(ec), C.byref(sc), C.byref(gc), self.batch, index, C.byref(self._h))
        if rc != 0:
            msg = self._lib.rg_episode_last_error(None)
            self._h = fp()
            raise RgEpisodeError(rc, msg.decode() if msg else "create failed")

    def _check(self, rc):
        if rc != 0:
            raise RgEpisodeError(rc, self._lib.rg_episode_last_error(self._h).decode())

    def _s(self):
        return None if self.device is None else goto_abi._stream(self.device)

    def reset(self, mask_ptr, targets_ptr, episode_state_ptr, task_state_ptr, sim_state_ptr, sim_obs, paths, obs_ptr, final_obs_ptr,
              reset_mask_ptr):
        """rg_episode_reset; sim_obs: srb_abi.CObsPtrs (or None), paths: goto_abi.CPathPtrs (or None)."""
        self._check(self._lib.rg_episode_reset(self._h, mask_ptr, targets_ptr, episode_state_ptr, task_state_ptr, sim_state_ptr,
                                               None if sim_obs is None else C.byref(sim_obs), None if paths is None else C.byref(paths),
                                               obs_ptr, final_obs_ptr, reset_mask_ptr, self._s()))

    def accumulate(self, episode_state_ptr, reward_ptr, done_ptr):
        self._check(self._lib.rg_episode_accumulate(self._h, episode_state_ptr, reward_ptr, done_ptr, self._s()))

    def close(self):
        if self._h:
            self._lib.rg_episode_destroy(self._h)
            self._h = fp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
