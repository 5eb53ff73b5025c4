"""ctypes shim over the C-ABI of include/rg_scan.h (the terrain height scan of librg_mpc.so).

Plumbing only, like episode_abi: it loads the same library, mirrors rg_scan_config, turns negative status codes into
exceptions and owns one rg_scan_handle.  There is NO CPU fallback: without the library or a GPU the handle raises.
Every buffer is a caller-owned tensor (layouts: rg_scan.h); the terrain is the simulator's srb_abi.CTerrain.
"""
import ctypes as C

from robot_gym_amd.core import srb_abi
from robot_gym_amd.core.c_abi import STATUS, Handle, RgError, create_status as _create_status, d, fill_config, fp, i32, load, merged, resolve_device  # noqa: F401 -- STATUS stays a name of this module

ABI_VERSION = 1
MAX_POINTS = 256         # RG_SCAN_MAX_POINTS
DEVICE_NONE = -1         # RG_SCAN_DEVICE_NONE: a host-only handle


class RgScanError(RgError):
    unit = "rg_scan"


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("nx", i32), ("ny", i32), ("reserved0", i32), ("x_first", d), ("dx", d), ("y_first", d), ("dy", d),
        ("z_offset", d), ("clip", d), ("scale", d), ("reserved1", i32), ("reserved2", i32),
    ]


EXPORTS = ("rg_scan_create", "rg_scan_destroy", "rg_scan_last_error", "rg_scan_abi_version", "rg_scan_config_size", "rg_scan_set_terrain",
           "rg_scan_observe")

# an 8 x 6 grid from 0.2 m behind the body to 0.5 m ahead of it and 0.25 m to either side; z_offset None: the MPCConfig's body_height
DEFAULTS = dict(nx=8, ny=6, x_first=-0.2, dx=0.1, y_first=-0.25, dy=0.1, z_offset=None, clip=1.0, scale=1.0)
INT_FIELDS = ("nx", "ny")

# rg_scan.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "set_terrain": (i32, [fp, C.POINTER(srb_abi.CTerrain)]),
    "observe": (i32, [fp, fp, fp, fp, fp, fp]),
}


def load_library(path=None):
    """The rg_scan_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_scan", "the height scan has no CPU fallback", SIGNATURES, {"config": CConfig}, {}, ABI_VERSION, path)


def scan_fields(mpc_cfg=None, **settings):
    """The value of every rg_scan_config field as a dict: DEFAULTS overridden by `settings`; a z_offset of None is the
    body_height of mpc_cfg (an MPCConfig; None: ghost)."""
    out = merged(DEFAULTS, settings, "scan")
    if out["z_offset"] is None:
        if mpc_cfg is None:
            from robot_gym_amd.core.config import MPCConfig
            mpc_cfg = MPCConfig.for_robot("ghost")
        out["z_offset"] = float(mpc_cfg.body_height)
    return out


def make_cconfig(mpc_cfg=None, **settings):
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = c.reserved1 = c.reserved2 = 0
    return fill_config(c, scan_fields(mpc_cfg, **settings), INT_FIELDS)


def create_status(cconfig=None, batch=1, device=DEVICE_NONE, mpc_cfg=None):
    """(status, text) of rg_scan_create; destroys the handle when one is made.  cconfig: a CConfig (None: the defaults for
    mpc_cfg)."""
    lib = load_library()
    cconfig = make_cconfig(mpc_cfg) if cconfig is None else cconfig
    return _create_status(lib, "rg_scan", C.byref(cconfig), int(batch), int(device))


class ScanHandle(Handle):
    """Owns one rg_scan_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_scan_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE."""

    unit, error = "rg_scan", RgScanError

    def __init__(self, batch, mpc_cfg=None, device=None, **settings):
        lib = load_library()
        self.batch = int(batch)
        self.fields = scan_fields(mpc_cfg, **settings)
        self.device, index = resolve_device(device, RgScanError, "the height scan has no CPU fallback", DEVICE_NONE)
        cc = make_cconfig(mpc_cfg, **settings)
        self._create(lib, C.byref(cc), self.batch, index)

    def set_terrain(self, t: srb_abi.CTerrain = None):
        """rg_scan_set_terrain; None: the plane.  The tensors behind t.key / t.heights are the caller's to keep alive."""
        self._check(self._lib.rg_scan_set_terrain(self._h, None if t is None else C.byref(t)))

    def observe(self, sim_state_ptr, mask_ptr, out_ptr, prev_ptr):
        self._check(self._lib.rg_scan_observe(self._h, sim_state_ptr, mask_ptr, out_ptr, prev_ptr, self._s()))
