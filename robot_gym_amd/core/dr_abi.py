"""ctypes shim over the C-ABI of include/rg_dr.h (the domain randomisation of librg_mpc.so).

Plumbing only, like scan_abi: it loads the same library, mirrors rg_dr_config, turns negative status codes into exceptions
and owns one rg_dr_handle.  There is NO CPU fallback: without the library or a GPU the handle raises.  Every buffer is a
caller-owned tensor (layouts: rg_dr.h); the simulator is named by its srb_abi.SrbHandle.
"""
import ctypes as C

from robot_gym_amd.core.c_abi import STATUS, Handle, RgError, create_status as _create_status, d, fill_config, fp, i32, load, merged, resolve_device  # noqa: F401 -- STATUS stays a name of this module

ABI_VERSION = 1
ROWS = 8                 # RG_DR_ROWS
ROW_KEY, ROW_DRAWS, ROW_MASS_SCALE, ROW_INERTIA_SCALE, ROW_WORLD = range(5)
BODY_ROWS = 19           # RG_DR_BODY_ROWS: mass, I[9], I^-1[9]
PURPOSE_MASS, PURPOSE_INERTIA, PURPOSE_WORLD, PURPOSE_PUSH_START, PURPOSE_PUSH_COMPONENT, PURPOSE_PUSH_GATE = range(6)
DEVICE_NONE = -1         # RG_DR_DEVICE_NONE: a host-only handle


class RgDrError(RgError):
    unit = "rg_dr"


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("worlds", i32), ("seed", C.c_uint64), ("mass_lo", d), ("mass_hi", d), ("inertia_lo", d), ("inertia_hi", d),
        ("push_interval", i32), ("push_ticks", i32), ("push_probability", d), ("push_force_xy", d), ("push_force_z", d), ("push_torque_xy", d),
        ("push_torque_z", d), ("substeps", i32), ("reserved0", i32),
    ]


EXPORTS = ("rg_dr_create", "rg_dr_destroy", "rg_dr_last_error", "rg_dr_abi_version", "rg_dr_config_size", "rg_dr_state_rows", "rg_dr_capture_body",
           "rg_dr_reset", "rg_dr_apply", "rg_dr_push", "rg_dr_get_body")

# the identity: no scale, no new world, no push.  Every magnitude is the caller's choice.
DEFAULTS = dict(worlds=0, seed=0, mass_lo=1.0, mass_hi=1.0, inertia_lo=1.0, inertia_hi=1.0, push_interval=0, push_ticks=0, push_probability=0.0,
                push_force_xy=0.0, push_force_z=0.0, push_torque_xy=0.0, push_torque_z=0.0, substeps=10)
INT_FIELDS = ("worlds", "seed", "push_interval", "push_ticks", "substeps")

# rg_dr.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "capture_body": (i32, [fp, fp]),
    "reset": (i32, [fp, fp, fp, fp, fp, fp]),
    "apply": (i32, [fp, fp, fp, fp, fp]),
    "push": (i32, [fp, fp, fp, fp, fp]),
    "get_body": (i32, [fp, fp, fp, fp]),
}


def load_library(path=None):
    """The rg_dr_* entries of librg_mpc.so (c_abi.LIB_PATH).  Raises (never falls back) when the library is missing."""
    return load("rg_dr", "the domain randomisation has no CPU fallback", SIGNATURES, {"config": CConfig}, {"state_rows": ROWS}, ABI_VERSION, path)


def make_cconfig(**settings):
    c = CConfig()
    c.abi_version = ABI_VERSION
    c.reserved0 = 0
    fields = merged(DEFAULTS, settings, "randomiser")
    fields["seed"] = int(fields["seed"]) & 0xFFFFFFFFFFFFFFFF
    return fill_config(c, fields, INT_FIELDS)


def create_status(cconfig=None, batch=1, device=DEVICE_NONE):
    """(status, text) of rg_dr_create; destroys the handle when one is made.  cconfig: a CConfig (None: the defaults)."""
    lib = load_library()
    cconfig = make_cconfig() if cconfig is None else cconfig
    return _create_status(lib, "rg_dr", C.byref(cconfig), int(batch), int(device))


def _srb(sim_handle):
    """The rg_srb_handle behind an srb_abi.SrbHandle (or a raw address, or None)."""
    return getattr(sim_handle, "_h", sim_handle)


class DrHandle(Handle):
    """Owns one rg_dr_handle and launches on torch's current stream of its device.  device=DEVICE_NONE makes the host-only
    handle of rg_dr_create: it needs no GPU, every call checks its arguments and then raises NO_DEVICE.  `srb` arguments are
    srb_abi.SrbHandle objects."""

    unit, error = "rg_dr", RgDrError

    def __init__(self, batch, device=None, **settings):
        lib = load_library()
        self.batch = int(batch)
        self.fields = merged(DEFAULTS, settings, "randomiser")
        self.device, index = resolve_device(device, RgDrError, "the domain randomisation has no CPU fallback", DEVICE_NONE)
        self._create(lib, C.byref(make_cconfig(**settings)), self.batch, index)

    def capture_body(self, srb):
        self._check(self._lib.rg_dr_capture_body(self._h, _srb(srb)))

    def reset(self, srb, mask_ptr, state_ptr, terrain_key_ptr):
        self._check(self._lib.rg_dr_reset(self._h, _srb(srb), mask_ptr, state_ptr, terrain_key_ptr, self._s()))

    def apply(self, srb, mask_ptr, state_ptr):
        self._check(self._lib.rg_dr_apply(self._h, _srb(srb), mask_ptr, state_ptr, self._s()))

    def push(self, sim_state_ptr, state_ptr, ext_ptr):
        self._check(self._lib.rg_dr_push(self._h, sim_state_ptr, state_ptr, ext_ptr, self._s()))

    def get_body(self, srb, out_ptr):
        self._check(self._lib.rg_dr_get_body(self._h, _srb(srb), out_ptr, self._s()))
