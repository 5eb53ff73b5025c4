"""ctypes shim over the entries of include/rg_srb_friction.h (the tick with Coulomb friction of the batched single-rigid-body
simulator of librg_mpc.so, and the draw of its coefficient).

Plumbing only, like dr_abi: the entries have no handle of their own, they take the simulator's, so this module declares them on
the library srb_abi loads and calls them on an srb_abi.SrbHandle.  There is NO CPU fallback.  Every buffer is a caller-owned
tensor (layouts: rg_srb_friction.h), checked here -- type, dtype, shape, contiguity, device -- before the library sees its
address.  srb_abi itself is left as it is: its declarations are held to a recording.
"""
import ctypes as C
import math

from robot_gym_amd.core import srb_abi
from robot_gym_amd.core.c_abi import d, fp, i32, stream
from robot_gym_amd.core.srb_abi import CObsPtrs, RgSrbError, STATE_ROWS, checked_ptr

PURPOSE_MU = 48                      # RG_SRB_FRICTION_PURPOSE_MU: block 3 of the registry of rg_stream.h
SLIP_GAIN, SLIP_SPEED_MAX = 0.01, 1.0    # the Python layer's defaults: choices, not measurements (rg_srb_friction.h)

EXPORTS = ("rg_srb_step_friction", "rg_srb_friction_draw")

SIGNATURES = {
    "rg_srb_step_friction": (i32, [fp, fp, fp, fp, fp, i32, fp, C.POINTER(CObsPtrs), fp, d, d, fp, fp, fp]),
    "rg_srb_friction_draw": (i32, [fp, fp, fp, fp, C.c_uint64, d, d, fp, fp]),
}

_declared = set()


def load_library(path=None):
    """The library of srb_abi.load_library with the two friction entries declared.  Raises (never falls back) when the library
    is missing or lacks an entry."""
    lib = srb_abi.load_library(path)
    if id(lib) not in _declared:
        for name, (restype, argtypes) in SIGNATURES.items():
            if not hasattr(lib, name):
                raise ImportError(f"librg_mpc.so lacks {name}: rebuild it (make -C robot_gym_amd/csrc); the friction tick has no CPU fallback")
            f = getattr(lib, name)
            f.restype, f.argtypes = restype, argtypes
        _declared.add(id(lib))
    return lib


def _srb(sim_handle):
    """The rg_srb_handle behind an srb_abi.SrbHandle (or a raw address, or None)."""
    return getattr(sim_handle, "_h", sim_handle)


def checked_settings(slip_gain, slip_speed_max):
    """(slip_gain, slip_speed_max) as floats once they are what the library takes: finite and >= 0."""
    out = []
    for name, v in (("slip_gain", slip_gain), ("slip_speed_max", slip_speed_max)):
        try:
            x = float(v)
        except (TypeError, ValueError):
            raise ValueError(f"step_friction: {name} must be a number, got {v!r}") from None
        if not (math.isfinite(x) and x >= 0.0):
            raise ValueError(f"step_friction: {name} must be finite and >= 0, got {v!r}")
        out.append(x)
    return tuple(out)


def checked_range(lo, hi, what="friction_draw"):
    """(lo, hi) as floats once they are what rg_srb_friction_draw takes: 0 <= lo <= hi, both finite."""
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the range must be a pair of numbers (lo, hi), got {(lo, hi)!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo <= hi):
        raise ValueError(f"{what}: the range needs 0 <= lo <= hi, both finite, got ({lo}, {hi})")
    return lo, hi


def step_friction_ptrs(batch, device, state, grf, foot_target, leg_state, mu, ext=None, touch=None, slip=None):
    """(state, grf, foot_target, leg_state, mu, ext, touch, slip) addresses for rg_srb_step_friction, every tensor checked first."""
    import torch
    B, e = int(batch), "step_friction"
    return (checked_ptr(state, "state", torch.float64, (STATE_ROWS, B), device, e),
            checked_ptr(grf, "grf", torch.float32, (B, 12), device, e),
            checked_ptr(foot_target, "foot_target", torch.float32, (B, 12), device, e),
            checked_ptr(leg_state, "leg_state", torch.int32, (B, 4), device, e),
            checked_ptr(mu, "mu", torch.float64, (B,), device, e),
            checked_ptr(ext, "ext", torch.float64, (6, B), device, e, optional=True),
            checked_ptr(touch, "touch", torch.int32, (4, B), device, e, optional=True),
            checked_ptr(slip, "slip", torch.float64, (4, B), device, e, optional=True))


def friction_draw_ptrs(batch, device, mask, key, draws, mu):
    """(mask, key, draws, mu) addresses for rg_srb_friction_draw, every tensor checked first."""
    import torch
    B, e = int(batch), "friction_draw"
    return (checked_ptr(mask, "mask", torch.int32, (B,), device, e), checked_ptr(key, "key", torch.float64, (B,), device, e),
            checked_ptr(draws, "draws", torch.float64, (B,), device, e), checked_ptr(mu, "mu", torch.float64, (B,), device, e))


def _check(srb, lib, rc):
    if rc != 0:
        raise RgSrbError(rc, lib.rg_srb_last_error(_srb(srb)).decode())


def step_friction(srb, state, grf, foot_target, leg_state, measured, ext, obs: CObsPtrs, mu, slip_gain=SLIP_GAIN, slip_speed_max=SLIP_SPEED_MAX,
                  touch=None, slip=None):
    """rg_srb_step_friction on the srb_abi.SrbHandle `srb` and TENSORS (ext, touch and slip may be None), on torch's current
    stream of the handle's device."""
    lib = load_library()
    gain, vmax = checked_settings(slip_gain, slip_speed_max)
    if measured not in (0, 1, False, True):
        raise ValueError(f"step_friction: measured must be 0 or 1, got {measured!r}")
    p = step_friction_ptrs(srb.batch, srb.device, state, grf, foot_target, leg_state, mu, ext, touch, slip)
    _check(srb, lib, lib.rg_srb_step_friction(_srb(srb), p[0], p[1], p[2], p[3], int(measured), p[5], C.byref(obs), p[4], gain, vmax, p[6], p[7],
                                              stream(srb.device)))


def friction_draw(srb, mask, key, draws, seed, lo, hi, mu):
    """rg_srb_friction_draw on the srb_abi.SrbHandle `srb`: mu[b] drawn in [lo, hi] for the robots of the mask.  key and draws
    are float64 [B] rows (rows 0 and 1 of a DomainRandomizer's state)."""
    lib = load_library()
    lo, hi = checked_range(lo, hi)
    p = friction_draw_ptrs(srb.batch, srb.device, mask, key, draws, mu)
    _check(srb, lib, lib.rg_srb_friction_draw(_srb(srb), p[0], p[1], p[2], int(seed) & 0xFFFFFFFFFFFFFFFF, lo, hi, p[3], stream(srb.device)))
