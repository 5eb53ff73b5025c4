"""What the ctypes shims over librg_mpc.so (mpc_abi, srb_abi, goto_abi, episode_abi, posctl_abi, policy_abi, ppo_abi, ddpg_abi,
rnn_abi, scan_abi, dr_abi, sensor_abi, est_abi, friction_abi) share: the type aliases and the library's path, the error and handle base classes, the loader with its version, size
and constant checks, the device and stream of a handle, and the settings, config and host-array helpers.  Only the shims
import it.  Everything that belongs to one unit -- structures, constants, defaults, entry methods -- stays in that unit's module.
"""
import ctypes as C
import os

import numpy as np

d, i32, i64, fp = C.c_double, C.c_int32, C.c_int64, C.c_void_p
STATUS = {0: "OK", -1: "INVALID", -2: "HIP", -3: "NO_DEVICE", -4: "ALLOC"}

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "csrc")
# RG_MPC_LIB: load another build of the same C-ABI (kernel A/B experiments); never a fallback
LIB_PATH = os.environ.get("RG_MPC_LIB") or os.path.abspath(os.path.join(_CSRC, "librg_mpc.so"))


class RgError(RuntimeError):
    """A negative status of a unit's entry with its last_error text.  A subclass sets `unit` (and `names` where its header's
    status codes are not STATUS)."""
    unit, names = None, STATUS

    def __init__(self, status, text):
        super().__init__(f"{self.unit} status {status} ({self.names.get(status, '?')}): {text}")
        self.status = status


_libs = {}        # path -> CDLL: one per path for the whole process
_loaded = set()   # (unit, path) whose entries are declared and checked


def load(unit, what, signatures, sizes, constants, version, path=None):
    """The library at `path` (None: LIB_PATH) with the entries of `unit` declared and checked against the binding.
    signatures: {entry: (restype, argtypes)} without the unit's prefix; destroy, last_error, abi_version and the getters of
    `sizes` and `constants` are declared here.  sizes: {name: Structure} against <unit>_<name>_size(); constants: {name: value}
    against <unit>_<name>().  `what` ends the text of the ImportError for a missing library.  Raises, never falls back."""
    p = path or LIB_PATH
    if p not in _libs:
        if not os.path.exists(p):
            raise ImportError(f"{p} not found: build it with `make -C robot_gym_amd/csrc` (or __graft_entry__.build()); {what}")
        _libs[p] = C.CDLL(p)
    L = _libs[p]
    if (unit, p) in _loaded:
        return L
    getters = ["abi_version"] + [f"{name}_size" for name in sizes] + list(constants)
    for entry, (restype, argtypes) in {"destroy": (None, [fp]), "last_error": (C.c_char_p, [fp]), **{g: (i32, []) for g in getters},
                                       **signatures}.items():
        f = getattr(L, f"{unit}_{entry}")
        f.restype, f.argtypes = restype, argtypes
    if getattr(L, f"{unit}_abi_version")() != version:
        raise ImportError(f"librg_mpc.so {unit} ABI version mismatch")
    for name, struct in sizes.items():
        got = getattr(L, f"{unit}_{name}_size")()
        if got != C.sizeof(struct):
            raise ImportError(f"{unit}_{name} size mismatch: lib {got} vs binding {C.sizeof(struct)}")
    for name, value in constants.items():
        got = getattr(L, f"{unit}_{name}")()
        if got != value:
            raise ImportError(f"{unit} {name.replace('_', ' ')} mismatch: lib {got} vs binding {value}")
    _loaded.add((unit, p))
    return L


def create_status(lib, unit, *args):
    """(status, text) of the unit's create called with `args` and a slot for the handle; destroys the handle when one is made."""
    h = fp()
    rc = getattr(lib, f"{unit}_create")(*args, C.byref(h))
    text = getattr(lib, f"{unit}_last_error")(None).decode() if rc else ""
    if h:
        getattr(lib, f"{unit}_destroy")(h)
    return rc, text


def resolve_device(device, error, what, none=None):
    """(torch.device, index) of a handle's `device`: None or an index-less "cuda" is torch's current device; without a GPU
    raises error(-3, "no GPU: <what>").  `none` is the unit's DEVICE_NONE where its create takes one: it gives (None, none),
    the host-only handle, and torch is not needed."""
    if none is not None and device == none:
        return None, none
    import torch
    if not torch.cuda.is_available():
        raise error(-3, f"no GPU: {what}")
    index = None if device is None else torch.device(device).index
    dev = torch.device("cuda", torch.cuda.current_device() if index is None else index)
    return dev, dev.index


def stream(device):
    """torch's current stream of `device` as the hipStream_t the entries take."""
    import torch
    return fp(torch.cuda.current_stream(device).cuda_stream)


class Handle:
    """Owns one handle of a unit: create, the status check of every entry, close.  A subclass sets `unit` and `error`, calls
    _create from its __init__ and writes out one method per entry: self._check(self._lib.<entry>(self._h, ..., self._s()))."""
    unit = error = _h = None

    def _create(self, lib, *args):
        """<unit>_create(*args, &handle); raises `error` with the library's text when it fails."""
        self._lib, self._h = lib, fp()
        self._last_error, self._destroy = getattr(lib, f"{self.unit}_last_error"), getattr(lib, f"{self.unit}_destroy")
        rc = getattr(lib, f"{self.unit}_create")(*args, C.byref(self._h))
        if rc != 0:
            msg = self._last_error(None)
            self._h = fp()
            raise self.error(rc, msg.decode() if msg else "create failed")

    def _check(self, rc):
        if rc != 0:
            raise self.error(rc, self._last_error(self._h).decode())

    def _s(self):
        return None if self.device is None else stream(self.device)

    def close(self):
        if self._h:
            self._destroy(self._h)
            self._h = fp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merged(defaults, settings, what):
    """`defaults` overridden by `settings` as a new dict; a setting that is no default raises."""
    unknown = set(settings) - set(defaults)
    if unknown:
        raise TypeError(f"unknown {what} setting(s) {sorted(unknown)}")
    return {**defaults, **settings}


def fill_config(c, fields, int_fields=()):
    """Writes the dict `fields` into the structure `c` and returns it: a sequence element by element as float after a check
    of its length, the names of `int_fields` with int, every other value with float."""
    for name, v in fields.items():
        if hasattr(v, "__len__"):
            arr = getattr(c, name)
            if len(v) != len(arr):
                raise ValueError(f"config field {name}: expected {len(arr)} values, got {len(v)}")
            for k, x in enumerate(v):
                arr[k] = float(x)
        else:
            setattr(c, name, int(v) if name in int_fields else float(v))
    return c


def host_array(a, dtype, shape, name):
    """`a` as a contiguous numpy array of `dtype`, which must have `shape`."""
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype))
    if a.shape != shape:
        raise ValueError(f"{name} must have shape {list(shape)}, got {list(a.shape)}")
    return a


def index_array(idx):
    """A list of robots as a flat contiguous int32 numpy array; None (every robot) stays None."""
    return None if idx is None else np.ascontiguousarray(np.asarray(idx, dtype=np.int32).reshape(-1))


def host_ptr(a):
    """The address of a host array; None is the C-ABI's NULL."""
    return None if a is None else a.ctypes.data
