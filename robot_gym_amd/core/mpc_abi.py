"""ctypes shim over the C-ABI of include/rg_mpc.h (librg_mpc.so).

This is the "new C-ABI shim under robot_gym/core" of the north star.  It is plumbing: it
loads the HIP library, mirrors rg_mpc_config / rg_mpc_state_ptrs / rg_mpc_out_ptrs, and turns
negative status codes into exceptions.  There is NO CPU fallback: if the library is missing
or no GPU is present the constructor raises.
"""
import ctypes as C

from robot_gym_amd.core.c_abi import LIB_PATH, Handle, RgError, d, fp, i32, i64, load  # noqa: F401 -- LIB_PATH: read by tools and tests

ABI_VERSION = 5
AUDIT_PERIOD = 8   # RG_MPC_AUDIT_PERIOD: the audit lane picks on the first tick and then on every 8th one (ticks 4, 12, 20 ...)


class RgMpcError(RgError):
    unit = "rg_mpc"

    def __init__(self, status, text):     # its own, shorter text: no status name
        RuntimeError.__init__(self, f"rg_mpc status {status}: {text}")
        self.status = status


class CConfig(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("horizon", i32), ("dt_plan", d), ("mass", d), ("inertia", d * 9), ("body_height", d),
        ("weights", d * 13), ("alpha", d), ("mu", d * 4), ("fz_max_scale", d), ("fz_min_scale", d), ("gravity", d),
        ("stance_duration", d * 4), ("duty_factor", d * 4), ("init_phase", d * 4), ("init_state", i32 * 4),
        ("contact_phase_thresh", d), ("window", i32), ("kin_mode", i32), ("foot_clearance", d), ("swing_kp", d * 3),
        ("max_clearance", d), ("hip", d * 12), ("motor_kp", d * 12), ("motor_kd", d * 12), ("motor_dir", d * 12),
        ("motor_off", d * 12), ("jxyz", d * 36), ("jrpy", d * 36), ("jaxis", d * 36), ("toe_xyz", d * 12),
        ("toe_com", d * 12), ("base_com", d * 3), ("ik_iters", i32), ("solver", i32), ("ik_damping", d),
        ("ik_max_step", d), ("admm_iters", i32), ("reserved0", i32), ("admm_rho", d), ("admm_relax", d),
        ("admm_tol", d), ("admm_check", i32), ("contact_lookahead", i32), ("warm_start", i32), ("reserved2", i32),
        ("admm_rho2", d), ("admm_switch", i32), ("admm_accel", i32), ("admm_extrap", d),
        ("accel_cos2", d), ("accel_rmax", d), ("accel_rmin", d), ("accel_rate_cap", d),
        ("audit_k", i32), ("reserved3", i32), ("audit_tol", d), ("admm_rho34_scale", d), ("admm_rho_sched_scale", d),
        ("lane_grid", i32), ("conv_alpha_doubled", i32), ("conv_feet_rotation", i32), ("conv_com_height", i32), ("conv_first_latch", i32),
        ("conv_window_divide", i32), ("conv_friction_rows", i32),
    ]


class CStatePtrs(C.Structure):
    _fields_ = [(n, fp) for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac", "contact", "cmd", "contact_sched", "t_robot")]


class COutPtrs(C.Structure):
    _fields_ = [(n, fp) for n in ("action", "grf", "tau_stance", "leg_state", "desired_state", "phase", "foot_target", "v_body")]


EXPORTS = ("rg_mpc_create", "rg_mpc_reset", "rg_mpc_reset_at", "rg_mpc_reset_masked", "rg_mpc_set_command", "rg_mpc_set_gait", "rg_mpc_set_body", "rg_mpc_state_layout", "rg_mpc_state_check", "rg_mpc_save_state", "rg_mpc_load_state", "rg_mpc_copy_state", "rg_mpc_step", "rg_mpc_step_host", "rg_mpc_hybrid_to_torque",
           "rg_mpc_hybrid_to_torque_substeps",
           "rg_mpc_last_bin_counts", "rg_mpc_last_solver_stats", "rg_mpc_last_iterations", "rg_mpc_audit_stats", "rg_mpc_last_direct_count", "rg_mpc_profile_begin", "rg_mpc_profile_stride", "rg_mpc_profile_end", "rg_mpc_kernel_names", "rg_mpc_plan_description", "rg_mpc_profile_window_names", "rg_mpc_debug_poison_lds", "rg_mpc_destroy", "rg_mpc_last_error",
           "rg_mpc_abi_version", "rg_mpc_config_size")

_I32P, _I64P, _DP = C.POINTER(i32), C.POINTER(i64), C.POINTER(d)
# rg_mpc.h's entries past those every unit has; the int32 getters are declared with the checks they serve
SIGNATURES = {
    "create": (i32, [C.POINTER(CConfig), i32, i32, C.POINTER(fp)]),
    "reset": (i32, [fp, _I32P, i32, d, fp]),
    "reset_at": (i32, [fp, _I32P, _DP, i32, fp]),
    "reset_masked": (i32, [fp, fp, d, fp]),
    "set_command": (i32, [fp, fp, fp]),
    "set_gait": (i32, [fp, fp, fp, fp, fp, fp]),
    "set_body": (i32, [fp, _I32P, i32, fp, fp, fp, fp, fp, fp]),
    "state_layout": (i32, [C.POINTER(CConfig), _I64P, C.POINTER(C.c_char_p)]),
    "state_check": (i32, [C.POINTER(CConfig), fp, i32, i64, _I32P, i32]),
    "save_state": (i32, [fp, _I32P, i32, fp, fp]),
    "load_state": (i32, [fp, _I32P, i32, fp, _DP, fp]),
    "copy_state": (i32, [fp, _I32P, _I32P, i32, fp]),
    "step": (i32, [fp, d, C.POINTER(CStatePtrs), C.POINTER(COutPtrs), fp]),
    "step_host": (i32, [fp, d, fp, fp, i64, C.POINTER(CStatePtrs), C.POINTER(COutPtrs), fp, fp]),
    "hybrid_to_torque": (i32, [fp, fp, fp, fp, fp, fp]),
    "hybrid_to_torque_substeps": (i32, [fp, fp, fp, fp, fp, i32, fp]),
    "last_bin_counts": (i32, [fp, C.POINTER(i32 * 5), fp]),
    "last_solver_stats": (i32, [fp, _I64P, _I32P, _I32P, _I32P, _I32P, fp]),
    "last_iterations": (i32, [fp, _I32P, _I32P, fp]),
    "audit_stats": (i32, [fp, _I64P, _I64P, _DP, _DP, _I64P, _I64P, i32, fp]),
    "last_direct_count": (i32, [fp, _I32P, _I64P, fp]),
    "profile_begin": (i32, [fp, i32]),
    "profile_stride": (i32, [fp, i32]),
    "profile_end": (i32, [fp, C.POINTER(C.c_float * 6), C.POINTER(i32 * 5), fp]),
    "kernel_names": (C.c_char_p, []),
    "plan_description": (C.c_char_p, [fp]),
    "profile_window_names": (C.c_char_p, [fp]),
    "debug_poison_lds": (i32, [fp, fp]),
}


def load_library(path=None):
    """Load librg_mpc.so.  Raises (never falls back) when the HIP extension is missing."""
    return load("rg_mpc", "the MPC path has no CPU fallback", SIGNATURES, {"config": CConfig}, {}, ABI_VERSION, path)


def _i32_array(idx):
    """An index list as a ctypes int32 array (None stays None)."""
    if idx is None:
        return None
    import numpy as np
    a = np.asarray(idx).reshape(-1)
    if a.size and a.dtype.kind not in "iu":
        if not np.all(np.equal(np.mod(a.astype(np.float64), 1), 0)):
            raise ValueError("index lists must hold integers")
    a = a.astype(np.int64) if a.dtype.kind != "u" else a
    if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
        raise ValueError(f"index {int(a.max()) if a.max() >= (1 << 31) else int(a.min())} outside the int32 range of the C-ABI")
    a = np.ascontiguousarray(a, dtype=np.int32)
    return (i32 * len(a)).from_buffer_copy(a.tobytes()) if len(a) else (i32 * 0)()


def state_layout(cfg):
    """rg_mpc_state_layout: (row_bytes, description line) of the state rows of `cfg` (no handle, no GPU)."""
    lib = load_library()
    nb, desc = C.c_int64(), C.c_char_p()
    rc = lib.rg_mpc_state_layout(C.byref(make_cconfig(cfg)), C.byref(nb), C.byref(desc))
    if rc != 0:
        raise RgMpcError(rc, lib.rg_mpc_last_error(None).decode())
    return nb.value, desc.value.decode()


def state_check(cfg, rows, dst=None, batch=0):
    """rg_mpc_state_check on host rows (a numpy buffer of n rows): raises RgMpcError naming the first bad row, robot and field."""
    import numpy as np
    lib = load_library()
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0] if rows.ndim > 1 else (0 if rows.size == 0 else 1)
    rc = lib.rg_mpc_state_check(C.byref(make_cconfig(cfg)), rows.ctypes.data if rows.size else None, int(n), int(rows.nbytes),
                                _i32_array(dst), int(batch))
    if rc != 0:
        raise RgMpcError(rc, lib.rg_mpc_last_error(None).decode())


def make_cconfig(cfg):
    """MPCConfig -> CConfig."""
    c = CConfig()
    c.abi_version = ABI_VERSION
    for name, ctype in CConfig._fields_:
        if name == "abi_version":
            continue
        v = getattr(cfg, name)
        if isinstance(v, (tuple, list)) or hasattr(v, "__len__"):
            arr = getattr(c, name)
            if len(v) != len(arr):
                raise ValueError(f"config field {name}: expected {len(arr)} values, got {len(v)}")
            for k, x in enumerate(v):
                arr[k] = x
        else:
            setattr(c, name, v)
    return c


class MpcHandle(Handle):
    """Owns one rg_mpc_handle (one device, one stream)."""

    unit, error = "rg_mpc", RgMpcError

    def __init__(self, cfg, batch, device=0):
        lib = load_library()
        self.batch = int(batch)
        self.device = int(device)
        self._create(lib, C.byref(make_cconfig(cfg)), self.batch, self.device)

    def reset(self, idx=None, t0=0.0, stream=None):
        if idx is None:
            self._check(self._lib.rg_mpc_reset(self._h, None, self.batch, float(t0), stream))
        else:
            arr = (i32 * len(idx))(*[int(i) for i in idx])
            self._check(self._lib.rg_mpc_reset(self._h, arr, len(idx), float(t0), stream))

    def reset_at(self, t0s, idx=None, stream=None):
        n = len(t0s)
        t0 = (d * n)(*[float(x) for x in t0s])
        ia = None if idx is None else (i32 * n)(*[int(i) for i in idx])
        self._check(self._lib.rg_mpc_reset_at(self._h, ia, t0, n, stream))

    def reset_masked(self, mask_ptr, t0=0.0, stream=None):
        """rg_mpc_reset_masked: mask_ptr is a DEVICE int32 [batch]; nothing is staged and nothing waits."""
        self._check(self._lib.rg_mpc_reset_masked(self._h, mask_ptr, float(t0), stream))

    def set_command(self, cmd_ptr, stream=None):
        self._check(self._lib.rg_mpc_set_command(self._h, cmd_ptr, stream))

    def step(self, t, state_ptrs: CStatePtrs, out_ptrs: COutPtrs, stream=None):
        self._check(self._lib.rg_mpc_step(self._h, float(t), C.byref(state_ptrs), C.byref(out_ptrs), stream))

    def step_host(self, t, host_slab_ptr, dev_slab_ptr, slab_bytes, state_ptrs: CStatePtrs, out_ptrs: COutPtrs, action_host_ptr, stream=None):
        """rg_mpc_step_host: upload the pinned state slab, step, download the action slab and wait -- one call across the ABI."""
        self._check(self._lib.rg_mpc_step_host(self._h, float(t), host_slab_ptr, dev_slab_ptr, int(slab_bytes), C.byref(state_ptrs), C.byref(out_ptrs), action_host_ptr, stream))

    def set_gait(self, stance_ptr, duty_ptr, phase_ptr, init_state_ptr=None, stream=None):
        self._check(self._lib.rg_mpc_set_gait(self._h, stance_ptr, duty_ptr, phase_ptr, init_state_ptr, stream))

    def set_body(self, idx=None, n=0, mass=None, inertia=None, body_height=None, mu=None, hip=None, stream=None):
        """rg_mpc_set_body: host float64 arrays, component-major [k][n] (contiguous numpy), or None to keep a field.  All None
        with idx None and n 0 returns every robot to the config."""
        import numpy as np
        keep = []

        def ptr(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            keep.append(a)
            return a.ctypes.data
        ia = None if idx is None else (i32 * len(idx))(*[int(i) for i in idx])
        self._check(self._lib.rg_mpc_set_body(self._h, ia, int(n), ptr(mass), ptr(inertia), ptr(body_height), ptr(mu), ptr(hip), stream))

    def save_state(self, idx, n, rows_ptr, stream=None):
        """rg_mpc_save_state: n rows (idx None: every robot) into host memory at rows_ptr; waits."""
        self._check(self._lib.rg_mpc_save_state(self._h, _i32_array(idx), int(n), rows_ptr, stream))

    def load_state(self, idx, n, rows_ptr, clock_shift=None, stream=None):
        """rg_mpc_load_state: n host rows at rows_ptr into the robots idx (None: every robot); validated first; waits."""
        cs = None if clock_shift is None else (d * n)(*[float(x) for x in clock_shift])
        self._check(self._lib.rg_mpc_load_state(self._h, _i32_array(idx), int(n), rows_ptr, cs, stream))

    def copy_state(self, src, dst, stream=None):
        """rg_mpc_copy_state: robot src[k]'s state into robot dst[k], on the device, asynchronously on `stream`."""
        if len(src) != len(dst):
            raise ValueError("copy_state: src and dst must have the same length")
        self._check(self._lib.rg_mpc_copy_state(self._h, _i32_array(src), _i32_array(dst), len(src), stream))

    def hybrid_to_torque(self, action_ptr, q_ptr, qd_ptr, tau_ptr, stream=None, substeps=None):
        if substeps is None:
            self._check(self._lib.rg_mpc_hybrid_to_torque(self._h, action_ptr, q_ptr, qd_ptr, tau_ptr, stream))
        else:
            self._check(self._lib.rg_mpc_hybrid_to_torque_substeps(self._h, action_ptr, q_ptr, qd_ptr, tau_ptr, int(substeps), stream))

    def last_bin_counts(self, stream=None):
        out = (i32 * 5)()
        self._check(self._lib.rg_mpc_last_bin_counts(self._h, C.byref(out), stream))
        return list(out)

    def last_solver_stats(self, stream=None):
        s_, m_, n_, r_, f_ = C.c_int64(), i32(), i32(), i32(), i32()
        self._check(self._lib.rg_mpc_last_solver_stats(self._h, C.byref(s_), C.byref(m_), C.byref(n_), C.byref(r_), C.byref(f_), stream))
        return {"iters_sum": s_.value, "iters_max": m_.value, "qp_robots": n_.value, "retried_exact": r_.value,
                "failures": f_.value, "iters_mean": (s_.value / n_.value) if n_.value else 0.0}

    def audit_stats(self, reset=False, stream=None):
        """Audit lane: converged ADMM solves re-solved exactly on the side stream (cumulative; waits for the work in flight)."""
        a, o, f_, dr = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        mr, me = d(), d()
        self._check(self._lib.rg_mpc_audit_stats(self._h, C.byref(a), C.byref(o), C.byref(mr), C.byref(me), C.byref(f_), C.byref(dr),
                                                 1 if reset else 0, stream))
        return {"audited": a.value, "audit_over_tol": o.value, "audit_max_rel": mr.value, "audit_max_rel_elem": me.value,
                "audit_exact_failures": f_.value, "audit_dropped": dr.value}

    def last_direct_count(self, stream=None):
        """(robots the front kernel sent straight to the exact solver in the last step, ticks so far whose direct lists ran in
        a launch of their own next to the ADMM launch)."""
        n, k = i32(), C.c_int64()
        self._check(self._lib.rg_mpc_last_direct_count(self._h, C.byref(n), C.byref(k), stream))
        return n.value, k.value

    def profile_begin(self, max_steps):
        self._check(self._lib.rg_mpc_profile_begin(self._h, int(max_steps)))

    def last_iterations(self, batch, stream=None):
        """(iterations[B], stance_legs[B]) of the last step as numpy int32 arrays."""
        import numpy as np
        it = np.zeros(batch, dtype=np.int32)
        nc = np.zeros(batch, dtype=np.int32)
        self._check(self._lib.rg_mpc_last_iterations(self._h, it.ctypes.data_as(C.POINTER(i32)), nc.ctypes.data_as(C.POINTER(i32)), stream))
        return it, nc

    def profile_stride(self, stride):
        self._check(self._lib.rg_mpc_profile_stride(self._h, int(stride)))

    def profile_end(self, stream=None):
        ms = (C.c_float * 6)()
        rb = (i32 * 5)()
        n = self._lib.rg_mpc_profile_end(self._h, C.byref(ms), C.byref(rb), stream)
        if n < 0:
            self._check(n)
        return n, list(ms), list(rb)

    def debug_poison_lds(self, stream=None):
        self._check(self._lib.rg_mpc_debug_poison_lds(self._h, stream))

    def profile_window_names(self):
        return self._lib.rg_mpc_profile_window_names(self._h).decode().split(",")

    def plan(self):
        """rg_mpc_plan_description as a dict: what create chose (solver, horizon, batch, lanes, exact12, mu, schedule, audit, direct) and
        whether per-robot body rows are set (body: config / per_robot)."""
        return dict(kv.split("=", 1) for kv in self._lib.rg_mpc_plan_description(self._h).decode().split())

    def kernel_names(self):
        return self._lib.rg_mpc_kernel_names().decode().split(",")
