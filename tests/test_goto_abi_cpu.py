"""The go-to-target task's C-ABI (include/rg_goto.h) without a GPU: librg_mpc.so exports every rg_goto_* entry the header
declares, the ctypes binding matches the header, create validates the configuration (naming the field) before it looks for
a device, and -- on a host-only handle (RG_GOTO_DEVICE_NONE) -- set_path, pre_step, post_step and observe reject bad sizes
and null pointers the same way."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.core import goto_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.gym import goto_path
from tests import goto_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_goto.h")
NAN, INF = float("nan"), float("inf")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_library_exports_every_declared_entry():
    lib = goto_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_goto_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 10
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(goto_abi.EXPORTS) == declared


def _struct_fields(name):
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", _header()))[name]
    return re.findall(r"\b(int32_t|double|float)\s+\*?([a-z_0-9]+)(?:\[(\d+)\])?\s*;", body)


def test_config_layout_matches_header():
    lib = goto_abi.load_library()
    assert lib.rg_goto_abi_version() == goto_abi.ABI_VERSION == 1
    assert lib.rg_goto_config_size() == C.sizeof(goto_abi.CConfig)
    ctypes_of = {"int32_t": C.c_int32, "double": C.c_double}
    want = [(n, ctypes_of[t] * int(k) if k else ctypes_of[t]) for t, n, k in _struct_fields("rg_goto_config")]
    got = goto_abi.CConfig._fields_
    assert [n for n, _ in want] == [n for n, _ in got]
    for (n, tw), (_, tg) in zip(want, got):
        assert C.sizeof(tw) == C.sizeof(tg), n
    assert [n for _, n, _ in _struct_fields("rg_goto_path_ptrs")] == [n for n, _ in goto_abi.CPathPtrs._fields_] == list(goto_abi.PATH_FIELDS)
    assert set(goto_abi.DEFAULTS) == {n for n, _ in got} - {"abi_version", "reserved0", "reserved1"}


def test_state_rows_and_limits_match_header_binding_and_model():
    lib = goto_abi.load_library()
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_GOTO_\w+) (\d+)", _header())}
    assert lib.rg_goto_state_rows() == defs["RG_GOTO_STATE_ROWS"] == goto_abi.STATE_ROWS == len(goto_model.new_state()) == 50
    for name in ("POS", "PREV", "POT", "PROGRESS", "NEXT_CP", "PATH_DONE", "ENV_STEPS", "DONE", "REASON", "OVERFLOW", "VISIBLE", "CHAIN",
                 "LATCHED", "TRACK_ERR", "OBS"):
        assert defs[f"RG_GOTO_ROW_{name}"] == getattr(goto_abi, f"ROW_{name}"), name
    assert goto_abi.ROW_OBS + 2 * goto_abi.MAX_CAM_PTS == goto_abi.STATE_ROWS
    assert (defs["RG_GOTO_MAX_CAM_PTS"], defs["RG_GOTO_MAX_VISIBLE"], defs["RG_GOTO_MAX_PATH"], defs["RG_GOTO_HDR_ROWS"]) == \
        (goto_abi.MAX_CAM_PTS, goto_abi.MAX_VISIBLE, goto_abi.MAX_PATH, goto_abi.HDR_ROWS)
    for k, name in enumerate(goto_abi.REASONS):
        assert defs[f"RG_GOTO_REASON_{name.upper()}"] == k == goto_model.REASON[name]


def test_config_carries_the_controller_offsets():
    for robot in ("ghost", "k3lso"):
        cfg = MPCConfig.for_robot(robot)
        cc = goto_abi.make_cconfig(cfg)
        assert list(cc.cmd_offset) == [cfg.vx_offset, cfg.vy_offset, cfg.wz_offset]
        assert (cc.num_cam_pts, cc.n_max, cc.max_visible, cc.substeps, cc.dt_sim) == (8, 1024, 128, 10, 0.001)
    with pytest.raises(TypeError):
        goto_abi.make_cconfig(None, window=0.2)
    with pytest.raises(ValueError):
        goto_abi.make_cconfig(None, action_low=(0.0,))


@pytest.mark.parametrize("field,value,text", [
    ("window_height", 0.0, "config.window_height"), ("window_height", NAN, "config.window_height"), ("window_top_width", -0.1, "config.window_top_width"),
    ("window_bottom_width", 0.0, "config.window_bottom_width"), ("window_distance", INF, "config.window_distance"),
    ("max_track_err", 0.0, "config.max_track_err"), ("progress_window", -1.0, "config.progress_window"), ("progress_limit", NAN, "config.progress_limit"),
    ("target_radius", 0.0, "config.target_radius"), ("time_penalty", INF, "config.time_penalty"), ("checkpoint_reward_total", NAN, "config.checkpoint_reward_total"),
    ("max_time", 0.0, "config.max_time"), ("continuity_break", 0.0, "config.continuity_break"), ("action_low", (NAN, 0.0), "config.action_low[0]"),
    ("action_high", (0.35, INF), "config.action_high[1]"), ("action_low", (0.5, -0.4), "config.action_low[0]"), ("cmd_offset", (0.0, 0.0, NAN), "config.cmd_offset[2]"),
    ("dt_sim", 0.0, "config.dt_sim"), ("substeps", 0, "config.substeps"), ("substeps", 1025, "config.substeps"),
    ("num_cam_pts", 0, "config.num_cam_pts"), ("num_cam_pts", 17, "config.num_cam_pts"), ("num_checkpoints", 0, "config.num_checkpoints"),
    ("n_max", 1, "config.n_max"), ("n_max", 65537, "config.n_max"), ("max_visible", 1, "config.max_visible"), ("max_visible", 129, "config.max_visible"),
])
def test_create_rejects_a_bad_config_naming_the_field(field, value, text):
    for device in (0, goto_abi.DEVICE_NONE):
        rc, msg = goto_abi.create_status(None, 8, device, **{field: value})
        assert rc == -1 and text in msg, (rc, msg)


def test_create_rejects_bad_batch_version_and_reserved():
    for batch in (0, -3, (1 << 24) + 1):
        rc, msg = goto_abi.create_status(None, batch)
        assert rc == -1 and "batch" in msg
    for name, value in (("abi_version", 99), ("reserved0", 1), ("reserved1", 1)):
        cc = goto_abi.make_cconfig()
        setattr(cc, name, value)
        rc, msg = goto_abi.create_status(cc, 4)
        assert rc == -1 and name in msg
    lib = goto_abi.load_library()
    assert lib.rg_goto_create(None, 4, 0, C.byref(C.c_void_p())) == -1


def test_a_good_config_reaches_the_device_probe():
    """Without a GPU a valid configuration is NO_DEVICE (validation passed); with one, create succeeds."""
    for task in ({}, dict(num_cam_pts=5, n_max=64, max_visible=16)):
        rc, msg = goto_abi.create_status(MPCConfig.for_robot("ghost"), 8, **task)
        if torch.cuda.is_available():
            assert rc == 0, msg
        else:
            assert rc == -3 and "HIP device" in msg
    if not torch.cuda.is_available():
        with pytest.raises(goto_abi.RgGotoError):
            goto_abi.GotoHandle(4)
        with pytest.raises(RuntimeError):
            from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
            BatchedGoEnv(4)


# ---- argument checks of the per-call entries, on a host-only handle ----------------------------------------------

B, N_MAX = 4, 256


@pytest.fixture()
def host():
    h = goto_abi.GotoHandle(B, None, goto_abi.DEVICE_NONE, n_max=N_MAX)
    paths = [goto_path.build_path(goto_path.plan_path(t)) for t in ((2.0, 0.0), (0.0, -2.0), (1.0, 1.0), (-1.5, 1.0))]
    rows = goto_path.pack_paths(paths, N_MAX)
    dummy = np.zeros(8)     # stands for device memory: a host-only handle never follows these pointers
    ptrs = goto_abi.CPathPtrs(*([dummy.ctypes.data] * 5))
    yield h, rows, ptrs, dummy.ctypes.data
    h.close()


def _err(call):
    with pytest.raises(goto_abi.RgGotoError) as e:
        call()
    return e.value.status, str(e.value)


def test_valid_calls_on_a_host_only_handle_stop_at_the_device(host):
    h, rows, ptrs, p = host
    assert _err(lambda: h.set_path(ptrs, p, None, **rows))[0] == -3
    sub = {k: (v[:, [2, 0]] if k == "target" else v[[2, 0]]) for k, v in rows.items()}
    assert _err(lambda: h.set_path(ptrs, p, [2, 0], **sub))[0] == -3
    assert _err(lambda: h.pre_step(p, p, ptrs, p, p))[0] == -3
    assert _err(lambda: h.post_step(p, p, ptrs, p, p, p))[0] == -3
    assert _err(lambda: h.observe(p, p, ptrs, p))[0] == -3


def test_set_path_rejects_bad_sizes_and_values(host):
    h, rows, ptrs, p = host

    def with_(**change):
        r = {k: v.copy() for k, v in rows.items()}
        for k, (where, value) in change.items():
            r[k][where] = value
        return r
    cases = [(with_(npts=(1, N_MAX + 1)), "npts 257 above n_max 256"), (with_(npts=(3, 1)), "npts 1 below 2"), (with_(npts=(0, 0)), "npts 0 below 2"),
             (with_(length=(2, 0.0)), "length"), (with_(length=(2, NAN)), "length"), (with_(target=((1, 3), INF)), "target"),
             (with_(x=((1, 5), NAN)), "x, y and s"), (with_(s=((0, 7), INF)), "x, y and s"),
             (with_(first_same_x=((2, 4), 5)), "first_same_x"), (with_(first_same_x=((2, 4), -1)), "first_same_x")]
    for r, text in cases:
        status, msg = _err(lambda: h.set_path(ptrs, p, None, **r))
        assert status == -1 and text in msg, msg
    status, msg = _err(lambda: h.set_path(ptrs, p, None, **with_(length=(2, 0.0))))
    assert "entry 2 (robot 2)" in msg
    one = {k: (v[:, :1] if k == "target" else v[:1]) for k, v in rows.items()}
    two = {k: (v[:, :2] if k == "target" else v[:2]) for k, v in rows.items()}
    assert "robot out of range" in _err(lambda: h.set_path(ptrs, p, [B], **one))[1]
    assert "robot out of range" in _err(lambda: h.set_path(ptrs, p, [-1], **one))[1]
    assert "given twice" in _err(lambda: h.set_path(ptrs, p, [1, 1], **two))[1]
    lib = goto_abi.load_library()
    args = [rows[k].ctypes.data for k in ("npts", "length", "target", "x", "y", "s", "first_same_x")]
    assert lib.rg_goto_set_path(h._h, None, B - 1, *args, C.byref(ptrs), p, None) == -1      # n must be the batch without an index list
    assert "n must be the batch" in lib.rg_goto_last_error(h._h).decode()
    with pytest.raises(ValueError):
        h.set_path(ptrs, p, None, **{**rows, "x": rows["x"][:, :100]})


def test_null_pointers_are_named(host):
    h, rows, ptrs, p = host
    lib = goto_abi.load_library()
    args = [rows[k].ctypes.data for k in ("npts", "length", "target", "x", "y", "s", "first_same_x")]
    last = lambda: lib.rg_goto_last_error(h._h).decode()
    for k in range(7):
        a = list(args)
        a[k] = None
        assert lib.rg_goto_set_path(h._h, None, B, *a, C.byref(ptrs), p, None) == -1 and "null host array" in last()
    assert lib.rg_goto_set_path(h._h, None, B, *args, None, p, None) == -1 and "null paths" in last()
    assert lib.rg_goto_set_path(h._h, None, B, *args, C.byref(ptrs), None, None) == -1 and "null task_state" in last()
    holed = goto_abi.CPathPtrs(p, p, None, p, p)
    assert lib.rg_goto_post_step(h._h, p, p, C.byref(holed), p, p, p, None) == -1 and "null paths" in last()
    for k, name in enumerate(("task_state", "sim_state", "paths", "action", "cmd_out")):
        a = [p, p, C.byref(ptrs), p, p]
        a[k] = None
        assert lib.rg_goto_pre_step(h._h, *a, None) == -1 and f"pre_step: null {name}" in last(), last()
    for k, name in enumerate(("task_state", "sim_state", "paths", "obs", "reward or done", "reward or done")):
        a = [p, p, C.byref(ptrs), p, p, p]
        a[k] = None
        assert lib.rg_goto_post_step(h._h, *a, None) == -1 and f"post_step: null {name}" in last(), last()
    for k, name in enumerate(("task_state", "sim_state", "paths", "obs")):
        a = [p, p, C.byref(ptrs), p]
        a[k] = None
        assert lib.rg_goto_observe(h._h, *a, None) == -1 and f"observe: null {name}" in last(), last()
    for call in (lambda: lib.rg_goto_pre_step(None, p, p, C.byref(ptrs), p, p, None), lambda: lib.rg_goto_post_step(None, p, p, C.byref(ptrs), p, p, p, None),
                 lambda: lib.rg_goto_set_path(None, None, B, *args, C.byref(ptrs), p, None)):
        assert call() == -1 and "null handle" in lib.rg_goto_last_error(None).decode()
