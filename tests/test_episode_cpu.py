"""The episode reset on the device (include/rg_episode.h) without a GPU: librg_mpc.so exports every rg_episode_* entry and
rg_mpc_reset_masked, the ctypes binding matches the header, create validates its three configurations (naming the field)
before it looks for a device, a host-only handle checks arguments and then returns NO_DEVICE; the numpy model of the target
stream has the properties the header states; and the kernels of rg_episode.hip cross-compile for gfx950 without scratch or
spills, within their LDS budget."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import episode_abi, goto_abi, mpc_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.gym import goto_path
from tests import episode_model as EM
from tests import kernel_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_episode.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")


def _header(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


# ---- ABI ------------------------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = episode_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_episode_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 8
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(episode_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None or name.endswith(("_version", "_size", "_rows")), name


def test_masked_controller_reset_is_exported_and_listed():
    lib = mpc_abi.load_library()
    assert hasattr(lib, "rg_mpc_reset_masked") and "rg_mpc_reset_masked" in mpc_abi.EXPORTS
    assert "rg_mpc_reset_masked" in _header(os.path.join(ROOT, "include", "rg_mpc.h"))
    assert lib.rg_mpc_reset_masked.argtypes == [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    assert lib.rg_mpc_abi_version() == 5
    assert lib.rg_mpc_reset_masked(None, None, 0.0, None) == -1   # a null handle is refused, not followed


def test_config_layout_matches_header():
    lib = episode_abi.load_library()
    assert lib.rg_episode_abi_version() == episode_abi.ABI_VERSION == 1
    assert lib.rg_episode_config_size() == C.sizeof(episode_abi.CConfig)
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", _header()))["rg_episode_config"]
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_EPISODE_\w+) (\d+)", _header())}
    sizes = {"int32_t": 4, "double": 8, "uint64_t": 8}
    want = []
    for t, n, dims in re.findall(r"\b(int32_t|double|uint64_t)\s+([a-z_0-9]+)((?:\[\w+\])*)\s*;", body):
        count = 1
        for dim in re.findall(r"\[(\w+)\]", dims):
            count *= int(dim) if dim.isdigit() else defs[dim]
        want.append((n, sizes[t] * count))
    got = episode_abi.CConfig._fields_
    assert [n for n, _ in want] == [n for n, _ in got]
    for (n, size), (_, tg) in zip(want, got):
        assert size == C.sizeof(tg), n
    assert sum(s for _, s in want) == C.sizeof(episode_abi.CConfig)   # no padding anywhere
    assert set(episode_abi.DEFAULTS) == {n for n, _ in got} - {"abi_version", "reserved0", "reserved1", "num_obstacles", "obstacles"}


def test_rows_limits_and_defaults_match_header_binding_and_planner():
    lib = episode_abi.load_library()
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_EPISODE_\w+) (\d+)", _header())}
    assert lib.rg_episode_state_rows() == defs["RG_EPISODE_ROWS"] == episode_abi.ROWS == EM.ROWS == 12
    for name in ("EPISODE", "PLAN_STATUS", "RETURN", "LENGTH", "LAST_RETURN", "LAST_LENGTH", "LAST_REASON", "NPTS", "NWAY", "KEY", "ENDED"):
        assert defs[f"RG_EPISODE_ROW_{name}"] == getattr(episode_abi, f"ROW_{name}") == getattr(EM, f"ROW_{name}"), name
    for k, name in enumerate(episode_abi.PLAN_STATUS):
        assert defs[f"RG_EPISODE_PLAN_{name.upper()}"] == k
    assert (defs["RG_EPISODE_MAX_WAYPOINTS"], defs["RG_EPISODE_MAX_OBSTACLES"], defs["RG_EPISODE_MAX_OSCILLATION"]) == \
        (episode_abi.MAX_WAYPOINTS, episode_abi.MAX_OBSTACLES, episode_abi.MAX_OSCILLATION) == (64, 16, 8)
    D = episode_abi.DEFAULTS
    assert (D["kp"], D["eta"], D["area_width"], D["grid"], D["robot_radius"], D["spacing"], D["oscillation_length"]) == \
        (goto_path.KP, goto_path.ETA, goto_path.AREA_WIDTH, goto_path.GRID, goto_path.ROBOT_RADIUS, goto_path.SPACING, goto_path.OSCILLATION_LENGTH)
    assert D["max_waypoints"] == 64
    cc = episode_abi.make_cconfig([(1, 1), (-1.5, 0.5)], seed=7)
    assert (cc.num_obstacles, cc.seed, cc.obstacles[1][0], cc.obstacles[1][1]) == (2, 7, -1.5, 0.5)
    with pytest.raises(TypeError):
        episode_abi.make_cconfig(reso=0.2)
    with pytest.raises(ValueError):
        episode_abi.make_cconfig([(0, 0)] * 17)
    # the other ABIs keep their versions and their configurations
    assert goto_abi.load_library().rg_goto_abi_version() == 1 and srb_abi.load_library().rg_srb_abi_version() == 1
    assert "rg_episode.h" in open(os.path.join(ROOT, "include", "rg_goto.h")).read()


@pytest.mark.parametrize("field,value,text", [
    ("kp", 0.0, "config.kp"), ("kp", NAN, "config.kp"), ("eta", -1.0, "config.eta"), ("eta", INF, "config.eta"), ("area_width", 0.0, "config.area_width"),
    ("grid", -0.5, "config.grid"), ("robot_radius", 0.0, "config.robot_radius"), ("spacing", 0.0, "config.spacing"), ("spacing", NAN, "config.spacing"),
    ("oscillation_length", 0, "config.oscillation_length"), ("oscillation_length", 9, "config.oscillation_length"),
    ("max_waypoints", 1, "config.max_waypoints"), ("max_waypoints", 65, "config.max_waypoints"), ("num_obstacles", -1, "config.num_obstacles"),
    ("num_obstacles", 17, "config.num_obstacles"), ("abi_version", 2, "config.abi_version"), ("reserved0", 1, "config.reserved0"),
    ("reserved1", 1, "config.reserved1"),
])
def test_create_rejects_a_bad_config_naming_the_field(field, value, text):
    cc = episode_abi.make_cconfig()
    setattr(cc, field, value)
    for device in (0, episode_abi.DEVICE_NONE):
        rc, msg = episode_abi.create_status(cc, device=device)
        assert rc == -1 and text in msg, (rc, msg)


def test_create_checks_obstacles_batch_and_the_other_two_configurations():
    cc = episode_abi.make_cconfig([(1.0, 1.0)])
    cc.obstacles[9][1] = NAN
    rc, msg = episode_abi.create_status(cc)
    assert rc == -1 and "config.obstacles[9][1]" in msg
    for batch in (0, -3, (1 << 24) + 1):
        rc, msg = episode_abi.create_status(batch=batch)
        assert rc == -1 and "batch" in msg
    cfg = MPCConfig.for_robot("ghost")
    sc = srb_abi.make_cconfig(cfg)
    sc.body_height = 0.0
    rc, msg = episode_abi.create_status(scfg=sc, mpc_cfg=cfg)
    assert rc == -1 and msg.startswith("srb config.body_height"), msg
    gc = goto_abi.make_cconfig(cfg, n_max=1)
    rc, msg = episode_abi.create_status(gcfg=gc, mpc_cfg=cfg)
    assert rc == -1 and msg.startswith("goto config.n_max"), msg
    lib = episode_abi.load_library()
    assert lib.rg_episode_create(None, None, None, 4, -1, C.byref(C.c_void_p())) == -1
    rc, msg = episode_abi.create_status()   # valid, host-only: a handle is made
    assert rc == 0, msg


def test_host_only_handle_checks_arguments_then_reports_no_device():
    h = episode_abi.EpisodeHandle(4, MPCConfig.for_robot("ghost"), episode_abi.DEVICE_NONE, obstacles=[(1, 1)], seed=3)
    lib = episode_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p, q = dummy.ctypes.data, dummy.ctypes.data + 8
    so = srb_abi.CObsPtrs(*([p] * 9))
    pp = goto_abi.CPathPtrs(*([p] * 5))
    last = lambda: lib.rg_episode_last_error(h._h).decode()
    good = [p, p, p, p, p, C.byref(so), C.byref(pp), p, p, q]
    assert lib.rg_episode_reset(h._h, *good, None) == -3 and "host-only" in last()
    good_no_targets = list(good)
    good_no_targets[1] = None
    assert lib.rg_episode_reset(h._h, *good_no_targets, None) == -3
    names = ("mask", None, "episode_state", "task_state", "sim_state", "sim_obs", "paths", "obs", "final_obs", "reset_mask_out")
    for k, name in enumerate(names):
        if name is None:
            continue
        a = list(good)
        a[k] = None
        assert lib.rg_episode_reset(h._h, *a, None) == -1 and f"reset: null {name}" in last(), last()
    a = list(good)
    a[5] = C.byref(srb_abi.CObsPtrs(p, p, None, p, p, p, p, p, p))
    assert lib.rg_episode_reset(h._h, *a, None) == -1 and "null sim_obs" in last()
    a = list(good)
    a[6] = C.byref(goto_abi.CPathPtrs(p, p, p, None, p))
    assert lib.rg_episode_reset(h._h, *a, None) == -1 and "null paths" in last()
    a = list(good)
    a[9] = p
    assert lib.rg_episode_reset(h._h, *a, None) == -1 and "alias" in last()
    assert lib.rg_episode_accumulate(h._h, p, p, p, None) == -3
    for k, name in enumerate(("episode_state", "reward", "done")):
        a = [p, p, p]
        a[k] = None
        assert lib.rg_episode_accumulate(h._h, *a, None) == -1 and f"accumulate: null {name}" in last(), last()
    assert lib.rg_episode_reset(None, *good, None) == -1 and "null handle" in lib.rg_episode_last_error(None).decode()
    with pytest.raises(episode_abi.RgEpisodeError) as e:
        h.accumulate(p, p, p)
    assert e.value.status == -3
    h.close()


# ---- the target stream ------------------------------------------------------------------------------------------------

def _stream(seed, keys, episodes):
    return np.array([[EM.draw_target(seed, k, e) for e in episodes] for k in keys])


def test_target_stream_lies_on_the_grid_outside_the_inner_square():
    t = _stream(0, range(400), range(10)).reshape(-1, 2)
    assert np.all(np.abs(t) <= 2.5)
    assert np.array_equal(np.rint(t * 100.0) / 100.0, t)                       # on the 0.01 grid
    inner = (np.abs(t) < 1.0) & (t != 0.0)
    assert not inner.any()                                                     # nothing in (-1, 1) but an exact 0
    assert not np.any((t[:, 0] == 0.0) & (t[:, 1] == 0.0))
    assert not np.any(np.signbit(t) & (t == 0.0))                              # no -0.0
    assert len({tuple(r) for r in t}) > 0.9 * len(t) * 0.5                     # not a stuck stream
    for axis in range(2):                                                      # both signs, both axes, the pushed values too
        assert (t[:, axis] >= 1.0).any() and (t[:, axis] <= -1.0).any() and (np.abs(t[:, axis]) == 1.0).any()


def test_a_robots_stream_depends_on_its_key_and_episode_only():
    a = _stream(5, range(64), range(4))
    b = _stream(5, [63, 7, 0], range(4))          # another batch, another order: the same robots draw the same targets
    assert np.array_equal(b, a[[63, 7, 0]])
    assert np.array_equal(_stream(5, [7], [3, 0])[0], a[7][[3, 0]])            # no state: any episode, in any order
    assert not np.array_equal(_stream(6, range(64), range(4)), a)              # the seed matters
    assert len({tuple(r) for r in a[:, 0]}) > 32                               # robots differ
    # the redraw: a uniform that rounds to 0 on both axes is never returned
    assert EM.coordinate(0.5) == 0.0 and EM.coordinate(0.5 + 1e-4) == 0.0 and EM.coordinate(0.5 + 2e-3) == 1.0
    assert EM.coordinate(0.0) == -2.5 and EM.coordinate(1.0 - 2.0 ** -53) == 2.5 and EM.coordinate(0.5 - 2e-3) == -1.0


def test_forced_planner_is_the_planner_and_flags_only_close_calls():
    rng = np.random.default_rng(1)
    flagged = 0
    for _ in range(60):
        t = goto_path.random_target(rng)
        for obstacles in ((), ((1, 1), (-1.5, 0.5), (0.5, -1.5), (2, 0))):
            pts, flags = EM.plan_path_forced(t, obstacles)
            assert np.array_equal(pts, goto_path.plan_path(t, obstacles))
            flagged += bool(flags)
    assert flagged < 0.5 * 120
    # (2, 1.5): the cell (1.5, 1.5) lies exactly one cell from the target -- the stop test is a close call there
    pts, flags = EM.plan_path_forced((2.0, 1.5))
    plain, is_flagged, variants = EM.plan_variants((2.0, 1.5))
    assert is_flagged == bool(flags) and (len(variants) >= 2 if is_flagged else variants == [plain])


# ---- resources of rg_episode.hip --------------------------------------------------------------------------------------

KERNELS = {"rg_episode_plan_kernel", "rg_episode_reset_kernel", "rg_episode_accumulate_kernel", "rg_episode_ctl_reset_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_episode.hip")


def test_every_episode_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_episode_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


# plan kernel: way points x / y / cumulative length (3 * 64 float64), obstacles x / y (2 * 16 float64), the last cells of the
# descent (2 * 8 int32).  reset kernel: the task's five arrays of RG_GOTO_MAX_VISIBLE float64.
LDS_BUDGET = {"rg_episode_plan_kernel": 3 * 64 * 8 + 2 * 16 * 8 + 2 * 8 * 4, "rg_episode_reset_kernel": 5 * 128 * 8,
              "rg_episode_accumulate_kernel": 0, "rg_episode_ctl_reset_kernel": 0}


def test_lds_is_within_the_budget(remarks):
    for name, budget in LDS_BUDGET.items():
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= budget, (name, remarks[name])


# What the device-only compile reports today (upper bounds; occupancy a lower bound).  The reset kernel carries the
# simulator's reset with its leg IK: like rg_srb_reset_kernel it fills the architectural VGPRs and runs one wave per SIMD.
REGISTERS = {"rg_episode_plan_kernel": dict(vgprs=52, agprs=0, occupancy=8), "rg_episode_reset_kernel": dict(vgprs=256, agprs=3, occupancy=1),
             "rg_episode_accumulate_kernel": dict(vgprs=13, agprs=0, occupancy=8), "rg_episode_ctl_reset_kernel": dict(vgprs=32, agprs=0, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_has_no_inline_assembly_no_atomics_and_contraction_off():
    src = open(os.path.join(SRC, "rg_episode.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    assert code.index("#pragma clang fp contract(off)") < code.index("__global__")
    for inc in ("rg_mpc_dev.h", "rg_srb_dev.inc", "rg_goto_dev.inc", "rg_reset_body.inc"):
        assert code.index("#pragma clang fp contract(off)") < code.index(f'#include "{inc}"'), inc
    assert code.count("__launch_bounds__(kWave)") == 2   # one wave per workgroup: __syncthreads and every branch are wave-uniform
    for inc in ("rg_srb_dev.inc", "rg_goto_dev.inc", "rg_reset_body.inc"):   # the code shared with the old kernels
        shared = open(os.path.join(SRC, inc)).read()
        assert "asm" not in re.sub(r"//.*", "", shared) and "atomic" not in shared.lower(), inc
    assert "atomic" not in open(os.path.join(SRC, "rg_goto.hip")).read().lower()
    kernel_checks.assert_built_into_both("rg_episode.hip")
