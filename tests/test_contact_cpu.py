"""Measured foot contact (include/rg_srb_contact.h) without a GPU: known answers of the rule on the model
(tests/contact_model.py), its equivalence with the schedule tick while nothing touches, the ABI of rg_srb_step_contact
(header, binding, library; refusals that name the argument; validation before any device probe), the resources of
robot_gym_amd/csrc/rg_srb_contact.hip from one device-only compile, and the CPU reference closed loop with measured
contact: nobody falls, every robot walks, the EARLY_CONTACT branch of the controller is entered, and the bands of
tests/contact_fixtures.py are twice what this run produces."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.core import srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import contact_fixtures as CF
from tests import contact_model as CM
from tests import kernel_checks
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import terrain_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")


# ---- known answers ---------------------------------------------------------------------------------------------------

def _standing(B, ground=None):
    """B ghost robots at p.z = 0.5 with identity rotation over an all-zero grid, all four feet planted."""
    cfg = MPCConfig.for_robot("ghost")
    m = CM.ContactSRBModel(B, cfg, ground or TM.Grid(np.zeros((5, 4)), 0.5, (-1.0, -1.0)))
    m.reset(height=np.full(B, 0.5))
    assert (m.state[M.ROW_P + 2] == 0.5).all() and (m.state[M.ROW_QUAT + 3] == 1.0).all() and (m.state[M.ROW_STANCE:M.ROW_STANCE + 4] == 1).all()
    return cfg, m


def _targets(cfg, B, z):
    ft = np.tile(np.asarray(cfg.hip, dtype=np.float32).reshape(1, 12), (B, 1))
    ft[:, 2::3] = z
    return ft


def test_a_swung_foot_at_the_ground_touches_and_the_next_float_above_it_does_not():
    cfg, m = _standing(2)
    above = np.nextafter(np.float32(-0.5), np.float32(0.0))
    assert above > -0.5
    ft = _targets(cfg, 2, np.float32(-0.5))
    ft[1, 2::3] = above
    ls = np.zeros((2, 4), np.int32)                       # every leg SWING
    before = m.state.copy()
    m.step_contact(np.zeros((2, 12), np.float32), ft, ls)
    st = m.state
    assert (m.touch[:, 0] == 1).all() and (st[M.ROW_STANCE:M.ROW_STANCE + 4, 0] == 1).all()        # c.z == 0 <= 0: touches
    assert (st[M.ROW_FOOT + 2::3, 0][:4] == 0.0).all()
    assert (m.touch[:, 1] == 0).all() and (st[M.ROW_STANCE:M.ROW_STANCE + 4, 1] == 0).all()        # one float32 higher: in the air
    assert (st[M.ROW_FOOT + 2::3, 1][:4] == 0.5 + np.float64(above)).all() and (st[M.ROW_FOOT + 2::3, 1][:4] > 0).all()
    assert (m.obs["contact"][:, 0] == 1).all() and (m.obs["contact"][:, 1] == 0).all()             # obs.contact is the measurement
    # the feet went to the target in x and y
    hip = np.asarray(cfg.hip).reshape(4, 3)
    for l in range(4):
        assert (st[M.ROW_FOOT + 3 * l, :] == before[M.ROW_P, :] + np.float64(np.float32(hip[l, 0]))).all()


def test_lose_contact_is_swung_and_early_contact_is_not():
    cfg, m = _standing(1)
    ft = _targets(cfg, 1, np.float32(-0.4))               # 10 cm above the ground
    ls = np.array([[CM.LOSE_CONTACT, CM.EARLY_CONTACT, CM.STANCE, CM.SWING]], np.int32)
    m.step_contact(np.zeros((1, 12), np.float32), ft, ls)
    st = m.state
    assert st[M.ROW_STANCE:M.ROW_STANCE + 4, 0].tolist() == [0.0, 1.0, 1.0, 0.0]
    fz = st[M.ROW_FOOT + 2::3, 0][:4]
    assert fz[0] == fz[3] == 0.5 + np.float64(np.float32(-0.4)) and fz[1] == fz[2] == 0.0
    assert (m.touch == 0).all()
    # the two feet in the air: an EARLY_CONTACT leg lands where it is, like a STANCE leg, and touch stays 0 (it is no touch-down
    # of a swung foot); a LOSE_CONTACT leg whose target is under the ground touches
    ft2 = _targets(cfg, 1, np.float32(-0.6))
    fx = st[M.ROW_FOOT + 9, 0]
    m.step_contact(np.zeros((1, 12), np.float32), ft2, np.array([[CM.LOSE_CONTACT, CM.STANCE, CM.STANCE, CM.EARLY_CONTACT]], np.int32))
    assert m.state[M.ROW_STANCE:M.ROW_STANCE + 4, 0].tolist() == [1.0, 1.0, 1.0, 1.0]
    assert m.touch[:, 0].tolist() == [1, 0, 0, 0]
    assert (m.state[M.ROW_FOOT + 2::3, 0][:4] == 0.0).all() and m.state[M.ROW_FOOT + 9, 0] == fx      # leg 3 landed where it was


def test_force_goes_through_feet_on_the_ground_only():
    cfg, m = _standing(3)
    up = np.zeros((3, 12), np.float32)
    up[:, 2::3] = -np.float32(cfg.mass * cfg.gravity / 4.0) * 2        # grf is negated: the ground pushes up with twice the weight
    ft = _targets(cfg, 3, np.float32(-0.4))
    ft[1, 2::3] = np.float32(-0.55)                                    # robot 1: every target under the ground
    ls = np.zeros((3, 4), np.int32)
    ls[2] = CM.STANCE                                                  # robot 2: planted
    m.step_contact(up, ft, ls)
    vz = m.state[M.ROW_V + 2]
    g = cfg.gravity
    assert abs(vz[0] - (-g * 0.01)) < 1e-12                            # in the air: no force in spite of the grf, free fall
    assert (m.touch[:, 0] == 0).all()
    assert abs(vz[1] - (g * 0.01)) < 1e-9 and (m.touch[:, 1] == 1).all()          # touching: the force acts
    assert abs(vz[2] - vz[1]) < 1e-12 and (m.touch[:, 2] == 0).all()              # as on planted feet


def test_the_plane_is_the_literal_zero_and_a_frozen_robot_touches_nothing():
    cfg, m = _standing(2, TM.Flat())
    m.state[M.ROW_STATUS, 1] = 1.0
    ft = _targets(cfg, 2, np.float32(-0.7))
    before = m.state.copy()
    m.step_contact(np.zeros((2, 12), np.float32), ft, np.zeros((2, 4), np.int32))
    assert (m.touch[:, 0] == 1).all() and (m.touch[:, 1] == 0).all()
    assert (m.state[M.ROW_FOOT + 2::3, 0][:4] == 0.0).all() and not np.signbit(m.state[M.ROW_FOOT + 2::3, 0][:4]).any()
    assert m.state[:, 1].tobytes() == before[:, 1].tobytes()


# ---- equivalence with the schedule tick ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def equivalence():
    return {robot: CF.equivalence_recording(MPCConfig.for_robot(robot), 67, 40, 350 + n, CF.stream_ground("random", 67))
            for n, robot in enumerate(F.ROBOTS)}


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_step_contact_is_step_bit_for_bit_while_nothing_touches(robot, equivalence):
    rec = equivalence[robot]
    assert rec.lowest > 0.0 and np.isfinite(rec.lowest)                # the stream is the one described: no swung target at the ground
    swings = sum(int((d == 0).sum()) for _, _, d, _ in rec.inputs)
    assert swings > 100 and not rec.model.fallen().any()
    s = rec.s
    m = CM.ContactSRBModel(rec.B, rec.cfg, rec.ground)
    m.set_body(idx=rec.body_idx, mass=s["mass"][rec.body_idx], inertia=s["inertia"][:, rec.body_idx])
    m.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
    assert m.state.tobytes() == rec.states[0].tobytes()
    for k, (g, ft, d, ext) in enumerate(rec.inputs):
        m.step_contact(g, ft, d, ext)
        assert m.state.tobytes() == rec.states[k + 1].tobytes(), k
        for name, want in rec.obs[k + 1].items():
            assert m.obs[name].tobytes() == want.tobytes(), (k, name)
        assert (m.touch == 0).all()


# ---- the ABI -----------------------------------------------------------------------------------------------------------

def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_header_binding_and_library_agree_on_the_entry():
    lib = srb_abi.load_library()
    hdr = _header("rg_srb_contact.h")
    declared = sorted(set(re.findall(r"\b(rg_srb_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(srb_abi.CONTACT_EXPORTS) == ["rg_srb_step_contact"]
    assert hasattr(lib, "rg_srb_step_contact")
    args = re.search(r"int rg_srb_step_contact\(([^)]*)\)", hdr).group(1)
    names = [a.strip().split()[-1].lstrip("*") for a in args.split(",")]
    assert names == ["h", "state", "grf", "foot_target", "leg_state", "ext", "obs", "touch", "stream"]
    assert len(lib.rg_srb_step_contact.argtypes) == len(names)
    whole = open(os.path.join(ROOT, "include", "rg_srb.h")).read()
    assert whole.index('#include "rg_srb_terrain.h"') < whole.index('#include "rg_srb_contact.h"')
    # nothing else of the ABI moved
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_SRB_\w+) (\d+)", _header("rg_srb.h"))}
    assert defs["RG_SRB_ABI_VERSION"] == 1 and defs["RG_SRB_STATE_ROWS"] == 43
    from robot_gym_amd.core import mpc_abi
    mpc = _header("rg_mpc.h")
    for name, value in (("SWING", CM.SWING), ("STANCE", CM.STANCE), ("EARLY_CONTACT", CM.EARLY_CONTACT), ("LOSE_CONTACT", CM.LOSE_CONTACT)):
        assert re.search(rf"RG_LEG_{name}\s*=\s*{value}\b", mpc), name
        assert getattr(srb_abi, f"LEG_{name}") == value
    assert mpc_abi.LIB_PATH


def test_a_null_handle_is_refused_by_name_without_a_device():
    lib = srb_abi.load_library()
    obs = srb_abi.CObsPtrs()
    assert lib.rg_srb_step_contact(None, None, None, None, None, None, C.byref(obs), None, None) == -1
    assert b"step_contact: null handle" in lib.rg_srb_last_error(None)


CPU = torch.device("cpu")


def _good(B=5):
    return dict(state=torch.zeros(43, B, dtype=torch.float64), grf=torch.zeros(B, 12), foot_target=torch.zeros(B, 12),
                leg_state=torch.zeros(B, 4, dtype=torch.int32), ext=torch.zeros(6, B, dtype=torch.float64), touch=torch.zeros(4, B, dtype=torch.int32))


def test_the_binding_accepts_what_the_library_takes():
    a = _good()
    ptrs = srb_abi.step_contact_ptrs(5, CPU, **a)
    assert ptrs == tuple(a[k].data_ptr() for k in ("state", "grf", "foot_target", "leg_state", "ext", "touch"))
    a["ext"] = a["touch"] = None
    assert srb_abi.step_contact_ptrs(5, CPU, **a)[4:] == (None, None)                    # the two optional arguments: NULL


BAD_ARGS = [(name, how) for name in ("state", "grf", "foot_target", "leg_state", "ext", "touch") for how in ("dtype", "shape", "batch", "strided", "device", "type")]
BAD_ARGS += [(name, "none") for name in ("state", "grf", "foot_target", "leg_state")]


@pytest.mark.parametrize("name,how", BAD_ARGS)
def test_the_binding_refuses_a_bad_tensor_naming_the_argument(name, how, monkeypatch):
    # validation comes before any device probe: nothing here may ask torch for a device, and the library is never reached
    for probe in ("is_available", "current_device", "current_stream", "device_count"):
        monkeypatch.setattr(torch.cuda, probe, lambda *a, **k: pytest.fail(f"torch.cuda.{probe} called before validation"))
    a = _good()
    t = a[name]
    if how == "dtype":
        a[name] = t.to(torch.float16 if t.dtype != torch.float16 else torch.float32)
    elif how == "shape":
        a[name] = t.t().contiguous()
    elif how == "batch":
        a[name] = _good(6)[name]
    elif how == "strided":
        big = torch.zeros(t.shape[0], 2 * t.shape[1], dtype=t.dtype)
        a[name] = big[:, ::2]
        assert a[name].shape == t.shape and not a[name].is_contiguous()
    elif how == "device":
        a[name] = t.to("meta")                         # right in every other respect, on another device
    elif how == "type":
        a[name] = t.numpy()
    elif how == "none":
        a[name] = None
    with pytest.raises(ValueError, match=rf"step_contact: {name}\b"):
        srb_abi.step_contact_ptrs(5, CPU, **a)


def test_the_simulator_refuses_an_unknown_contact_mode_before_it_looks_for_a_device(monkeypatch):
    from robot_gym_amd.sim import BatchedSRBSim
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("device probe before validation"))
    with pytest.raises(ValueError, match="contact"):
        BatchedSRBSim(4, contact="late")


# ---- resources of rg_srb_contact.hip ---------------------------------------------------------------------------------------

KERNELS = {"rg_srb_contact_step_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_srb_contact.hip")


def test_the_contact_kernel_is_reported_and_uses_no_scratch_and_no_lds(remarks):
    assert set(remarks) == KERNELS
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds): where the terrain step kernel is (256 + 40), a few accumulation
# registers below it -- the ground lookups sit outside the sub-step loop.
REGISTERS = {"rg_srb_contact_step_kernel": dict(vgprs=256, agprs=34)}


def test_contact_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_contact_source_keeps_contraction_off_and_both_library_targets_compile_it():
    src = open(os.path.join(SRC, "rg_srb_contact.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_mpc_dev.h"') < src.index("__global__")
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_srb_ground.inc"')
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_srb_tick.inc"') < src.index("__global__")
    tick = open(os.path.join(SRC, "rg_srb_tick.inc")).read()
    for text in (src, tick):
        assert "asm" not in re.sub(r"//.*", "", text) and "atomic" not in text and "__shared__" not in text
    assert "fma(" not in open(os.path.join(SRC, "rg_srb_ground.inc")).read() and "fma(" not in tick
    kernel_checks.assert_built_into_both("rg_srb_contact.hip")


# ---- the CPU closed loop with measured contact -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rough():
    out = {}
    for robot in F.ROBOTS:
        cmd, hs = F.cases(robot)
        traj, loop, walked = CF.run_cpu(robot, CF.reference_ground(len(hs)))
        out[robot] = (cmd, traj, loop, walked)
    return out


def test_with_measured_contact_nobody_falls_every_robot_walks_and_early_contact_is_entered(rough):
    for robot, (cmd, traj, loop, walked) in rough.items():
        assert not loop.model.fallen().any(), robot
        assert (loop.model.state[M.ROW_STEPS] == 10 * F.TICKS).all()
        assert all(np.isfinite(v).all() for v in traj.values())
        assert (walked >= CF.WALKED * CF.TF.commanded_distance(cmd)).all(), robot
        entered = int((loop.early > 0).sum())
        print(robot, "robots in EARLY_CONTACT", entered, "leg-ticks", int(loop.early.sum()), "touch-downs", int(loop.touched.sum()),
              "LOSE_CONTACT leg-ticks", int(loop.lose.sum()))
        assert 2 * entered >= loop.B, (robot, entered)                     # a condition on the inputs: the branch runs in closed loop
        assert entered == CF.EARLY_ROBOTS[robot], (robot, entered)         # what the GPU test measures itself against
        assert int(loop.lose.sum()) == 0                                   # a commanded-stance foot is always planted
        assert int(loop.touched.sum()) >= int((loop.early > 0).sum())
        worst = F.worst_in_window(F.window(traj, F.TICKS - F.WINDOW), cmd, loop.cfg.body_height)
        print(robot, {k: float(v.max()) for k, v in worst.items()})
        assert not F.outside_bands(worst, CF.BANDS), (robot, F.outside_bands(worst, CF.BANDS))
        # a stance foot stands on the ground, exactly
        m, st = loop.model, loop.model.state
        for l in range(4):
            on = st[M.ROW_STANCE + l] == 1.0
            h = m.ground_height(st[M.ROW_FOOT + 3 * l], st[M.ROW_FOOT + 3 * l + 1])
            assert (st[M.ROW_FOOT + 3 * l + 2][on] == h[on]).all()


def test_the_contact_bands_are_twice_what_this_run_produces(rough):
    total = {k: 0.0 for k in CF.BANDS}
    for robot, (cmd, traj, loop, walked) in rough.items():
        worst = F.worst_in_window(F.window(traj, F.TICKS - F.WINDOW), cmd, loop.cfg.body_height)
        for k in total:
            total[k] = max(total[k], float(worst[k].max()))
    print("measured worst", total)
    for k, band in CF.BANDS.items():
        assert abs(band - 2 * total[k]) <= 0.01 * band, (k, band, total[k])


def test_on_the_step_grid_all_four_robots_enter_early_contact():
    traj, loop, walked = CF.run_cpu("ghost", CF.step_ground(), cmd=CF.STEP_CMD, height_scale=CF.STEP_START)
    print("EARLY_CONTACT leg-ticks", loop.early, "touch-downs", loop.touched, "x", loop.model.state[M.ROW_P])
    assert not loop.model.fallen().any()
    assert (loop.early > 0).all() and (loop.touched > 0).all()
    assert (np.abs(loop.model.state[M.ROW_P]) > CF.STEP_AT).all()           # every robot reached the step
    assert int(loop.lose.sum()) == 0
