"""The motor model (include/rg_srb_motor.h) without a GPU: the ABI of rg_srb_motor_apply and rg_srb_motor_draw (header, binding,
library; refusals that name the argument; validation before any device probe), known answers of the rule on the model
(tests/motor_model.py), the draw, the resources of robot_gym_amd/csrc/rg_srb_motor.hip from one device-only compile, and the CPU
reference closed loop with motors between the oracle and the simulator model, with the band of tests/motor_fixtures.py."""
import ctypes as C
import glob
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from robot_gym_amd.core import dr_abi, est_abi, friction_abi, motor_abi, sensor_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import kernel_checks
from tests import motor_fixtures as MF
from tests import motor_model as MM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import stream_model as SM
from tests.posctl_fixtures import REL_TOL, within_ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
CPU = torch.device("cpu")
PURPOSE = r"(?:#define (RG_\w*PURPOSE_\w+) (\d+)|enum \{ (RG_\w*PURPOSE_\w+) = (\d+) \})"


# ---- the ABI -----------------------------------------------------------------------------------------------------------

def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _arg_names(hdr, entry):
    args = re.search(rf"int {entry}\(([^)]*)\)", hdr).group(1)
    return [a.strip().split()[-1].lstrip("*") for a in args.split(",")]


def _purposes(text):
    return {a or c: int(b or d) for a, b, c, d in re.findall(PURPOSE, text)}


def test_header_binding_and_library_agree_on_both_entries():
    lib = motor_abi.load_library()
    hdr = _header("rg_srb_motor.h")
    declared = sorted(set(re.findall(r"\b(rg_srb_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(motor_abi.EXPORTS) == ["rg_srb_motor_apply", "rg_srb_motor_draw"]
    assert _arg_names(hdr, "rg_srb_motor_apply") == ["h", "state", "grf", "strength", "torque_limit", "grf_out", "tau_cmd", "tau_out", "stream"]
    assert _arg_names(hdr, "rg_srb_motor_draw") == ["h", "mask", "key", "draws", "seed", "lo", "hi", "strength", "stream"]
    for name in motor_abi.EXPORTS:
        assert hasattr(lib, name) and len(getattr(lib, name).argtypes) == len(_arg_names(hdr, name)), name
        assert getattr(lib, name).restype is C.c_int32
    assert all(t is C.c_void_p for t in lib.rg_srb_motor_apply.argtypes)
    assert [lib.rg_srb_motor_draw.argtypes[i] for i in (4, 5, 6)] == [C.c_uint64, C.c_double, C.c_double]
    whole = open(os.path.join(ROOT, "include", "rg_srb.h")).read()
    assert whole.index('#include "rg_srb_friction.h"') < whole.index('#include "rg_srb_motor.h"') < whole.index("#endif /* RG_SRB_H */")
    assert "unless a motor model stands in front" in whole
    # nothing else of the ABI moved, and srb_abi and friction_abi declare what they declared
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_SRB_\w+) (\d+)", _header("rg_srb.h"))}
    assert defs["RG_SRB_ABI_VERSION"] == 1 and defs["RG_SRB_STATE_ROWS"] == 43 and defs["RG_SRB_ROW_Q"] == 25 == M.ROW_Q
    assert not any("motor" in k for k in list(srb_abi.SIGNATURES) + list(srb_abi.EXPORTS) + list(friction_abi.SIGNATURES))
    assert motor_abi.MOTORS == MM.MOTORS == 12


def test_the_purpose_lies_in_block_four_and_is_disjoint_from_every_other():
    mine = _purposes(_header("rg_srb_motor.h"))
    assert mine == {"RG_SRB_MOTOR_PURPOSE_STRENGTH": 64} and motor_abi.PURPOSE_STRENGTH == MM.PURPOSE_STRENGTH == 64
    assert 64 // 16 == 4
    others = {}
    for path in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(path) != "rg_srb_motor.h":
            others.update(_purposes(open(path).read()))
    assert len(others) == 17 and 64 not in others.values() and all(v // 16 != 4 for v in others.values()), others
    assert len(set(others.values())) == 17
    bound = {v for abi in (dr_abi, sensor_abi, est_abi, friction_abi) for n, v in vars(abi).items() if n.startswith("PURPOSE_")}
    assert bound == set(others.values())
    registry = open(os.path.join(ROOT, "include", "rg_stream.h")).read()
    assert re.search(r"block 4\s+64\.\.79\s+rg_srb_motor\.h\s+64 ", registry) and "(block 5, 80..95)" in registry
    src = open(os.path.join(SRC, "rg_srb_motor.hip")).read()
    assert "static_assert(purposes_in_block(4, RG_SRB_MOTOR_PURPOSE_STRENGTH)" in src


ADDR = 4096      # a non-null address: with a null handle nothing is read through it


def _apply_args(**change):
    a = dict(state=ADDR, grf=ADDR, strength=ADDR, torque_limit=ADDR, grf_out=ADDR, tau_cmd=None, tau_out=None)
    a.update(change)
    return [None] + [a[k] for k in ("state", "grf", "strength", "torque_limit", "grf_out", "tau_cmd", "tau_out")] + [None]


def _draw_args(**change):
    a = dict(mask=ADDR, key=ADDR, draws=ADDR, seed=7, lo=0.7, hi=1.0, strength=ADDR)
    a.update(change)
    return [None] + [a[k] for k in ("mask", "key", "draws", "seed", "lo", "hi", "strength")] + [None]


def test_a_null_handle_is_refused_by_name_without_a_device():
    lib = motor_abi.load_library()
    assert lib.rg_srb_motor_apply(*_apply_args()) == -1
    assert b"motor_apply: null handle" in lib.rg_srb_last_error(None)
    assert lib.rg_srb_motor_apply(*_apply_args(tau_cmd=ADDR, tau_out=ADDR)) == -1
    assert b"motor_apply: null handle" in lib.rg_srb_last_error(None)
    assert lib.rg_srb_motor_draw(*_draw_args()) == -1
    assert b"motor_draw: null handle" in lib.rg_srb_last_error(None)


APPLY_REFUSALS = [(dict([(n, None)]), f"motor_apply: null {n}") for n in ("state", "grf", "strength", "torque_limit", "grf_out")]
DRAW_REFUSALS = [(dict([(n, None)]), f"motor_draw: null {n}") for n in ("mask", "key", "draws", "strength")]
DRAW_REFUSALS += [(dict(lo=-0.1), "motor_draw: lo"), (dict(lo=math.nan), "motor_draw: lo"), (dict(lo=math.inf), "motor_draw: lo"),
                  (dict(lo=0.9, hi=0.2), "motor_draw: hi"), (dict(hi=math.nan), "motor_draw: hi"), (dict(hi=math.inf), "motor_draw: hi")]


@pytest.mark.parametrize("change,text", APPLY_REFUSALS, ids=[t for _, t in APPLY_REFUSALS])
def test_motor_apply_refuses_each_null_argument_by_name_without_a_device(change, text):
    lib = motor_abi.load_library()
    assert lib.rg_srb_motor_apply(*_apply_args(**change)) == -1
    assert text.encode() in lib.rg_srb_last_error(None), lib.rg_srb_last_error(None)


@pytest.mark.parametrize("change,text", DRAW_REFUSALS, ids=[t + str(i) for i, (_, t) in enumerate(DRAW_REFUSALS)])
def test_motor_draw_refuses_each_null_or_bad_argument_by_name_without_a_device(change, text):
    lib = motor_abi.load_library()
    assert lib.rg_srb_motor_draw(*_draw_args(**change)) == -1
    assert text.encode() in lib.rg_srb_last_error(None), lib.rg_srb_last_error(None)


def _good(B=5):
    rows = lambda: torch.zeros(12, B, dtype=torch.float64)
    return dict(state=torch.zeros(43, B, dtype=torch.float64), grf=torch.zeros(B, 12), strength=rows(), torque_limit=rows(), grf_out=torch.zeros(B, 12),
                tau_cmd=rows(), tau_out=rows())


def test_the_binding_accepts_what_the_library_takes():
    a = _good()
    assert motor_abi.motor_apply_ptrs(5, CPU, **a) == tuple(a[k].data_ptr() for k in ("state", "grf", "strength", "torque_limit", "grf_out", "tau_cmd", "tau_out"))
    a["tau_cmd"] = a["tau_out"] = None
    a["grf_out"] = a["grf"]                                  # in place
    p = motor_abi.motor_apply_ptrs(5, CPU, **a)
    assert p[5:] == (None, None) and p[1] == p[4]
    d = dict(mask=torch.zeros(5, dtype=torch.int32), key=torch.zeros(5, dtype=torch.float64), draws=torch.zeros(5, dtype=torch.float64),
             strength=torch.zeros(12, 5, dtype=torch.float64))
    assert motor_abi.motor_draw_ptrs(5, CPU, **d) == tuple(d[k].data_ptr() for k in ("mask", "key", "draws", "strength"))


BAD_ARGS = [(name, how) for name in ("state", "grf", "strength", "torque_limit", "grf_out", "tau_cmd", "tau_out") for how in ("dtype", "batch", "strided", "device", "type")]
BAD_ARGS += [(name, "none") for name in ("state", "grf", "strength", "torque_limit", "grf_out")]


@pytest.mark.parametrize("name,how", BAD_ARGS)
def test_the_binding_refuses_a_bad_tensor_naming_the_argument(name, how, monkeypatch):
    for probe in ("is_available", "current_device", "current_stream", "device_count"):
        monkeypatch.setattr(torch.cuda, probe, lambda *a, **k: pytest.fail(f"torch.cuda.{probe} called before validation"))
    a = _good()
    t = a[name]
    if how == "dtype":
        a[name] = t.to(torch.float16)
    elif how == "batch":
        a[name] = _good(6)[name]
    elif how == "strided":
        a[name] = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]
        assert a[name].shape == t.shape and not a[name].is_contiguous()
    elif how == "device":
        a[name] = t.to("meta")
    elif how == "type":
        a[name] = t.numpy()
    elif how == "none":
        a[name] = None
    with pytest.raises(ValueError, match=rf"motor_apply: {name}\b"):
        motor_abi.motor_apply_ptrs(5, CPU, **a)


def test_the_python_layer_refuses_bad_values_before_it_looks_for_a_device(monkeypatch):
    from robot_gym_amd.sim import BatchedSRBSim, MotorModel
    from robot_gym_amd.sim.randomizer import DomainRandomizer
    for probe in ("is_available", "current_device", "current_stream", "device_count"):
        monkeypatch.setattr(torch.cuda, probe, lambda *a, **k: pytest.fail(f"torch.cuda.{probe} called before validation"))
    for bad in (-0.1, math.nan, math.inf, "strong", None, True, [1.0] * 11, np.ones((4, 3)), np.ones((12, 2, 2)), torch.full((12,), -1.0), object()):
        with pytest.raises(ValueError, match="MotorModel: strength"):
            MotorModel(strength=bad)
    for bad in (-1.0, math.nan, "none", [5.0] * 13, np.full((12, 3), -2.0), torch.tensor([math.nan] * 12)):
        with pytest.raises(ValueError, match="MotorModel: torque_limit"):
            MotorModel(torque_limit=bad)
    # what is accepted: a float, twelve values, [12, B], a limit of +inf or None, a strength of 0 or above 1
    m = MotorModel(strength=np.linspace(0.0, 1.2, 12), torque_limit=torch.full((12, 4), math.inf, dtype=torch.float64))
    s, lim = m.rows(4)
    assert s.shape == lim.shape == (12, 4) and (s[:, 2] == np.linspace(0.0, 1.2, 12)).all() and np.isinf(lim).all()
    assert all(np.isinf(MotorModel(torque_limit=v).rows(3)[1]).all() for v in (None, math.inf)) and (MotorModel().rows(3)[0] == 1.0).all()
    # a [12, B] argument of another batch, and something that is no model, are refused by the simulator before the device
    with pytest.raises(ValueError, match=r"MotorModel: torque_limit must have one column per robot \(\[12, 5\]\)"):
        BatchedSRBSim(5, motors=m)
    with pytest.raises(ValueError, match=r"MotorModel: strength must have one column per robot"):
        BatchedSRBSim(5, motors=MotorModel(strength=np.ones((12, 4))))
    with pytest.raises(ValueError, match="motors must be a MotorModel"):
        BatchedSRBSim(5, motors=0.8)
    # the setters validate before they ask whether the model is bound
    for bad in (-0.5, math.inf, [1.0] * 3):
        with pytest.raises(ValueError, match="set_strength: values"):
            m.set_strength(bad)
    with pytest.raises(ValueError, match="set_torque_limit: values"):
        m.set_torque_limit(-3.0)
    with pytest.raises(RuntimeError, match="bind"):
        m.set_strength(0.5)
    with pytest.raises(RuntimeError, match="bind"):
        m.copy_columns([0], [1])
    for bad in (0.7, (1.0, 0.7), (-0.1, 0.2), (0.1, math.inf), (0.1, 0.2, 0.3), "ab"):
        with pytest.raises(ValueError, match="motor_strength"):
            DomainRandomizer(motor_strength=bad)
    # a simulator without a motor model has no strength rows for the draw to write
    sim = types.SimpleNamespace(terrain=None, mu=None, motors=None, batch=4, device=CPU, substeps=10)
    dr = DomainRandomizer(motor_strength=(0.7, 1.0))
    with pytest.raises(ValueError, match="needs a simulator built with a motor model"):
        dr.bind(sim)
    assert dr._handle is None and DomainRandomizer().motor_strength is None and dr.motor_strength == (0.7, 1.0)
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.1, math.inf), (math.nan, 0.5), ("a", 1)):
        with pytest.raises(ValueError, match="motor_draw"):
            motor_abi.checked_range(lo, hi)


# ---- known answers of the rule on the model --------------------------------------------------------------------------------

ROBOTS = F.ROBOTS


def _standing(robot, B=3):
    """(chain, q [12, B] of the reset pose, the four legs' Jacobians there as [9] lists of [B] arrays, mdir [4, 3])."""
    cfg = MPCConfig.for_robot(robot)
    m = M.SRBModel(B, cfg)
    m.reset()
    chain, q = M.Chain(cfg), m.state[M.ROW_Q:M.ROW_Q + 12].copy()
    J = [chain.fk(np.full(B, l), [q[3 * l + j] for j in range(3)])[1] for l in range(4)]
    return chain, q, J, chain.mdir


def _forces(B, seed=1):
    rng = np.random.default_rng(seed)
    g = rng.uniform(-30.0, 30.0, (B, 12))
    g[:, 2::3] = rng.uniform(-90.0, -20.0, (B, 4))       # the ground pushes up: grf is the negated force
    return g.astype(np.float32)


ONE, INF = np.ones((12, 3)), np.full((12, 3), np.inf)


@pytest.mark.parametrize("robot", ROBOTS)
def test_strength_one_without_a_limit_returns_the_input_bits(robot):
    chain, q, J, mdir = _standing(robot)
    g = _forces(3)
    g[1, 3:6] = 0.0                                        # a swinging leg: zero force passes through
    g[2, 0] = np.float32(-0.0)
    out, tau_cmd, tau, sat = MM.apply(chain, q, g, ONE, INF)
    assert out.tobytes() == g.tobytes() and tau.tobytes() == tau_cmd.tobytes() and not sat.any()
    assert (tau_cmd[3:6, 1] == 0.0).all() and (tau_cmd[:, 0] != 0.0).all()
    # the controller's own expression, by hand for one motor
    l, j, b = 2, 1, 0
    gd = g[b, 3 * l:3 * l + 3].astype(np.float64)
    assert tau_cmd[3 * l + j, b] == ((gd[0] * J[l][j][b] + gd[1] * J[l][3 + j][b]) + gd[2] * J[l][6 + j][b]) * mdir[l, j]
    # zero force passes through whatever the strength and the limit, and its torques are zero
    z = np.zeros((3, 12), np.float32)
    out, tau_cmd, tau, sat = MM.apply(chain, q, z, 0.3 * ONE, 0.0 * ONE)
    assert out.tobytes() == z.tobytes() and not sat.any() and (tau_cmd == 0.0).all() and (tau == 0.0).all()
    # a limit above every torque, and a limit exactly at it, pass through too
    g = _forces(3, 2)
    _, tau_cmd, _, _ = MM.apply(chain, q, g, ONE, INF)
    for lim in (np.abs(tau_cmd), 2.0 * np.abs(tau_cmd)):
        out, _, tau, sat = MM.apply(chain, q, g, ONE, lim)
        assert out.tobytes() == g.tobytes() and not sat.any() and tau.tobytes() == tau_cmd.tobytes()


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("s", [0.5, 0.9, 1.2, 0.0])
def test_a_uniform_strength_on_one_leg_scales_its_force(robot, s):
    """Strength above 1 takes the solve branch like strength below 1; strength 0 delivers nothing."""
    chain, q, J, mdir = _standing(robot)
    g = _forces(3, 3)
    strength = ONE.copy()
    strength[3:6] = s
    out, tau_cmd, tau, sat = MM.apply(chain, q, g, strength, INF)
    assert sat[1].all() and not sat[[0, 2, 3]].any()
    keep = [i for i in range(12) if i not in (3, 4, 5)]
    assert out[:, keep].tobytes() == g[:, keep].tobytes()
    assert within_ulp(out[:, 3:6], s * g[:, 3:6].astype(np.float64)).all()
    assert (tau[3:6] == s * tau_cmd[3:6]).all() and tau[keep].tobytes() == tau_cmd[keep].tobytes()
    assert s != 0.0 or (out[:, 3:6] == 0.0).all()


@pytest.mark.parametrize("robot", ROBOTS)
@pytest.mark.parametrize("joint", [0, 1, 2])
def test_one_joint_at_half_its_commanded_torque(robot, joint):
    chain, q, J, mdir = _standing(robot)
    g = _forces(3, 4)
    l = 3
    _, tau_cmd, _, _ = MM.apply(chain, q, g, ONE, INF)
    lim = INF.copy()
    lim[3 * l + joint] = 0.5 * np.abs(tau_cmd[3 * l + joint])
    out, tc, tau, sat = MM.apply(chain, q, g, ONE, lim)
    assert tc.tobytes() == tau_cmd.tobytes() and sat[l].all() and not sat[:3].any()
    # the other legs' bits, and the other two torques of this leg, are untouched; the clipped one keeps its sign
    assert out[:, :9].tobytes() == g[:, :9].tobytes()
    other = [3 * l + j for j in range(3) if j != joint]
    assert tau[other].tobytes() == tau_cmd[other].tobytes() and tau[:9].tobytes() == tau_cmd[:9].tobytes()
    assert (tau[3 * l + joint] == 0.5 * tau_cmd[3 * l + joint]).all()
    # J' g' reproduces c o mdir, in float64 before the cast ...
    A = [J[l][0], J[l][3], J[l][6], J[l][1], J[l][4], J[l][7], J[l][2], J[l][5], J[l][8]]
    rhs = [tau[3 * l + j] * mdir[l, j] for j in range(3)]
    x, det = MM.solve3(A, rhs)
    assert (det != 0.0).all()
    for j in range(3):
        got = (x[0] * J[l][j] + x[1] * J[l][3 + j]) + x[2] * J[l][6 + j]
        assert (np.abs(got - rhs[j]) <= REL_TOL * np.maximum(1.0, np.abs(rhs[j]))).all(), j
    # ... and the delivered floats are that solution's
    assert np.stack(x, 1).astype(np.float32).tobytes() == out[:, 9:].tobytes() and (out[:, 9:] != g[:, 9:]).any()


def test_a_nan_force_on_one_leg_gives_nan_on_that_leg_only():
    chain, q, J, mdir = _standing("ghost")
    g = _forces(3, 5)
    g[1, 7] = np.nan
    strength = ONE.copy()
    strength[:, 2] = 0.8
    for lim in (INF, 1e4 * ONE):       # a finite limit does not turn a NaN torque into a finite one
        out, tau_cmd, tau, sat = MM.apply(chain, q, g, strength, lim)
        assert np.isnan(out[1, 6:9]).all() and np.isnan(tau[6:9, 1]).all() and np.isnan(tau_cmd[6:9, 1]).all() and sat[2, 1]
        rest = np.ones((3, 12), dtype=bool)
        rest[1, 6:9] = False
        assert np.isfinite(out[rest]).all() and np.isfinite(np.delete(tau, [6, 7, 8], 0)).all()
        assert out[0].tobytes() == g[0].tobytes() and out[1, :6].tobytes() == g[1, :6].tobytes() and out[1, 9:].tobytes() == g[1, 9:].tobytes()
        assert sat[:, 2].all() and not sat[:, 0].any() and sat[:, 1].tolist() == [False, False, True, False]
    # an infinite force passes through as it is under no limit, and the tick of rg_srb.h handles it; under a limit it is clipped
    g[1, 7] = np.inf
    out, tau_cmd, tau, sat = MM.apply(chain, q, g, ONE, INF)
    assert out.tobytes() == g.tobytes() and not np.isfinite(tau_cmd[6:9, 1]).any()


def test_a_jacobian_with_determinant_zero_takes_the_uniform_scale():
    chain, q, J, mdir = _standing("ghost", B=2)
    g = _forces(2, 6)
    one, zero = np.ones(2), np.zeros(2)
    flat = [one, zero, zero, zero, one, zero, zero, zero, zero]           # the third joint moves nothing: det = 0 exactly
    strength, lim = np.ones((12, 2)), np.full((12, 2), np.inf)
    strength[0], strength[1], strength[2] = 0.5, 0.8, 0.1                  # tau_2 = 0: its ratio counts as 1
    out, tau_cmd, tau, sat = MM.apply(chain, q, g, strength, lim, jac=lambda l, Jl: flat if l == 0 else Jl)
    gd = g.astype(np.float64)
    assert (tau_cmd[0] == gd[:, 0] * mdir[0, 0]).all() and (tau_cmd[1] == gd[:, 1] * mdir[0, 1]).all() and (tau_cmd[2] == 0.0).all()
    assert sat[0].all() and out[:, :3].tobytes() == (0.5 * gd[:, :3]).astype(np.float32).tobytes() and out[:, 3:].tobytes() == g[:, 3:].tobytes()
    _, _, _, solved, scaled = MM.leg_rule([g[:, i] for i in range(3)], flat, list(mdir[0]), [strength[j] for j in range(3)], [lim[j] for j in range(3)])
    assert scaled.all() and not solved.any()
    # a limit decides the scale when it binds harder: joint 1 at a quarter of its torque
    lim[1] = 0.25 * np.abs(tau_cmd[1])
    out, _, tau, _ = MM.apply(chain, q, g, strength, lim, jac=lambda l, Jl: flat if l == 0 else Jl)
    k = np.fmin(np.fmin(tau[0] / tau_cmd[0], tau[1] / tau_cmd[1]), 1.0)
    assert (np.abs(k - 0.25) < 1e-15).all() and out[:, :3].tobytes() == (k[:, None] * gd[:, :3]).astype(np.float32).tobytes()
    # a regular Jacobian with the same settings takes the solve
    _, _, _, solved, scaled = MM.leg_rule([g[:, i] for i in range(3)], J[0], list(mdir[0]), [strength[j] for j in range(3)], [lim[j] for j in range(3)])
    assert solved.all() and not scaled.any()


def test_the_kernel_inputs_saturate_in_like_numbers_and_keep_clear_of_their_limits():
    """The conditions the GPU test's inputs are held to, on the model alone (motor_fixtures.kernel_cases asserts them): between a
    fifth and four fifths of the legs saturate, and no |a_j| lies within REL_TOL * max(1, limit) of its limit."""
    cases = MF.kernel_cases()
    assert sorted({B for _, B in cases}) == [1, 15, 16, 17, 63, 65, 257] and {r for r, _ in cases} == set(ROBOTS)
    for robot in ROBOTS:
        sat, legs = sum(int(cases[robot, B]["sat"].sum()) for B in MF.BATCHES), 4 * sum(MF.BATCHES)
        zero = sum(int((cases[robot, B]["grf"].reshape(-1, 3) == 0).all(1).sum()) for B in MF.BATCHES)
        inf = sum(int(np.isinf(cases[robot, B]["limit"]).sum()) for B in MF.BATCHES)
        print(robot, "saturated legs", sat, "of", legs, "zero-force legs", zero, "limits at +inf", inf, "of", 3 * legs)
        assert zero > 100 and 0.2 * 3 * legs < inf < 0.9 * 3 * legs


@pytest.mark.parametrize("robot", ROBOTS)
def test_a_foot_on_the_knee_axis_is_a_configuration_the_library_takes_and_exactly_singular(robot):
    """The inputs of the GPU test of the kernel's singular branch (motor_fixtures.singular_case asserts det == 0.0 exactly on leg
    0, the uniform scale there and the solve on the other legs): the configuration differs from the robot's in the toe of leg 0
    alone, and the simulator's configuration check takes it."""
    import dataclasses
    c = MF.singular_case(robot)
    cfg, regular = c["cfg"], MPCConfig.for_robot(robot)
    changed = {f.name for f in dataclasses.fields(cfg) if getattr(cfg, f.name) != getattr(regular, f.name)}
    assert changed <= {"toe_xyz", "toe_com"} and changed and cfg.toe_xyz[3:] == regular.toe_xyz[3:] and cfg.toe_com[3:] == regular.toe_com[3:]
    assert (M.Chain(cfg).tip[0] == 0.0).all() and (M.Chain(cfg).tip[1:] == M.Chain(regular).tip[1:]).all()
    srb_abi.make_cconfig(cfg)
    assert c["scaled"][0].all() and not c["scaled"][1:].any() and c["B"] == 17
    assert np.isfinite(c["limit"][1, 0::2]).all() and np.isinf(np.delete(c["limit"], 1, 0)).all()      # one binding limit
    assert all(len(set(c["strength"][:3, b].tolist())) == 3 for b in range(17))                    # strengths that differ per joint


def test_the_settings_only_the_c_abi_accepts_are_refused_by_the_python_layer_and_defined_on_the_model():
    """motor_fixtures.abi_cases asserts on the model what each case is about; here: MotorModel refuses every one of the settings, so
    rg_srb_motor_apply on raw tensors is the only way to them, and the header states each."""
    from robot_gym_amd.sim import MotorModel
    cases = MF.abi_cases()
    assert sorted(cases) == sorted(["strength_zero", "limit_zero", "limit_nan", "limit_negative", "strength_inf_on_a_swinging_leg",
                                    "negative_zero_and_denormal_force", "all_zero_force"])
    for name, field, what in (("limit_nan", "limit", "torque_limit"), ("limit_negative", "limit", "torque_limit"),
                              ("strength_inf_on_a_swinging_leg", "strength", "strength")):
        with pytest.raises(ValueError, match=f"MotorModel: {what}"):
            MotorModel(**{what: cases[name][field]})
    # strength 0 and limit 0 are values MotorModel takes; the C ABI is where their zeros' signs are pinned
    MotorModel(strength=cases["strength_zero"]["strength"], torque_limit=cases["limit_zero"]["limit"])
    text = " ".join(open(os.path.join(ROOT, "include", "rg_srb_motor.h")).read().replace(" *", " ").split())
    for sentence in ("strength 0:", "limit 0:", "a NaN limit is no limit", "a negative limit is not an interval", "+inf strength:",
                     "-0.0 and denormal floats", "an all-zero grf passes through by bits"):
        assert sentence in text, sentence


# ---- the draw --------------------------------------------------------------------------------------------------------------

def test_the_draw_lies_in_its_range_follows_the_key_and_leaves_the_rest():
    B, seed, lo, hi = 200, 12345, 0.7, 1.0
    rng = np.random.default_rng(3)
    key = rng.integers(-1000, 1000, B).astype(np.float64)
    draws = rng.integers(0, 50, B).astype(np.float64)
    mask = (rng.uniform(size=B) < 0.6).astype(np.int32)
    s = np.full((12, B), -7.0)
    MM.draw(s, mask, key, draws, seed, lo, hi)
    on = mask != 0
    assert (s[:, ~on] == -7.0).all() and on.sum() > 80 and (~on).sum() > 40
    assert (s[:, on] >= lo).all() and (s[:, on] <= hi).all() and s[:, on].std() > 0.06
    # every motor draws its own value: the motor is the last word of the chain, the purpose is one
    assert all(len(set(s[:, b].tolist())) == 12 for b in np.nonzero(on)[0])
    for b, m in ((int(np.nonzero(on)[0][0]), 0), (int(np.nonzero(on)[0][-1]), 11)):
        assert s[m, b] == lo + (hi - lo) * SM.uniform(seed, int(key[b]), int(draws[b]), 64, m)
    # the value follows the key and the draw count, not the position in the batch
    perm = rng.permutation(B)
    again = np.full((12, B), -7.0)
    MM.draw(again, mask[perm], key[perm], draws[perm], seed, lo, hi)
    assert again.tobytes() == np.ascontiguousarray(s[:, perm]).tobytes()
    other = np.full((12, B), -7.0)
    MM.draw(other, mask, key, draws + 1.0, seed, lo, hi)
    assert (other[:, on] != s[:, on]).all()
    assert SM.uniform(seed, 5, 0, 64, 0) != SM.uniform(seed, 5, 0, friction_abi.PURPOSE_MU, 0) != SM.uniform(seed + 1, 5, 0, 64, 0)
    flat = np.zeros((12, 4))
    MM.draw(flat, np.ones(4, np.int32), np.arange(4.0), np.zeros(4), 1, 0.5, 0.5)
    assert (flat == 0.5).all()


# ---- resources of rg_srb_motor.hip -----------------------------------------------------------------------------------------

KERNELS = {"rg_srb_motor_apply_kernel", "rg_srb_motor_draw_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_srb_motor.hip")


def test_both_motor_kernels_are_reported_and_use_no_scratch_and_no_lds(remarks):
    assert set(remarks) == KERNELS
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds): the apply kernel is leg_fk, unrolled over its three joints, and a
# 3 x 3 solve, 166 VGPRs and three waves per SIMD; the draw twelve hashes.
REGISTERS = {"rg_srb_motor_apply_kernel": dict(vgprs=168, agprs=0, occupancy=3), "rg_srb_motor_draw_kernel": dict(vgprs=20, agprs=0, occupancy=8)}


def test_motor_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_motor_source_keeps_contraction_off_and_both_library_targets_compile_it():
    src = open(os.path.join(SRC, "rg_srb_motor.hip")).read()
    code = re.sub(r"//.*", "", src)
    pragma = code.index("#pragma clang fp contract(off)")
    assert pragma < code.index('#include "rg_mpc_dev.h"') < code.index('#include "rg_srb_dev.inc"') < code.index('#include "rg_stream_dev.inc"') < code.index("__global__")
    assert code.count("#pragma clang fp contract") == 1 and len(re.findall(r"__global__", code)) == len(KERNELS)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "fma(" not in code and "__shfl" not in code
    kernel_checks.assert_built_into_both("rg_srb_motor.hip", header="rg_srb_motor.h")
    # no step kernel, and no file one includes, knows of this unit: the rule stays in its own file
    for other in sorted(os.listdir(SRC)):
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_srb_motor.hip":
            assert "motor_apply" not in open(os.path.join(SRC, other)).read() and "rg_srb_motor" not in open(os.path.join(SRC, other)).read(), other


# ---- the CPU closed loop with motors ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def loops():
    """{(robot, name): the loop after 400 ticks}: without a model, with every limit at twice the peak, with strength 0, and with
    every limit at LIMIT_FRACTION of the peak."""
    out = {}
    for robot in ROBOTS:
        peak = np.asarray(MF.PEAK[robot])
        out[robot, "none"] = MF.run_cpu(robot)
        out[robot, "twice"] = MF.run_cpu(robot, limit=MF.limit_rows(peak, 2.0, 32))
        out[robot, "dead"] = MF.run_cpu(robot, strength=0.0)
        out[robot, "limited"] = MF.run_cpu(robot, limit=MF.limit_rows(peak, MF.LIMIT_FRACTION, 32))
    return out


@pytest.mark.parametrize("robot", ROBOTS)
def test_closed_loop_with_motors(robot, loops):
    none, twice, dead, limited = (loops[robot, n] for n in ("none", "twice", "dead", "limited"))
    print(robot, "peak |tau_cmd| per motor without a model, N m:", np.round(none.peak, 4).tolist())
    assert none.identical and none.saturated == 0 and not none.model.fallen().any() and (none.model.state[M.ROW_STEPS] == 10 * F.TICKS).all()
    assert (np.abs(none.peak - np.asarray(MF.PEAK[robot])) <= 1e-4).all()
    # a limit no torque reaches: every tick's delivered force is the input bit for bit, and the run is the run without a model
    assert twice.identical and twice.saturated == 0 and twice.model.state.tobytes() == none.model.state.tobytes()
    assert all(twice.model.obs[k].tobytes() == none.model.obs[k].tobytes() for k in none.model.obs)
    # motors that deliver nothing: every robot falls
    assert dead.model.fallen().all() and (dead.worst_tau == 0.0).all()
    # between the two: legs saturate, and no delivered torque exceeds its limit
    fallen = int(limited.model.fallen().sum())
    print(robot, "limit", MF.LIMIT_FRACTION, "of the peak: saturated leg-ticks", limited.saturated, "of", 4 * 32 * F.TICKS, "fallen", fallen)
    assert limited.saturated > 0 and not limited.identical
    assert (limited.worst_tau <= MF.LIMIT_FRACTION * np.asarray(MF.PEAK[robot])).all()


@pytest.mark.parametrize("robot", ROBOTS)
def test_the_band_is_twice_what_this_run_produces(robot, loops):
    limited = loops[robot, "limited"]
    got = (limited.saturated, int(limited.model.fallen().sum()))
    print(robot, "measured", got, "recorded", MF.MEASURED[robot])
    assert got == MF.MEASURED[robot]
    assert MF.SATURATED_BAND[robot] == 2 * got[0] and MF.FALLEN_BAND[robot] == 2 * got[1]
