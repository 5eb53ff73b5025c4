#!/usr/bin/env python3
"""Golden vectors of the position-mode controllers, recorded by DRIVING THE REFERENCE CLASSES (authoring machine only).

Needs the reference checkout (RG_REFERENCE); writes small data files next to this script.  Nothing of the reference's
source travels: only seeded inputs and the outputs its code produced.  The `mpc_controller` stub of make_golden.py is
installed (the robots' ctrl_constants import it), numpy 2's missing `np.math` is restored to `math` (solve_bin_factor,
bezier_controller.py:48-49) and the Bezier module's wall clock is replaced by each stream's clock, the one deliberate
change of include/rg_posctl.h (deviation 1).  A reset is modelled as a fresh reference object whose clock origin
`_last_time` is the reset time (deviation 2).  Inputs are float32-representable, so the device is fed identical numbers.

  bezier_gait.npz    BezierController.update_controller_params + get_action (bezier_controller.py:154-227), S streams x
                     T ticks: params, clocks, resets, phi / last_time / alpha and angles per tick, frames at every
                     FRAME_EVERY-th tick, the angles of get_action before any update, the class's own constants
  pose_ik.npz        PoseController.get_action (pose_controller.py:54-99) on poses inside and beyond its slider ranges,
                     and the pose constants of ghost and k3lso (ctrl_constants.py:43-62)
  motor_position.npz RobotMotorModel.convert_to_torque, POSITION branch (simple_motor.py:122-140), over the ACTION_REPEAT
                     sub-steps of one control tick, ghost motor constants
  posctl_configs.npz the same three recordings on the NON-DEFAULT configurations of CONFIGS below (keys "c<i>_..."), none of
                     them symmetric the way the reference's own constants are: the geometry comes from a namespace in
                     place of the ctrl-constants module, the Bezier attributes _start_frames / _offset / step_offset and
                     the pose attribute _frames are set on the constructed object, and the motor model takes its gains as
                     arguments.  Short streams in the style of _stream_inputs, frames at EVERY tick, plus boundary
                     streams whose clocks make the comparisons of step_trajectory exact equalities (p == step_offset,
                     phi + offset == 1) or put _last_time ahead of the clock (negative phase).  The configuration values
                     are stored in the file; the tests build their PosCtlConfig from it.

Every file is compared with the committed one before it is replaced, and the script says whether its arrays are identical.

Every IK domain (kinematics.solve_IK, pose/kinematics.py:68-71) the recording meets is asserted to stay >= 1e-6 away from
+-1, the one discontinuity an ulp-level difference could flip.  Run with --time to print the reference's CPU cost per
robot-tick as well.
"""
import math
import os
import sys
import time
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, OUT)
import make_golden  # noqa: E402,F401  (installs the mpc_controller stub and puts the reference on sys.path)

np.math = math

S_STREAMS, T_TICKS, FRAME_EVERY = 24, 128, 16
DOMAIN_MARGIN = 1e-6
N_POSE = 384
N_MOTOR = 24


class Clock:
    now = 0.0

    def time(self):
        return self.now


CLOCK = Clock()
DOMAINS = []


def _install_hooks():
    from robot_gym.controllers.bezier import bezier_controller
    from robot_gym.controllers.pose import kinematics
    bezier_controller.time = CLOCK            # time.time() -> the stream's clock
    plain = kinematics.check_domain

    def check_domain(domain):
        DOMAINS.append(float(domain))
        return plain(domain)
    kinematics.check_domain = check_domain


def _check_margin(where):
    if DOMAINS:
        worst = min(abs(abs(x) - 1.0) for x in DOMAINS)
        assert worst >= DOMAIN_MARGIN, f"{where}: an IK domain lies within {worst:.3g} of +-1"
    DOMAINS.clear()


class Robot:
    """What the controllers read of a robot: its ctrl constants module."""

    def __init__(self, name="ghost"):
        import importlib
        self._ctrl = importlib.import_module(f"robot_gym.model.robots.{name}.ctrl_constants")
        self._motor = importlib.import_module(f"robot_gym.model.robots.{name}.motor_constants")

    def GetCtrlConstants(self):
        return self._ctrl

    def GetMotorConstants(self):
        return self._motor


def f32(x):
    return np.asarray(x, dtype=np.float32)


def _save(name, **arrays):
    """Write tests/golden/<name>, and say whether its arrays equal the ones of the file it replaces."""
    path = os.path.join(OUT, name)
    verdict = "new file"
    if os.path.exists(path):
        old = np.load(path)
        same = sorted(old.files) == sorted(arrays) and all(
            old[k].dtype == np.asarray(v).dtype and old[k].shape == np.asarray(v).shape and
            old[k].tobytes() == np.ascontiguousarray(v).tobytes() for k, v in arrays.items())
        verdict = "arrays identical to the committed file" if same else "ARRAYS CHANGED"
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, {verdict}")
    return verdict


def _stream_inputs(s, rng, T=None):
    """params [T, 4] float32, clock [T] float64, reset [T] bool, t0 [T] float64 of stream s."""
    T = T_TICKS if T is None else T
    kind = s % 12
    # clocks: regular control ticks (ACTION_REPEAT * SIMULATION_TIME_STEP = 0.01 s) or irregular spacing
    if kind in (2, 6, 9, 11) or s >= 12 and s % 3 == 0:
        dt = rng.uniform(0.002, 0.03, T)
        dt[rng.uniform(0, 1, T) < 0.05] *= 6.0          # occasional long gaps
    else:
        dt = np.full(T, 0.01)
    start = {7: 37.25, 8: 0.003}.get(kind, float(rng.choice([0.0, 0.0, 1.5, 12.0])) if s >= 12 else 0.0)
    clock = start + np.concatenate([[0.0], np.cumsum(dt[1:])])
    # params: held for stretches, or fresh every tick
    every_tick = kind in (3, 6, 10) or (s >= 12 and s % 2 == 1)
    seg = np.ones(T, dtype=bool) if every_tick else (np.arange(T) % int(rng.integers(12, 40)) == 0)
    seg[0] = True
    p = np.zeros((T, 4))
    cur = None
    for k in range(T):
        if seg[k]:
            cur = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-180, 180), rng.uniform(-1.5, 1.5), rng.uniform(0.2, 1.0)])
            if rng.uniform() < 0.15:
                cur[0] = 0.0                          # exact zero step length
            if rng.uniform() < 0.15:
                cur[2] = 0.0                          # exact zero rotation
            if rng.uniform() < 0.1:
                cur[1] = float(rng.choice([-180.0, 180.0, 0.0, 90.0, -90.0]))
        p[k] = cur
    period = {0: 0.3, 1: 0.4, 2: 1.0, 4: 0.005, 5: 0.015, 9: 0.015}.get(kind)
    if period is not None:
        p[:, 3] = period
    if kind == 3:
        p[:, 3] = rng.uniform(-1.0, 1.0, T)                # the slider's whole range: negative periods hit the floor
    if kind == 10:
        p[:, 3] = rng.choice([-0.4, 0.0, 0.005, 0.01, 0.3], T)
    if kind == 11:
        p[:, 0] = 0.0
        p[:, 2] = 0.0
    if kind == 8:
        p[:, 1] = rng.choice([-180.0, 180.0], T)
    # resets: at a few ticks, origin at the tick's clock (or a little before)
    reset = np.zeros(T, dtype=bool)
    t0 = np.zeros(T)
    if kind in (5, 6, 7) or s >= 12:
        for k in rng.choice(np.arange(8, T), size=int(rng.integers(1, 4)), replace=False):
            reset[k] = True
            t0[k] = clock[k] - float(rng.choice([0.0, 0.0, 0.004, 0.02]))
    return f32(p), clock, reset, t0


def gen_bezier(timing=False):
    from robot_gym.controllers.bezier.bezier_controller import BezierController
    robot = Robot("ghost")
    rng = np.random.default_rng(20261016)
    S, T = S_STREAMS, T_TICKS
    params = np.zeros((S, T, 4), dtype=np.float32)
    clock = np.zeros((S, T))
    reset = np.zeros((S, T), dtype=bool)
    t0 = np.zeros((S, T))
    phi = np.zeros((S, T))
    last_time = np.zeros((S, T))
    alpha = np.zeros((S, T))
    angles = np.zeros((S, T, 12), dtype=np.float32)
    frame_ticks = np.arange(FRAME_EVERY - 1, T, FRAME_EVERY)
    frames = np.zeros((S, len(frame_ticks), 4, 3))
    first = BezierController(robot, None)
    angles_first = np.asarray(first.get_action(), dtype=np.float64)
    _check_margin("get_action before any update")
    spent, ticks = 0.0, 0
    for s in range(S):
        params[s], clock[s], reset[s], t0[s] = _stream_inputs(s, rng)
        ctrl = BezierController(robot, None)
        for k in range(T):
            if reset[s, k]:
                ctrl = BezierController(robot, None)
                ctrl._last_time = float(t0[s, k])
            CLOCK.now = float(clock[s, k])
            t_a = time.perf_counter()
            ctrl.update_controller_params(tuple(float(x) for x in params[s, k]))
            a = ctrl.get_action()
            spent += time.perf_counter() - t_a
            ticks += 1
            phi[s, k], last_time[s, k], alpha[s, k] = ctrl._phi, ctrl._last_time, ctrl._alpha
            angles[s, k] = np.asarray(a, dtype=np.float64)
            if (k + 1) % FRAME_EVERY == 0:
                frames[s, (k + 1) // FRAME_EVERY - 1] = ctrl._frame
            _check_margin(f"stream {s} tick {k}")
    if timing:
        print(f"reference BezierController update_controller_params + get_action: {1e3 * spent / ticks:.3f} ms per robot-tick "
              f"({ticks} ticks, one CPU thread)")
    ref = BezierController(robot, None)
    _save("bezier_gait.npz", params=params, clock=clock, reset=reset, t0=t0, phi=phi,
                        last_time=last_time, alpha=alpha, angles=angles, frame_ticks=frame_ticks, frames=frames,
                        angles_first=angles_first, start_frames=np.asarray(ref._start_frames, dtype=np.float64),
                        leg_offset=np.asarray(ref._offset, dtype=np.float64), step_offset=np.float64(ref.step_offset))


def _pose_constants(name):
    c = Robot(name).GetCtrlConstants()
    return {f"{name}_hip_leg_foot": np.array([c.hip, c.leg, c.foot], dtype=np.float64),
            f"{name}_hip_v": np.array([c.hip_front_right_v, c.hip_front_left_v, c.hip_rear_right_v, c.hip_rear_left_v], dtype=np.float64),
            f"{name}_pose_frames": np.array([[c.x_dist / 2, -c.y_dist / 2, -c.height], [c.x_dist / 2, c.y_dist / 2, -c.height],
                                             [-c.x_dist / 2, -c.y_dist / 2, -c.height], [-c.x_dist / 2, c.y_dist / 2, -c.height]]),
            f"{name}_motor_kp": np.array(Robot(name).GetMotorConstants().MOTOR_POSITION_GAINS, dtype=np.float64),
            f"{name}_motor_kd": np.array(Robot(name).GetMotorConstants().MOTOR_VELOCITY_GAINS, dtype=np.float64)}


def gen_pose():
    from robot_gym.controllers.pose.pose_controller import PoseController
    rng = np.random.default_rng(616)
    n = N_POSE
    lo = np.array([-.02, -.02, -.065, -np.pi / 4, -np.pi / 4, -np.pi / 4])   # the sliders, pose_controller.py:24-31
    hi = np.array([.02, .02, .03, np.pi / 4, np.pi / 4, np.pi / 4])
    pose = rng.uniform(lo, hi, (n, 6))
    wide = np.arange(n) >= n // 2                                          # half beyond the slider ranges
    pose[wide] = rng.uniform(3 * lo, 3 * hi, (int(wide.sum()), 6))
    pose[::17, 3:] = 0.0                                                   # pure translations
    pose[5::23, :3] = 0.0                                                  # pure rotations
    pose[0] = 0.0
    pose = f32(pose)
    ctrl = PoseController(Robot("ghost"), None)
    out = np.zeros((n, 12))
    for k in range(n):
        ctrl.update_controller_params((pose[k, :3].astype(np.float64), pose[k, 3:].astype(np.float64)))
        out[k] = np.asarray(ctrl.get_action(), dtype=np.float64)
        _check_margin(f"pose {k}")
    consts = {}
    for name in ("ghost", "k3lso"):
        consts.update(_pose_constants(name))
    _save("pose_ik.npz", pose=pose, angles=out, **consts)


def gen_motor_position():
    from robot_gym.model.robots import simple_motor
    from robot_gym.model.robots.ghost import motor_constants
    from robot_gym.core import sim_constants
    rng = np.random.default_rng(9090)
    # the model the robot builds (robot.py:40-45): POSITION mode, no torque limits
    model = simple_motor.RobotMotorModel(kp=motor_constants.MOTOR_POSITION_GAINS, kd=motor_constants.MOTOR_VELOCITY_GAINS,
                                         motor_control_mode=simple_motor.MOTOR_CONTROL_POSITION, num_motors=12)
    n, S = N_MOTOR, sim_constants.ACTION_REPEAT
    cmd = f32(rng.uniform(-1.5, 1.5, (n, 12)))
    q0 = rng.uniform(-1.5, 1.5, (n, 1, 12))
    qd = f32(rng.uniform(-8, 8, (n, S, 12))).astype(np.float64)
    q = f32(q0 + np.cumsum(qd, axis=1) * sim_constants.SIMULATION_TIME_STEP).astype(np.float64)
    tau = np.zeros((n, S, 12))
    for k in range(n):
        for s in range(S):   # the loop of Simulation.ApplyStepAction (core/simulation.py:175-179)
            tau[k, s], _ = model.convert_to_torque(cmd[k].astype(np.float64), q[k, s], qd[k, s], qd[k, s], simple_motor.MOTOR_CONTROL_POSITION)
    _save("motor_position.npz", angles=cmd, q=q, qd=qd, tau=tau, action_repeat=np.array(S),
                        motor_kp=np.asarray(motor_constants.MOTOR_POSITION_GAINS, dtype=np.float64),
                        motor_kd=np.asarray(motor_constants.MOTOR_VELOCITY_GAINS, dtype=np.float64),
                        control_mode=np.array(simple_motor.MOTOR_CONTROL_POSITION))


# ---- non-default configurations ----

CFG_T = 20            # ticks per stream
CFG_N_POSE = 32
CFG_N_MOTOR, CFG_SUBSTEPS = 4, 5
# name, (hip, leg, foot), leg_offset, step_offset, the _stream_inputs streams replayed on it.  Offsets: four different
# values, the reference's two commented-out walk sets (bezier_controller.py:30, 36), dyadic ones for the exact equalities.
CONFIGS = (
    ("asym", (0.061, 0.1123, 0.1387), (0., 0.3, 0.8, 0.55), 0.6, (3, 18, 22)),
    ("walk_dyadic", (0.052, 0.118, 0.131), (0., 0.5, 0.5, 0.), 0.625, (0, 13, 21)),
    ("dyadic_four", (0.058, 0.099, 0.152), (0., 0.25, 0.75, 0.5), 0.375, (6, 10, 23)),
    ("crossed", (0.049, 0.1207, 0.1411), (0.1, 0.6, 0., 0.45), 0.35, (2, 15, 19)),
    ("long_thigh", (0.04, 0.15, 0.12), (0.5, 0., 0.2, 0.7), 0.7, (1, 14, 20)),
    ("short_thigh", (0.07, 0.09, 0.16), (0.5, 0., 0., 0.5), 0.55, (5, 16, 17)),
)
SIGNS = np.array([[1, -1], [1, 1], [-1, -1], [-1, 1]])       # FR, FL, RR, RL: the side of x and y


def _config(i, rng):
    """Configuration i: every leg's hip vertex and both foot frames moved on their own, so no two legs mirror each other."""
    name, (hip, leg, foot), offsets, step_offset, _ = CONFIGS[i]

    def frames(x, y, z, dz):
        f = np.zeros((4, 3))
        f[:, 0] = SIGNS[:, 0] * (x / 2 + rng.uniform(-0.012, 0.012, 4))
        f[:, 1] = SIGNS[:, 1] * (y / 2 + rng.uniform(-0.012, 0.012, 4))
        f[:, 2] = z + rng.uniform(-dz, dz, 4)
        return np.round(f, 4)
    cfg = dict(hip_leg_foot=np.array([hip, leg, foot]), hip_v=frames(0.23, 0.075, 0.0, 0.006),
               pose_frames=frames(0.23, 0.185, -0.2, 0.012), start_frames=frames(0.23, 0.155, -0.22, 0.012),
               leg_offset=np.array(offsets), step_offset=np.float64(step_offset),
               motor_kp=np.round(rng.permutation(160.0 + 9.0 * np.arange(12)) + rng.uniform(0, 1, 12), 2),
               motor_kd=np.round(rng.permutation(0.7 + 0.21 * np.arange(12)) + rng.uniform(0, 0.05, 12), 3))
    if name == "crossed":
        # two start frames on the other side of the body's axis than their legs: center_to_foot[1] > 0
        # (bezier_controller.py:139) is then not a function of the leg index
        cfg["start_frames"][0, 1] = 0.021      # FR, a right leg
        cfg["start_frames"][3, 1] = -0.034     # RL, a left leg
    for k in ("motor_kp", "motor_kd"):
        assert len(set(cfg[k].tolist())) == 12
    return cfg


def _ctrl_namespace(cfg):
    """What both controllers read of robot.GetCtrlConstants().  x_dist / y_dist / height only seed PoseController._frames,
    which is replaced on the object."""
    hip, leg, foot = (float(x) for x in cfg["hip_leg_foot"])
    hv = cfg["hip_v"]
    ctrl = types.SimpleNamespace(hip=hip, leg=leg, foot=foot, x_dist=0.23, y_dist=0.185, height=0.2, hip_front_right_v=hv[0].copy(),
                                 hip_front_left_v=hv[1].copy(), hip_rear_right_v=hv[2].copy(), hip_rear_left_v=hv[3].copy())
    return types.SimpleNamespace(GetCtrlConstants=lambda: ctrl)


def _boundary_streams(cfg):
    """Three streams of CFG_T ticks whose comparisons are exact in float64 -> params, clock, reset, t0 (each [3, T, ...])."""
    T = CFG_T
    off, so = cfg["leg_offset"], float(cfg["step_offset"])
    params = np.zeros((3, T, 4))
    clock = np.zeros((3, T))
    reset = np.zeros((3, T), dtype=bool)
    t0 = np.zeros((3, T))
    # 0: period 1, clock on a grid of 1/32 with the ticks nearest to them moved onto  step_offset - offset  and
    #    1 - offset  of every leg where that sum is exact: p == step_offset and phi + offset == 1
    special = []
    for l in range(4):
        for target in (so, 1.0):
            c = target - off[l]
            if 0.0 < c < 0.98 and c + off[l] == target and c not in special:
                special.append(c)
    fill = [k / 32.0 for k in range(32) if k / 32.0 not in special]
    grid = np.array(special + fill[:T - len(special)])
    assert len(special) >= 2 and len(set(grid.tolist())) == T
    clock[0] = np.sort(grid)
    params[0] = [0.75, 30.0, 0.5, 1.0]
    # 1: a reset whose clock origin lies half a second ahead of the clock: the phase is negative for 16 ticks
    clock[1] = 2.0 + np.arange(T) / 32.0
    params[1] = [-1.0, -120.0, -0.625, 0.5]
    reset[1, 2] = True
    t0[1, 2] = clock[1, 2] + 0.5
    # 2: periods at the float32 next to the floor on either side, below it, zero and negative; zero rotation and length
    near = np.float32(0.01)
    clock[2] = 0.25 + np.arange(T) / 256.0
    params[2, :, 0] = np.where(np.arange(T) % 5 == 0, 0.0, 1.25)
    params[2, :, 1] = 90.0
    params[2, :, 2] = np.where(np.arange(T) % 3 == 0, 0.0, -0.375)
    params[2, :, 3] = np.resize([near, np.nextafter(near, np.float32(1)), 0.005, 0.0, -0.3, 0.0625], T)
    p32 = f32(params)
    assert np.array_equal(p32.astype(np.float64)[:2], params[:2])        # dyadic: nothing lost in float32
    return p32, clock, reset, t0


def _record_gait(cfg, params, clock, reset, t0, where):
    from robot_gym.controllers.bezier.bezier_controller import BezierController
    robot = _ctrl_namespace(cfg)

    def make():
        c = BezierController(robot, None)
        c._start_frames = np.asmatrix(cfg["start_frames"])
        c._offset = np.array(cfg["leg_offset"])
        c.step_offset = float(cfg["step_offset"])
        return c
    S, T = clock.shape
    out = dict(phi=np.zeros((S, T)), last_time=np.zeros((S, T)), alpha=np.zeros((S, T)), angles=np.zeros((S, T, 12), dtype=np.float32),
               frames=np.zeros((S, T, 4, 3)))
    out["angles_first"] = np.asarray(make().get_action(), dtype=np.float64)
    _check_margin(f"{where}: get_action before any update")
    for s in range(S):
        ctrl = make()
        for k in range(T):
            if reset[s, k]:
                ctrl = make()
                ctrl._last_time = float(t0[s, k])
            CLOCK.now = float(clock[s, k])
            ctrl.update_controller_params(tuple(float(x) for x in params[s, k]))
            out["angles"][s, k] = np.asarray(ctrl.get_action(), dtype=np.float64)
            out["phi"][s, k], out["last_time"][s, k], out["alpha"][s, k] = ctrl._phi, ctrl._last_time, ctrl._alpha
            out["frames"][s, k] = ctrl._frame
            _check_margin(f"{where} stream {s} tick {k}")
    return out


def _record_pose(cfg, rng, where):
    from robot_gym.controllers.pose.pose_controller import PoseController
    n = CFG_N_POSE
    lo = np.array([-.02, -.02, -.065, -np.pi / 4, -np.pi / 4, -np.pi / 4])
    hi = np.array([.02, .02, .03, np.pi / 4, np.pi / 4, np.pi / 4])
    pose = rng.uniform(lo, hi, (n, 6))
    pose[n // 2:] = rng.uniform(3 * lo, 3 * hi, (n - n // 2, 6))
    pose[3::11, 3:] = 0.0
    pose[5::13, :3] = 0.0
    pose[0] = 0.0
    pose = f32(pose)
    ctrl = PoseController(_ctrl_namespace(cfg), None)
    ctrl._frames = np.asmatrix(cfg["pose_frames"])
    out = np.zeros((n, 12))
    for k in range(n):
        ctrl.update_controller_params((pose[k, :3].astype(np.float64), pose[k, 3:].astype(np.float64)))
        out[k] = np.asarray(ctrl.get_action(), dtype=np.float64)
        _check_margin(f"{where} pose {k}")
    return pose, out


def _record_motor(cfg, rng):
    from robot_gym.model.robots import simple_motor
    from robot_gym.core import sim_constants
    model = simple_motor.RobotMotorModel(kp=list(cfg["motor_kp"]), kd=list(cfg["motor_kd"]),
                                         motor_control_mode=simple_motor.MOTOR_CONTROL_POSITION, num_motors=12)
    n, S = CFG_N_MOTOR, CFG_SUBSTEPS
    cmd = f32(rng.uniform(-1.5, 1.5, (n, 12)))
    qd = f32(rng.uniform(-8, 8, (n, S, 12)))
    q = f32(rng.uniform(-1.5, 1.5, (n, 1, 12)) + np.cumsum(qd.astype(np.float64), axis=1) * sim_constants.SIMULATION_TIME_STEP)
    tau = np.zeros((n, S, 12))
    for k in range(n):
        for s in range(S):
            tau[k, s], _ = model.convert_to_torque(cmd[k].astype(np.float64), q[k, s].astype(np.float64), qd[k, s].astype(np.float64),
                                                   qd[k, s].astype(np.float64), simple_motor.MOTOR_CONTROL_POSITION)
    return cmd, q, qd, tau


def gen_configs():
    rng = np.random.default_rng(20261017)
    arrays = dict(names=np.array([c[0] for c in CONFIGS]))
    for i, (name, _, _, _, streams) in enumerate(CONFIGS):
        cfg = _config(i, rng)
        parts = [_stream_inputs(s, rng, CFG_T) for s in streams]
        bp, bc, br, bt = _boundary_streams(cfg)
        params = np.concatenate([np.stack([p[0] for p in parts]), bp])
        clock = np.concatenate([np.stack([p[1] for p in parts]), bc])
        reset = np.concatenate([np.stack([p[2] for p in parts]), br])
        t0 = np.concatenate([np.stack([p[3] for p in parts]), bt])
        gait = _record_gait(cfg, params, clock, reset, t0, name)
        pose, pose_angles = _record_pose(cfg, rng, name)
        cmd, q, qd, tau = _record_motor(cfg, rng)
        rec = dict(cfg, params=params, clock=clock, reset=reset, t0=t0, boundary_streams=np.arange(len(parts), len(parts) + 3),
                   pose=pose, pose_angles=pose_angles, motor_cmd=cmd, motor_q=q, motor_qd=qd, motor_tau=tau, **gait)
        arrays.update({f"c{i}_{k}": np.asarray(v) for k, v in rec.items()})
    _save("posctl_configs.npz", **arrays)

if __name__ == "__main__":
    _install_hooks()
    gen_bezier(timing="--time" in sys.argv)
    gen_pose()
    gen_motor_position()
    gen_configs()
