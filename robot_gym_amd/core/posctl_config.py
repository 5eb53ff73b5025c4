"""Configuration of the position-mode controllers (include/rg_posctl.h, rg_posctl_config).

Values restate the reference modules cited per field:
  ctrl   robot_gym/model/robots/<robot>/ctrl_constants.py:43-62 (the "Pose Controller" section; ghost and k3lso agree)
  motor  robot_gym/model/robots/<robot>/motor_constants.py:13-15
  bezier robot_gym/controllers/bezier/bezier_controller.py:21-40 (instance attributes of BezierController)
"""
from dataclasses import dataclass, fields
from typing import Tuple


def _frames(x_dist, y_dist, height):
    """Foot frames (FR, FL, RR, RL) the way both controllers build them: (+-x_dist/2, -+y_dist/2, -height)."""
    return (x_dist / 2, -y_dist / 2, -height, x_dist / 2, y_dist / 2, -height,
            -x_dist / 2, -y_dist / 2, -height, -x_dist / 2, y_dist / 2, -height)


def _hip_vertices(l, w):
    """hip_front_right_v .. hip_rear_left_v (ctrl_constants.py:55-58): (+-l/2, -+w/2, 0)."""
    return (l / 2, -w / 2, 0.0, l / 2, w / 2, 0.0, -l / 2, -w / 2, 0.0, -l / 2, w / 2, 0.0)


# BezierController's own body box (bezier_controller.py:21-24), not the ctrl constants
BEZIER_X_DIST, BEZIER_Y_DIST, BEZIER_HEIGHT = 0.23, 0.155, 0.22

# ctrl_constants.py:46-53, identical for ghost and k3lso
_POSE = {
    "ghost": dict(l=0.23, w=0.075, hip=0.055, leg=0.10652, foot=0.145, y_dist=0.185, x_dist=0.23, height=0.2),
    "k3lso": dict(l=0.23, w=0.075, hip=0.055, leg=0.10652, foot=0.145, y_dist=0.185, x_dist=0.23, height=0.2),
}
# motor_constants.py:13, :15 (ghost and k3lso)
_MOTOR = {
    "ghost": dict(kp=(220.0,) * 12, kd=(1.0, 2.0, 2.0) * 4),
    "k3lso": dict(kp=(220.0,) * 12, kd=(1.0, 2.0, 2.0) * 4),
}


@dataclass
class PosCtlConfig:
    hip: float = 0.055
    leg: float = 0.10652
    foot: float = 0.145
    hip_v: Tuple[float, ...] = _hip_vertices(0.23, 0.075)
    pose_frames: Tuple[float, ...] = _frames(0.23, 0.185, 0.2)
    start_frames: Tuple[float, ...] = _frames(BEZIER_X_DIST, BEZIER_Y_DIST, BEZIER_HEIGHT)
    leg_offset: Tuple[float, ...] = (0.0, 0.0, 0.8, 0.8)   # bezier_controller.py:39
    step_offset: float = 0.5                               # :40
    motor_kp: Tuple[float, ...] = (220.0,) * 12
    motor_kd: Tuple[float, ...] = (1.0, 2.0, 2.0) * 4

    @classmethod
    def for_robot(cls, robot="ghost", **overrides):
        if robot not in _POSE:
            raise KeyError(f"unknown robot {robot!r}; known: {sorted(_POSE)}")
        p, m = _POSE[robot], _MOTOR[robot]
        cfg = cls(hip=p["hip"], leg=p["leg"], foot=p["foot"], hip_v=_hip_vertices(p["l"], p["w"]),
                  pose_frames=_frames(p["x_dist"], p["y_dist"], p["height"]), motor_kp=m["kp"], motor_kd=m["kd"])
        for k, v in overrides.items():
            if k not in {f.name for f in fields(cls)}:
                raise AttributeError(f"PosCtlConfig has no field {k!r}")
            setattr(cfg, k, v)
        return cfg


def config_from_robot(robot, **overrides):
    """PosCtlConfig from the live robot's constant modules -- what the reference controllers read at construction
    (GetCtrlConstants: bezier_controller.py:15, pose_controller.py:13) and the motor model's gains (GetMotorConstants)."""
    ctrl, motor = robot.GetCtrlConstants(), robot.GetMotorConstants()
    hip_v = tuple(float(x) for name in ("hip_front_right_v", "hip_front_left_v", "hip_rear_right_v", "hip_rear_left_v")
                  for x in getattr(ctrl, name))
    cfg = PosCtlConfig(hip=float(ctrl.hip), leg=float(ctrl.leg), foot=float(ctrl.foot), hip_v=hip_v,
                       pose_frames=_frames(float(ctrl.x_dist), float(ctrl.y_dist), float(ctrl.height)),
                       motor_kp=tuple(float(x) for x in motor.MOTOR_POSITION_GAINS),
                       motor_kd=tuple(float(x) for x in motor.MOTOR_VELOCITY_GAINS))
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg
