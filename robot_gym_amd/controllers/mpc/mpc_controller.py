"""Drop-in `MPCController` for the reference's PyBullet environments (batch = 1 plumbing).

Same plugin surface as the reference class (robot_gym/controllers/mpc/mpc_controller.py:14-113):
class attribute MOTOR_CONTROL_MODE, __init__(robot, get_time_since_reset), kinematics_model,
setup_ui_params / read_ui_params, update_controller_params, get_action, reset,
get_standing_action.  Instead of driving the third-party Python/C++ stack per robot it pushes
the robot's state through the HIP controller with B = 1; registering it under
robot_gym/util/cli/mapper.py:7-9 makes it selectable.
"""
import numpy as np
import torch

from robot_gym_amd.controllers.controller import Controller
from robot_gym_amd.controllers.mpc.batched import BatchedMPCController, PackedState
from robot_gym_amd.controllers.mpc.kinematics import ChainKinematics, PybulletKinematics
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.model.robots.robot_constants import ROBOTS

MOTOR_CONTROL_HYBRID = 3  # reference model/robots/simple_motor.py:11


def config_from_robot(robot, robot_name=None, **overrides):
    """MPCConfig from the live robot's constant modules, i.e. the values the reference reads in
    _setup_controller (mpc_controller.py:28-66) -- GetCtrlConstants / GetConstants / GetMotorConstants."""
    ctrl, geom, motor = robot.GetCtrlConstants(), robot.GetConstants(), robot.GetMotorConstants()
    if robot_name is None:
        hips = tuple(tuple(float(v) for v in p) for p in geom.DEFAULT_HIP_POSITIONS)
        robot_name = next((n for n, rc in ROBOTS.items() if tuple(tuple(float(v) for v in p) for p in rc.default_hip_positions) == hips), "ghost")
    cfg = MPCConfig.for_robot(robot_name)
    cfg.mass = float(ctrl.MPC_BODY_MASS)
    cfg.inertia = tuple(float(x) for x in ctrl.MPC_BODY_INERTIA)
    cfg.body_height = float(ctrl.MPC_BODY_HEIGHT)
    cfg.stance_duration = tuple(float(x) for x in ctrl.STANCE_DURATION_SECONDS)
    cfg.duty_factor = tuple(float(x) for x in ctrl.DUTY_FACTOR)
    cfg.init_phase = tuple(float(x) for x in ctrl.INIT_PHASE_FULL_CYCLE)
    cfg.init_state = tuple(int(getattr(s, "value", s)) for s in ctrl.INIT_LEG_STATE)
    cfg.vx_offset, cfg.vy_offset, cfg.wz_offset = float(ctrl.VX_OFFSET), float(ctrl.VY_OFFSET), float(ctrl.WZ_OFFSET)
    cfg.hip = tuple(float(v) for p in geom.DEFAULT_HIP_POSITIONS for v in p)
    cfg.motor_kp = tuple(float(x) for x in motor.MOTOR_POSITION_GAINS)
    cfg.motor_kd = tuple(float(x) for x in motor.MOTOR_VELOCITY_GAINS)
    cfg.motor_dir = tuple(float(x) for x in motor.MOTOR_DIRECTION)
    cfg.motor_off = tuple(float(x) for x in motor.MOTOR_OFFSET)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


class MPCController(Controller):
    MOTOR_CONTROL_MODE = MOTOR_CONTROL_HYBRID

    def __init__(self, robot, get_time_since_reset, device=None, config=None, zero_copy=True):
        """zero_copy (default): the tick's kernels read the robot's state from the pinned host slab and write the action row
        into pinned host memory themselves (BatchedMPCController.bind_host_state); False: one upload, the launches, one
        download (rg_mpc_step_host)."""
        super().__init__(robot, get_time_since_reset)
        self._cfg = config or config_from_robot(robot)
        self._chain = ChainKinematics(self._cfg)
        self._kinematics = PybulletKinematics(robot, self._chain)
        self._batched = BatchedMPCController(1, self._cfg, device=device, extra_outputs=True)
        self._dev = self._batched.device
        self._state = PackedState(1, self._dev)     # one pinned slab: one H2D copy per tick instead of eight
        self._host = {n: t.numpy() for n, t in self._state.host.items()}
        self._act_host = torch.zeros(1, 60, dtype=torch.float32, pin_memory=True)
        self._batched.bind_host_state(self._state, self._act_host, zero_copy=zero_copy)   # per tick: one call across the C-ABI
        self._act_np = self._act_host[0].numpy()
        # column views of the one robot's slab entries, made once (batch 1: every field's column is contiguous)
        self._col = {n: a[:, 0] for n, a in self._host.items()}
        self._jac_view = self._host["jac"][:, 0].reshape(4, 3, 3)
        self.update_controller_params((0.0, 0.0, 0.0))

    @property
    def kinematics_model(self):
        return self._kinematics

    @staticmethod
    def setup_ui_params(pybullet_client):
        return tuple(pybullet_client.addUserDebugParameter(n, -2., 2., 0.) for n in ("Vx", "Vy", "Wz"))

    @staticmethod
    def read_ui_params(pybullet_client, ui):
        return tuple(pybullet_client.readUserDebugParameter(i) for i in ui)

    def update_controller_params(self, params):
        if len(params) not in (2, 3):
            raise ValueError("params must be (vx, wz) or (vx, vy, wz)")
        self._batched.update_controller_params(torch.tensor([list(map(float, params))], dtype=torch.float32))

    def _gather_state(self):
        rb, c = self._robot, self._col
        c["rpy"][:] = rb.GetBaseRollPitchYaw()
        c["rpy_rate"][:] = rb.GetBaseRollPitchYawRate()
        c["v_world"][:] = rb.GetBaseVelocity()
        c["quat"][:] = rb.GetTrueBaseOrientation()
        c["q"][:] = rb.GetMotorAngles()
        c["foot_pos"][:] = np.asarray(rb.GetFootPositionsInBaseFrame(), dtype=np.float32).reshape(12)
        self._kinematics.all_leg_jacobians(self._jac_view)
        c["contact"][:] = rb.GetFootContacts()

    def get_action(self):
        self._gather_state()                                             # the robot's getters into the pinned slab
        self._batched.get_action_host(self.get_time_since_reset())       # upload, the tick's launches, download, wait
        return self._act_np.copy()

    def reset(self):
        self._batched.reset(None, t0=self.get_time_since_reset())

    def save_state(self):
        """This robot's controller state (a one-row ControllerState; include/rg_mpc.h "State rows") -- what copy.deepcopy of
        the reference's controller would keep, to pair with PyBullet's saveState."""
        return self._batched.save_state()

    def load_state(self, state, clock_shift=None):
        """Restore a one-row ControllerState -- saved from this controller, or robot k of a batched controller
        (`state.select([k])`) -- e.g. after PyBullet's restoreState.  clock_shift: added to the saved reset time when this
        controller's clock (get_time_since_reset) runs shifted against the one the state was saved under."""
        if len(state) != 1:
            raise ValueError(f"MPCController.load_state: one row expected, got {len(state)}")
        self._batched.load_state(state, idx=[0], clock_shift=clock_shift)

    @staticmethod
    def get_standing_action():
        return 0., 0.
