"""Batched single-rigid-body simulator: B closed-loop robots per GPU with no host in the loop (include/rg_srb.h).

An extension -- the reference simulates in PyBullet, one process per environment.  The model is the one the MPC plans
with: one rigid body pushed by the controller's first-step ground-reaction forces at kinematic stance feet, semi-implicit
Euler, on the plane z = 0 or on a heightfield (terrain=, robot_gym_amd/sim/terrain.py: a landing foot takes the ground's
height where it lands, the fall test measures the body's clearance, a reset is followed by settle()).  It is for
closed-loop validation of the controller, branched rollouts (clone) and RL on the reduced model.  Contact is the gait
schedule (contact="schedule", the default) or measured (contact="measured", include/rg_srb_contact.h): a swinging foot that
comes to the ground stops there and reports contact, and the controller's EARLY_CONTACT rule reacts.  Late contact, a
reach limit and body collision are not measured in either mode (a foot descending at a finite speed made every robot of the
CPU model fall: rg_srb_contact.h).  The feet grip whatever the force (friction=None, the default) or the ground has a Coulomb
friction coefficient per robot (friction=, include/rg_srb_friction.h): a stance foot asked for more tangential force than mu
times its normal force passes on that much, and slides; sim.slip holds the metres each foot slid on the last tick.
The forces are delivered as planned (motors=None, the default) or pass through a motor model first (motors=MotorModel(...),
robot_gym_amd/sim/motor_model.py, include/rg_srb_motor.h): a strength ratio and a torque limit per motor.
PyTorch-ROCm is used only for device buffers and the current stream; all arithmetic
happens in librg_mpc.so.

    ctl = BatchedMPCController(B, cfg); sim = BatchedSRBSim(B, cfg)
    ctl.reset(); sim.reset()
    ctl.update_controller_params(commands)
    for _ in range(ticks):
        ctl.get_action(0.0, sim.obs)      # sim.obs carries t_robot, the per-robot clock
        sim.step(ctl)
"""
import numpy as np
import torch

from robot_gym_amd.controllers.mpc.batched import STATE_FIELDS
from robot_gym_amd.core import friction_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.sim.motor_model import MotorModel

CONTACT_MODES = ("schedule", "measured")
CONTROLLER_OUTPUTS = (("grf", 12, torch.float32), ("foot_target", 12, torch.float32), ("desired_state", 4, torch.int32))


def friction_values(friction, n, what):
    """`friction` as a float64 [n] host array: a float or "inf" for every robot, or one value per robot (array or tensor).
    Anything else is a ValueError naming `what`; no device is touched."""
    if isinstance(friction, str):
        if friction != "inf":
            raise ValueError(f"{what} must be a number, 'inf', or one value per robot, got {friction!r}")
        return np.full(n, np.inf)
    if isinstance(friction, bool):
        raise ValueError(f"{what} must be a number, 'inf', or one value per robot, got {friction!r}")
    try:
        a = np.asarray(friction.detach().cpu() if torch.is_tensor(friction) else friction, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, 'inf', or one value per robot, got {friction!r}") from None
    if a.ndim == 0:
        return np.full(n, float(a))
    if a.shape != (n,):
        raise ValueError(f"{what} must be a number, 'inf', or one value per robot ([{n}]), got shape {list(a.shape)}")
    return np.ascontiguousarray(a)


class BatchedSRBSim:
    """state: float64 [43, B] device tensor (rows: rg_srb.h); obs: the next tick's observation, a dict of component-major
    device tensors in STATE_FIELDS order plus `t_robot`, accepted by BatchedMPCController.get_action as is."""

    def __init__(self, batch, cfg: MPCConfig = None, device=None, dt_sim=0.001, substeps=10, fall_height_scale=0.5, fall_tilt=1.0,
                 terrain=None, contact="schedule", friction=None, slip_gain=friction_abi.SLIP_GAIN, slip_speed_max=friction_abi.SLIP_SPEED_MAX,
                 motors=None):
        if contact not in CONTACT_MODES:
            raise ValueError(f"contact must be one of {CONTACT_MODES}, got {contact!r}")
        # friction: None (the feet grip: nothing is allocated and step dispatches as without it), or the coefficient of every
        # robot: a float, a (B,) array or tensor, or "inf" (the friction tick with every robot gripping)
        mu0 = None if friction is None else friction_values(friction, int(batch), "friction")
        self.slip_gain, self.slip_speed_max = friction_abi.checked_settings(slip_gain, slip_speed_max)
        # motors: None (the forces are delivered as planned: nothing is allocated, nothing launched) or a MotorModel, which is bound
        # to this simulator: step then applies it to the controller's grf and steps on the delivered force
        if motors is not None and not isinstance(motors, MotorModel):
            raise ValueError(f"motors must be a MotorModel or None, got {motors!r}")
        if motors is not None:
            motors.rows(batch)
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedSRBSim needs a HIP device (no CPU fallback)")
        self.cfg = cfg or MPCConfig.for_robot("ghost")
        self.batch = int(batch)
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"BatchedSRBSim runs on a HIP device, not {dev}")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self.dt_sim, self.substeps = float(dt_sim), int(substeps)
        self._handle = srb_abi.SrbHandle(self.cfg, self.batch, self.device, dt_sim=dt_sim, substeps=substeps,
                                         fall_height_scale=fall_height_scale, fall_tilt=fall_tilt)
        B = self.batch
        self.state = torch.zeros(srb_abi.STATE_ROWS, B, dtype=torch.float64, device=self.device)
        self.obs = {name: torch.zeros(comps, B, dtype=dt, device=self.device) for name, comps, dt in STATE_FIELDS}
        self.obs["t_robot"] = torch.zeros(B, dtype=torch.float64, device=self.device)
        self._obs_ptrs = srb_abi.CObsPtrs()
        for name in srb_abi.OBS_FIELDS:
            setattr(self._obs_ptrs, name, self.obs[name].data_ptr())
        self.state[srb_abi.ROW_STATUS] = 1.0   # nothing runs before the first reset
        self.contact = contact
        # measured mode: 1 where a swung foot touched the ground on the last tick.  All zero in schedule mode.
        self.touch = torch.zeros(4, B, dtype=torch.int32, device=self.device)
        self.terrain = None
        if terrain is not None:
            self.set_terrain(terrain)
        # friction: mu float64 [B], the coefficient of each robot (+inf, NaN or negative: it grips); slip float64 [4, B], the metres
        # each foot slid on the last tick.  Both None without friction.
        self.mu = self.slip = None
        if mu0 is not None:
            self.mu = torch.as_tensor(mu0, device=self.device)
            self.slip = torch.zeros(4, B, dtype=torch.float64, device=self.device)
        self.motors = None if motors is None else motors.bind(self)

    def set_terrain(self, terrain):
        """The ground: a RandomTerrain or GridTerrain of robot_gym_amd.sim.terrain (it is bound to this batch and device and
        its tensors are kept alive here), or None for the plane.  No state changes: reset(), or settle(), afterwards."""
        if terrain is None:
            self._handle.set_terrain(None)
        else:
            self._handle.set_terrain(terrain.bind(self.batch, self.device))
        self.terrain = terrain

    def ground_height(self, xy, robot=None):
        """float64 [n] device tensor: the ground's height at xy [n,2] (a device tensor, or host values) under robot[k] (int
        [n]; None: entry k is robot k, n <= batch).  0 on the plane.  Enqueued on the current stream."""
        xy = xy if torch.is_tensor(xy) else torch.as_tensor(np.asarray(xy, dtype=np.float64))
        xy = xy.to(self.device, torch.float64)
        if xy.dim() != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError(f"ground_height: xy must be [n,2], got {list(xy.shape)}")
        n = xy.shape[0]
        cm = xy.t().contiguous()
        rp = None
        if robot is not None:
            robot = robot if torch.is_tensor(robot) else torch.as_tensor(np.asarray(robot, dtype=np.int32))
            robot = robot.to(self.device, torch.int32).contiguous()
            if tuple(robot.shape) != (n,):
                raise ValueError(f"ground_height: robot must be [{n}], got {list(robot.shape)}")
            rp = robot.data_ptr()
        out = torch.empty(n, dtype=torch.float64, device=self.device)
        self._handle.ground_height(cm.data_ptr(), rp, n, out.data_ptr())
        return out

    def settle(self, mask=None):
        """Stand the robots b with mask[b] != 0 (int32 [B] device tensor; None: all) whose status is 0 on the ground: every
        foot at the ground's height under it, the body raised by the mean of the four, the observation rewritten.  What a
        reset on a terrain ends with (reset() does it itself).  Enqueued on the current stream; nothing waits."""
        mp = None
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype != torch.int32 or tuple(mask.shape) != (self.batch,) or not mask.is_contiguous() or mask.device != self.device:
                raise ValueError(f"settle: mask must be a contiguous int32 [{self.batch}] tensor on {self.device}")
            mp = mask.data_ptr()
        self._handle.settle(self.state.data_ptr(), mp, self._obs_ptrs)

    def reset(self, idx=None, xy=None, yaw=None, height=None):
        """Robots idx (None: all) to (xy[k], height[k]) with heading yaw[k], standing: xy [n,2], yaw [n], height [n] host
        values (None: origin, 0, body_height).  On a terrain the height is above the mean ground under the four feet (the
        library settles the robots it resets).  Waits for its own small upload.  The controller is reset by its own reset."""
        if idx is not None:
            idx = np.asarray(idx.cpu() if torch.is_tensor(idx) else idx, dtype=np.int64).reshape(-1)
        n = self.batch if idx is None else len(idx)
        host = lambda a: None if a is None else np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float64)
        xy = host(xy)
        if xy is not None:
            if xy.shape != (n, 2):
                raise ValueError(f"reset: xy must be [{n},2], got {list(xy.shape)}")
            xy = np.ascontiguousarray(xy.T)
        bc = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(a, (n,)))
        self._handle.reset(self.state.data_ptr(), self._obs_ptrs, idx, xy, bc(host(yaw)), bc(host(height)))

    def set_body(self, mass=None, inertia=None, idx=None):
        """The TRUE body of robots idx (None: all): mass [n], inertia [9,n] or [n,3,3].  Both None returns every robot to
        the config's body.  The simulated body may differ from the one the planner believes in."""
        self._handle.set_body(idx, mass, inertia)

    def set_friction(self, mu, idx=None):
        """The friction coefficient of robots idx (None: all): a float, "inf", or an array or tensor with one value per robot
        named.  +inf, NaN and negative values mean the robot grips.  Needs a simulator built with friction=."""
        if self.mu is None:
            raise RuntimeError("set_friction: this simulator was built without friction (BatchedSRBSim(..., friction=...))")
        if idx is None:
            self.mu.copy_(torch.as_tensor(friction_values(mu, self.batch, "set_friction: mu"), device=self.device))
            return
        at = self._index(idx)
        self.mu[at] = torch.as_tensor(friction_values(mu, at.numel(), "set_friction: mu"), device=self.device)

    def step(self, ctl_or_outputs, ext=None):
        """One control tick from the controller's outputs of this tick: a BatchedMPCController (its `extra` tensors) or a
        dict with grf [B,12], foot_target [B,12] float32 and desired_state [B,4] int32; in measured mode leg_state [B,4] int32
        in place of desired_state (a ValueError names it when it is missing).  ext: float64 [6,B] world force and torque
        about the CoM, or None.  With friction the tick is rg_srb_step_friction in either mode, on the same outputs, and writes
        self.slip.  With a motor model the tick, whichever it is, runs on the force the motors deliver (self.motors.grf) in place of
        grf.  Enqueued on the current stream; nothing waits."""
        out = getattr(ctl_or_outputs, "extra", ctl_or_outputs)
        get = lambda name: out.get(name) if hasattr(out, "get") else None
        if self.motors is not None:
            if get("grf") is None:
                raise KeyError("step: controller output 'grf' missing (a BatchedMPCController needs extra_outputs=True)")
            planned, delivered = out, self.motors.apply(get("grf"))
            get = lambda name: delivered if name == "grf" else planned.get(name)
        if self.mu is not None:
            # the friction tick in either contact mode: it steps on leg_state (measured) or desired_state (schedule)
            measured = self.contact == "measured"
            legs = "leg_state" if measured else "desired_state"
            if get(legs) is None:
                raise ValueError(f"step: contact={self.contact!r} with friction steps on the controller's {legs!r} [B,4] int32 output, which is "
                                 "missing (a BatchedMPCController needs extra_outputs=True)")
            for name, _, _ in CONTROLLER_OUTPUTS[:2]:
                if get(name) is None:
                    raise KeyError(f"step: controller output {name!r} missing (a BatchedMPCController needs extra_outputs=True)")
            friction_abi.step_friction(self._handle, self.state, get("grf"), get("foot_target"), get(legs), int(measured), ext, self._obs_ptrs,
                                       self.mu, self.slip_gain, self.slip_speed_max, self.touch, self.slip)
            return
        if self.contact == "measured":
            if get("leg_state") is None:
                raise ValueError("step: contact='measured' steps on the controller's 'leg_state' [B,4] int32 output, which is missing "
                                 "(a BatchedMPCController needs extra_outputs=True)")
            for name, _, _ in CONTROLLER_OUTPUTS[:2]:
                if get(name) is None:
                    raise KeyError(f"step: controller output {name!r} missing (a BatchedMPCController needs extra_outputs=True)")
            self._handle.step_contact(self.state, get("grf"), get("foot_target"), get("leg_state"), ext, self._obs_ptrs, self.touch)
            return
        ptrs = []
        for name, comps, dt in CONTROLLER_OUTPUTS:
            t = get(name)
            if t is None:
                raise KeyError(f"step: controller output {name!r} missing (a BatchedMPCController needs extra_outputs=True)")
            if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (self.batch, comps) or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"step: {name} must be a contiguous {dt} [{self.batch},{comps}] tensor on {self.device}")
            ptrs.append(t.data_ptr())
        ext_ptr = None
        if ext is not None:
            if not torch.is_tensor(ext) or ext.dtype != torch.float64 or tuple(ext.shape) != (6, self.batch) or not ext.is_contiguous() or ext.device != self.device:
                raise ValueError(f"step: ext must be a contiguous float64 [6,{self.batch}] tensor on {self.device}")
            ext_ptr = ext.data_ptr()
        self._handle.step(self.state.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ext_ptr, self._obs_ptrs)

    def fallen(self):
        """bool [B] device tensor: robots whose status is not 0 (fallen, or never reset)."""
        return self.state[srb_abi.ROW_STATUS] != 0

    def _index(self, idx):
        """idx as an int64 tensor on this device; one that already is such a tensor is taken as it is (no host copy)."""
        if torch.is_tensor(idx) and idx.device == self.device and idx.dtype == torch.int64:
            return idx.reshape(-1)
        if torch.is_tensor(idx):
            return idx.to(self.device, torch.int64).reshape(-1)
        return torch.as_tensor(np.asarray(idx, dtype=np.int64).reshape(-1), device=self.device)

    def copy_columns(self, src_idx, dst_idx):
        """State, observation and (random terrain) world key of robot src_idx[k] into robot dst_idx[k], on the GPU (all sources read first).  With int64
        index tensors of this device nothing touches the host; host indices cost one blocking upload each."""
        src, dst = self._index(src_idx), self._index(dst_idx)
        if src.numel() != dst.numel():
            raise ValueError("copy_columns: src and dst differ in length")
        self.state.index_copy_(1, dst, self.state.index_select(1, src))
        for t in list(self.obs.values()) + [self.touch] + ([] if self.mu is None else [self.mu, self.slip]):   # the floor a robot walks on goes with it
            t.index_copy_(t.dim() - 1, dst, t.index_select(t.dim() - 1, src))
        if self.motors is not None:   # and so do its motors
            self.motors.copy_columns(src, dst)
        keys = getattr(self.terrain, "keys", None)
        if keys is not None:   # the world a robot walks in goes with it
            keys.index_copy_(0, dst, keys.index_select(0, src))

    def close(self):
        self._handle.close()


def rollout(ctl, sim, commands=None, ticks=1, record_every=0, ext=None, on_tick=None, estimator=None):
    """The closed loop ctl.get_action(0.0, sim.obs) -> sim.step(ctl) for `ticks` control ticks on the current stream, with no
    synchronisation inside.  commands: [B,2] (vx, wz) or [B,3] (vx, vy, wz) for update_controller_params, a callable of the
    tick returning such values (or None: keep), or None (the controller keeps the command it has).  ext: None, a [6,B]
    float64 tensor, or a callable of the tick returning one or None (random pushes from a DomainRandomizer bound to this
    simulator: ext=lambda k: dr.pushes()).  on_tick: a callable of the tick, called after each tick (a
    test reads the solver statistics of every tick with it; what it does is the caller's, a wait included).  estimator: a
    StateEstimator (robot_gym_amd/sim/state_estimator.py) bound to this simulator, or None: with one the controller is given
    estimator.estimate() instead of sim.obs (reset it with estimator.on_reset() after sim.reset()).  Returns (final state [43,B], trajectory): the
    trajectory is None, or with record_every = n > 0 the states after ticks n, 2n, ... as one [T,43,B] device tensor."""
    if commands is not None and not callable(commands):
        ctl.update_controller_params(commands)
    traj = []
    for k in range(int(ticks)):
        if callable(commands):
            c = commands(k)
            if c is not None:
                ctl.update_controller_params(c)
        ctl.get_action(0.0, sim.obs if estimator is None else estimator.estimate())
        sim.step(ctl, ext(k) if callable(ext) else ext)
        if record_every and (k + 1) % record_every == 0:
            traj.append(sim.state.clone())
        if on_tick is not None:
            on_tick(k)
    return sim.state.clone(), (torch.stack(traj) if traj else None)


def clone(ctl, sim, src, dst, estimator=None):
    """Branch rollouts: controller state (ctl.copy_state), simulation state and observation of robot src[k] into robot
    dst[k].  For bit-identical continuations keep dst = src modulo 16 (rg_mpc.h, direct routing).  rg_mpc_copy_state takes host
    index lists, so src / dst given as device tensors are read back for it once.  estimator: the StateEstimator bound to this
    simulator, or None; its columns go with the robot."""
    host = lambda i: i.cpu().numpy() if torch.is_tensor(i) else i
    ctl.copy_state(host(src), host(dst))
    sim.copy_columns(src, dst)
    if estimator is not None:
        estimator.copy_columns(src, dst)
