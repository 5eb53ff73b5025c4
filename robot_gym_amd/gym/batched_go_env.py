"""The go-to-target task for B closed-loop robots on one GPU: controller, simulator and task with no host in the loop.

The reference's GoEnv (gym/envs/go_to/go_env.py) per robot: a planned path to a target, a 2 * num_cam_pts observation of
the path seen through a trapezoidal window in the robot's frame, the action (vx, wz), a progress / track-error reward and
six termination causes (include/rg_goto.h).  The planner and the path builder run on the host at a reset
(robot_gym_amd/gym/goto_path.py); a step is four launches on the current stream and nothing else:

    env = BatchedGoEnv(B, cfg)                # cfg None: ghost with its command offsets zeroed (see __init__)
    obs = env.reset()                         # [B, 16] float32 device tensor
    obs, reward, done = env.step(action)      # action [B, 2] (vx, wz) device tensor; no synchronisation, no host copy

obs, reward and done are views of buffers the next step overwrites.  By default there is no auto-reset: a done robot stays
frozen (reward 0, done 1, its last observation) until reset(idx) -- host work -- or reset_on_device() -- none.

    env = BatchedGoEnv(B, cfg, auto_reset=True)   # step() resets finished robots on the device (include/rg_episode.h)
    obs, reward, done = env.step(action)          # the usual vector-env contract: on the tick a robot finishes, reward and
                                                  # done are the terminal ones, obs is the first observation of its next
                                                  # episode and env.final_obs holds the terminal one

    env = BatchedGoEnv(B, cfg, terrain=RandomTerrain(), height_scan=HeightScan())   # robot_gym_amd/sim/height_scan.py
    env.obs                                       # [B, 16 + 48]: the path columns as they are without the scan, then the
                                                  # height of the body above the ground under 48 points around the robot

    env = BatchedGoEnv(B, cfg, terrain=RandomTerrain(), auto_reset=True,             # robot_gym_amd/sim/randomizer.py: per episode a
                       randomizer=DomainRandomizer(mass_scale=(0.8, 1.2), new_world_each_episode=True))   # true body and a world, drawn on the device

    env = BatchedGoEnv(B, cfg, auto_reset=True, sensor_model=SensorModel(path=dict(noise_sigma=0.005), obs_delay=(0, 2), act_delay=(0, 1)))
    env.obs, env.final_obs                        # robot_gym_amd/sim/sensor_model.py: what the sensors DELIVER (noise, bias, dropout,
    env.true_obs, env.true_final_obs              # latency); the buffers the task and scan kernels write stay clean

    env = BatchedGoEnv(B, cfg, auto_reset=True, state_estimator=StateEstimator(imu=dict(bias_half_width=(0.03, 0.03, 0.0)),
                                                                               contact=dict(rise_ticks=2, miss_probability=0.02)))
    env.est_obs                                   # robot_gym_amd/sim/state_estimator.py: what the CONTROLLER is given (IMU, gyro, velocity,
                                                  # encoder and foot-switch errors); env.sim.obs stays the truth
"""
import numpy as np
import torch

from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
from robot_gym_amd.core import episode_abi, goto_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.gym import goto_path
from robot_gym_amd.sim.srb import BatchedSRBSim


class BatchedGoEnv:
    """Owns ctl (BatchedMPCController), sim (BatchedSRBSim) and the task (goto_abi.GotoHandle) with its buffers:
    task_state float64 [50, B], the path slab (path_x / path_y / path_s float64 [B, n_max], path_first_same_x int32
    [B, n_max], path_hdr float64 [4, B]) and the outputs; and the episode reset on the device (episode_abi.EpisodeHandle)
    with episode_state float64 [12, B] (rows: rg_episode.h), final_obs and reset_mask int32 [B] (the robots the last
    reset_on_device reset).  episode_settings: planner settings of episode_abi.DEFAULTS other than the seed; they govern BOTH
    resets: reset() plans on the host with them (goto_path.plan_path / build_path), reset_on_device() on the device.
    height_scan: a HeightScan (robot_gym_amd/sim/height_scan.py) or None; with one, N = height_scan.num_points rows follow the path
    rows of obs and final_obs (one more launch per step, two under auto_reset, and one elementwise op for the mask of the robots
    that were not done before the tick: a done robot is frozen and keeps its scan rows too); without one, N = 0 and nothing changes.
    randomizer: a DomainRandomizer (robot_gym_amd/sim/randomizer.py) or None; with one, each reset (host or device) draws the
    robot's true body and, if asked, its world, and each step pushes (one more launch per reset, one per step with pushes on).
    sensor_model: a SensorModel (robot_gym_amd/sim/sensor_model.py) or None; with one, obs and final_obs are what the sensors deliver
    (true_obs and true_final_obs stay what the task and scan wrote) and the action passes through the actuator model before
    pre_step (two more launches per step, three under auto_reset); without one nothing changes.
    state_estimator: a StateEstimator (robot_gym_amd/sim/state_estimator.py) or None; with one, the controller is given est_obs, the
    estimator's view of sim.obs, instead of sim.obs (one more launch per step, one per reset); the simulator, the task, the scan
    and the sensor model keep reading the true state; without one nothing changes."""

    def __init__(self, batch, cfg: MPCConfig = None, targets=None, obstacles=None, seed=0, device=None, sim_settings=None, auto_reset=False,
                 episode_settings=None, terrain=None, contact="schedule", height_scan=None, randomizer=None, sensor_model=None, state_estimator=None,
                 friction=None, motor_model=None, **task):
        # The default robot is ghost WITH ITS COMMAND OFFSETS ZEROED: vy_offset / wz_offset trim a drift of the reference's
        # PyBullet robot that the reduced model does not have, and with them a straight command walks a curve off the path.
        # A cfg passed in is taken as it is, offsets included.
        self.cfg = cfg or MPCConfig.for_robot("ghost", vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
        self.batch = B = int(batch)
        self.ctl = BatchedMPCController(B, self.cfg, device=device)
        self.device = dev = self.ctl.device
        # terrain: a RandomTerrain / GridTerrain (robot_gym_amd/sim/terrain.py) or None, the plane.  The planner, the path and the
        # task see x and y only; the simulator stands every reset robot on the ground (sim.settle) before the task observes.
        # contact: "schedule" or "measured" (BatchedSRBSim): measured stops a swinging foot at the ground; a reset robot stands on
        # four feet either way, so the reset paths are the same.
        # friction: None (the feet grip) or the ground's friction coefficient (BatchedSRBSim: a float, one value per robot, or
        # "inf"); a DomainRandomizer(friction=(lo, hi)) draws it per episode.  An explicit keyword, not one of sim_settings, which
        # also feeds the episode handle.  A reset leaves a robot's coefficient as it is.
        # motor_model: None (forces are delivered as planned) or a MotorModel (robot_gym_amd/sim/motor_model.py), passed on like
        # friction; it lives in the simulator (env.sim.motors), so clone and the rollouts carry it with no argument of their own;
        # a DomainRandomizer(motor_strength=(lo, hi)) draws its strengths per episode.  A reset leaves a robot's motors as they are.
        self.sim = BatchedSRBSim(B, self.cfg, device=dev, terrain=terrain, contact=contact, friction=friction, motors=motor_model,
                                 **(sim_settings or {}))
        task.setdefault("dt_sim", self.sim.dt_sim)
        task.setdefault("substeps", self.sim.substeps)
        self._handle = goto_abi.GotoHandle(B, self.cfg, dev, **task)
        self.fields = self._handle.fields
        self.num_cam_pts, self.n_max = int(self.fields["num_cam_pts"]), int(self.fields["n_max"])
        self.task_state = torch.zeros(goto_abi.STATE_ROWS, B, dtype=torch.float64, device=dev)
        self.path_x = torch.zeros(B, self.n_max, dtype=torch.float64, device=dev)
        self.path_y = torch.zeros_like(self.path_x)
        self.path_s = torch.zeros_like(self.path_x)
        self.path_first_same_x = torch.zeros(B, self.n_max, dtype=torch.int32, device=dev)
        self.path_hdr = torch.zeros(goto_abi.HDR_ROWS, B, dtype=torch.float64, device=dev)
        self._paths = goto_abi.CPathPtrs(self.path_x.data_ptr(), self.path_y.data_ptr(), self.path_s.data_ptr(),
                                         self.path_first_same_x.data_ptr(), self.path_hdr.data_ptr())
        # component-major, as the kernels write it: the task and episode kernels address rows with stride B and write the path rows
        # 0 .. 2 * num_cam_pts - 1; the scan rows, if any, lie below them
        self.height_scan = height_scan
        self._scan_rows = 0 if height_scan is None else height_scan.num_points
        self._obs_cm = torch.zeros(2 * self.num_cam_pts + self._scan_rows, B, dtype=torch.float32, device=dev)
        self.reward = torch.zeros(B, dtype=torch.float32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        # the offset-corrected command goes straight into the tensor the controller reads with the state
        self.sim.obs["cmd"] = self.cmd = torch.zeros(3, B, dtype=torch.float32, device=dev)
        self._rng = np.random.default_rng(seed)
        self._fixed_targets = None if targets is None else np.asarray(targets, dtype=np.float64).reshape(-1, 2)
        self.obstacles = () if obstacles is None else obstacles
        self.targets = np.zeros((B, 2))
        self.paths = [None] * B
        self.auto_reset = bool(auto_reset)
        self._episode = episode_abi.EpisodeHandle(B, self.cfg, dev, obstacles=self.obstacles, sim_settings=sim_settings, task_settings=task,
                                                  seed=seed, **(episode_settings or {}))
        self.episode_state = torch.zeros(episode_abi.ROWS, B, dtype=torch.float64, device=dev)
        self.episode_state[episode_abi.ROW_KEY] = torch.arange(B, dtype=torch.float64, device=dev)   # the robot's key in the target stream
        self._final_obs_cm = torch.zeros_like(self._obs_cm)
        if height_scan is not None:
            height_scan.bind(self.sim)
            self._scan_obs, self._scan_final = self._obs_cm[2 * self.num_cam_pts:], self._final_obs_cm[2 * self.num_cam_pts:]
            # the robots whose scan a step takes: those not done BEFORE the tick.  A done robot is frozen (rg_goto.h, 5.): the task
            # latches its path rows, but the simulator goes on integrating it, so its scan rows are kept by leaving it out here
            self._live = torch.ones(B, dtype=torch.int32, device=dev)
        self.reset_mask = torch.zeros(B, dtype=torch.int32, device=dev)
        # randomizer: a DomainRandomizer (robot_gym_amd/sim/randomizer.py) or None.  With one, every reset draws the robot's true
        # body (and world) before the simulator stands it up, and every step pushes; without one nothing changes.
        self.randomizer = randomizer
        if randomizer is not None:
            randomizer.bind(self.sim)
        # sensor_model: a SensorModel or None.  The task and scan kernels keep writing _obs_cm and _final_obs_cm, which must stay
        # clean (the path observation latches its previous value); the model writes buffers of its own, which obs and final_obs show.
        self.sensor_model = sensor_model
        if sensor_model is not None:
            rows = 2 * self.num_cam_pts
            sensor_model.bind(B, dev, rows + self._scan_rows, 2, path_rows=(0, rows), scan_rows=(rows, rows + self._scan_rows))
        # state_estimator: a StateEstimator or None.  It stands between sim.obs and the controller only; the simulator reads its own
        # buffers back, so they stay clean and the estimate goes to tensors of the estimator's.
        self.state_estimator = state_estimator
        if state_estimator is not None:
            state_estimator.bind(self.sim)
        # the constructor's targets as a per-robot device table, uploaded once
        self._target_table = None
        if self._fixed_targets is not None:
            tab = self._fixed_targets[np.arange(B) % len(self._fixed_targets)]
            self._target_table = torch.as_tensor(np.ascontiguousarray(tab.T), device=dev)
        self._mirrors_stale = False

    @property
    def obs(self):
        """[B, 2 * num_cam_pts + N] view of the observation buffer: with a sensor model, of what it delivers."""
        return self._obs_cm.t() if self.sensor_model is None else self.sensor_model.obs_out.t()

    @property
    def est_obs(self):
        """The dict of component-major tensors the controller was given on the last step: the state estimator's; sim.obs itself
        without one."""
        return self.sim.obs if self.state_estimator is None else self.state_estimator.obs

    @property
    def true_obs(self):
        """[B, 2 * num_cam_pts + N] view of the observation the task and scan kernels wrote; obs itself without a sensor model."""
        return self._obs_cm.t()

    @property
    def true_final_obs(self):
        """[B, 2 * num_cam_pts + N] view: final_obs as the task and scan kernels wrote it."""
        return self._final_obs_cm.t()

    @property
    def final_obs(self):
        """[B, 2 * num_cam_pts + N] view: the observation each robot had before its last reset on the device (the terminal one);
        with a sensor model, the one it delivered."""
        return self._final_obs_cm.t() if self.sensor_model is None else self.sensor_model.final_obs.t()

    @property
    def episode_count(self):
        """int64 [B]: resets on the device each robot has had."""
        return self.episode_state[episode_abi.ROW_EPISODE].to(torch.int64)

    @property
    def last_return(self):
        """float64 [B]: return of the episode each robot ended last (latched at its reset on the device)."""
        return self.episode_state[episode_abi.ROW_LAST_RETURN]

    @property
    def last_length(self):
        """int64 [B]: ticks of that episode."""
        return self.episode_state[episode_abi.ROW_LAST_LENGTH].to(torch.int64)

    @property
    def last_reason(self):
        """int64 [B]: RG_GOTO_REASON_* of that episode."""
        return self.episode_state[episode_abi.ROW_LAST_REASON].to(torch.int64)

    @property
    def plan_status(self):
        """int64 [B]: RG_EPISODE_PLAN_* of each robot's last reset on the device (episode_abi.PLAN_STATUS names them); a robot
        whose plan failed was not reset and stays done."""
        return self.episode_state[episode_abi.ROW_PLAN_STATUS].to(torch.int64)

    @property
    def done_reason(self):
        """int64 [B] device tensor of RG_GOTO_REASON_* codes (goto_abi.REASONS names them)."""
        return self.task_state[goto_abi.ROW_REASON].to(torch.int64)

    @property
    def observation_space_bounds(self):
        """(low, high) of GoEnv's observation box, [2 * num_cam_pts] each (go_env.py:105-108), then per scan point
        -|clip * scale| and |clip * scale| (infinite where the scan does not clip)."""
        low, high = [0.0, -0.2] * self.num_cam_pts, [0.3, 0.2] * self.num_cam_pts
        if self.height_scan is not None:
            edge = abs(self.height_scan.clip * self.height_scan.scale) if self.height_scan.clip > 0 else np.inf
            low, high = low + [-edge] * self._scan_rows, high + [edge] * self._scan_rows
        return (np.array(low, dtype=np.float32), np.array(high, dtype=np.float32))

    @property
    def action_space_bounds(self):
        return (np.array(self.fields["action_low"], dtype=np.float32), np.array(self.fields["action_high"], dtype=np.float32))

    def reset(self, idx=None, targets=None):
        """Robots idx (None: all): plan and build a path to targets [n,2] (None: the constructor's targets, cycled over the
        robots, or random ones as go_env.py:163-175) under the planner settings of episode_settings, upload it, put the robot
        at the path's start facing along it, reset the controller, and observe.  A plan the device would refuse (rg_episode.h,
        d.) is a ValueError here, before anything is written.  Host work and blocking copies; returns obs [B, 2 * num_cam_pts + N]."""
        B = self.batch
        idx = np.arange(B) if idx is None else np.asarray(idx.cpu() if torch.is_tensor(idx) else idx, dtype=np.int64).reshape(-1)
        n = len(idx)
        if n == 0:
            return self.obs
        if targets is not None:
            tg = np.asarray(targets.cpu() if torch.is_tensor(targets) else targets, dtype=np.float64).reshape(-1, 2)
            if len(tg) != n:
                raise ValueError(f"reset: {len(tg)} targets for {n} robots")
        elif self._fixed_targets is not None:
            tg = self._fixed_targets[idx % len(self._fixed_targets)]
        else:
            tg = np.array([goto_path.random_target(self._rng) for _ in range(n)])
        cache = {}
        built = []
        ef = self._episode.fields   # the planner settings the device reset plans with: both resets plan the same path
        plan = {k: ef[k] for k in ("kp", "eta", "area_width", "grid", "robot_radius", "oscillation_length", "max_waypoints")}
        for t in tg:
            key = (float(t[0]), float(t[1]))
            if key not in cache:
                cache[key] = goto_path.build_path(goto_path.plan_path(key, self.obstacles, **plan), int(self.fields["num_checkpoints"]), target=key,
                                                  spacing=ef["spacing"], n_max=self.n_max)
            built.append(cache[key])
        for k, b in enumerate(idx):
            self.paths[b], self.targets[b] = built[k], tg[k]
        rows = goto_path.pack_paths(built, self.n_max)
        whole = n == B and np.array_equal(idx, np.arange(B))
        self._mirrors_stale = self._mirrors_stale and not whole
        running = [episode_abi.ROW_RETURN, episode_abi.ROW_LENGTH, episode_abi.ROW_ENDED]   # a new episode: nothing accumulated yet
        if whole:
            self.episode_state[running] = 0.0
        else:
            self.episode_state[torch.as_tensor(running, device=self.device)[:, None], torch.as_tensor(idx, device=self.device)[None, :]] = 0.0
        self._handle.set_path(self._paths, self.task_state.data_ptr(), None if whole else idx, **rows)
        if self.randomizer is not None:
            # before the simulator's reset: its own settle then stands the robot in the world drawn here
            drawn = torch.zeros(B, dtype=torch.int32, device=self.device)
            drawn[torch.as_tensor(idx, device=self.device)] = 1
            self.randomizer.on_reset(drawn)
        self.sim.reset(None if whole else idx, xy=np.array([p.start_xy for p in built]), yaw=np.array([p.start_angle for p in built]))
        self.ctl.reset(None if whole else idx)
        if self.state_estimator is not None:
            self.state_estimator.on_reset(None if whole else idx)
        self._handle.observe(self.task_state.data_ptr(), self.sim.state.data_ptr(), self._paths, self._obs_cm.data_ptr())
        if self.height_scan is not None:
            # set_path cleared the done flag of the robots it was given; a done robot outside idx keeps its last scan
            self.height_scan.observe(self.sim.state, out=self._scan_obs, mask=torch.eq(self.task_state[goto_abi.ROW_DONE], 0.0, out=self._live))
        if self.sensor_model is not None:
            fresh = torch.zeros(B, dtype=torch.int32, device=self.device)
            fresh[torch.as_tensor(idx, device=self.device)] = 1
            self.sensor_model.on_reset(fresh, self._obs_cm)
        return self.obs

    def step(self, action):
        """action: [B,2] (vx, wz) float32 tensor on this device.  pre_step -> controller -> simulator -> post_step on the
        current stream.  Returns (obs [B, 2 * num_cam_pts + N], reward [B], done [B] int32)."""
        if not torch.is_tensor(action) or tuple(action.shape) != (self.batch, 2) or action.device != self.device:
            raise ValueError(f"step: action must be a [{self.batch},2] tensor on {self.device}")
        if action.dtype != torch.float32 or not action.is_contiguous():
            action = action.to(torch.float32).contiguous()   # the kernel reads the rows as they are: a float32 action costs no torch op
        if self.sensor_model is not None:
            action = self.sensor_model.act(action)   # noise and latency; pre_step clips what arrives to the action box
        ts, ss = self.task_state.data_ptr(), self.sim.state.data_ptr()
        if self.height_scan is not None:
            torch.eq(self.task_state[goto_abi.ROW_DONE], 0.0, out=self._live)   # before post_step sets the flag of a robot that finishes now
        self._handle.pre_step(ts, ss, self._paths, action.data_ptr(), self.cmd.data_ptr())
        self.ctl.get_action(0.0, self.sim.obs if self.state_estimator is None else self.state_estimator.estimate())
        self.sim.step(self.ctl, None if self.randomizer is None else self.randomizer.pushes())
        self._handle.post_step(ts, ss, self._paths, self._obs_cm.data_ptr(), self.reward.data_ptr(), self.done.data_ptr())
        if self.height_scan is not None:
            self.height_scan.observe(self.sim.state, out=self._scan_obs, mask=self._live)   # of a robot that just finished: its terminal scan
        if self.sensor_model is not None:
            self.sensor_model.observe(self._obs_cm)   # of a robot that just finished: its delivered terminal observation
        if self.auto_reset:
            self._episode.accumulate(self.episode_state.data_ptr(), self.reward.data_ptr(), self.done.data_ptr())
            self.reset_on_device(self.done)
            self.ctl.reset_masked(self.reset_mask)
        return self.obs, self.reward, self.done

    def reset_on_device(self, mask=None, targets=None):
        """reset() with no host work and no synchronisation, for the robots b with mask[b] != 0: target, plan, path, task state,
        simulator and observation (include/rg_episode.h), enqueued on the current stream.  mask: int32 [B] tensor on this
        device (None: self.done).  targets: float64 [B,2] or [2,B] tensor on this device (with B == 2: [B,2]); None: the
        constructor's targets if it had any, else drawn from the device's target stream; NaN entries are drawn too.
        Usable with or without auto_reset.  It writes self.reset_mask (1 where a robot was reset, 0 elsewhere and where the
        plan failed: that robot stays done, plan_status says why) and self.final_obs; the CONTROLLER is reset by
        self.ctl.reset_masked(self.reset_mask), which step() calls under auto_reset and a caller of this method calls itself.
        The host mirrors self.paths / self.targets are maintained by reset() only: which robots were reset here is not known
        on the host, so every entry becomes None (NaN in self.targets) until reset() fills it again.  Returns obs."""
        B = self.batch
        mask = self.done if mask is None else mask
        if not torch.is_tensor(mask) or mask.dtype != torch.int32 or tuple(mask.shape) != (B,) or mask.device != self.device or not mask.is_contiguous():
            raise ValueError(f"reset_on_device: mask must be a contiguous int32 [{B}] tensor on {self.device}")
        if targets is None:
            targets = self._target_table
        else:
            if not torch.is_tensor(targets) or targets.dtype != torch.float64 or targets.device != self.device or tuple(targets.shape) not in ((B, 2), (2, B)):
                raise ValueError(f"reset_on_device: targets must be a float64 [{B},2] or [2,{B}] tensor on {self.device}")
            targets = targets.t().contiguous() if tuple(targets.shape) == (B, 2) else targets.contiguous()
        self._episode.reset(mask.data_ptr(), None if targets is None else targets.data_ptr(), self.episode_state.data_ptr(), self.task_state.data_ptr(),
                            self.sim.state.data_ptr(), self.sim._obs_ptrs, self._paths, self._obs_cm.data_ptr(), self._final_obs_cm.data_ptr(),
                            self.reset_mask.data_ptr())
        if self.randomizer is not None:
            self.randomizer.on_reset(self.reset_mask)   # a robot whose plan failed is not in reset_mask and draws nothing
        if self.state_estimator is not None:
            self.state_estimator.on_reset(self.reset_mask)   # after the simulator's reset; a robot whose plan failed keeps its episode
        if self.sim.terrain is not None:
            # the episode reset stands the robot on the plane; the task observation it wrote reads x, y and heading only, which
            # settle leaves as they are
            self.sim.settle(self.reset_mask)
        if self.height_scan is not None:
            # one launch for the robots that were reset: the terminal scan moves into final_obs, the first scan of the new episode
            # takes its place
            self.height_scan.observe(self.sim.state, out=self._scan_obs, mask=self.reset_mask, prev=self._scan_final)
        if self.sensor_model is not None:
            # after the clean buffer holds the first observation of the new episode: the delivered terminal one moves into the
            # model's final_obs, new delays are drawn and the rings start over.  A robot whose plan failed draws nothing.
            self.sensor_model.on_reset(self.reset_mask, self._obs_cm, prev=self.sensor_model.final_obs)
        if not self._mirrors_stale:
            self.paths = [None] * B
            self.targets[:] = np.nan
            self._mirrors_stale = True
        return self.obs

    def clone(self, src, dst):
        """Branch rollouts: controller, simulator, task state, path and episode state of robot src[k] into robot dst[k].  For
        bit-identical continuations keep dst = src modulo 16 (robot_gym_amd.sim.clone).  The episode-state column carries the
        robot's key in the target stream, so a clone draws the targets its source draws."""
        from robot_gym_amd.sim.srb import clone as sim_clone
        sim_clone(self.ctl, self.sim, src, dst)   # copies sim.obs too, the command among it
        s, t = self.sim._index(src), self.sim._index(dst)
        for ten, dim in ((self.task_state, 1), (self.path_hdr, 1), (self.path_x, 0), (self.path_y, 0), (self.path_s, 0),
                         (self.path_first_same_x, 0), (self._obs_cm, 1), (self.episode_state, 1), (self._final_obs_cm, 1),
                         (self._target_table, 1)):
            if ten is not None:
                ten.index_copy_(dim, t, ten.index_select(dim, s))
        if self.randomizer is not None:
            self.randomizer.copy_columns(s, t)   # the draws the source will make, and its body; the world went with sim_clone
        if self.sensor_model is not None:
            self.sensor_model.copy_columns(s, t)   # rings, delays, ticks and the stream's key: the clone sees what its source sees
        if self.state_estimator is not None:
            self.state_estimator.copy_columns(s, t)   # draws, ticks, contact runs and the stream's key: the clone's controller is given what its source's is
        sh, th = s.cpu().numpy(), t.cpu().numpy()
        for a, b in zip(sh, th):
            self.paths[b], self.targets[b] = self.paths[a], self.targets[a]

    def close(self):
        if self.state_estimator is not None:
            self.state_estimator.close()
        if self.sensor_model is not None:
            self.sensor_model.close()
        if self.randomizer is not None:
            self.randomizer.close()
        if self.height_scan is not None:
            self.height_scan.close()
        self._episode.close()
        self._handle.close()
        self.sim.close()
