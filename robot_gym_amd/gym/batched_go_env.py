"""The go-to-target task for B closed-loop robots on one GPU: controller, simulator and task with no host in the loop.

The reference's GoEnv (gym/envs/go_to/go_env.py) per robot: a planned path to a target, a 2 * num_cam_pts observation of
the path seen through a trapezoidal window in the robot's frame, the action (vx, wz), a progress / track-error reward and
six termination causes (include/rg_goto.h).  The planner and the path builder run on the host at a reset
(robot_gym_amd/gym/goto_path.py); a step is four launches on the current stream and nothing else:

    env = BatchedGoEnv(B, cfg)                # cfg None: ghost with its command offsets zeroed (see __init__)
    obs = env.reset()                         # [B, 16] float32 device tensor
    obs, reward, done = env.step(action)      # action [B, 2] (vx, wz) device tensor; no synchronisation, no host copy

obs, reward and done are views of buffers the next step overwrites.  There is no auto-reset: a done robot stays frozen
(reward 0, done 1, its last observation) until reset(idx).
"""
import numpy as np
import torch

from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
from robot_gym_amd.core import goto_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.gym import goto_path
from robot_gym_amd.sim.srb import BatchedSRBSim


class BatchedGoEnv:
    """Owns ctl (BatchedMPCController), sim (BatchedSRBSim) and the task (goto_abi.GotoHandle) with its buffers:
    task_state float64 [50, B], the path slab (path_x / path_y / path_s float64 [B, n_max], path_first_same_x int32
    [B, n_max], path_hdr float64 [4, B]) and the outputs."""

    def __init__(self, batch, cfg: MPCConfig = None, targets=None, obstacles=None, seed=0, device=None, sim_settings=None, **task):
        # The default robot is ghost WITH ITS COMMAND OFFSETS ZEROED: vy_offset / wz_offset trim a drift of the reference's
        # PyBullet robot that the reduced model does not have, and with them a straight command walks a curve off the path.
        # A cfg passed in is taken as it is, offsets included.
        self.cfg = cfg or MPCConfig.for_robot("ghost", vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
        self.batch = B = int(batch)
        self.ctl = BatchedMPCController(B, self.cfg, device=device)
        self.device = dev = self.ctl.device
        self.sim = BatchedSRBSim(B, self.cfg, device=dev, **(sim_settings or {}))
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
        self._obs_cm = torch.zeros(2 * self.num_cam_pts, B, dtype=torch.float32, device=dev)   # component-major, as the kernel writes it
        self.reward = torch.zeros(B, dtype=torch.float32, device=dev)
        self.done = torch.zeros(B, dtype=torch.int32, device=dev)
        # the offset-corrected command goes straight into the tensor the controller reads with the state
        self.sim.obs["cmd"] = self.cmd = torch.zeros(3, B, dtype=torch.float32, device=dev)
        self._rng = np.random.default_rng(seed)
        self._fixed_targets = None if targets is None else np.asarray(targets, dtype=np.float64).reshape(-1, 2)
        self.obstacles = () if obstacles is None else obstacles
        self.targets = np.zeros((B, 2))
        self.paths = [None] * B

    @property
    def obs(self):
        """[B, 2 * num_cam_pts] view of the observation buffer."""
        return self._obs_cm.t()

    @property
    def done_reason(self):
        """int64 [B] device tensor of RG_GOTO_REASON_* codes (goto_abi.REASONS names them)."""
        return self.task_state[goto_abi.ROW_REASON].to(torch.int64)

    @property
    def observation_space_bounds(self):
        """(low, high) of GoEnv's observation box, [2 * num_cam_pts] each (go_env.py:105-108)."""
        return (np.array([0.0, -0.2] * self.num_cam_pts, dtype=np.float32), np.array([0.3, 0.2] * self.num_cam_pts, dtype=np.float32))

    @property
    def action_space_bounds(self):
        return (np.array(self.fields["action_low"], dtype=np.float32), np.array(self.fields["action_high"], dtype=np.float32))

    def reset(self, idx=None, targets=None):
        """Robots idx (None: all): plan and build a path to targets [n,2] (None: the constructor's targets, cycled over the
        robots, or random ones as go_env.py:163-175), upload it, put the robot at the path's start facing along it, reset
        the controller, and observe.  Host work and blocking copies; returns obs [B, 2 * num_cam_pts]."""
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
        for t in tg:
            key = (float(t[0]), float(t[1]))
            if key not in cache:
                cache[key] = goto_path.build_path(goto_path.plan_path(key, self.obstacles), int(self.fields["num_checkpoints"]), target=key)
            built.append(cache[key])
        for k, b in enumerate(idx):
            self.paths[b], self.targets[b] = built[k], tg[k]
        rows = goto_path.pack_paths(built, self.n_max)
        whole = n == B and np.array_equal(idx, np.arange(B))
        self._handle.set_path(self._paths, self.task_state.data_ptr(), None if whole else idx, **rows)
        self.sim.reset(None if whole else idx, xy=np.array([p.start_xy for p in built]), yaw=np.array([p.start_angle for p in built]))
        self.ctl.reset(None if whole else idx)
        self._handle.observe(self.task_state.data_ptr(), self.sim.state.data_ptr(), self._paths, self._obs_cm.data_ptr())
        return self.obs

    def step(self, action):
        """action: [B,2] (vx, wz) float32 tensor on this device.  pre_step -> controller -> simulator -> post_step on the
        current stream.  Returns (obs [B, 2 * num_cam_pts], reward [B], done [B] int32)."""
        if not torch.is_tensor(action) or tuple(action.shape) != (self.batch, 2) or action.device != self.device:
            raise ValueError(f"step: action must be a [{self.batch},2] tensor on {self.device}")
        if action.dtype != torch.float32 or not action.is_contiguous():
            action = action.to(torch.float32).contiguous()   # the kernel reads the rows as they are: a float32 action costs no torch op
        ts, ss = self.task_state.data_ptr(), self.sim.state.data_ptr()
        self._handle.pre_step(ts, ss, self._paths, action.data_ptr(), self.cmd.data_ptr())
        self.ctl.get_action(0.0, self.sim.obs)
        self.sim.step(self.ctl)
        self._handle.post_step(ts, ss, self._paths, self._obs_cm.data_ptr(), self.reward.data_ptr(), self.done.data_ptr())
        return self.obs, self.reward, self.done

    def clone(self, src, dst):
        """Branch rollouts: controller, simulator, task state and path of robot src[k] into robot dst[k].  For bit-identical
        continuations keep dst = src modulo 16 (robot_gym_amd.sim.clone)."""
        from robot_gym_amd.sim.srb import clone as sim_clone
        sim_clone(self.ctl, self.sim, src, dst)   # copies sim.obs too, the command among it
        s, t = self.sim._index(src), self.sim._index(dst)
        for ten, dim in ((self.task_state, 1), (self.path_hdr, 1), (self.path_x, 0), (self.path_y, 0), (self.path_s, 0),
                         (self.path_first_same_x, 0), (self._obs_cm, 1)):
            ten.index_copy_(dim, t, ten.index_select(dim, s))
        sh, th = s.cpu().numpy(), t.cpu().numpy()
        for a, b in zip(sh, th):
            self.paths[b], self.targets[b] = self.paths[a], self.targets[a]

    def close(self):
        self._handle.close()
        self.sim.close()
