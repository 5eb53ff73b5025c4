"""Sensor and actuator model on the device (include/rg_sensor.h): what the policy sees is the clean observation with a
per-episode bias, white noise, quantisation, dropout and a per-episode latency; what it commands reaches the task with noise
and a per-episode latency.  A stateless counter-based stream keyed by a per-robot key: reproducible, clonable
(copy_columns), with no host work in the loop.  All arithmetic happens in librg_mpc.so.

    sm = SensorModel(path=dict(noise_sigma=0.005, dropout_probability=0.02), scan=dict(noise_sigma=0.01, bias_half_width=0.02, quantum=0.005),
                     obs_delay=(0, 2), act_delay=(0, 1), act_noise_sigma=(0.02, 0.05))
    env = BatchedGoEnv(B, cfg, terrain=RandomTerrain(), height_scan=HeightScan(), auto_reset=True, sensor_model=sm)
    env.obs, env.final_obs              # what the sensors DELIVER;  env.true_obs, env.true_final_obs: what the task and scan wrote

    sm = SensorModel(groups=[(0, 12, dict(noise_sigma=0.01))], obs_delay=(1, 3)).bind(B, device, obs_dim=12, act_dim=2)   # on its own
    sm.on_reset(mask, clean)            # clean: float32 [D, B];  mask: int32 [B]
    seen = sm.observe(clean)            # [D, B], once per tick
    applied = sm.act(action)            # [B, A], once per tick

The defaults are the identity, and the identity copies bits.  Limits (rg_sensor.h): the controller's own state estimate is not
this model's (StateEstimator, state_estimator.py, is); dropout is per row, not per frame; the noise is white and bounded (a sum of four uniforms, |n| < 3.4642 sigma, not a
Gaussian: that is what keeps tests/sensor_model.py bit-exact); a robot's delays are constant over an episode.
"""
import torch

from robot_gym_amd.core import sensor_abi
from robot_gym_amd.sim.stream_state import copy_robot_columns, stream_state


def _pair(v, name):
    try:
        lo, hi = (int(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"SensorModel: {name} must be a pair (lo, hi) of ticks, got {v!r}") from None
    return lo, hi


class SensorModel:
    """path, scan: settings (sensor_abi.GROUP_DEFAULTS' fields) of the group over the path rows and the scan rows of the env
    that binds the model; groups: explicit (begin, end, settings) triples instead.  obs_delay, act_delay: (lo, hi) ticks;
    act_noise_sigma, act_fill: one value per action component (fewer: 0 for the rest).  The library checks everything at
    bind(); nothing touches the device before it.
    After bind(): state float64 [8, B] (rows: rg_sensor.h; row 0 the robot's key in the stream, arange(B)), obs_ring float32
    [Lo, D, B], act_ring float32 [La, A, B], the delivered buffers obs_out, final_obs (float32 [D, B]) and act_out (float32 [B, A])."""

    def __init__(self, path=None, scan=None, groups=None, obs_delay=(0, 0), act_delay=(0, 0), act_noise_sigma=(), act_fill=(), seed=0):
        if groups is not None and (path is not None or scan is not None):
            raise ValueError("SensorModel: give groups, or path and scan, not both")
        for name, g in (("path", path), ("scan", scan)):
            if g is not None:
                sensor_abi.merged(sensor_abi.GROUP_DEFAULTS, g, f"sensor group ({name})")
        self.path, self.scan = (None if path is None else dict(path)), (None if scan is None else dict(scan))
        self.groups = None if groups is None else [(int(b), int(e), dict(s)) for b, e, s in groups]
        (olo, ohi), (alo, ahi) = _pair(obs_delay, "obs_delay"), _pair(act_delay, "act_delay")
        self.settings = dict(seed=int(seed), obs_delay_min=olo, obs_delay_max=ohi, act_delay_min=alo, act_delay_max=ahi,
                             act_noise_sigma=tuple(float(x) for x in act_noise_sigma), act_fill=tuple(float(x) for x in act_fill))
        self.batch = self.device = self.obs_dim = self.act_dim = self._handle = self.bound_groups = None
        self.state = self.obs_ring = self.act_ring = self.obs_out = self.final_obs = self.act_out = None

    def bind(self, batch, device, obs_dim, act_dim, path_rows=None, scan_rows=None):
        """Creates the handle and the buffers for `batch` robots with obs_dim rows and act_dim action components on `device`.
        path_rows, scan_rows: the (begin, end) the `path` and `scan` shorthands stand for (BatchedGoEnv passes its own); an
        empty range drops its group.  Returns self."""
        if self._handle is not None:
            raise RuntimeError("SensorModel: already bound (one model per env)")
        groups = self.groups
        if groups is None:
            groups = []
            for name, g, rows in (("path", self.path, path_rows), ("scan", self.scan, scan_rows)):
                if g is None:
                    continue
                if rows is None:
                    raise ValueError(f"SensorModel: `{name}` needs {name}_rows at bind() (BatchedGoEnv passes them), or use groups=")
                if rows[1] > rows[0]:
                    groups.append((int(rows[0]), int(rows[1]), g))
        B, D, A = int(batch), int(obs_dim), int(act_dim)
        self._handle = sensor_abi.SensorHandle(B, device, obs_dim=D, act_dim=A, groups=groups, **self.settings)
        self.batch, self.device, self.obs_dim, self.act_dim = B, self._handle.device, D, A
        dev = self.device
        self.bound_groups = groups
        self.state = stream_state(sensor_abi.ROWS, B, dev)
        self.obs_ring = torch.zeros(self.settings["obs_delay_max"] + 1, D, B, dtype=torch.float32, device=dev)
        self.act_ring = torch.zeros(self.settings["act_delay_max"] + 1, A, B, dtype=torch.float32, device=dev)
        self.obs_out = torch.zeros(D, B, dtype=torch.float32, device=dev)
        self.final_obs = torch.zeros(D, B, dtype=torch.float32, device=dev)
        self.act_out = torch.zeros(B, A, dtype=torch.float32, device=dev)
        return self

    def _bound(self, what):
        if self._handle is None:
            raise RuntimeError(f"SensorModel: bind(...) before {what}")

    def _tensor(self, t, dtype, shape, what):
        if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
            raise ValueError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)} tensor on {self.device}")
        return t.data_ptr()

    @property
    def delays(self):
        """float64 [2, B] view of the state: the observation delay and the action delay, in ticks, each robot has now."""
        self._bound("delays")
        return self.state[sensor_abi.ROW_OBS_DELAY:sensor_abi.ROW_ACT_DELAY + 1]

    def on_reset(self, mask, clean, prev=None):
        """A new episode for the robots b with mask[b] != 0 (int32 [B] device tensor): prev (float32 [D, B], if given) takes
        their delivered observation, then delays are drawn, `clean` (float32 [D, B], the first clean observation of the episode)
        is measured into every ring slot and obs_out, and the action ring is filled with act_fill.  Enqueued on the current
        stream; nothing waits."""
        self._bound("on_reset")
        D, B = self.obs_dim, self.batch
        self._handle.reset(self._tensor(mask, torch.int32, (B,), "on_reset: mask"), self.state.data_ptr(),
                           self._tensor(clean, torch.float32, (D, B), "on_reset: clean"), self.obs_ring.data_ptr(), self.obs_out.data_ptr(),
                           None if prev is None else self._tensor(prev, torch.float32, (D, B), "on_reset: prev"), self.act_ring.data_ptr())

    def observe(self, clean):
        """This tick's observation of every robot from `clean` (float32 [D, B]): returns obs_out, the DELIVERED [D, B] tensor,
        after enqueuing the kernel that writes it."""
        self._bound("observe")
        self._handle.observe(self.state.data_ptr(), self._tensor(clean, torch.float32, (self.obs_dim, self.batch), "observe: clean"),
                             self.obs_ring.data_ptr(), self.obs_out.data_ptr())
        return self.obs_out

    def act(self, action):
        """This tick's action of every robot from `action` (float32 [B, A]): returns act_out [B, A], what reaches the plant.
        Not clipped."""
        self._bound("act")
        self._handle.act(self.state.data_ptr(), self._tensor(action, torch.float32, (self.batch, self.act_dim), "act: action"),
                         self.act_ring.data_ptr(), self.act_out.data_ptr())
        return self.act_out

    def copy_columns(self, src, dst):
        """The state, ring and delivered columns of robot src[k] into robot dst[k] (index tensors or lists): the clone sees and
        applies what its source does, the key included."""
        self._bound("copy_columns")
        copy_robot_columns(((self.state, 1), (self.obs_ring, 2), (self.act_ring, 2), (self.obs_out, 1), (self.final_obs, 1), (self.act_out, 0)), src, dst,
                           index=lambda idx: torch.as_tensor(idx, dtype=torch.int64, device=self.device).reshape(-1))

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None
        self.state = self.obs_ring = self.act_ring = self.obs_out = self.final_obs = self.act_out = None
