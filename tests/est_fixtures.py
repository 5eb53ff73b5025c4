"""What the state estimator's CPU and GPU tests share: the full configuration with every effect on, a true contact trace with
lift-offs and touch-downs, and the closed loop with a per-episode roll and pitch bias -- the CPU reference loop of
tests/srb_fixtures.py with tests/est_model.py between the model and the oracle, and the figures both sides are judged by.

The closed-loop property: the controller levels the ESTIMATED body, so with a roll and pitch bias alone the true roll and pitch
settle near minus the error, and the slope of the settled true angle on the drawn error is negative (about -1).  The CPU test
(tests/test_est_cpu.py) recomputes CPU_SLOPES and fails if a constant here is not its measurement; the GPU test holds the
kernels' slopes to them."""
import numpy as np

from tests import est_model as EM
from tests import srb_fixtures as F
from tests import srb_model as M

# every effect on, at magnitudes of a real quadruped's sensors
FULL = dict(seed=11, imu_bias_half_width=(0.03, 0.02, 0.05), imu_noise_sigma=(0.002, 0.003, 0.001), gyro_bias_half_width=(0.01, 0.02, 0.03),
            gyro_noise_sigma=(0.05, 0.04, 0.03), velocity_bias_half_width=(0.05, 0.04, 0.03), velocity_noise_sigma=(0.02, 0.03, 0.01),
            encoder_bias_half_width=0.01, encoder_noise_sigma=0.002, encoder_quantum=2.0 * np.pi / 4096.0, contact_miss_probability=0.1,
            contact_ghost_probability=0.05, contact_rise_ticks=2)

# each effect alone: the fields it switches on and the observation rows it may move
EFFECTS = {
    "imu": (dict(imu_bias_half_width=(0.03, 0.0, 0.0), imu_noise_sigma=(0.0, 0.002, 0.0)), ("rpy", "quat")),
    "gyro": (dict(gyro_bias_half_width=(0.0, 0.02, 0.0), gyro_noise_sigma=(0.05, 0.0, 0.0)), ("rpy_rate",)),
    "velocity": (dict(velocity_bias_half_width=(0.05, 0.0, 0.0), velocity_noise_sigma=(0.0, 0.0, 0.01)), ("v_world",)),
    "encoder_bias": (dict(encoder_bias_half_width=0.01), ("q", "foot_pos", "jac")),
    "encoder_noise": (dict(encoder_noise_sigma=0.002), ("q", "foot_pos", "jac")),
    "encoder_quantum": (dict(encoder_quantum=2.0 * np.pi / 4096.0), ("q", "foot_pos", "jac")),
    "contact_rise": (dict(contact_rise_ticks=2), ("contact",)),
    "contact_miss": (dict(contact_miss_probability=0.3), ("contact",)),
    "contact_ghost": (dict(contact_ghost_probability=0.3), ("contact",)),
}


def contact_trace(rng, ticks, B):
    """int32 [ticks, 4, B]: each foot holds its state for 1 to 6 ticks, then toggles -- runs shorter and longer than a debounce of 2."""
    out = np.zeros((ticks, 4, B), dtype=np.int32)
    state = rng.integers(0, 2, (4, B))
    left = rng.integers(1, 7, (4, B))
    for t in range(ticks):
        out[t] = state
        left = left - 1
        flip = left == 0
        state = np.where(flip, 1 - state, state)
        left = np.where(flip, rng.integers(1, 7, (4, B)), left)
    return out


# ---- the closed loop -------------------------------------------------------------------------------------------------------

TILT_HALF_WIDTH = 0.03            # rad, roll and pitch
TILT = dict(seed=5, imu_bias_half_width=(TILT_HALF_WIDTH, TILT_HALF_WIDTH, 0.0))
LOOP_ROBOTS = 32                  # per robot model, as tests/srb_fixtures.py affords: 64 in all
LOOP_TICKS = F.TICKS              # 4 s
LOOP_TAIL = F.TICKS // 4          # the last quarter


def drawn_tilt(keys, draw=0):
    """The roll and pitch error [2, n] of robots with `keys` in their episode `draw` under TILT: the header's bias."""
    cfg = EM.settings(**TILT)
    key, d = np.asarray(keys).astype(np.uint64), np.full(len(keys), draw, dtype=np.uint64)
    return np.stack([EM.bias(cfg, key, d, TILT_HALF_WIDTH, EM.OBS_ROW_RPY + i) for i in range(2)])


def fit(x, y):
    """Least-squares line y = a + slope x -> (slope, standard error of the slope)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(x)
    xc = x - x.mean()
    sxx = float((xc * xc).sum())
    slope = float((xc * y).sum()) / sxx
    resid = y - y.mean() - slope * xc
    return slope, float(np.sqrt((resid * resid).sum() / (n - 2) / sxx))


def slopes(error, roll_tail, pitch_tail):
    """error [2, n]; roll_tail, pitch_tail [T, n] true angles over the tail -> dict(roll=(slope, se), pitch=(slope, se))."""
    return dict(roll=fit(error[0], roll_tail.mean(0)), pitch=fit(error[1], pitch_tail.mean(0)))


class EstCpuLoop(F.CpuLoop):
    """CpuLoop with the estimator model between the model's observation and the oracle."""

    def __init__(self, robot, cmd, height_scale, est_cfg, nthreads=0):
        super().__init__(robot, cmd, height_scale, nthreads)
        self.est_cfg = EM.settings(**est_cfg)
        self.chain = M.Chain(self.cfg)
        self.est_state = EM.new_state(self.B)
        EM.reset(np.ones(self.B), self.est_state)
        self.est_obs = None

    def tick(self, ext=None):
        m = self.model
        self.est_obs = EM.estimate(self.est_cfg, self.chain, self.est_state, m.obs)
        out = self.oracle.step(float(m.obs["t_robot"][0]), F.oracle_inputs(self.O, self.est_obs, self.cmd))
        self.last = out
        m.step(out["grf"].astype(np.float32), out["foot_target"].reshape(self.B, 12).astype(np.float32), out["desired"], ext)
        return F.figures(m.state)


def run_cpu_tilt(robot):
    """-> (slopes dict, the loop): LOOP_ROBOTS robots of `robot` at zero command and the nominal height for LOOP_TICKS under TILT."""
    loop = EstCpuLoop(robot, np.zeros((LOOP_ROBOTS, 3), dtype=np.float32), np.ones(LOOP_ROBOTS), TILT)
    traj = F.stack([loop.tick() for _ in range(LOOP_TICKS)])
    return slopes(drawn_tilt(np.arange(LOOP_ROBOTS)), traj["roll"][-LOOP_TAIL:], traj["pitch"][-LOOP_TAIL:]), loop, traj


# (slope, standard error of the fit) of the CPU closed loop, per robot model: measured by run_cpu_tilt, recomputed by
# tests/test_est_cpu.py::test_closed_loop_levels_the_estimated_body
CPU_SLOPES = {
    "ghost": dict(roll=(-1.0424340861613484, 8.003090513343972e-05), pitch=(-1.0135687287795392, 3.422998077778819e-05)),
    "k3lso": dict(roll=(-1.0383094515020999, 5.083636642473813e-05), pitch=(-1.013599137801741, 3.692550873228677e-05)),
}
