"""The go-to env with every device model on at once, in numpy: the settings of the stack (STACK) and its replay (Replay), which
advances tests/dr_model.py, tests/scan_model.py over tests/terrain_model.py, tests/sensor_model.py and tests/est_model.py in the
order BatchedGoEnv.reset, step and reset_on_device call the kernels, from what a run recorded.  Numpy only: nothing here needs a
device.  tests/test_env_stack_cpu.py feeds the replay records made by the models themselves, one change at a time;
tests/test_env_stack_gpu.py feeds it the env.

The comparison rule is the project's: everything bit for bit, but the estimator's quat, rpy, foot_pos and jac, which are within
one float32 ulp of the model's rounded value (within_ulp, as _compare of tests/test_est_gpu.py)."""
import numpy as np

from robot_gym_amd.core.config import MPCConfig
from tests import dr_model as DM
from tests import est_fixtures as EF
from tests import est_model as EM
from tests import scan_model
from tests import sensor_model as SM
from tests import srb_model as M
from tests import terrain_model as TM
from tests.posctl_fixtures import within_ulp

SEED = 29                 # ONE seed for the three models and the env: the purposes 0..5, 16..21 and 32..35 keep the streams apart
PATH_ROWS, SCAN_ROWS = 16, 48
# the settings of tests/test_dr_gpu.py (PUSH) and tests/test_sensor_gpu.py (ENV_SENSOR), restated so that nothing here imports
# torch; tests/test_env_stack_cpu.py holds them to the originals
PUSH = dict(push_interval=8, push_ticks=3, push_probability=0.5, push_force_xy=30.0, push_force_z=10.0, push_torque_xy=5.0, push_torque_z=2.0)
SENSOR = dict(path=dict(noise_sigma=0.004, bias_half_width=0.01, dropout_probability=0.05, dropout_value=0.0, quantum=0.001),
              scan=dict(noise_sigma=0.01, bias_half_width=0.02, dropout_probability=0.02, dropout_value=1.0, quantum=0.005),
              obs_delay=(0, 2), act_delay=(0, 1), act_noise_sigma=(0.02, 0.05), act_fill=(0.1, 0.0))
STACK = dict(
    env=dict(contact="measured", auto_reset=True, max_time=0.45, seed=SEED),      # 45 sub-steps: the time limit ends every episode on tick 5
    terrain=dict(),                                                               # RandomTerrain()
    height_scan=dict(),                                                           # HeightScan()
    randomizer=dict(mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2), new_world_each_episode=True, seed=SEED, **PUSH),
    sensor_model=dict(SENSOR, seed=SEED),
    state_estimator={**EF.FULL, "seed": SEED},                                    # the flat fields of rg_est_config
)
EPISODE_TICKS = 5

# targets for the resets by hand, under the env's planner (episode_abi.DEFAULTS, no obstacle).  FAIL: the non-finite ones of
# tests/episode_edges.py (STREAM) and a short one as in test_host_reset_passes_its_settings_on_and_refuses_what_the_device_refuses:
# its (0.0, 0.02) is one path point at that test's spacing of 0.015 m but two, a plan, at this env's 0.01 m, so (0.0, 0.015) here
OK_TARGETS = ((1.0, 1.0), (-1.0, 2.0), (-2.0, 1.5), (2.5, -2.5))
FAIL_TARGETS = ((float("inf"), 1.0), (1.0, float("-inf")), (0.0, 0.015))
REFUSED_ON_THE_HOST = (0.0, 0.015)

EXACT = ("q", "rpy_rate", "v_world", "contact", "t_robot")
ROUNDED = ("quat", "rpy", "foot_pos", "jac")
UNITS = ("randomizer", "scan", "sensor", "estimator")
# what a record holds of the env after a call, by unit (every array component-major, [rows, B]; applied [B, 2] as pre_step reads it)
FIELDS = {
    "randomizer": ("dr_state", "body", "keys", "ext"),
    "scan": ("scan",),
    "sensor": ("obs", "final_obs", "applied", "sensor_state", "obs_ring", "act_ring"),
    "estimator": ("est_obs", "est_state"),
}


def default_cfg():
    """The robot BatchedGoEnv takes without a cfg."""
    return MPCConfig.for_robot("ghost", vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)


def base_body(cfg, B):
    """[19, B]: mass, I and I^-1 of the config's body.  The env's own base is read from the device (its I^-1 is the simulator's
    inversion); this one serves the records the models make."""
    inertia = np.asarray(cfg.inertia, dtype=np.float64).reshape(3, 3)
    col = np.concatenate([[cfg.mass], inertia.ravel(), np.linalg.inv(inertia).ravel()])
    return np.tile(col[:, None], (1, B))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Replay:
    """The model state of the four units and numpy copies of what they read.  base: the body table [19, B] the randomizer
    captured at bind; terrain: dict(amplitude, cell, seed) of the RandomTerrain; z_offset: the scan's (the config's body_height).
    host_reset, device_reset and step advance the models as the env's call of the same name does and return `want`: what the env
    must now hold, under the names of FIELDS.  mismatches(want, got) names every field that differs, with its unit in front."""

    def __init__(self, B, base, cfg=None, stack=STACK, terrain=None, substeps=10):
        self.B = B
        self.cfg = cfg or default_cfg()
        r = dict(stack["randomizer"])
        (mlo, mhi), (ilo, ihi) = r.pop("mass_scale", (1.0, 1.0)), r.pop("inertia_scale", (1.0, 1.0))
        self.dr_cfg = DM.settings(worlds=int(bool(r.pop("new_world_each_episode", False))), mass_lo=mlo, mass_hi=mhi, inertia_lo=ilo, inertia_hi=ihi,
                                  substeps=substeps, **r)
        s = dict(stack["sensor_model"])
        (olo, ohi), (alo, ahi) = s.pop("obs_delay", (0, 0)), s.pop("act_delay", (0, 0))
        groups = [(0, PATH_ROWS, s.pop("path")), (PATH_ROWS, PATH_ROWS + SCAN_ROWS, s.pop("scan"))]
        self.sensor_cfg = SM.settings(obs_dim=PATH_ROWS + SCAN_ROWS, act_dim=2, groups=groups, obs_delay_min=olo, obs_delay_max=ohi, act_delay_min=alo,
                                      act_delay_max=ahi, **s)
        self.est_cfg = EM.settings(**stack["state_estimator"])
        self.chain = M.Chain(self.cfg)
        self.terrain = {"amplitude": 0.06, "cell": 0.05, "seed": 0, **stack["terrain"], **(terrain or {})}      # RandomTerrain's defaults
        self.z_offset = float(self.cfg.body_height)
        self.base = np.array(base, dtype=np.float64, copy=True)
        self.keys = np.arange(B, dtype=np.int64)
        self.dr_state, self.body = DM.new_state(B, world=self.keys), self.base.copy()
        self.sensor = SM.new_buffers(self.sensor_cfg, B)
        self.final = np.zeros((PATH_ROWS + SCAN_ROWS, B), dtype=np.float32)
        self.est_state = EM.new_state(B)
        # a robot that is done and not reset since is FROZEN (rg_goto.h, 5.): the task latches its path rows and the env leaves it out
        # of the step's scan, so its scan rows stay what they were although the simulator goes on integrating it
        self.frozen = np.zeros(B, dtype=bool)
        self.scan_rows = np.zeros((SCAN_ROWS, B), dtype=np.float32)
        self.worst = {}           # largest deviation of the ROUNDED row groups seen by mismatches(), in float32 ulp of the model's value

    # ---- what the env must hold ------------------------------------------------------------------------------------------

    def scan(self, sim_state):
        ground = TM.Random(self.terrain["amplitude"], self.terrain["cell"], self.terrain["seed"], self.keys)
        return scan_model.scan(sim_state, ground, z_offset=self.z_offset)

    def draws(self):
        """The draw rows of the three units, [3, B]."""
        return np.stack([self.dr_state[DM.ROW_DRAWS], self.sensor["state"][SM.ROW_DRAWS], self.est_state[EM.ROW_DRAWS]])

    def _scan(self, sim_state, take):
        """The scan rows of the robots `take` (bool [B]) from sim_state; the others keep theirs."""
        self.scan_rows = np.where(take[None, :], self.scan(sim_state), self.scan_rows)

    def _held(self):
        return dict(dr_state=self.dr_state.copy(), body=self.body.copy(), keys=self.keys.copy(), scan=self.scan_rows.copy(),
                    obs=self.sensor["obs_out"].copy(), final_obs=self.final.copy(), sensor_state=self.sensor["state"].copy(),
                    obs_ring=self.sensor["obs_ring"].copy(), act_ring=self.sensor["act_ring"].copy(), est_state=self.est_state.copy())

    # ---- one method per env call -----------------------------------------------------------------------------------------

    def _reset(self, mask, sim_state, true_obs, prev):
        mask = np.asarray(mask) != 0
        DM.reset(self.dr_cfg, mask, self.dr_state, self.base, self.body, self.keys)       # the draw, before the robot is stood up
        EM.reset(mask, self.est_state)
        self.frozen &= ~mask
        self._scan(sim_state, mask)                                                       # in the world just drawn
        # the sensors' first measurement is of the clean buffer AFTER the scan of the new world is in it
        SM.reset(self.sensor_cfg, mask, self.sensor, np.ascontiguousarray(true_obs, dtype=np.float32), prev)
        return self._held()

    def host_reset(self, idx, sim_state, true_obs):
        """BatchedGoEnv.reset(idx) (None: every robot).  sim_state [43, B] and true_obs [64, B]: the env's after the call."""
        mask = np.ones(self.B, dtype=bool) if idx is None else np.isin(np.arange(self.B), np.asarray(idx))
        return self._reset(mask, sim_state, true_obs, None)

    def device_reset(self, reset_mask, sim_state, true_obs):
        """BatchedGoEnv.reset_on_device: reset_mask is the env's (1 where a robot WAS reset).  The delivered terminal
        observation moves into final_obs."""
        return self._reset(reset_mask, sim_state, true_obs, self.final)

    def step(self, rec):
        """BatchedGoEnv.step.  rec: action [B, 2] float32, sim_state0 [43, B] and sim_obs0 (dict) from BEFORE the call;
        sim_state, true_obs and true_final_obs [64, B] and done [B] from after it, and reset_mask (None without auto_reset)."""
        applied = SM.act(self.sensor_cfg, self.sensor, np.ascontiguousarray(rec["action"], dtype=np.float32))
        est = EM.estimate(self.est_cfg, self.chain, self.est_state, rec["sim_obs0"])
        ext = DM.push(self.dr_cfg, rec["sim_state0"], self.dr_state)                      # from the step counts before the tick
        mask = rec.get("reset_mask")
        true = np.ascontiguousarray(rec["true_obs"], dtype=np.float32)
        self._scan(rec["sim_state"], ~self.frozen)                                        # a robot that finishes on this tick: its terminal scan
        self.frozen |= np.asarray(rec["done"]) != 0
        if mask is None:
            SM.observe(self.sensor_cfg, self.sensor, true)
            want = self._held()
        else:
            # the clean observation measured on this tick: of a robot that was reset it is the terminal one, which the episode
            # reset moved into true_final_obs before it wrote the first observation of the new episode
            seen = np.where((np.asarray(mask) != 0)[None, :], rec["true_final_obs"], true)
            SM.observe(self.sensor_cfg, self.sensor, np.ascontiguousarray(seen, dtype=np.float32))
            want = self.device_reset(mask, rec["sim_state"], true)
        want.update(applied=applied, ext=ext, est_obs=est)
        return want

    # ---- the comparison ----------------------------------------------------------------------------------------------------

    def mismatches(self, want, got):
        """["unit: field (n differ)"] for every field of `want` that `got` does not hold by the project's rule; [] if none."""
        out = []
        for unit in UNITS:
            for field in FIELDS[unit]:
                if field not in want:
                    continue
                if field != "est_obs":
                    if not _same_bits(np.asarray(got[field], dtype=np.asarray(want[field]).dtype), want[field]):
                        n = int((np.asarray(got[field]) != np.asarray(want[field])).sum()) if np.shape(got[field]) == np.shape(want[field]) else -1
                        out.append(f"{unit}: {field} ({n} differ)")
                    continue
                for n in EXACT:
                    if not _same_bits(got[field][n], want[field][n]):
                        out.append(f"{unit}: {field}.{n} ({int((got[field][n] != want[field][n]).sum())} differ)")
                for n in ROUNDED:
                    g, w = got[field][n], want[field][n]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        ulps = np.abs(g.astype(np.float64) - w.astype(np.float64)) / np.spacing(np.abs(w)).astype(np.float64)
                    ok = within_ulp(g, w)
                    if not ok.all():
                        out.append(f"{unit}: {field}.{n} ({int((~ok).sum())} beyond one ulp, worst {float(np.nanmax(ulps)):.3g})")
                    else:
                        self.worst[n] = max(self.worst.get(n, 0.0), float(ulps.max()))
        return out
