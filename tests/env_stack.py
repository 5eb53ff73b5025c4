"""The go-to env with every device model on at once, in numpy: the settings of the stack (STACK) and its replay (Replay), which
advances tests/dr_model.py, tests/scan_model.py over tests/terrain_model.py, tests/sensor_model.py and tests/est_model.py in the
order BatchedGoEnv.reset, step and reset_on_device call the kernels, from what a run recorded.  Numpy only: nothing here needs a
device.  tests/test_env_stack_cpu.py feeds the replay records made by the models themselves, one change at a time;
tests/test_env_stack_gpu.py feeds it the env.

The comparison rule is the project's: everything bit for bit, but the estimator's quat, rpy, foot_pos and jac, which are within
one float32 ulp of the model's rounded value (within_ulp, as _compare of tests/test_est_gpu.py).

STACK_FULL is STACK with a floor that has friction and motors in front of the tick.  A Replay of it also holds three more units:
the floor (mu, drawn by tests/friction_model.draw), the motors (strength, drawn by tests/motor_model.draw, the torque limits, and
per step motor_model.apply on the recorded angles and the controller's recorded force) and the plant (friction_model.
FrictionSRBModel over terrain_model.Random with measured contact, stepped once per env step from the recorded state on the
DEVICE's delivered force).  mu, strength and the limits are bit for bit; the delivered force and the torques follow the rule of
tests/test_motor_gpu.py::test_kernel_against_the_motor_model, the plant srb_streams.Comparison."""
import numpy as np

from robot_gym_amd.core.config import MPCConfig
from tests import dr_model as DM
from tests import contact_fixtures as CF
from tests import est_fixtures as EF
from tests import est_model as EM
from tests import friction_fixtures as FF
from tests import friction_model as FM
from tests import motor_fixtures as MF
from tests import motor_model as MM
from tests import scan_model
from tests import sensor_model as SM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
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

# The stack with a floor and motors as well (STACK_FULL): STACK plus a friction coefficient and a motor strength drawn per episode
# and a torque limit per motor.  The limits go by the robot's index modulo len(LIMIT_FRACTIONS): None is +inf, a number that share
# of motor_fixtures.PEAK of the env's robot.  The ranges and the fractions are chosen on the oracle-driven CPU loop
# (full_cpu_loop below; tests/test_env_stack_cpu.py asserts on it that legs slide, legs clip, nobody falls and few legs lie near
# their limit).  max_time 0.95: 95 sub-steps, the time limit ends every episode on tick 10 -- five ticks from a stand are too
# short for a foot to slide.
FRICTION_START, FRICTION_RANGE, STRENGTH_RANGE = 0.3, (0.2, 0.9), (0.75, 1.0)
LIMIT_FRACTIONS = (None, 0.85, 0.95)
EPISODE_TICKS_FULL = 10
STACK_FULL = dict(
    STACK,
    env=dict(STACK["env"], max_time=0.95, friction=FRICTION_START),
    motors=dict(strength=1.0, limit_fractions=LIMIT_FRACTIONS),                   # MotorModel(strength=, torque_limit=limit_rows(B))
    randomizer=dict(STACK["randomizer"], friction=FRICTION_RANGE, motor_strength=STRENGTH_RANGE),
)


def limit_rows(B, robot="ghost", fractions=LIMIT_FRACTIONS):
    """[12, B] float64: the torque limits of STACK_FULL's MotorModel for a batch of B."""
    peak = np.asarray(MF.PEAK[robot], dtype=np.float64)
    cols = [np.full(12, np.inf) if fractions[b % len(fractions)] is None else fractions[b % len(fractions)] * peak for b in range(B)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


# targets for the resets by hand, under the env's planner (episode_abi.DEFAULTS, no obstacle).  FAIL: the non-finite ones of
# tests/episode_edges.py (STREAM) and a short one as in test_host_reset_passes_its_settings_on_and_refuses_what_the_device_refuses:
# its (0.0, 0.02) is one path point at that test's spacing of 0.015 m but two, a plan, at this env's 0.01 m, so (0.0, 0.015) here
OK_TARGETS = ((1.0, 1.0), (-1.0, 2.0), (-2.0, 1.5), (2.5, -2.5))
FAIL_TARGETS = ((float("inf"), 1.0), (1.0, float("-inf")), (0.0, 0.015))
REFUSED_ON_THE_HOST = (0.0, 0.015)

EXACT = ("q", "rpy_rate", "v_world", "contact", "t_robot")
ROUNDED = ("quat", "rpy", "foot_pos", "jac")
UNITS = ("randomizer", "scan", "sensor", "estimator", "floor", "motors", "plant")
# what a record holds of the env after a call, by unit (every array component-major, [rows, B]; applied [B, 2] as pre_step reads it).
# The last three units are STACK_FULL's: mu [B]; strength and torque_limit [12, B], the delivered force [B, 12] float32 and the two
# torque tables [12, B] of the last tick; the simulator's state [43, B], observation (dict), touch and slip [4, B] after a tick.
FIELDS = {
    "randomizer": ("dr_state", "body", "keys", "ext"),
    "scan": ("scan",),
    "sensor": ("obs", "final_obs", "applied", "sensor_state", "obs_ring", "act_ring"),
    "estimator": ("est_obs", "est_state"),
    "floor": ("mu",),
    "motors": ("strength", "torque_limit", "delivered", "tau_cmd", "tau"),
    "plant": ("sim_state", "sim_obs", "touch", "slip"),
}
TICK_FIELDS = ("delivered", "tau_cmd", "tau", "sim_state", "sim_obs", "touch", "slip")     # compared by their own rules, not by bits


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
    must now hold, under the names of FIELDS.  mismatches(want, got) names every field that differs, with its unit in front.
    With stack=STACK_FULL (self.full) it holds mu, strength, the limits and the plant as well; step then also reads grf,
    foot_target, leg_state and delivered from the record (_tick), and count adds up what the ticks were made of."""

    def __init__(self, B, base, cfg=None, stack=STACK, terrain=None, substeps=10):
        self.B = B
        self.cfg = cfg or default_cfg()
        r = dict(stack["randomizer"])
        (mlo, mhi), (ilo, ihi) = r.pop("mass_scale", (1.0, 1.0)), r.pop("inertia_scale", (1.0, 1.0))
        # STACK_FULL: the floor and the motors the randomizer draws, and the plant the env steps
        self.friction, self.motor_strength = r.pop("friction", None), r.pop("motor_strength", None)
        self.full = self.friction is not None
        if self.full:
            self.mu = np.full(B, float(stack["env"]["friction"]))
            self.strength = np.full((12, B), float(stack["motors"]["strength"]))
            self.limit = limit_rows(B, self.cfg.robot, stack["motors"]["limit_fractions"])
            self.plant = FM.FrictionSRBModel(B, self.cfg, TM.Flat())      # its ground, body and mu are set before every tick
            self.cmp = S.Comparison()
            # what the ticks were made of (robot-ticks, or leg-ticks of running robots): the test asserts on them
            self.count = dict(compared=0, resets=0, sliding=0, clipped=0, near_limit=0, force_legs=0, solved=0, pushed=0)
            self.worst_tick = dict(grf=0.0, tau=0.0, slip=0.0)
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
        full = dict(mu=self.mu.copy(), strength=self.strength.copy(), torque_limit=self.limit.copy()) if self.full else {}
        return dict(dr_state=self.dr_state.copy(), body=self.body.copy(), keys=self.keys.copy(), scan=self.scan_rows.copy(),
                    obs=self.sensor["obs_out"].copy(), final_obs=self.final.copy(), sensor_state=self.sensor["state"].copy(),
                    obs_ring=self.sensor["obs_ring"].copy(), act_ring=self.sensor["act_ring"].copy(), est_state=self.est_state.copy(), **full)

    def _tick(self, rec, ext):
        """STACK_FULL: what the motors and the tick of this step must have made of the recorded inputs, from the body, floor,
        world and strengths held BEFORE this step's reset.  rec also holds grf [B, 12] float32, foot_target and leg_state (the
        controller's outputs of this tick) and delivered [B, 12] float32 (the device's motors.grf)."""
        q = rec["sim_state0"][M.ROW_Q:M.ROW_Q + 12]
        planned = np.ascontiguousarray(rec["grf"], dtype=np.float32)
        out, tau_cmd, tau, sat = MM.apply(self.chain, q, planned, self.strength, self.limit)
        p = self.plant
        p.state[:] = rec["sim_state0"]
        for n in p.obs:
            p.obs[n][...] = rec["sim_obs0"][n]
        p.mass, p.I, p.Iinv = self.body[0].copy(), self.body[1:10].copy(), self.body[10:19].copy()
        p.mu[:] = self.mu
        p.ground = TM.Random(self.terrain["amplitude"], self.terrain["cell"], self.terrain["seed"], self.keys.copy())
        # the tick integrates the force the DEVICE delivered: each unit is held to its model on recorded inputs
        p.step_friction(np.ascontiguousarray(rec["delivered"], dtype=np.float32), np.ascontiguousarray(rec["foot_target"], dtype=np.float32),
                        rec["leg_state"], 1, ext)
        running = rec["sim_state0"][M.ROW_STATUS] == 0.0
        return dict(delivered=out, tau_cmd=tau_cmd, tau=tau, sim_state=p.state.copy(), sim_obs={n: v.copy() for n, v in p.obs.items()},
                    touch=p.touch.copy(), slip=p.slip.copy(),
                    _tick=dict(planned=planned, sat=sat, near=MF.near_limit(self.strength, tau_cmd, self.limit), running=running,
                               clipped=(np.abs(tau) == self.limit).reshape(4, 3, -1).any(1), pushed=(ext != 0).any(0)))

    # ---- one method per env call -----------------------------------------------------------------------------------------

    def _reset(self, mask, sim_state, true_obs, prev):
        mask = np.asarray(mask) != 0
        if self.full:
            # DomainRandomizer.on_reset: the friction draw, the motor draw, then rg_dr_reset, which counts the draw -- all three read
            # the same draw count.  A reset never touches a torque limit.
            key, draws, seed = self.dr_state[DM.ROW_KEY].copy(), self.dr_state[DM.ROW_DRAWS].copy(), self.dr_cfg["seed"]
            FM.draw(self.mu, mask, key, draws, seed, *self.friction)
            MM.draw(self.strength, mask, key, draws, seed, *self.motor_strength)
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
        tick = self._tick(rec, ext) if self.full else {}                                  # before this step's reset draws anything
        if self.full:
            # a robot that was reset holds the first state of its new episode: it alone is left out of the plant's comparison
            tick["_tick"]["reset"] = np.zeros(self.B, dtype=bool) if mask is None else np.asarray(mask) != 0
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
        want.update(applied=applied, ext=ext, est_obs=est, **tick)
        return want

    # ---- the comparison ----------------------------------------------------------------------------------------------------

    def mismatches(self, want, got):
        """["unit: field (n differ)"] for every field of `want` that `got` does not hold by the project's rule; [] if none."""
        out = []
        for unit in UNITS:
            for field in FIELDS[unit]:
                if field not in want or field in TICK_FIELDS:
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
        if "_tick" in want:
            out += self._tick_mismatches(want, got)
        return out

    def _tick_mismatches(self, want, got):
        """The motors and the plant of one step, by their own rules.  motors: tests/motor_fixtures.delivered_mismatches, the rule
        of test_kernel_against_the_motor_model, without the legs near a limit (counted).  plant: srb_streams.Comparison on state
        and observation, touch exactly, slip within S.REL_TOL * max(1, |w|), without the robots of this step's reset_mask."""
        info, out, count = want["_tick"], [], self.count
        planned, sat, near, running, reset = info["planned"], info["sat"], info["near"], info["running"], info["reset"]
        bad, worst, worst_tau = MF.delivered_mismatches(planned, (want["delivered"], want["tau_cmd"], want["tau"], sat),
                                                        (got["delivered"], got["tau_cmd"], got["tau"]), skip=near)
        out += [f"motors: {b}" for b in bad]
        self.worst_tick["grf"], self.worst_tick["tau"] = max(self.worst_tick["grf"], worst), max(self.worst_tick["tau"], worst_tau)
        force = (planned.reshape(self.B, 4, 3) != 0).any(2).T & running[None, :]            # the stance legs of running robots
        count["force_legs"] += int(force.sum())
        count["solved"] += int((sat & force).sum())
        count["near_limit"] += int((near & force).sum())
        count["clipped"] += int((info["clipped"] & force).sum())
        count["pushed"] += int(info["pushed"].sum())
        count["resets"] += int(reset.sum())
        keep = np.nonzero(~reset)[0]
        count["compared"] += len(keep)
        if keep.size == 0:
            return out
        cols = lambda d: {k: (v[..., keep] if np.ndim(v) else v) for k, v in d.items()}      # noqa: E731
        cmp = S.Comparison()
        cmp.check(np.asarray(got["sim_state"])[:, keep], cols(got["sim_obs"]), want["sim_state"][:, keep], cols(want["sim_obs"]))
        where = dict(ints="sim_state", state="sim_state", q="sim_state", t_robot="sim_obs", contact="sim_obs", obs="sim_obs", qjac="sim_obs")
        out += [f"plant: {where[k]}.{k} ({n} differ)" for k, n in cmp.bad.items() if n]
        for k, v in cmp.worst.items():
            self.cmp.worst[k] = max(self.cmp.worst[k], v)
        if not (np.asarray(got["touch"])[:, keep] == want["touch"][:, keep]).all():
            out.append(f"plant: touch ({int((np.asarray(got['touch'])[:, keep] != want['touch'][:, keep]).sum())} differ)")
        g, w = np.asarray(got["slip"])[:, keep], want["slip"][:, keep]
        rel = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        self.worst_tick["slip"] = max(self.worst_tick["slip"], float(rel.max()))
        if not (rel <= S.REL_TOL).all():
            out.append(f"plant: slip ({int((~(rel <= S.REL_TOL)).sum())} beyond the tolerance)")
        count["sliding"] += int((w > 0).sum())
        return out


# ---- the CPU loop the settings of STACK_FULL are chosen on ---------------------------------------------------------------------

FULL_LOOP_TICKS = 100


class FullCpuLoop(FF.FrictionCpuLoop):
    """friction_fixtures.FrictionCpuLoop (the oracle, measured contact, a floor with friction) with motor_model.MotorSRBModel in
    front of the friction model.  count: leg-ticks of running robots -- force_legs (stance legs with a force), sliding, clipped
    (some joint at a finite limit) and near_limit (motor_fixtures.near_limit)."""

    def __init__(self, robot, cmd, height_scale, ground, mu, strength, limit):
        super().__init__(robot, cmd, height_scale, ground, mu)
        self.motors = MM.MotorSRBModel(self.model, strength, limit)
        self.count = dict(force_legs=0, sliding=0, clipped=0, near_limit=0)

    def tick(self, ext=None):
        m, mot, count = self.model, self.motors, self.count
        out = self.oracle.step(float(m.obs["t_robot"][0]), F.oracle_inputs(self.O, m.obs, self.cmd))
        self.last = out
        planned = out["grf"].astype(np.float32)
        running = m.state[M.ROW_STATUS] == 0.0
        delivered = mot.apply(planned)
        force = (planned.reshape(self.B, 4, 3) != 0).any(2).T & running[None, :]
        count["force_legs"] += int(force.sum())
        count["clipped"] += int(((np.abs(mot.tau) == mot.limit).reshape(4, 3, -1).any(1) & force).sum())
        count["near_limit"] += int((MF.near_limit(mot.strength, mot.tau_cmd, mot.limit) & force).sum())
        m.step_friction(delivered, out["foot_target"].reshape(self.B, 12).astype(np.float32), np.asarray(out["leg_state"]).reshape(self.B, 4), 1, ext)
        count["sliding"] += int(((m.slip > 0) & running[None, :]).sum())
        self.slid += m.slip


def full_cpu_loop(robot="ghost", ticks=FULL_LOOP_TICKS):
    """The loop after `ticks` ticks of the 32 srb_fixtures.cases on the reference's random terrain with measured contact, every
    robot's mu and strengths drawn as the env's first reset draws them (FRICTION_RANGE, STRENGTH_RANGE, seed SEED, key = the
    robot's index, draw 0) and the limits of limit_rows(32).  What it gives, 100 ticks (tests/test_env_stack_cpu.py measures it
    again and fails if a figure here is not its measurement):
        ghost   force legs 7552   sliding 117   clipped 334   near a limit 0   fallen 0
    of them in the first ten ticks, an episode of the env: 960, 81, 19, 0.  With the limits at (None, 0.6, 0.95) of the peak ten of
    the 32 robots fall within the 100 ticks, at (None, 0.9, 1.0) with strengths 0.8 .. 1 only 7 leg-ticks clip in the first ten.
    """
    cmd, hs = F.cases(robot)
    B = len(hs)
    key, zero = np.arange(B, dtype=np.float64), np.zeros(B)
    mu = FM.draw(np.zeros(B), np.ones(B), key, zero, SEED, *FRICTION_RANGE)
    strength = MM.draw(np.ones((12, B)), np.ones(B), key, zero, SEED, *STRENGTH_RANGE)
    loop = FullCpuLoop(robot, cmd, hs, CF.reference_ground(B), mu, strength, limit_rows(B, robot))
    for _ in range(ticks):
        loop.tick()
    return loop


FULL_LOOP_MEASURED = dict(ghost=dict(force_legs=7552, sliding=117, clipped=334, near_limit=0, fallen=0))
