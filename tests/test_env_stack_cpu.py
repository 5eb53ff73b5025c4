"""The composed env's test helpers without a GPU (tests/env_stack.py): the reach of the stack's settings from the models alone,
the plan status of the targets the hand-made resets use, and that Replay reports, with the unit's name, each error of ordering it
is there to notice -- on records the models make themselves, one change at a time."""
import numpy as np
import pytest

from robot_gym_amd.core import episode_abi
from tests import dr_model as DM
from tests import env_stack as ES
from tests import episode_model as PM
from tests import est_model as EM
from tests import sensor_model as SM

B, TICKS = 64, 60
DRAWS = range(1 + TICKS // ES.EPISODE_TICKS)      # the draw words of the run: 0 at reset(), then one per reset on ticks 5, 10, ..., 60


def test_the_stack_restates_the_unit_tests_settings():
    from tests.est_fixtures import FULL
    from tests.test_dr_gpu import PUSH
    from tests.test_sensor_gpu import ENV_SENSOR
    assert ES.PUSH == PUSH and ES.SENSOR == {k: v for k, v in ENV_SENSOR.items() if k != "seed"}
    assert {k: v for k, v in ES.STACK["state_estimator"].items() if k != "seed"} == {k: v for k, v in FULL.items() if k != "seed"}
    seeds = {ES.STACK[k]["seed"] for k in ("env", "randomizer", "sensor_model", "state_estimator")}
    assert seeds == {ES.SEED}                                                   # one seed for all
    purposes = [set(range(DM.MASS, DM.PUSH_GATE + 1)), set(range(SM.OBS_DELAY, SM.ACT_NOISE + 1)), set(range(EM.BIAS, EM.GHOST + 1))]
    assert purposes == [set(range(0, 6)), set(range(16, 22)), set(range(32, 36))]      # which is what keeps a shared seed apart


def test_the_stacks_settings_reach_every_delay_different_bodies_and_pushes_inside_an_episode():
    r = ES.Replay(B, ES.base_body(ES.default_cfg(), B))
    s, d = r.sensor_cfg, r.dr_cfg
    for purpose, lo, hi in ((SM.OBS_DELAY, s["obs_delay_min"], s["obs_delay_max"]), (SM.ACT_DELAY, s["act_delay_min"], s["act_delay_max"])):
        first = {SM.delay_draw(ES.SEED, key, 0, purpose, lo, hi) for key in range(B)}
        every = {SM.delay_draw(ES.SEED, key, draw, purpose, lo, hi) for key in range(B) for draw in DRAWS}
        assert first == every == set(range(lo, hi + 1)), (purpose, first, every)        # already at the first draw, and on every later one
    for draw in DRAWS:
        sm = [DM.draw_scales(d, key, draw)[0] for key in range(B)]
        assert len(set(sm)) == B and 0.8 <= min(sm) and max(sm) <= 1.2
    # the ticks of an episode are 0 .. 4 (step counts 0, 10, ..., 40): all in window 0 of 8 ticks
    pushed = np.array([[[bool(DM.push_one(d, key, draw, 10.0 * k).any()) for k in range(ES.EPISODE_TICKS)] for key in range(B)] for draw in (1, 2)])
    print("pushed robot-ticks of episodes 1 and 2:", int(pushed.sum()), "of", pushed.size)
    for draw in range(2):
        some = pushed[draw].any(1)
        assert some.any() and not some.all()                                               # some robots are pushed inside the episode, some never
        assert pushed[draw].any(0).sum() >= 2                                              # on more than one of its ticks


def test_the_targets_meant_to_fail_fail_and_the_others_plan():
    settings = {k: episode_abi.DEFAULTS[k] for k in PM.PLAN_KEYS + ("spacing",)}
    from robot_gym_amd.core import goto_abi
    n_max = goto_abi.DEFAULTS["n_max"]
    status = [PM.plan_status(t, (), n_max, **settings) for t in ES.FAIL_TARGETS]
    assert status == [PM.PLAN_TARGET, PM.PLAN_TARGET, PM.PLAN_SHORT]
    assert ES.REFUSED_ON_THE_HOST in ES.FAIL_TARGETS and np.isfinite(ES.REFUSED_ON_THE_HOST).all()
    for t in ES.OK_TARGETS:
        c = PM.plan_case(t, (), n_max, **settings)
        assert c["status"] == PM.PLAN_OK and not c["flagged"] and not c["near_tie"], t


# ---- records made by the models ----------------------------------------------------------------------------------------------

class ModelEnv:
    """The stack made of the numpy models, called in BatchedGoEnv's order, over a simulator that is a random walk with a step
    count: what it records is what the env would.  mutate: one deliberate error of ordering (MUTATIONS)."""

    def __init__(self, mutate=None, seed=0):
        self.m = ES.Replay(B, ES.base_body(ES.default_cfg(), B))      # its buffers and settings; the ORDER is this class's
        self.mutate, self.rng, self.tick = mutate, np.random.default_rng(seed), 0
        self.sim_state = np.zeros((43, B))
        self.true, self.true_final = (np.zeros((ES.PATH_ROWS + ES.SCAN_ROWS, B), dtype=np.float32) for _ in range(2))
        self.applied, self.ext, self.est_obs = np.zeros((B, 2), dtype=np.float32), np.zeros((6, B)), None

    def _stand(self, on):
        n = int(on.sum())
        yaw = self.rng.uniform(-3.0, 3.0, n)
        self.sim_state[:, on] = 0.0
        self.sim_state[0:2, on] = self.rng.uniform(-2.0, 2.0, (2, n))
        self.sim_state[2, on] = self.m.z_offset + self.rng.uniform(-0.02, 0.02, n)
        self.sim_state[5, on], self.sim_state[6, on] = np.sin(yaw / 2), np.cos(yaw / 2)

    def _path(self, on):
        self.true[:ES.PATH_ROWS, on] = self.rng.uniform(-0.2, 0.3, (ES.PATH_ROWS, int(on.sum()))).astype(np.float32)

    def got(self):
        m = self.m
        return dict(dr_state=m.dr_state.copy(), body=m.body.copy(), keys=m.keys.copy(), ext=self.ext.copy(), scan=self.true[ES.PATH_ROWS:].copy(),
                    obs=m.sensor["obs_out"].copy(), final_obs=m.final.copy(), applied=self.applied.copy(), sensor_state=m.sensor["state"].copy(),
                    obs_ring=m.sensor["obs_ring"].copy(), act_ring=m.sensor["act_ring"].copy(), est_obs=self.est_obs, est_state=m.est_state.copy())

    def reset(self):
        m, on = self.m, np.ones(B, dtype=bool)
        DM.reset(m.dr_cfg, on, m.dr_state, m.base, m.body, m.keys)
        self._stand(on)
        EM.reset(on, m.est_state)
        self._path(on)
        self.true[ES.PATH_ROWS:] = m.scan(self.sim_state)
        SM.reset(m.sensor_cfg, on, m.sensor, self.true)
        self.sim_obs = EM.random_obs(self.rng, B, m.chain)

    def step(self, action):
        m = self.m
        self.tick += 1
        ends = self.sim_state[DM.STEPS_ROW] >= 10.0 * (ES.EPISODE_TICKS - 1)              # the robots this tick resets
        rec = dict(action=action, sim_state0=self.sim_state.copy(), sim_obs0={n: v.copy() for n, v in self.sim_obs.items()})
        self.applied = SM.act(m.sensor_cfg, m.sensor, action)
        if self.mutate == "estimator reset one tick early":
            EM.reset(ends, m.est_state)
        self.est_obs = EM.estimate(m.est_cfg, m.chain, m.est_state, self.sim_obs)
        self.ext = DM.push(m.dr_cfg, self.sim_state, m.dr_state)
        self.sim_state[0:2] += self.rng.uniform(-0.03, 0.03, (2, B))
        self.sim_state[DM.STEPS_ROW] += 10.0
        self.sim_obs = EM.random_obs(self.rng, B, m.chain)
        self._path(np.ones(B, dtype=bool))
        self.true[ES.PATH_ROWS:] = m.scan(self.sim_state)
        SM.observe(m.sensor_cfg, m.sensor, self.true)
        # the reset on the device, for the robots that ended
        self.true_final[:, ends] = self.true[:, ends]
        self._path(ends)
        DM.reset(m.dr_cfg, ends, m.dr_state, m.base, m.body, m.keys)
        if self.mutate != "estimator reset one tick early":
            EM.reset(ends, m.est_state)
        self._stand(ends)
        stale = self.true.copy()
        self.true[ES.PATH_ROWS:, ends] = m.scan(self.sim_state)[:, ends]
        SM.reset(m.sensor_cfg, ends, m.sensor, stale if self.mutate == "sensor reset before the scan" else self.true, m.final)
        if self.mutate == "push from the step counts after the tick":
            self.ext = DM.push(m.dr_cfg, self.sim_state, m.dr_state)
        if self.tick == 7 and self.mutate in STRAY:                                       # tick 7 resets nobody
            state, row = STRAY[self.mutate](m)
            state[row, 3] += 1.0
        rec.update(sim_state=self.sim_state.copy(), true_obs=self.true.copy(), true_final_obs=self.true_final.copy(), done=ends.astype(np.int32),
                   reset_mask=ends.astype(np.int32))
        return rec


STRAY = {"stray draw in the randomizer": lambda m: (m.dr_state, DM.ROW_DRAWS), "stray draw in the sensor model": lambda m: (m.sensor["state"], SM.ROW_DRAWS),
         "stray draw in the estimator": lambda m: (m.est_state, EM.ROW_DRAWS)}
# mutation: the one unit Replay must name on the first tick it reports anything
MUTATIONS = {None: None, "stray draw in the randomizer": "randomizer", "stray draw in the sensor model": "sensor", "stray draw in the estimator": "estimator",
             "sensor reset before the scan": "sensor", "estimator reset one tick early": "estimator", "push from the step counts after the tick": "randomizer"}


@pytest.mark.parametrize("mutate", list(MUTATIONS), ids=lambda m: str(m).replace(" ", "_"))
def test_replay_names_the_unit_of_each_error_of_ordering_and_reports_nothing_without_one(mutate):
    env = ModelEnv(mutate)
    replay = ES.Replay(B, ES.base_body(ES.default_cfg(), B))
    env.reset()
    assert replay.mismatches(replay.host_reset(None, env.sim_state, env.true), env.got()) == []
    rng = np.random.default_rng(1)
    reports = []
    for t in range(12):                                                                    # resets on ticks 5 and 10
        rec = env.step(rng.uniform(-0.3, 0.4, (B, 2)).astype(np.float32))
        found = replay.mismatches(replay.step(rec), env.got())
        if found and not reports:
            reports = [(t + 1, f) for f in found]
    print(mutate, reports)
    if mutate is None:
        assert reports == [] and (replay.draws() == 3).all() and replay.worst and max(replay.worst.values()) == 0.0
        return
    assert reports and {f.split(":")[0] for _, f in reports} == {MUTATIONS[mutate]}, reports
    fields = [f for _, f in reports]
    if mutate in STRAY:
        assert reports[0][0] == 7 and len(fields) == 1 and "state" in fields[0]             # on the tick of the error, the state alone
    elif mutate == "push from the step counts after the tick":
        assert all("ext" in f for f in fields)
    else:
        assert reports[0][0] == ES.EPISODE_TICKS                                           # the first tick with a reset
    if mutate == "sensor reset before the scan":
        assert any("obs_ring" in f for f in fields) and any("obs " in f for f in fields)
