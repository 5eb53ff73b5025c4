"""BatchedGoEnv with every device model on at once (tests/env_stack.py: STACK) -- random terrain, measured contact, the height
scan, a DomainRandomizer, a SensorModel and a StateEstimator under ONE seed -- held tick by tick to the four numpy models through
env_stack.Replay: the whole stack under auto-reset, the sensor model's transparency to the plant, the three defaults together as
the identity, a partial host reset, a device reset by hand with plans that fail and the frozen ticks after it, and a clone.
Everything bit for bit but the estimator's quat, rpy, foot_pos and jac (one float32 ulp, the rule of tests/test_est_gpu.py).

Then the same with a floor and motors on (tests/env_stack.py: STACK_FULL -- friction, a MotorModel with torque limits, a randomizer
that draws mu and the strengths): the full stack replayed with the plant itself held to the friction model on every tick, the
defaults of all five together as the identity, a partial host reset, and a clone."""
import time

import numpy as np
import pytest
import torch

from robot_gym_amd.core import srb_abi
from tests import dr_model as DM
from tests import env_stack as ES
from tests import est_model as EM
from tests import sensor_model as SM
from tests.test_est_gpu import _grouped

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = 64
MODELS = ("randomizer", "sensor_model", "state_estimator")


def _stack(batch=B, without=(), **env_kw):
    """The env of ES.STACK; without: names of MODELS to leave out; env_kw over STACK's."""
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain, SensorModel, StateEstimator
    from robot_gym_amd.sim.height_scan import HeightScan
    make = dict(randomizer=lambda: DomainRandomizer(**ES.STACK["randomizer"]), sensor_model=lambda: SensorModel(**ES.STACK["sensor_model"]),
                state_estimator=lambda: StateEstimator(**_grouped(ES.STACK["state_estimator"])))
    models = {name: make[name]() for name in MODELS if name not in without}
    return BatchedGoEnv(batch, device=DEV, terrain=RandomTerrain(**ES.STACK["terrain"]), height_scan=HeightScan(**ES.STACK["height_scan"]),
                        **models, **{**ES.STACK["env"], **env_kw})


def _np(t):
    return t.detach().contiguous().cpu().numpy()


def _bits(t):
    t = t.contiguous()
    return (t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)).cpu()


def _replay(env, stack=ES.STACK):
    """A Replay of a freshly built env (before its first reset: the body on the device is the base)."""
    t = env.sim.terrain
    assert env.sensor_model.bound_groups == [(0, ES.PATH_ROWS, ES.SENSOR["path"]), (ES.PATH_ROWS, ES.PATH_ROWS + ES.SCAN_ROWS, ES.SENSOR["scan"])]
    return ES.Replay(env.batch, _np(env.randomizer.body()), cfg=env.cfg, stack=stack, terrain=dict(amplitude=t.amplitude, cell=t.cell, seed=t.seed),
                     substeps=env.sim.substeps)


def _before(env, action):
    return dict(action=_np(action), sim_state0=_np(env.sim.state), sim_obs0={n: _np(env.sim.obs[n]) for n in srb_abi.OBS_FIELDS})


def _after(env, auto_reset=True):
    return dict(sim_state=_np(env.sim.state), true_obs=_np(env.true_obs.t()), true_final_obs=_np(env.true_final_obs.t()), done=_np(env.done),
                reset_mask=_np(env.reset_mask) if auto_reset else None)


def _got(env):
    dr, sm, est = env.randomizer, env.sensor_model, env.state_estimator
    return dict(dr_state=_np(dr.state), body=_np(dr.body()), keys=_np(env.sim.terrain.keys), ext=_np(dr.ext), scan=_np(env.true_obs.t())[ES.PATH_ROWS:],
                obs=_np(env.obs.t()), final_obs=_np(env.final_obs.t()), applied=_np(sm.act_out), sensor_state=_np(sm.state), obs_ring=_np(sm.obs_ring),
                act_ring=_np(sm.act_ring), est_obs={n: _np(est.obs[n]) for n in srb_abi.OBS_FIELDS}, est_state=_np(est.state))


def _actions(T, batch=B, seed=21):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(T, batch, 2, generator=gen) * torch.tensor([0.5, 0.6]) + torch.tensor([0.0, -0.3])).to(DEV)


def _draw_rows(env):
    return torch.stack([env.randomizer.state[DM.ROW_DRAWS], env.sensor_model.state[SM.ROW_DRAWS], env.state_estimator.state[EM.ROW_DRAWS]]).to(torch.int64)


def _model_tensors(env):
    """Every tensor of the three models a robot outside a reset must keep to the byte, by name (the body is a copy)."""
    dr, sm, est = env.randomizer, env.sensor_model, env.state_estimator
    return dict(dr_state=dr.state, body=dr.body(), keys=env.sim.terrain.keys, sensor_state=sm.state, obs_ring=sm.obs_ring, act_ring=sm.act_ring,
                final_obs=sm.final_obs, est_state=est.state)


def _snapshot(tensors):
    return {n: t.clone() for n, t in tensors.items()}


def _unchanged(before, after, cols, what):
    """The columns `cols` (a bool device tensor over the robots, the last dimension) hold the same bits."""
    for n, was in before.items():
        assert torch.equal(_bits(was[..., cols]), _bits(after[n][..., cols])), (what, n)


# ---- a. the whole stack replayed -----------------------------------------------------------------------------------------------

def test_the_whole_stack_is_the_four_models_on_every_tick():
    """reset(), then 60 ticks with resets on the device on ticks 5, 10, ...: after every call the randomizer's state, body, world
    keys and ext, the scan rows, the delivered obs and final_obs, the applied action, the sensor state and rings, est_obs and the
    estimator state are what env_stack.Replay makes of the recorded simulator state and clean observations; the three draw rows
    are 1 + episode_count.  Lower bounds from the settings: resets >= 10 B (a time limit of 5 ticks) and every delay of both ranges
    (tests/test_env_stack_cpu.py).  Printed and asserted non-zero only, nobody having measured them: pushed robot-ticks and ticks
    with a false or a missed foot contact in closed loop (figures: LAB_NOTES.md, "Composed env")."""
    t0 = time.perf_counter()
    T = 60
    env = _stack()
    replay = _replay(env)
    env.reset()
    assert replay.mismatches(replay.host_reset(None, _np(env.sim.state), _np(env.true_obs.t())), _got(env)) == []
    assert bool((_draw_rows(env) == 1).all()) and bool((env.sim.terrain.keys != torch.arange(B, device=DEV)).all())
    actions = _actions(T)
    resets = pushed = pushed_ticks = false_ticks = missed_ticks = noisy = 0
    delays = [set(), set()]
    for t in range(T):
        rec = _before(env, actions[t])
        env.step(actions[t])
        rec.update(_after(env))
        got = _got(env)
        assert replay.mismatches(replay.step(rec), got) == [], t
        assert bool((_draw_rows(env) == (1 + env.episode_count)[None, :]).all()), t
        resets += int(rec["reset_mask"].sum())
        on = (got["ext"] != 0).any(0)
        pushed, pushed_ticks = pushed + int(on.sum()), pushed_ticks + bool(on.any())
        seen, true = got["est_obs"]["contact"] != 0, rec["sim_obs0"]["contact"] != 0
        false_ticks, missed_ticks = false_ticks + bool((seen & ~true).any()), missed_ticks + bool((~seen & true).any())
        noisy += int((got["obs"] != rec["true_obs"]).sum())
        delays[0] |= set(got["sensor_state"][SM.ROW_OBS_DELAY].tolist())
        delays[1] |= set(got["sensor_state"][SM.ROW_ACT_DELAY].tolist())
    print("env stack replay: ulp", {n: round(v, 3) for n, v in replay.worst.items()}, "resets", resets, "pushed robot-ticks", pushed, "of", T * B,
          "ticks with a push", pushed_ticks, "ticks with a false contact", false_ticks, "with a missed contact", missed_ticks, "of", T,
          "delivered values off the clean ones", noisy, "seconds", round(time.perf_counter() - t0, 2))
    assert resets >= 10 * B
    assert 0 < pushed < T * B and pushed_ticks > 0
    assert delays == [{0.0, 1.0, 2.0}, {0.0, 1.0}]
    assert false_ticks + missed_ticks > 0 and noisy > 0
    assert set(replay.worst) == set(ES.ROUNDED)
    env.close()


# ---- b. the sensor model is transparent to the plant ---------------------------------------------------------------------------

def test_the_plant_under_the_sensor_model_is_the_plant_given_the_applied_action():
    T = 40
    a, b = _stack(), _stack(without=("sensor_model",))
    a.reset()
    b.reset()
    actions = _actions(T)

    def same(t):
        for n in ("reward", "done", "reset_mask", "episode_state"):
            assert torch.equal(_bits(getattr(a, n)), _bits(getattr(b, n))), (t, n)
        assert torch.equal(_bits(a.sim.state), _bits(b.sim.state)), t
        assert torch.equal(_bits(a.randomizer.state), _bits(b.randomizer.state)) and torch.equal(_bits(a.randomizer.body()), _bits(b.randomizer.body())), t
        assert torch.equal(a.sim.terrain.keys, b.sim.terrain.keys) and torch.equal(_bits(a.state_estimator.state), _bits(b.state_estimator.state)), t
        for n in srb_abi.OBS_FIELDS:
            assert torch.equal(_bits(a.est_obs[n]), _bits(b.est_obs[n])), (t, n)
        assert torch.equal(_bits(a.true_obs), _bits(b.obs)) and torch.equal(_bits(a.true_final_obs), _bits(b.final_obs)), t

    same(-1)
    for t in range(T):
        a.step(actions[t])
        b.step(a.sensor_model.act_out.clone())
        same(t)
    assert int(a.episode_count.sum()) >= (T // ES.EPISODE_TICKS) * B and bool((a.obs != a.true_obs).any())
    assert not torch.equal(a.sensor_model.act_out, actions[T - 1])                         # B was not simply given the policy's action
    a.close()
    b.close()


# ---- c. the three defaults together are the identity ---------------------------------------------------------------------------

def test_the_three_default_models_together_change_nothing():
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain, SensorModel, StateEstimator
    from robot_gym_amd.sim.height_scan import HeightScan
    T = 40
    make = lambda **kw: BatchedGoEnv(B, device=DEV, terrain=RandomTerrain(), height_scan=HeightScan(), **ES.STACK["env"], **kw)   # noqa: E731
    plain, env = make(), make(randomizer=DomainRandomizer(), sensor_model=SensorModel(), state_estimator=StateEstimator())
    assert torch.equal(_bits(plain.reset()), _bits(env.reset())) and torch.equal(_bits(plain.sim.state), _bits(env.sim.state))
    actions = _actions(T)
    for t in range(T):
        p, e = plain.step(actions[t]), env.step(actions[t])
        for x, y in zip(p, e):
            assert torch.equal(_bits(x), _bits(y)), t
        assert torch.equal(_bits(plain.final_obs), _bits(env.final_obs)) and torch.equal(plain.reset_mask, env.reset_mask), t
        assert torch.equal(_bits(plain.sim.state), _bits(env.sim.state)) and torch.equal(_bits(plain.ctl.extra["grf"]), _bits(env.ctl.extra["grf"])), t
        assert torch.equal(_bits(plain.episode_state), _bits(env.episode_state)), t
    assert int(env.episode_count.sum()) >= (T // ES.EPISODE_TICKS) * B and bool((_draw_rows(env) == (1 + env.episode_count)[None, :]).all())
    plain.close()
    env.close()


# ---- d. a partial host reset -----------------------------------------------------------------------------------------------------

def test_a_partial_host_reset_draws_for_its_robots_and_leaves_the_others_bytes():
    env = _stack(auto_reset=False)
    replay = _replay(env)
    env.reset()
    assert replay.mismatches(replay.host_reset(None, _np(env.sim.state), _np(env.true_obs.t())), _got(env)) == []
    actions = _actions(3)
    for t in range(3):
        rec = _before(env, actions[t])
        env.step(actions[t])
        rec.update(_after(env, auto_reset=False))
        assert replay.mismatches(replay.step(rec), _got(env)) == [], t
    idx = np.arange(0, B, 3)
    inside = torch.zeros(B, dtype=torch.bool, device=DEV)
    inside[torch.as_tensor(idx, device=DEV)] = True
    before, draws0, keys0 = _snapshot(_model_tensors(env)), _draw_rows(env), env.sim.terrain.keys.clone()
    env.reset(idx, targets=[ES.OK_TARGETS[k % len(ES.OK_TARGETS)] for k in range(len(idx))])
    want = replay.host_reset(idx, _np(env.sim.state), _np(env.true_obs.t()))
    assert replay.mismatches(want, _got(env)) == []                                        # its scan among it, in the new world
    assert torch.equal(_draw_rows(env), draws0 + inside.to(torch.int64)[None, :])
    assert bool((env.sim.terrain.keys != keys0)[inside].all())
    sm, est = env.sensor_model, env.state_estimator
    assert bool((sm.obs_ring[:, :, inside] == sm.obs_out[None][:, :, inside]).all())        # the rings hold the first delivered observation
    assert bool((est.state[EM.ROW_RUN:EM.ROW_RUN + 4][:, inside] == float(EM.RUN_MAX)).all()) and bool((est.state[EM.ROW_TICKS, inside] == 0).all())
    _unchanged(before, _model_tensors(env), ~inside, "outside idx")
    # a refused host reset writes nothing, for anybody
    before = _snapshot(_model_tensors(env))
    with pytest.raises(ValueError, match="at least 2"):
        env.reset([1, 3], [ES.OK_TARGETS[0], ES.REFUSED_ON_THE_HOST])
    _unchanged(before, _model_tensors(env), torch.ones(B, dtype=torch.bool, device=DEV), "refused")
    env.close()


# ---- e. a device reset by hand, with plans that fail ---------------------------------------------------------------------------

def test_a_device_reset_by_hand_draws_only_for_the_robots_it_reset_and_frozen_robots_stay_frozen():
    """Robots b % 4 in (0, 1) are reset on the host after tick 3, so after tick 6 they are three ticks old and the others ended on
    tick 5.  The mask takes b % 4 in (1, 2): not done and done, in it and outside it.  The targets go by b // 4 % 3: one that
    plans, one that fails (ES.FAIL_TARGETS, by turns), NaN (drawn on the device)."""
    env = _stack(auto_reset=False)
    replay = _replay(env)
    env.reset()
    replay.host_reset(None, _np(env.sim.state), _np(env.true_obs.t()))
    actions = _actions(16)
    robots = np.arange(B)

    def tick(t):
        # done on an earlier tick and not reset since: frozen through this one (env.done itself stays 1 over a reset by hand)
        frozen, true0, sim0 = torch.as_tensor(replay.frozen.copy(), device=DEV), env.true_obs.clone(), env.sim.state.clone()
        rec = _before(env, actions[t])
        _, reward, done = env.step(actions[t])
        rec.update(_after(env, auto_reset=False))
        assert replay.mismatches(replay.step(rec), _got(env)) == [], t
        assert torch.equal(_bits(env.true_obs[frozen]), _bits(true0[frozen])), t
        assert bool((reward[frozen] == 0).all()) and bool((done[frozen] == 1).all()), t
        moved = (env.sim.state[:3] != sim0[:3]).any(0) & frozen                            # the simulator goes on integrating a frozen robot ...
        live = ((env.true_obs != true0)[:, ES.PATH_ROWS:].any(1) & ~frozen)                # ... and the others' scans do move
        return np.array([int(frozen.sum()), int(moved.sum()), int(live.sum())])

    for t in range(3):
        tick(t)
    idx = robots[robots % 4 < 2]
    env.reset(idx, targets=[ES.OK_TARGETS[k % len(ES.OK_TARGETS)] for k in range(len(idx))])
    assert replay.mismatches(replay.host_reset(idx, _np(env.sim.state), _np(env.true_obs.t())), _got(env)) == []
    for t in range(3, 6):
        tick(t)
    done = _np(env.done) != 0
    assert done[robots % 4 >= 2].all() and not done[robots % 4 < 2].all()                   # the time limit, on tick 5
    mask = ((robots % 4 == 1) | (robots % 4 == 2)).astype(np.int32)
    kind = (robots // 4) % 3
    targets = np.full((B, 2), np.nan)
    for b in robots:
        if kind[b] == 0:
            targets[b] = ES.OK_TARGETS[(b // 12) % len(ES.OK_TARGETS)]
        elif kind[b] == 1:
            targets[b] = ES.FAIL_TARGETS[(b // 12) % len(ES.FAIL_TARGETS)]
    tensors = lambda: dict(_model_tensors(env), obs=env.sensor_model.obs_out, true_obs=env._obs_cm, done=env.done,      # noqa: E731
                           **{"est_" + n: env.est_obs[n] for n in srb_abi.OBS_FIELDS})
    before, draws0 = _snapshot(tensors()), _draw_rows(env)
    env.reset_on_device(torch.as_tensor(mask, device=DEV), torch.as_tensor(targets, device=DEV))
    env.ctl.reset_masked(env.reset_mask)
    was_reset, status = _np(env.reset_mask) != 0, _np(env.plan_status)
    assert np.array_equal(was_reset, (mask != 0) & (status == 0))
    assert was_reset[(mask != 0) & (kind == 0)].all() and not was_reset[kind == 1].any() and (status[(mask != 0) & (kind == 1)] != 0).all()
    for want in (True, False):                                                             # done and not done among the reset and among the failed
        assert (done[was_reset] == want).any() and (done[(mask != 0) & (kind == 1)] == want).any()
    assert was_reset[(mask != 0) & (kind == 2)].any()                                      # drawn targets that planned
    on = torch.as_tensor(was_reset, device=DEV)
    assert torch.equal(_draw_rows(env), draws0 + on.to(torch.int64)[None, :])              # reset_mask == 0: a draw in none of the three streams
    _unchanged(before, tensors(), ~on, "not reset")                                        # and no byte moved; a failed one stays done among it
    assert replay.mismatches(replay.device_reset(was_reset, _np(env.sim.state), _np(env.true_obs.t())), _got(env)) == []
    frozen, moved, live = sum(tick(t) for t in range(6, 16))
    assert frozen >= 10 * int((done & ~was_reset).sum()) > 0 and moved > 0 and live > 0
    # a host reset of some robots leaves a frozen one's observation too
    idx = robots[robots % 8 == 0]
    still = torch.as_tensor(replay.frozen & (robots % 8 != 0), device=DEV)
    true0 = env.true_obs.clone()
    env.reset(idx, targets=[ES.OK_TARGETS[k % len(ES.OK_TARGETS)] for k in range(len(idx))])
    assert replay.mismatches(replay.host_reset(idx, _np(env.sim.state), _np(env.true_obs.t())), _got(env)) == []
    assert int(still.sum()) > 0 and torch.equal(_bits(env.true_obs[still]), _bits(true0[still]))
    env.close()


# ---- f. a clone under the whole stack --------------------------------------------------------------------------------------------

def test_a_clone_under_the_whole_stack_continues_as_its_source():
    batch = 32
    env = _stack(batch)
    env.reset()
    actions = _actions(33, batch, seed=2)
    for t in range(3):
        env.step(actions[t])
    src = np.arange(16)
    dst = src + 16                                                                         # dst = src modulo 16
    env.clone(src, dst)
    dr, sm, est, keys = env.randomizer, env.sensor_model, env.state_estimator, env.sim.terrain.keys
    pushed = 0
    for t in range(3, 33):                                                                 # across the resets on ticks 5, 10, ...
        a = actions[t].clone()
        a[dst] = a[src]
        obs, reward, done = env.step(a)
        pairs = dict(obs=obs.t(), final_obs=env.final_obs.t(), reward=reward, done=done, sim_state=env.sim.state, ext=dr.ext, body=dr.body(), keys=keys,
                     dr_state=dr.state, sensor_state=sm.state, est_state=est.state, obs_ring=sm.obs_ring, act_ring=sm.act_ring,
                     **{"est_" + n: env.est_obs[n] for n in srb_abi.OBS_FIELDS})
        for n, v in pairs.items():
            assert torch.equal(_bits(v[..., src]), _bits(v[..., dst])), (t, n)
        pushed += int((dr.ext[:, dst] != 0).any(0).sum())
    assert int(env.episode_count[dst].min()) >= 6 and pushed > 0 and len(torch.unique(keys[src])) == 16
    env.close()


# ================================================================================================================================
# STACK_FULL: the same stack with a floor that has friction and motors between the controller and the body (tests/env_stack.py)
# ================================================================================================================================

def _stack_full(batch, **env_kw):
    """The env of ES.STACK_FULL: STACK's plus friction=, a MotorModel with the limits of ES.limit_rows, and a randomizer that draws mu
    and the strengths; env_kw over STACK_FULL's."""
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import DomainRandomizer, MotorModel, RandomTerrain, SensorModel, StateEstimator
    from robot_gym_amd.sim.height_scan import HeightScan
    full = ES.STACK_FULL
    motors = MotorModel(strength=full["motors"]["strength"], torque_limit=torch.as_tensor(ES.limit_rows(batch)))
    return BatchedGoEnv(batch, device=DEV, terrain=RandomTerrain(**full["terrain"]), height_scan=HeightScan(**full["height_scan"]),
                        randomizer=DomainRandomizer(**full["randomizer"]), sensor_model=SensorModel(**full["sensor_model"]),
                        state_estimator=StateEstimator(**_grouped(full["state_estimator"])), motor_model=motors, **{**full["env"], **env_kw})


def _after_full(env, auto_reset=True):
    """_after plus the controller's outputs of the tick and the force the motors delivered."""
    out = env.ctl.extra
    return dict(_after(env, auto_reset), grf=_np(out["grf"]), foot_target=_np(out["foot_target"]), leg_state=_np(out["leg_state"]),
                delivered=_np(env.sim.motors.grf))


def _got_full(env):
    sim, mot = env.sim, env.sim.motors
    return dict(_got(env), mu=_np(sim.mu), strength=_np(mot.strength), torque_limit=_np(mot.torque_limit), delivered=_np(mot.grf), tau_cmd=_np(mot.tau_cmd),
                tau=_np(mot.tau), sim_state=_np(sim.state), sim_obs={n: _np(sim.obs[n]) for n in srb_abi.OBS_FIELDS}, touch=_np(sim.touch), slip=_np(sim.slip))


def _full_tensors(env):
    """_model_tensors plus the floor's and the motors' rows."""
    sim, mot = env.sim, env.sim.motors
    return dict(_model_tensors(env), mu=sim.mu, slip=sim.slip, strength=mot.strength, torque_limit=mot.torque_limit)


# ---- a. the full stack replayed ----------------------------------------------------------------------------------------------

def test_the_full_stack_is_its_seven_units_on_every_tick():
    """B = 67 (four waves and three robots), reset(), then 60 ticks with resets on the device on ticks 10, 20, ...: after every call
    the four units of STACK and mu, the strengths and the limits (bit for bit), the delivered force and the two torque tables (the
    rule of test_kernel_against_the_motor_model, on the recorded angles and the controller's recorded grf) and the simulator's
    state, observation, touch and slip (the friction model over the random terrain with measured contact, stepped once from the
    recorded state on the body, mu and world held before the step's reset, the model's push and the DEVICE's delivered force) are
    what env_stack.Replay makes of the record.  Only the robots of a step's reset_mask are left out of the plant's comparison.
    resets >= 5 B follows from the time limit of 10 ticks; the other counts are asserted non-zero only, nobody having measured
    them before this run (figures: LAB_NOTES.md, "Composed env").  The share of stance legs left out of the motors' comparison
    for lying near a limit is at most 1 %."""
    t0 = time.perf_counter()
    T, batch = 60, 67
    env = _stack_full(batch)
    replay = _replay(env, ES.STACK_FULL)
    assert replay.full and _np(env.sim.motors.torque_limit).tobytes() == replay.limit.tobytes()
    env.reset()
    assert replay.mismatches(replay.host_reset(None, _np(env.sim.state), _np(env.true_obs.t())), _got_full(env)) == []
    assert bool((_draw_rows(env) == 1).all())
    assert bool((env.sim.mu != ES.FRICTION_START).all()) and bool((env.sim.motors.strength != 1.0).all())       # the first draw is in
    actions = _actions(T, batch)
    for t in range(T):
        rec = _before(env, actions[t])
        env.step(actions[t])
        rec.update(_after_full(env))
        assert replay.mismatches(replay.step(rec), _got_full(env)) == [], t
        assert bool((_draw_rows(env) == (1 + env.episode_count)[None, :]).all()), t
    c = replay.count
    share = c["near_limit"] / max(c["force_legs"], 1)
    print("full stack replay: ulp", {n: round(v, 3) for n, v in replay.worst.items()}, "plant", replay.cmp.worst, "tick", replay.worst_tick, "counts", c,
          "of", T * batch, "robot-ticks; near-limit share", share, "seconds", round(time.perf_counter() - t0, 2))
    assert c["resets"] >= 5 * batch
    assert c["compared"] == T * batch - c["resets"]                                         # nothing else was skipped
    assert c["sliding"] > 0 and c["clipped"] > 0
    assert 0 < c["pushed"] < T * batch
    assert c["force_legs"] > 0 and c["solved"] == c["force_legs"]                          # strength != 1: every leg with a force took the solve
    assert share <= 0.01
    assert set(replay.worst) == set(ES.ROUNDED)
    env.close()


# ---- b. the defaults ---------------------------------------------------------------------------------------------------------

def test_the_defaults_of_floor_motors_and_models_together_change_nothing():
    """friction="inf" (the friction tick with every robot gripping), MotorModel() and the three default models against the bare env,
    both with terrain, measured contact, the scan and the time limit on: bit-identical over 40 ticks under auto-reset."""
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import DomainRandomizer, MotorModel, RandomTerrain, SensorModel, StateEstimator
    from robot_gym_amd.sim.height_scan import HeightScan
    T = 40
    kw0 = {k: v for k, v in ES.STACK_FULL["env"].items() if k != "friction"}              # measured contact, auto-reset, ten ticks an episode
    make = lambda **kw: BatchedGoEnv(B, device=DEV, terrain=RandomTerrain(), height_scan=HeightScan(), **kw0, **kw)   # noqa: E731
    plain = make()
    env = make(friction="inf", motor_model=MotorModel(), randomizer=DomainRandomizer(), sensor_model=SensorModel(), state_estimator=StateEstimator())
    assert plain.sim.mu is None and plain.sim.motors is None and env.sim.mu is not None and env.sim.motors is not None
    assert torch.equal(_bits(plain.reset()), _bits(env.reset())) and torch.equal(_bits(plain.sim.state), _bits(env.sim.state))
    actions = _actions(T)
    for t in range(T):
        p, e = plain.step(actions[t]), env.step(actions[t])
        for x, y in zip(p, e):                                                             # obs, reward, done
            assert torch.equal(_bits(x), _bits(y)), t
        assert torch.equal(_bits(plain.sim.state), _bits(env.sim.state)) and torch.equal(plain.sim.touch, env.sim.touch), t
        assert torch.equal(plain.reset_mask, env.reset_mask) and torch.equal(_bits(plain.final_obs), _bits(env.final_obs)), t
        assert torch.equal(_bits(env.sim.motors.grf), _bits(env.ctl.extra["grf"])) and bool((env.sim.slip == 0).all()), t
    assert int(env.episode_count.sum()) >= (T // ES.EPISODE_TICKS_FULL) * B
    plain.close()
    env.close()


# ---- c. a partial host reset -------------------------------------------------------------------------------------------------

def test_a_partial_host_reset_draws_floor_and_motors_for_its_robots_at_their_own_draw_counts():
    """Two partial resets, of every second robot and then of every third: a robot of both draws at draw count 2 while its neighbours
    draw at 1.  The robots of a reset hold the model's mu and strengths; for the others every byte of mu, slip, strength and
    torque_limit (and of the three models) stays; torque_limit stays for everybody."""
    env = _stack_full(B, auto_reset=False)
    replay = _replay(env, ES.STACK_FULL)
    env.reset()
    assert replay.mismatches(replay.host_reset(None, _np(env.sim.state), _np(env.true_obs.t())), _got_full(env)) == []
    limit0 = env.sim.motors.torque_limit.clone()
    actions = _actions(6)
    t = 0
    for every in (2, 3):
        for _ in range(3):
            rec = _before(env, actions[t])
            env.step(actions[t])
            rec.update(_after_full(env, auto_reset=False))
            assert replay.mismatches(replay.step(rec), _got_full(env)) == [], t
            t += 1
        idx = np.arange(0, B, every)
        inside = torch.zeros(B, dtype=torch.bool, device=DEV)
        inside[torch.as_tensor(idx, device=DEV)] = True
        before, draws0 = _snapshot(_full_tensors(env)), _draw_rows(env)
        env.reset(idx, targets=[ES.OK_TARGETS[k % len(ES.OK_TARGETS)] for k in range(len(idx))])
        assert replay.mismatches(replay.host_reset(idx, _np(env.sim.state), _np(env.true_obs.t())), _got_full(env)) == []
        assert torch.equal(_draw_rows(env), draws0 + inside.to(torch.int64)[None, :])
        after = _full_tensors(env)
        _unchanged(before, after, ~inside, f"outside every {every}")
        assert bool((after["mu"][inside] != before["mu"][inside]).all()) and bool((after["strength"][:, inside] != before["strength"][:, inside]).all())
        assert torch.equal(_bits(env.sim.motors.torque_limit), _bits(limit0))
    assert set(_draw_rows(env)[0].tolist()) == {1, 2, 3}                                   # reset(): 1; one partial reset: 2; both: 3
    env.close()


# ---- d. a clone under the full stack -----------------------------------------------------------------------------------------

def test_a_clone_under_the_full_stack_takes_floor_and_motors_along():
    """dst = src + 32 (dst = src modulo 16), taken on tick 3 of an episode: mu, slip, strength, torque_limit, tau and the delivered
    grf go with the robot; for 30 ticks, across the resets on ticks 10, 20, 30, the clone's state, touch, slip and delivered force are
    its source's bit for bit, and at every reset the clone draws the mu and the strengths its source draws."""
    env = _stack_full(B)
    env.reset()
    actions = _actions(33, B, seed=2)
    for t in range(3):
        env.step(actions[t])
    src = np.arange(32)
    dst = src + 32
    sim, mot = env.sim, env.sim.motors
    rows = lambda: dict(mu=sim.mu, slip=sim.slip, strength=mot.strength, torque_limit=mot.torque_limit, tau=mot.tau, tau_cmd=mot.tau_cmd, grf=mot.grf.t())   # noqa: E731
    for n in ("mu", "strength", "torque_limit", "tau", "grf"):
        assert not torch.equal(rows()[n][..., src], rows()[n][..., dst]), n                # they differ before
    env.clone(src, dst)
    for n, v in rows().items():
        assert torch.equal(_bits(v[..., src]), _bits(v[..., dst])), n
    assert _np(mot.torque_limit)[:, :32].tobytes() == np.ascontiguousarray(ES.limit_rows(B)[:, :32]).tobytes()
    mu0, strength0 = sim.mu.clone(), mot.strength.clone()
    slid = clipped = 0
    for t in range(3, 33):
        a = actions[t].clone()
        a[dst] = a[src]
        env.step(a)
        pairs = dict(rows(), sim_state=sim.state, touch=sim.touch, reset_mask=env.reset_mask, obs=env.obs.t())
        for n, v in pairs.items():
            assert torch.equal(_bits(v[..., src]), _bits(v[..., dst])), (t, n)
        slid += int((sim.slip[:, dst] > 0).sum())
        clipped += int((mot.tau[:, dst] != mot.tau_cmd[:, dst] * mot.strength[:, dst]).sum())
    assert int(env.episode_count[dst].min()) >= 3
    assert bool((sim.mu != mu0).all()) and bool((mot.strength != strength0).all())         # drawn again since, the same for both
    assert len(torch.unique(sim.mu[src])) == 32 and slid > 0 and clipped > 0
    env.close()
