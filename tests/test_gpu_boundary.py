"""GPU tests of the boundary pieces: motor-model kernel against reference goldens, the drop-in
MPCController and the batched VecEnv against the oracle (stub robots stand in for PyBullet), reset
semantics, and size-independent properties at BASELINE batch 4096."""
import os

import numpy as np
import pytest
import torch

from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd import synthetic
from tests import helpers

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_motor_model_kernel_matches_reference_goldens():
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    d = np.load(os.path.join(G, "motor_model.npz"))
    n = d["action"].shape[0]
    ctl = BatchedMPCController(n, MPCConfig.for_robot("ghost"), extra_outputs=False)
    act = torch.from_numpy(d["action"]).cuda()
    q = torch.from_numpy(np.ascontiguousarray(d["q"].T.astype(np.float32))).cuda()
    qd = torch.from_numpy(np.ascontiguousarray(d["qd"].T.astype(np.float32))).cuda()
    tau = ctl.hybrid_to_torque(act, q, qd).cpu().numpy()
    # float32 output of a float64 evaluation of the reference formula
    np.testing.assert_array_equal(tau, d["tau"].astype(np.float32))
    ctl.close()


def test_motor_model_over_action_repeat_matches_reference_goldens():
    """rg_mpc_hybrid_to_torque_substeps: one launch for the ACTION_REPEAT = 10 sub-steps of a control tick
    (reference core/simulation.py:175-179 -> simple_motor.py:128-140), bit-exact against the reference-generated fixture."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    d = np.load(os.path.join(G, "motor_model_substeps.npz"))
    n, S = d["q"].shape[0], d["q"].shape[1]
    ctl = BatchedMPCController(n, MPCConfig.for_robot("ghost"), extra_outputs=False)
    act = torch.from_numpy(d["action"]).cuda()
    q = torch.from_numpy(np.ascontiguousarray(d["q"].transpose(1, 2, 0).astype(np.float32))).cuda()      # [S,12,B]
    qd = torch.from_numpy(np.ascontiguousarray(d["qd"].transpose(1, 2, 0).astype(np.float32))).cuda()
    tau = ctl.hybrid_to_torque(act, q, qd)
    assert tuple(tau.shape) == (S, n, 12)
    np.testing.assert_array_equal(tau.cpu().numpy(), d["tau"].transpose(1, 0, 2).astype(np.float32))
    # the single-step entry point is the S = 1 case
    one = ctl.hybrid_to_torque(act, q[3].contiguous(), qd[3].contiguous())
    np.testing.assert_array_equal(one.cpu().numpy(), tau[3].cpu().numpy())
    with pytest.raises(ValueError):
        ctl.hybrid_to_torque(act, q[:, :11].contiguous(), qd[:, :11].contiguous())
    # the raw pointers behind `action` and `out` are checked too (wrong shape / dtype / stride / device would be an
    # out-of-bounds device access, not an exception)
    for bad_act in (act[:, :59].contiguous(), act.double(), act.t().contiguous().t(), act.cpu(), act[: n - 1].contiguous()):
        with pytest.raises(ValueError):
            ctl.hybrid_to_torque(bad_act, q, qd)
    for bad_out in (torch.empty(n, 12, device="cuda"), torch.empty(S, n, 12, dtype=torch.float64, device="cuda"), torch.empty(S, n, 12)):
        with pytest.raises(ValueError):
            ctl.hybrid_to_torque(act, q, qd, out=bad_out)
    with pytest.raises(ValueError):
        ctl.hybrid_to_torque(act, q.cpu(), qd.cpu())
    good = torch.empty(S, n, 12, device="cuda")
    assert ctl.hybrid_to_torque(act, q, qd, out=good) is good and torch.equal(good, tau)
    ctl.close()


from tests.fake_envs import StubRobot as _StubRobot, FakeGoEnv, SplitGoEnv, FakeRobotGymEnv


def test_dropin_mpc_controller_single_robot(oracle_lib):
    """config 1 plumbing: the Controller plugin surface, one robot, state pulled through Robot getters."""
    from robot_gym_amd.controllers.mpc.mpc_controller import MPCController
    from robot_gym_amd.controllers.controller import Controller
    cfg = MPCConfig.for_robot("ghost")
    state, cmd, t_off = synthetic.make_states(4, cfg, seed=8)
    clock = {"t": 0.37}
    robot = _StubRobot(cfg, state, 2)
    assert MPCController.MOTOR_CONTROL_MODE == 3 and issubclass(MPCController, Controller)
    ctl = MPCController(robot, lambda: clock["t"])
    assert hasattr(ctl.kinematics_model, "MapContactForceToJointTorques") and hasattr(ctl.kinematics_model, "ComputeMotorAnglesFromFootLocalPosition")
    assert MPCController.get_standing_action() == (0., 0.)
    ctl.reset()                                   # reset_time = clock()
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, 1)
    ob.states[0].reset_time = 0.37
    sub = {k: v[:, 2:3] for k, v in state.items() if k != "_flip"}
    for k, params in enumerate([(0.3, -0.1), (0.2, 0.05, 0.1), (0.2, 0.05, 0.1)]):
        clock["t"] = 0.37 + 0.01 * (k + 1)
        robot.contact = np.array([(k + i) % 2 == 0 for i in range(4)])
        ctl.update_controller_params(params)
        act = ctl.get_action()
        assert act.shape == (60,) and act.dtype == np.float32
        p3 = np.array([[params[0]], [0.0 if len(params) == 2 else params[1]], [params[-1]]], dtype=np.float32)
        inp = helpers.oracle_inputs(oracle_lib, sub, helpers.cmd_with_offsets(cfg, p3), robot.contact.astype(np.int32).reshape(4, 1))
        ref = ob.step(clock["t"], inp)
        m = helpers.compare_tick({"action": act[None]}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5 and m["gains"] == 0.0, m
    tau = ctl.kinematics_model.MapContactForceToJointTorques(1, [1.0, 2.0, 3.0])
    J = state["jac"][:, 2].reshape(4, 3, 3)[1].astype(np.float64)
    np.testing.assert_allclose([tau[3], tau[4], tau[5]], np.array([1.0, 2.0, 3.0]) @ J, rtol=1e-12)


def test_vec_env_one_batched_call_per_tick(oracle_lib):
    """MPCVecEnv over envs that keep their own step(): commands as the envs derive them (GoEnv clipping / standing action),
    one rg_mpc_step per tick, actions identical to B separate oracle controllers fed the same states."""
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    cfg = MPCConfig.for_robot("ghost")
    B = 8
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=12)
    envs = [(SplitGoEnv if b % 2 else FakeGoEnv)(cfg, state, b, BatchSlotController, on_target=(b == 5)) for b in range(B)]
    venv = MPCVecEnv(envs)                      # config and Jacobians come from the envs' own slot controllers
    assert len(venv) == B and venv[3] is envs[3]
    obs = venv.reset()
    assert obs.shape == (B, 2)
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, B)
    clean = {k: v for k, v in state.items() if k != "_flip"}
    rng = np.random.default_rng(12)
    for k in range(5):
        actions = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
        o, r, d, info = venv.step(actions)
        assert o.shape == (B, 2) and r.shape == (B,) and d.shape == (B,) and len(info) == B and venv.batched_calls == k + 1
        want = np.stack([np.clip(actions[:, 0], 0, 0.35), np.zeros(B), np.clip(actions[:, 1], -0.4, 0.4)]).astype(np.float32)
        want[:, 5] = 0.0                        # env 5 is on target: the controller's standing action
        ref = ob.step(0.01 * k, helpers.oracle_inputs(oracle_lib, clean, helpers.cmd_with_offsets(cfg, want), np.ones((4, B), dtype=np.int32)))
        got = np.stack([e.simulation.applied[-1] for e in envs])
        m = helpers.compare_tick({"action": got}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (k, m)
    venv.close()
    assert all(e.closed for e in envs)


def test_vec_env_partial_reset_including_env_0(oracle_lib):
    """Advisor finding of round 1: resetting env 0 alone must not move the gait clock of any other env.  Envs 0 and 3 are
    reset mid-episode; every env is compared with its own oracle controller (fresh ones for the two that were reset),
    leg states and gait phase included."""
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    cfg = MPCConfig.for_robot("ghost")
    B = 6
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=19)
    envs = [FakeRobotGymEnv(cfg, state, b, BatchSlotController) for b in range(B)]
    venv = MPCVecEnv(envs)
    venv.controller.close()
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    venv.controller = BatchedMPCController(B, cfg, device=venv._dev, extra_outputs=True)   # leg states / phase for the comparison
    venv.reset()
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, B)
    clean = {k: v for k, v in state.items() if k != "_flip"}
    coff = helpers.cmd_with_offsets(cfg, cmd)
    clock = np.zeros(B)                      # each env's own GetTimeSinceReset()
    ones = np.ones((4, B), dtype=np.int32)
    for k in range(40):
        if k == 17:
            venv.reset([0, 3])               # Simulation.reset(): clock back to 0, controller.reset()
            ob.reset([0, 3], 0.0)
            clock[[0, 3]] = 0.0
        venv.step(cmd.T.copy())
        ref = helpers.oracle_step_each(oracle_lib, ob, clock, helpers.oracle_inputs(oracle_lib, clean, coff, ones))
        clock = np.array([e.simulation.GetTimeSinceReset() for e in envs])
        got = np.stack([e.simulation.applied[-1] for e in envs])
        m = helpers.compare_tick({"action": got, "leg_state": venv.controller.extra["leg_state"].cpu().numpy(),
                                  "desired_state": venv.controller.extra["desired_state"].cpu().numpy(),
                                  "phase": venv.controller.extra["phase"].cpu().numpy()}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (k, m)
        assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["phase_bits"] == 0, (k, m)
    assert clock[0] == clock[3] and clock[1] > clock[0]
    venv.close()


def test_vec_env_two_handles_on_one_gpu_match_one_handle():
    """MPCVecEnv(devices=[0, 0]): the gym side of BASELINE configs[3] as far as one GPU can show it -- two controller handles
    and two streams (here on the same device), contiguous shards of ONE pinned state buffer and ONE action slab, no collective --
    gives bit-identical action rows to the single-handle wrapper over the same envs, a partial reset that crosses the shard
    boundary included (envs 30 and 31 sit on either side of it).  include/rg_mpc.h: "a process driving several GPUs keeps one
    handle per device"; API: reference agents/ppo/tools/batch_env.py:18-115."""
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    cfg = MPCConfig.for_robot("ghost")
    B = 62
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=23)
    rng = np.random.default_rng(23)
    acts = rng.uniform(-1, 1, (30, B, 2)).astype(np.float32)

    def run(devices):
        envs = [(SplitGoEnv if b % 2 else FakeGoEnv)(cfg, state, b, BatchSlotController) for b in range(B)]
        venv = MPCVecEnv(envs, devices=devices)
        venv.reset()
        rows, obs = [], []
        for k in range(30):
            if k == 13:
                venv.reset([5, 30, 31, 60])
            o, r, d, info = venv.step(acts[k])
            rows.append(np.stack([e.simulation.applied[-1] for e in envs]))
            obs.append(o)
        n = (len(venv.controllers), venv.batched_calls, [c.batch for c in venv.controllers])
        venv.close()
        return rows, obs, n
    rows1, obs1, n1 = run(None)
    rows2, obs2, n2 = run([0, 0])
    assert n1 == (1, 30, [62]) and n2 == (2, 30, [31, 31])
    for k, (a, b) in enumerate(zip(rows1, rows2)):
        assert np.array_equal(a, b), (k, float(np.abs(a - b).max()))
    assert all(np.array_equal(a, b) for a, b in zip(obs1, obs2))
    assert np.isfinite(rows2[-1]).all() and np.abs(rows2[-1]).max() > 1.0   # real commands, not zeros


# route: (worker processes, None = envs in this process; devices, None = one handle).  B = 13 over 2 or 3 shards gives uneven
# shards, and the worker slices ([0, 4) [4, 8) [8, 13), or [0, 6) [6, 13)) cross the shard boundaries.
VEC_ENV_ROUTES = {
    "in_process": (None, None),
    "in_process_3": (None, [0, 0, 0]),
    "workers": (3, None),
    "workers_2": (3, [0, 0]),
    "workers_3": (2, [0, 0, 0]),
    "workers_2_body_rows": (3, [0, 0]),
}
ROUTE_B, ROUTE_TICKS, ROUTE_SEED = 13, 30, 29
# env 0, and envs on both sides of every shard boundary (6|7; 4|5, 8|9) and worker boundary (3|4, 7|8; 5|6)
ROUTE_RESETS = {9: [0, 4, 6, 7, 9, 12], 19: [0, 2, 5, 8, 11]}


def _run_vec_env_route(O, route, fleet):
    """One MPCVecEnv over FakeRobotGymEnvs (observation: [GetTimeSinceReset(), steps applied]), checked tick by tick against
    B separate oracle controllers, each stepped at the clock its env reported before the tick.  fleet "ghost": one config;
    "body_rows": alternating ghost / k3lso planner models, no config= (per-robot body rows and offsets).  The configs are made
    here and handed to the envs, so that worker processes run the lane grid this suite runs with.
    Returns the action rows and observations of every tick and the worst figures over the run."""
    import functools
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    from robot_gym_amd.core.sharding import shard_bounds
    from tests.fake_envs import make_fake_env
    from tests.test_body_rows import RowOracle, k3lso_body, offsets_of
    workers, devices = VEC_ENV_ROUTES[route]
    B = ROUTE_B
    cfg = MPCConfig.for_robot("ghost")
    cfgs = [cfg if fleet == "ghost" or b % 2 == 0 else k3lso_body(cfg) for b in range(B)]
    ctors = [functools.partial(make_fake_env, "base", "ghost", ROUTE_SEED, B, b, config=cfgs[b]) for b in range(B)]
    if workers:
        venv = MPCVecEnv(blocking=False, constructors=ctors, workers=workers, devices=devices)
    else:
        venv = MPCVecEnv([c() for c in ctors], devices=devices)
    try:
        assert (venv.body_rows is not None) == (fleet == "body_rows")
        clean = {k: v for k, v in synthetic.make_states(B, cfg, seed=ROUTE_SEED)[0].items() if k != "_flip"}
        ob = RowOracle(O, cfgs, np.zeros(B)).ob
        acts = np.random.default_rng(ROUTE_SEED).uniform(-1, 1, (ROUTE_TICKS, B, 3)).astype(np.float32)
        ones = np.ones((4, B), dtype=np.int32)
        clock = venv.reset()[:, 0].copy()          # every env's own GetTimeSinceReset(), read from its observation
        assert clock.dtype == np.float64 and not clock.any()
        rows, obs, worst = [], [], {}
        for k in range(ROUTE_TICKS):
            if k in ROUTE_RESETS:
                idx = ROUTE_RESETS[k]
                clock[idx] = venv.reset(idx)[:, 0]
                assert not clock[idx].any()
                ob.reset(idx, 0.0)
            o, r, d, info = venv.step(acts[k])
            got = {"action": venv._act_host.numpy().copy()}
            for name in ("leg_state", "desired_state", "phase"):
                got[name] = np.concatenate([c.extra[name].cpu().numpy() for c in venv.controllers])
            coff = (acts[k].T + offsets_of(cfgs)).astype(np.float32)
            ref = helpers.oracle_step_each(O, ob, clock, helpers.oracle_inputs(O, clean, coff, ones))
            m = helpers.compare_tick(got, ref)
            assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (route, k, m)
            assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["phase_bits"] == 0, (route, k, m)
            for key in ("tau_rel_max", "q_abs"):
                worst[key] = max(worst.get(key, 0.0), m[key])
            assert np.all(o[:, 0] > clock)
            clock = o[:, 0].copy()
            rows.append(got["action"])
            obs.append(o)
        # the resets did what the test needs: at least two different clocks in every shard and every worker slice
        spans = [shard_bounds(B, s, len(devices or [0])) for s in range(len(devices or [0]))]
        spans += [(w.lo, w.lo + w.n) for w in venv._workers]
        assert all(len(set(clock[lo:hi])) >= 2 for lo, hi in spans), (spans, clock)
    finally:
        venv.close()
    return rows, obs, worst


@pytest.mark.parametrize("route", list(VEC_ENV_ROUTES))
def test_vec_env_routes_match_per_env_oracles(oracle_lib, monkeypatch, route):
    """Every way MPCVecEnv gets envs to the kernels -- envs in this process or in worker processes, one handle or several --
    against B separate float64 oracle controllers, robot by robot, after two partial resets that leave different clocks in
    every shard and worker slice.  With worker processes the state of every env travels through one shared slab; its clock
    rows hold B float64 values back to back, which a copy by column would hand to the wrong shard.  Each route's action rows
    are also bit-identical to those of the in-process, one-handle route over the same fleet."""
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController

    class WithExtras(BatchedMPCController):   # leg states and gait phase for the comparison
        def __init__(self, batch, cfg=None, device=None, extra_outputs=False):
            super().__init__(batch, cfg, device=device, extra_outputs=True)
    monkeypatch.setattr(vec_env, "BatchedMPCController", WithExtras)
    fleet = "body_rows" if route.endswith("_body_rows") else "ghost"
    rows, obs, worst = _run_vec_env_route(oracle_lib, route, fleet)
    print(f"route {route}: worst over {ROUTE_B} robots x {ROUTE_TICKS} ticks:", worst)
    if route != "in_process":
        rows1, obs1, _ = _run_vec_env_route(oracle_lib, "in_process", fleet)
        for k in range(ROUTE_TICKS):
            assert np.array_equal(rows[k], rows1[k]), (route, k, float(np.abs(rows[k] - rows1[k]).max()))
            assert np.array_equal(obs[k], obs1[k]), (route, k)


def test_partial_reset_matches_fresh_controllers(oracle_lib):
    """rg_mpc_reset on a subset == new oracle controllers for that subset (LocomotionController.reset)."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    cfg = MPCConfig.for_robot("ghost")
    B = 32
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=14, phase_offsets=False)
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, B)
    ctl = BatchedMPCController(B, cfg)
    ctl.update_controller_params(torch.from_numpy(cmd.T.copy()))
    coff = helpers.cmd_with_offsets(cfg, cmd)
    dev = {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
    idx = [1, 7, 8, 30]
    for k in range(30):
        t = 0.01 * k
        if k == 17:
            ctl.reset(idx, t0=t)
            ob.reset(idx, t)
        contact = synthetic.gait_consistent_contacts(cfg, np.full(B, t), state["_flip"])
        dev["contact"] = torch.from_numpy(contact).cuda()
        act = ctl.get_action(t, dev).cpu().numpy()
        ref = ob.step(t, helpers.oracle_inputs(oracle_lib, state, coff, contact))
        m = helpers.compare_tick({"action": act, "leg_state": ctl.extra["leg_state"].cpu().numpy(), "desired_state": ctl.extra["desired_state"].cpu().numpy(),
                                  "phase": ctl.extra["phase"].cpu().numpy()}, ref)
        assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (k, m)
    with pytest.raises(Exception):
        ctl.reset([B + 3])
    ctl.close()


def test_full_size_properties_batch_4096():
    """BASELINE batch: properties that need no oracle -- determinism, permutation equivariance
    (binning order must not leak into results), constraint satisfaction, swing legs carry no force."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    cfg = MPCConfig.for_robot("ghost")
    B = 4096
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=0)
    contact = synthetic.gait_consistent_contacts(cfg, t_off + 0.02, state["_flip"])
    names = ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")

    def run(perm):
        ctl = BatchedMPCController(B, cfg)
        ctl.reset_at(-t_off[perm])
        ctl.update_controller_params(torch.from_numpy(cmd.T[perm].copy()))
        dev = {n: torch.from_numpy(np.ascontiguousarray(state[n][:, perm])).cuda() for n in names}
        dev["contact"] = torch.from_numpy(np.ascontiguousarray(contact[:, perm])).cuda()
        for k in range(3):
            act = ctl.get_action(0.01 * k, dev)
        out = (act.cpu().numpy().copy(), ctl.extra["grf"].cpu().numpy().copy(), ctl.extra["desired_state"].cpu().numpy().copy(), ctl.bin_counts())
        ctl.close()
        return out

    ident = np.arange(B)
    a1, g1, d1, bins = run(ident)
    a2, g2, d2, _ = run(ident)
    assert np.array_equal(a1, a2) and np.array_equal(g1, g2)                 # bit-exact determinism
    perm = np.random.default_rng(1).permutation(B)
    a3, g3, d3, _ = run(perm)
    assert np.array_equal(a3, a1[perm]) and np.array_equal(g3, g1[perm])     # equivariance
    assert sum(bins) == B and bins[2] > 0 and bins[4] > 0
    f = -g1.reshape(B, 4, 3).astype(np.float64)                               # force on the body
    stance = d1 == 1
    mg = cfg.mass * cfg.gravity
    assert np.abs(f[~stance]).max() == 0.0
    fz = f[..., 2][stance]
    assert fz.min() >= 0.1 * mg * (1 - 1e-5) and fz.max() <= 10 * mg * (1 + 1e-5)
    assert (np.abs(f[..., 0][stance]) <= 0.45 * fz * (1 + 1e-5) + 1e-4).all()
    assert (np.abs(f[..., 1][stance]) <= 0.45 * fz * (1 + 1e-5) + 1e-4).all()
    assert np.isfinite(a1).all()


def test_parity_at_baseline_batch_4096(oracle_lib):
    """Full BASELINE batch against the oracle for two ticks (the oracle needs a few seconds on the GPU
    box's host cores): catches tails of the fixed-iteration ADMM that small batches miss."""
    cfg = MPCConfig.for_robot("ghost")
    state, cmd, t_off = synthetic.make_states(4096, cfg, seed=0)
    orc = helpers.run_oracle(oracle_lib, cfg, state, cmd, t_off, ticks=2, jitter=0.1)
    gpu = helpers.run_gpu(cfg, state, cmd, t_off, ticks=2, jitter=0.1)
    worst = 0.0
    for g, o in zip(gpu, orc):
        m = helpers.compare_tick(g, o)
        assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["phase_bits"] == 0, m
        assert m["tau_rel_max"] <= 1e-4 and m["grf_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, m
        worst = max(worst, m["tau_rel_max"])
    helpers.assert_audit_clean(gpu[-1]["audit"], min_audited=4)
    print("worst relative torque error over 8192 robot-ticks:", worst, gpu[-1]["audit"])


def test_step_argument_validation_reports_errors():
    """Bad calls come back as RgMpcError with the library's message (status codes never leak as crashes)."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.core.mpc_abi import RgMpcError
    cfg = MPCConfig.for_robot("ghost")
    state, cmd, t_off = synthetic.make_states(8, cfg, seed=1)
    ctl = BatchedMPCController(8, cfg)
    dev = {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
    dev["contact"] = torch.ones(4, 8, dtype=torch.int32, device="cuda")
    ctl.update_controller_params(torch.zeros(8, 3))
    with pytest.raises(KeyError):
        ctl.get_action(0.0, {k: v for k, v in dev.items() if k != "jac"})          # kin_mode 0 needs Jacobians
    with pytest.raises(ValueError):
        ctl.get_action(0.0, dict(dev, rpy=dev["rpy"].double()))                    # wrong dtype
    with pytest.raises(ValueError):
        ctl.update_controller_params(torch.zeros(8, 4))                             # (vx, wz) or (vx, vy, wz) only
    with pytest.raises(RgMpcError):
        ctl._handle.reset([99], 0.0)                                                # index out of range
    act = ctl.get_action(0.0, dev)                                                  # still usable afterwards
    assert torch.isfinite(act).all()
    ctl.close()


def test_introspection_views_agree():
    """Per-robot iteration view, solver statistics, bin counts and the packed host staging slab describe the same step."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController, PackedState
    cfg = MPCConfig.for_robot("ghost")
    B = 257
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=5)
    contact = synthetic.gait_consistent_contacts(cfg, t_off + 0.03, state["_flip"])
    ctl = BatchedMPCController(B, cfg)
    ctl.reset_at(-t_off)
    ctl.update_controller_params(torch.from_numpy(cmd.T.copy()))
    ps = PackedState(B, ctl.device)
    for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac"):
        ps.host[n].copy_(torch.from_numpy(np.ascontiguousarray(state[n])))
    ps.host["contact"].copy_(torch.from_numpy(contact))
    act_packed = ctl.get_action(0.03, ps.upload()).cpu().numpy().copy()
    it, nc = ctl._handle.last_iterations(B, ctl._stream())
    stats, bins = ctl.solver_stats(), ctl.bin_counts()
    assert int(it.sum()) == stats["iters_sum"] and int(it.max()) == stats["iters_max"]
    assert [int((nc == k).sum()) for k in range(5)] == list(bins)
    assert stats["qp_robots"] == int((nc > 0).sum()) and np.all(it[nc == 0] == 0) and np.all(it[nc > 0] > 0)
    assert ctl._handle.profile_window_names()[1] == "rg_qp_fused_kernel"
    # same step from separately allocated device tensors (fresh controller): identical actions
    ctl2 = BatchedMPCController(B, cfg)
    ctl2.reset_at(-t_off)
    ctl2.update_controller_params(torch.from_numpy(cmd.T.copy()))
    dev = {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
    dev["contact"] = torch.from_numpy(contact).cuda()
    assert np.array_equal(ctl2.get_action(0.03, dev).cpu().numpy(), act_packed)
    # and through rg_mpc_step_host (upload, step, download and wait in one call across the ABI): identical again
    ctl3 = BatchedMPCController(B, cfg)
    ctl3.reset_at(-t_off)
    ctl3.update_controller_params(torch.from_numpy(cmd.T.copy()))
    ps3 = PackedState(B, ctl3.device)
    ps3.host_slab.copy_(ps.host_slab)
    act_host = torch.zeros(B, 60, dtype=torch.float32, pin_memory=True)
    ctl3.bind_host_state(ps3, act_host)
    assert ctl3.get_action_host(0.03) is act_host and np.array_equal(act_host.numpy(), act_packed)
    with pytest.raises(ValueError):
        ctl3.bind_host_state(ps3, torch.zeros(B, 60))                     # not pinned
    with pytest.raises(ValueError):
        ctl3.bind_host_state(PackedState(B + 1, ctl3.device), act_host)   # another batch
    ctl.close(); ctl2.close(); ctl3.close()


def test_non_finite_state_is_counted_and_contained(oracle_lib):
    """Robots whose state holds a NaN / Inf are reported in `failures` (their command is meaningless: the cone
    projection's fmin/fmax turn NaNs into finite numbers); every other robot of the batch still matches the oracle."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    cfg = MPCConfig.for_robot("ghost")
    B = 96
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=17)
    bad = [5, 40]
    state["rpy"][0, bad[0]] = np.nan
    state["foot_pos"][2, bad[1]] = np.inf
    gpu = helpers.run_gpu(cfg, state, cmd, t_off, ticks=2)
    assert gpu[-1]["solver_stats"]["failures"] == len(bad)
    good = np.array([b for b in range(B) if b not in bad])
    clean = {k: (v[:, good] if hasattr(v, "shape") and v.ndim == 2 else v) for k, v in state.items()}
    orc = helpers.run_oracle(oracle_lib, cfg, clean, cmd[:, good], t_off[good], ticks=2)
    for g, o in zip(gpu, orc):
        m = helpers.compare_tick({"action": g["action"][good]}, o)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, m


def test_parity_config5_batch_4096_horizon_20(oracle_lib):
    """BASELINE configs[4] as specified: batch 4096, horizon 20, per-robot duty ~ U(0.5, 0.8), caller-supplied
    contact schedule with 10 % random drop-outs.  Two ticks against the oracle (240-variable exact QPs: ~10 s per tick on the
    GPU box's host cores), no failures, torques within 1e-4."""
    cfg = MPCConfig.for_robot("ghost", horizon=20, contact_lookahead=1)
    B = 4096
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=0)
    gait = synthetic.random_gaits(B, cfg, seed=0)
    sched_fn = lambda k, t_rel: synthetic.contact_schedule(cfg, t_rel, gait, dropout=0.1, seed=0, tick=k)
    gpu = helpers.run_gpu(cfg, state, cmd, t_off, ticks=2, jitter=0.1, gait=gait, sched_fn=sched_fn, poison=False)
    orc = helpers.run_oracle(oracle_lib, cfg, state, cmd, t_off, ticks=2, jitter=0.1, gait=gait, sched_fn=sched_fn)
    worst = 0.0
    for g, o in zip(gpu, orc):
        m = helpers.compare_tick(g, o)
        assert g["solver_stats"]["failures"] == 0, g["solver_stats"]
        assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["phase_bits"] == 0, m
        assert m["tau_rel_max"] <= 1e-4 and m["grf_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, m
        worst = max(worst, m["tau_rel_max"])
    helpers.assert_audit_clean(gpu[-1]["audit"], min_audited=4)
    print("config 5, worst relative torque error over 8192 robot-ticks:", worst, gpu[-1]["solver_stats"], gpu[-1]["audit"])


def test_batch_32768_properties_and_sampled_parity(oracle_lib):
    """BASELINE configs[3] per-node total (8 x 4096) on one GPU: every robot gets a finite, constraint-satisfying command,
    no failures, the stance-leg bins add up; a 256-robot sample of the batch matches the oracle run on just those robots."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    cfg = MPCConfig.for_robot("ghost")
    B = 32768
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=0)
    ctl = BatchedMPCController(B, cfg)
    ctl.reset_at(-t_off)
    ctl.update_controller_params(torch.from_numpy(cmd.T.copy()))
    names = ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")
    dev = {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in names}
    sample = np.random.default_rng(5).choice(B, 256, replace=False)
    sub = {k: (v[:, sample] if hasattr(v, "ndim") and v.ndim == 2 else v) for k, v in state.items()}
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, len(sample))
    for i, b in enumerate(sample):
        ob.states[i].reset_time = -float(t_off[b])
    coff = helpers.cmd_with_offsets(cfg, cmd)
    for k in range(3):
        contact = synthetic.gait_consistent_contacts(cfg, t_off + 0.01 * k, state["_flip"])
        dev["contact"] = torch.from_numpy(contact).cuda()
        act = ctl.get_action(0.01 * k, dev).cpu().numpy()
        ref = ob.step(0.01 * k, helpers.oracle_inputs(oracle_lib, sub, coff[:, sample], contact[:, sample]))
        m = helpers.compare_tick({"action": act[sample]}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5 and m["gains"] == 0.0, (k, m)
    stats, bins = ctl.solver_stats(), ctl.bin_counts()
    assert stats["failures"] == 0 and sum(bins) == B and np.isfinite(act).all()
    helpers.assert_audit_clean(ctl.audit_stats(), min_audited=6)
    f = -ctl.extra["grf"].cpu().numpy().astype(np.float64).reshape(B, 4, 3)
    stance = ctl.extra["desired_state"].cpu().numpy() == 1
    mg = cfg.mass * cfg.gravity
    assert np.abs(f[~stance]).max() == 0.0
    fz = f[..., 2][stance]
    assert fz.min() >= 0.1 * mg * (1 - 1e-5) and fz.max() <= 10 * mg * (1 + 1e-5)
    assert (np.abs(f[..., 0][stance]) <= 0.45 * fz * (1 + 1e-5) + 1e-4).all() and (np.abs(f[..., 1][stance]) <= 0.45 * fz * (1 + 1e-5) + 1e-4).all()
    ctl.close()


def test_bench_under_torchrun_world_size_1(tmp_path):
    """The multi-GPU code path on the one GPU a test box has: bench.py launched by torch.distributed.run as a FRESH child
    process (nothing here re-execs a process that touched the GPU), nccl (= RCCL) process group with device_id, the optional
    action all-gather inside the timed step, the barrier / MAX-over-ranks timing, the JSON contract.  No scaling claim."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(root, "bench.py"), "--gpus", "1", "--allgather", "--steps", "3", "--warmup", "1",
           "--batch", "512", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out")]
    res = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    line = [l for l in res.stdout.splitlines() if l.startswith("{") and '"metric"' in l][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["allgather"] is True and out["config"]["admm_iterations"]["failures"] == 0
    assert out["roofline"]["kernel"] == "rg_qp_fused_kernel" and out["roofline"]["avg_launch_ms"] > 0
    # --dump-outputs: the last timed step's action slab, and the all-gathered one (the same rows at world size 1)
    act, gathered = np.load(tmp_path / "out" / "action.npy"), np.load(tmp_path / "out" / "action_allgathered.npy")
    assert act.dtype == np.float32 and act.shape == (512, 60) and np.isfinite(act).all() and np.abs(act).max() > 0
    assert np.array_equal(gathered, act)


def test_bench_self_launch_one_rank(tmp_path):
    """`python bench.py --gpus N` starts its own ranks when RANK is not set (the driver's form for the scaling runs).  On the
    one GPU of a test box: --force-launcher makes --gpus 1 go through the same launcher -- a fresh torch.distributed.run child,
    started before the parent has touched the GPU -- and the --full line reports the RCCL world, per-rank kernel times and both
    the with- and without-all-gather rates."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--force-launcher", "--full", "--steps", "3", "--warmup", "1",
                          "--batch", "512", "--no-cpu-baseline"], cwd=root, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    c = out["config"]
    assert out["n_gpus"] == 1 and c["rccl_ranks"] == 1 and c["backend"] == "nccl" and c["dry_launch"] is False
    assert c["with_allgather_steps_per_s"] > 0 and c["without_allgather_steps_per_s"] == out["value"]
    assert len(c["kernel_ms_per_rank"]) == 1 and c["kernel_ms_per_rank"][0][1] > 0
    assert c["admm_iterations"]["failures"] == 0 and c["audit"]["audit_over_tol"] == 0


def test_bench_plain_run_reports_only_the_timed_pass(tmp_path):
    """`python bench.py --gpus 1` without --full: set-up, warm-up, the timed steps (with their per-kernel events: the
    roofline), --dump-outputs and the line -- no side pass and no CPU baseline, whose fields stay null / absent."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "512",
                          "--dump-outputs", str(tmp_path / "out")], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])
    c = out["config"]
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0 and out["dtype"] == "f64"
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 512) < 1e-6 * 512
    assert out["roofline"]["kernel"] == "rg_qp_fused_kernel" and out["roofline"]["avg_launch_ms"] > 0
    assert c["admm_iterations"]["failures"] == 0 and c["rccl_ranks"] == 1 and c["without_allgather_steps_per_s"] == out["value"]
    assert "cpu_baseline" not in out
    for k in ("static_inputs_steps_per_s", "cold_start_steps_per_s", "steady_state_steps_per_s", "audit_off_steady_state_steps_per_s",
              "sustained", "pcie_inclusive_steps_per_s", "dropin_get_action_latency_us", "with_allgather_steps_per_s"):
        assert c[k] is None, k
    act = np.load(tmp_path / "out" / "action.npy")
    assert act.shape == (512, 60) and np.isfinite(act).all()


def test_set_gait_validation_and_return_to_config_gait(oracle_lib):
    """rg_mpc_set_gait: shape errors are reported; an out-of-range row makes ITS robot a counted, contained failure every
    tick (the others still match the oracle); passing nothing returns to the config-wide gait."""
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    cfg = MPCConfig.for_robot("ghost")
    B = 24
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=71)
    gait = synthetic.random_gaits(B, cfg, seed=71)
    ctl = BatchedMPCController(B, cfg)
    with pytest.raises(ValueError):
        ctl.set_gait(gait["stance_duration"][:, :5], gait["duty_factor"], gait["init_phase"])
    with pytest.raises(Exception):
        ctl.set_gait(stance_duration=gait["stance_duration"])          # duty factor and phase must come with it
    bad = dict(gait, duty_factor=gait["duty_factor"].copy())
    bad["duty_factor"][:, 3] = 1.5
    bad["duty_factor"][:, 9] = float("nan")
    ctl.set_gait(**bad)
    ctl.reset_at(-t_off)
    ctl.update_controller_params(torch.from_numpy(cmd.T.copy()))
    dev = {n: torch.from_numpy(np.ascontiguousarray(state[n])).cuda() for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
    good = np.array([b for b in range(B) if b not in (3, 9)])
    sub = {k: (v[:, good] if hasattr(v, "ndim") and v.ndim == 2 else v) for k, v in state.items()}
    gsub = {k: v[:, good] for k, v in gait.items()}
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, len(good), gait=gsub)
    for i, b in enumerate(good):
        ob.states[i].reset_time = -float(t_off[b])
    coff = helpers.cmd_with_offsets(cfg, cmd)
    for k in range(4):
        contact = synthetic.gait_consistent_contacts(cfg, t_off + 0.01 * k, state["_flip"], gait)
        dev["contact"] = torch.from_numpy(contact).cuda()
        act = ctl.get_action(0.01 * k, dev).cpu().numpy()
        assert ctl.solver_stats()["failures"] == 2
        assert np.all(act[[3, 9]] == 0.0)
        ref = ob.step(0.01 * k, helpers.oracle_inputs(oracle_lib, sub, coff[:, good], contact[:, good]))
        m = helpers.compare_tick({"action": act[good]}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (k, m)
    # back to the config-wide gait: same as a controller that never had per-robot rows
    ctl.set_gait()
    ctl.reset_at(-t_off)
    ref_ctl = BatchedMPCController(B, cfg)
    ref_ctl.reset_at(-t_off)
    ref_ctl.update_controller_params(torch.from_numpy(cmd.T.copy()))
    dev["contact"] = torch.from_numpy(synthetic.gait_consistent_contacts(cfg, t_off, state["_flip"])).cuda()
    a1 = ctl.get_action(0.0, dev).cpu().numpy().copy()
    a2 = ref_ctl.get_action(0.0, dev).cpu().numpy()
    assert ctl.solver_stats()["failures"] == 0 and np.array_equal(a1, a2)
    ctl.close(); ref_ctl.close()


def test_vec_env_with_device_kinematics(oracle_lib):
    """kin_mode 1 under the VecEnv: only joint angles travel (no foot positions, no Jacobians gathered on the host)."""
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    cfg = MPCConfig.for_robot("k3lso", kin_mode=1)
    B = 6
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=73)
    envs = [FakeRobotGymEnv(cfg, state, b, BatchSlotController, config=cfg) for b in range(B)]
    calls = []
    venv = MPCVecEnv(envs, jacobian_fn=lambda env, leg: calls.append(leg))
    venv.reset()
    ocfg = helpers.oracle_config(oracle_lib, cfg)
    ob = oracle_lib.OracleBatch(ocfg, B)
    clean = {k: v for k, v in state.items() if k != "_flip"}
    for k in range(4):
        venv.step(cmd.T.copy())
        ref = ob.step(0.01 * k, helpers.oracle_inputs(oracle_lib, clean, helpers.cmd_with_offsets(cfg, cmd), np.ones((4, B), dtype=np.int32)))
        m = helpers.compare_tick({"action": np.stack([e.simulation.applied[-1] for e in envs])}, ref)
        assert m["tau_rel_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (k, m)
    assert calls == []
    venv.close()


def test_create_chooses_the_plan_from_config_and_batch():
    """rg_mpc_plan_description: the lane grid follows the batch (256 lanes per robot up to RG_MPC_WIDE_BATCH = 1024 robots under
    the default plan at horizon 10, one wave above; lane_grid forces either), the exact body serves one / two legs under the
    hybrid plan at both horizons, unequal friction coefficients pick the per-leg instantiations."""
    from robot_gym_amd.core.mpc_abi import MpcHandle
    def plan(batch, **over):
        h = MpcHandle(MPCConfig.for_robot("ghost", **{"lane_grid": 0, **over}), batch)   # (0 = the library's own choice, whatever --lane-grid the suite runs with)
        p = h.plan()
        h.close()
        return p
    assert plan(1)["lanes"] == "256" and plan(1024)["lanes"] == "256" and plan(1025)["lanes"] == "64" and plan(4096)["lanes"] == "64"
    assert plan(4096, lane_grid=2)["lanes"] == "256" and plan(64, lane_grid=1)["lanes"] == "64"
    assert plan(64, solver=2)["lanes"] == "64" and plan(64, contact_lookahead=1)["lanes"] == "64"      # the 256-lane grid is the default plan's
    p20 = plan(512, horizon=20)
    assert p20["lanes"] == "256" and p20["exact12"] == "1" and p20["solver"] == "hybrid" and p20["direct"] == "0"
    assert plan(512, horizon=20, contact_lookahead=1)["exact12"] == "0" and plan(512, horizon=20, solver=2)["exact12"] == "0"
    assert plan(8)["mu"] == "uniform" and plan(8, mu=(0.3, 0.45, 0.6, 0.45))["mu"] == "per_leg"
    assert plan(8, audit_k=0)["audit"] == "0" and plan(8)["audit"] == "1" and plan(8, solver=1)["audit"] == "0"
