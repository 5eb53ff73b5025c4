"""Per-robot body models (rg_mpc_set_body): mass, inertia, body height, friction and hip positions per robot in one handle.

Every GPU test compares with oracle controllers configured one by one (OracleBatch.cfgs filled per robot from
helpers.oracle_config), under the bars of the existing parity tests: per-joint torque within 1e-4 of max(|tau_j|, 1 N m),
leg states and phase bit-exact, no solver failure, audit lane clean."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from robot_gym_amd import synthetic
from robot_gym_amd.controllers.mpc.batched import BatchedMPCController, body_rows, check_body_args
from robot_gym_amd.core.config import MPCConfig
from tests import helpers


def k3lso_body(cfg):
    """ghost's config with k3lso's planner model and command offsets (kin_mode 0: what the two robots' configs differ in
    besides the leg chain)."""
    k = MPCConfig.for_robot("k3lso")
    return dataclasses.replace(cfg, body_height=k.body_height, hip=k.hip, mass=k.mass, inertia=k.inertia,
                               vx_offset=k.vx_offset, vy_offset=k.vy_offset, wz_offset=k.wz_offset)


def random_configs(cfg, B, seed):
    """Randomised planner models: mass +-25 %, inertia diagonal +-30 %, body height 0.36-0.44, mu 0.3-0.9 per leg, hips +-1 cm."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        I = np.array(cfg.inertia, dtype=np.float64).reshape(3, 3)
        I[np.diag_indices(3)] *= rng.uniform(0.7, 1.3, 3)
        out.append(dataclasses.replace(cfg, mass=cfg.mass * rng.uniform(0.75, 1.25), inertia=tuple(I.ravel()),
                                       body_height=rng.uniform(0.36, 0.44), mu=tuple(rng.uniform(0.3, 0.9, 4)),
                                       hip=tuple(np.array(cfg.hip) + rng.uniform(-0.01, 0.01, 12))))
    return out


# ---- per-robot oracle runner -------------------------------------------------------------------------------------------
class RowOracle:
    """B oracle controllers, robot b configured from cfgs[b] (and its gait row, if any)."""

    def __init__(self, O, cfgs, t_off, gait=None):
        self.O, self.B = O, len(cfgs)
        self.ob = O.OracleBatch(helpers.oracle_config(O, cfgs[0]), self.B, 0.0, 0)
        self.ob.cfgs = (O.Config * self.B)()
        self.set_cfgs(range(self.B), cfgs, gait)
        for b in range(self.B):
            O.lib().orc_reset(C.byref(self.ob.cfgs[b]), C.byref(self.ob.states[b]), 0.0, None)
            self.ob.states[b].reset_time = -float(t_off[b])

    def set_cfgs(self, idx, cfgs, gait=None):
        for k, b in enumerate(idx):
            c = helpers.oracle_config(self.O, cfgs[k] if len(cfgs) == len(idx) else cfgs[b])
            if gait is not None:
                for l in range(4):
                    c.stance_duration[l] = float(gait["stance_duration"][l][b])
                    c.duty_factor[l] = float(gait["duty_factor"][l][b])
                    c.init_phase[l] = float(gait["init_phase"][l][b])
                    if gait.get("init_state") is not None:
                        c.init_state[l] = int(gait["init_state"][l][b])
            C.memmove(C.byref(self.ob.cfgs[b]), C.byref(c), C.sizeof(c))

    def step(self, t, st, coff, contact):
        return self.ob.step(t, helpers.oracle_inputs(self.O, st, coff, contact))


def offsets_of(cfgs):
    return np.array([[c.vx_offset, c.vy_offset, c.wz_offset] for c in cfgs], dtype=np.float32).T


def gpu_controller(cfg, cfgs, t_off, cmd, gait=None, device="cuda:0", rows=True):
    import torch
    B = len(cfgs)
    ctl = BatchedMPCController(B, cfg, device=device)
    if gait is not None:
        ctl.set_gait(**gait)
    if rows:
        r = body_rows(cfgs)
        ctl.set_body(**{k: r[k] for k in ("mass", "inertia", "body_height", "mu", "hip")})
    ctl.reset_at(-t_off)
    coff = (cmd.astype(np.float32) + offsets_of(cfgs)).astype(np.float32)
    ctl.set_raw_command(torch.from_numpy(coff).to(device))
    return ctl, coff


def gpu_tick(ctl, st, contact, t, device="cuda:0"):
    import torch
    dev = {n: torch.from_numpy(np.ascontiguousarray(st[n])).to(device) for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
    dev["contact"] = torch.from_numpy(contact).to(device)
    ctl._handle.debug_poison_lds(ctl._stream())
    act = ctl.get_action(t, dev)
    torch.cuda.synchronize()
    o = {"action": act.cpu().numpy().copy()}
    for k, v in ctl.extra.items():
        o[k] = v.cpu().numpy().copy()
    o["solver_stats"] = ctl.solver_stats()
    return o


def assert_parity(g, o, where, sample=None):
    if sample is not None:
        g = {k: (v[sample] if isinstance(v, np.ndarray) else v) for k, v in g.items()}
        o = o[sample]
    m = helpers.compare_tick(g, o)
    assert m["tau_rel_elem_max"] <= 1e-4 and m["q_abs"] <= 1e-5, (where, m)
    assert m["leg_state_mismatch"] == 0 and m["desired_mismatch"] == 0 and m["phase_bits"] == 0, (where, m)
    assert g["solver_stats"]["failures"] == 0, (where, g["solver_stats"])


def run_rows_parity(O, cfg, cfgs, ticks, seed, gait=None, jitter=0.1, sample=None, change=None):
    """GPU handle with per-robot rows against per-robot oracles.  change = (tick, idx, new cfgs for idx): rows of a subset
    replaced mid-run (set_body with idx)."""
    B = len(cfgs)
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=seed)
    ro = RowOracle(O, cfgs, t_off, gait)
    ctl, coff = gpu_controller(cfg, cfgs, t_off, cmd, gait)
    cfgs = list(cfgs)
    for k in range(ticks):
        if change is not None and k == change[0]:
            _, idx, new = change
            r = body_rows(new)
            ctl.set_body(idx=idx, **r)
            ro.set_cfgs(idx, new, gait)
        t = k * 0.01
        st = helpers.perturb(state, k, jitter)
        contact = synthetic.gait_consistent_contacts(cfg, t + t_off, state["_flip"], gait)
        g = gpu_tick(ctl, st, contact, t)
        o = ro.step(t, st, coff, contact)
        assert_parity(g, o, k, sample)
    audit = ctl.audit_stats()
    plan = ctl._handle.plan()
    ctl.close()
    return audit, plan


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_body_rows_packs_a_mixed_fleet_and_refuses_other_differences():
    g = MPCConfig.for_robot("ghost")
    k = k3lso_body(g)
    r = body_rows([g, k, g])
    assert r["mass"].shape == (3,) and r["inertia"].shape == (9, 3) and r["body_height"].shape == (3,)
    assert r["mu"].shape == (4, 3) and r["hip"].shape == (12, 3)
    assert list(r["body_height"]) == [0.42, 0.38, 0.42]
    assert r["hip"][1, 1] == -0.105 and r["hip"][1, 0] == -0.1
    with pytest.raises(ValueError, match="admm_rho"):
        body_rows([g, dataclasses.replace(g, admm_rho=2e-4)])
    # the leg chain is not a row: the swing-leg IK uses it in both kin modes
    kin1 = dataclasses.replace(g, kin_mode=1)
    with pytest.raises(ValueError, match="jxyz"):
        body_rows([kin1, dataclasses.replace(MPCConfig.for_robot("k3lso"), kin_mode=1)])
    with pytest.raises(ValueError, match="jxyz"):
        body_rows([g, MPCConfig.for_robot("k3lso")])


def test_set_body_shape_errors_before_any_gpu_call():
    class NoGpu:
        def set_body(self, *a, **kw):
            raise AssertionError("reached the library")
    ctl = BatchedMPCController.__new__(BatchedMPCController)
    ctl.batch, ctl._handle = 4, NoGpu()
    with pytest.raises(ValueError, match="mass"):
        ctl.set_body(mass=np.ones(3))
    with pytest.raises(ValueError, match="inertia"):
        ctl.set_body(inertia=np.ones((4, 9)))
    with pytest.raises(ValueError, match="mu"):
        ctl.set_body(mu=np.ones((4, 2)), idx=[0, 1, 2])
    with pytest.raises(ValueError, match="hip"):
        ctl.set_body(hip=np.ones(12))
    with pytest.raises(ValueError):
        ctl.set_body(idx=[1])
    a = check_body_args(2, inertia=np.stack([np.eye(3), 2 * np.eye(3)]))
    assert a["inertia"].shape == (9, 2) and a["inertia"][0, 1] == 2.0


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_random_rows_match_per_robot_oracles(oracle_lib):
    """All five fields randomised per robot, B = 256, 40 ticks (the suite's --lane-grid picks the lane grid)."""
    cfg = MPCConfig.for_robot("ghost")
    audit, plan = run_rows_parity(oracle_lib, cfg, random_configs(cfg, 256, 3), 40, seed=31)
    assert plan["body"] == "per_robot" and plan["mu"] == "per_leg"
    helpers.assert_audit_clean(audit)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["h20", "lookahead"])
def test_random_rows_horizon20_and_contact_schedule(oracle_lib, variant):
    """The schedule body and its exact re-solves (horizon 20; contact_lookahead with per-robot gait rows)."""
    if variant == "h20":
        cfg, gait = MPCConfig.for_robot("ghost", horizon=20), None
    else:
        cfg = MPCConfig.for_robot("ghost", contact_lookahead=1)
        gait = synthetic.random_gaits(128, cfg, seed=8)
    audit, plan = run_rows_parity(oracle_lib, cfg, random_configs(cfg, 128, 5), 25, seed=33, gait=gait)
    helpers.assert_audit_clean(audit)


@pytest.mark.gpu
def test_mixed_fleet_batch_4096(oracle_lib):
    """Alternating ghost / k3lso planner models at B = 4096, compared on 256 sampled robots."""
    cfg = MPCConfig.for_robot("ghost")
    cfgs = [cfg if b % 2 == 0 else k3lso_body(cfg) for b in range(4096)]
    sample = np.sort(np.random.default_rng(4).choice(4096, 256, replace=False))
    audit, _ = run_rows_parity(oracle_lib, cfg, cfgs, 12, seed=35, sample=sample)
    helpers.assert_audit_clean(audit)


@pytest.mark.gpu
def test_rows_changed_mid_run_keep_parity_and_audit_clean(oracle_lib):
    """A subset's rows replaced at tick 20 (set_body with idx, as on a partial reset); 80 ticks: the audit ring (4 entries x
    8 ticks) wraps more than twice, and no audit re-solve sees rows of another tick."""
    cfg = MPCConfig.for_robot("ghost")
    cfgs = random_configs(cfg, 256, 7)
    idx = list(range(0, 256, 5))
    new = random_configs(cfg, len(idx), 8)
    audit, _ = run_rows_parity(oracle_lib, cfg, cfgs, 80, seed=37, change=(20, idx, new))
    helpers.assert_audit_clean(audit, min_audited=1)


def _run_plain(cfg, B, seed, ticks, prepare):
    import torch
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=seed)
    ctl, _ = gpu_controller(cfg, [cfg] * B, t_off, cmd, rows=False)
    plans = prepare(ctl)
    outs = []
    for k in range(ticks):
        t = k * 0.01
        st = helpers.perturb(state, k, 0.1)
        contact = synthetic.gait_consistent_contacts(cfg, t + t_off, state["_flip"])
        outs.append(gpu_tick(ctl, st, contact, t))
    ctl.close()
    torch.cuda.synchronize()
    return outs, plans


@pytest.mark.gpu
def test_rows_set_then_cleared_are_bit_identical_to_no_rows():
    cfg = MPCConfig.for_robot("ghost")
    B = 256

    def set_clear(ctl):
        r = body_rows(random_configs(cfg, B, 9))
        ctl.set_body(**r)
        p1 = ctl._handle.plan()
        ctl.set_body()
        return p1, ctl._handle.plan()
    a, (p_set, p_clear) = _run_plain(cfg, B, 41, 20, set_clear)
    b, (p_none,) = _run_plain(cfg, B, 41, 20, lambda ctl: (ctl._handle.plan(),))
    assert p_set["body"] == "per_robot" and p_clear["body"] == "config" and p_clear == p_none
    for k, (x, y) in enumerate(zip(a, b)):
        for key in ("action", "grf", "leg_state", "phase"):
            assert np.array_equal(x[key], y[key]), (k, key)


@pytest.mark.gpu
def test_invalid_rows_are_refused_and_leave_the_rows_untouched():
    from robot_gym_amd.core.mpc_abi import RgMpcError
    cfg = MPCConfig.for_robot("ghost")
    B = 64
    good = body_rows(random_configs(cfg, B, 10))

    def bad_calls(ctl):
        ctl.set_body(**good)
        for field, value, robot in (("mass", 0.0, 3), ("inertia", None, 7), ("mu", np.nan, 11)):
            r = {k: v.copy() for k, v in good.items()}
            if field == "inertia":
                r["inertia"][:, robot] = [1, 0, 0, 0, -1, 0, 0, 0, 1]   # not positive definite
            elif field == "mu":
                r["mu"][2, robot] = value
            else:
                r["mass"][robot] = value
            with pytest.raises(RgMpcError) as e:
                ctl.set_body(**r)
            assert e.value.status == -1 and f"robot {robot}" in str(e.value), str(e.value)
        return ()
    a, _ = _run_plain(cfg, B, 43, 10, bad_calls)
    b, _ = _run_plain(cfg, B, 43, 10, lambda ctl: (ctl.set_body(**good), ())[1])
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["action"], y["action"]), k


def _make_env(kind, seed, batch, b):
    """Picklable constructor (worker processes): even envs ghost, odd envs k3lso's planner model, or all one kind.  The slot
    controller gets the config explicitly (from the robot's constants it would take k3lso's leg chain as well, which one handle
    cannot hold per robot: the "k3lso_robot" kind)."""
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeRobotGymEnv
    g = MPCConfig.for_robot("ghost")
    cfg = {"ghost": g, "k3lso": k3lso_body(g), "mixed": g if b % 2 == 0 else k3lso_body(g),
           "bad": g if b % 2 == 0 else dataclasses.replace(g, admm_rho=2e-4),
           "k3lso_robot": g if b % 2 == 0 else MPCConfig.for_robot("k3lso")}[kind]
    state, _, _ = synthetic.make_states(batch, g, seed=seed)
    return FakeRobotGymEnv(cfg, state, b, BatchSlotController, config=cfg)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["in_process", "two_handles", "workers"])
def test_vec_env_mixed_fleet_matches_homogeneous_vec_envs(mode):
    """MPCVecEnv over alternating ghost / k3lso envs (no config=): per-robot rows and offsets; robot b's action matches robot b
    of an all-ghost or all-k3lso MPCVecEnv over the same states."""
    import functools
    from robot_gym_amd.gym.vec_env import MPCVecEnv
    B, seed = 32, 45
    acts = np.random.default_rng(seed).uniform(-1, 1, (8, B, 3)).astype(np.float32)

    def run(kind):
        kw = {"devices": [0, 0]} if mode == "two_handles" else {}
        if mode == "workers":
            venv = MPCVecEnv(constructors=[functools.partial(_make_env, kind, seed, B, b) for b in range(B)], blocking=False, workers=2)
            envs = None
        else:
            envs = [_make_env(kind, seed, B, b) for b in range(B)]
            venv = MPCVecEnv(envs, **kw)
        venv.reset()
        rows = []
        for k in range(8):
            venv.step(acts[k])
            rows.append(venv._act_host.numpy().copy())
        venv.close()
        return rows
    mixed, ghost, k3 = run("mixed"), run("ghost"), run("k3lso")
    for k in range(8):
        want = np.where((np.arange(B) % 2 == 0)[:, None], ghost[k], k3[k])
        a_g, a_w = mixed[k].reshape(B, 12, 5).astype(np.float64), want.reshape(B, 12, 5).astype(np.float64)
        rel = np.abs(a_g[:, :, 4] - a_w[:, :, 4]) / np.maximum(np.abs(a_w[:, :, 4]), 1.0)
        assert rel.max() <= 1e-4 and np.abs(a_g[:, :, 0] - a_w[:, :, 0]).max() <= 1e-5, k
    if mode == "in_process":   # a real k3lso next to a ghost: the leg chains differ (swing-leg IK), refused
        with pytest.raises(ValueError, match="jxyz"):
            MPCVecEnv([_make_env("k3lso_robot", seed, 4, b) for b in range(4)])
    with pytest.raises(ValueError, match="admm_rho"):
        if mode == "workers":
            MPCVecEnv(constructors=[functools.partial(_make_env, "bad", seed, 4, b) for b in range(4)], blocking=False, workers=2)
        else:
            MPCVecEnv([_make_env("bad", seed, 4, b) for b in range(4)])
