"""The motor model on the GPU (include/rg_srb_motor.h, robot_gym_amd/csrc/rg_srb_motor.hip): rg_srb_motor_apply against
tests/motor_model.py at batches around a wave and a workgroup for both robots, with sentinels, in place and with NULL outputs;
its tau_cmd against the controller's own tau_stance in the closed loop; the default model bit-identical to no model in three
simulator configurations and in the go-to env; the closed loop under the torque limit of the CPU reference loop inside that
loop's band (tests/motor_fixtures.py); a clone; rg_srb_motor_draw against the model bit for bit, and the randomiser's draws under
auto_reset replayed into the model; non-identity motors in front of each of the four ticks BatchedSRBSim.step dispatches to, the
delivered force and the tick both held to their models; the kernel's singular branch on a configuration with a foot on its knee
axis; and the settings only the C ABI accepts (strength 0 and +inf, limit 0, NaN and negative, -0.0 and denormal forces).

Every model run is made before the GPU is opened (`dev` depends on `cases`)."""
import numpy as np
import pytest
import torch

from robot_gym_amd.core import dr_abi, motor_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import contact_fixtures as CF
from tests import motor_fixtures as MF
from tests import motor_model as MM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
from tests.posctl_fixtures import REL_TOL, within_ulp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return MF.kernel_cases()


@pytest.fixture(scope="module")
def dev(cases):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


class Guarded:
    """Device buffers with S.PAD sentinels on each side."""

    def __init__(self, dev):
        self.dev, self.backs = dev, []

    def __call__(self, array):
        a = np.ascontiguousarray(array)
        t = torch.as_tensor(a)
        back = torch.full((2 * S.PAD + t.numel(),), S.GUARD, dtype=t.dtype, device=self.dev)
        view = back[S.PAD:S.PAD + t.numel()].view(t.shape)
        view.copy_(t.to(self.dev))
        self.backs.append(back)
        return view

    def intact(self):
        return all(bool((b[:S.PAD] == S.GUARD).all()) and bool((b[-S.PAD:] == S.GUARD).all()) for b in self.backs)


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", MF.BATCHES)
@pytest.mark.parametrize("robot", F.ROBOTS)
def test_kernel_against_the_motor_model(robot, B, cases, dev):
    c = cases[robot, B]
    handle = srb_abi.SrbHandle(c["cfg"], B, dev)
    guard = Guarded(dev)
    state = np.zeros((M.STATE_ROWS, B))
    state[M.ROW_Q:M.ROW_Q + 12] = c["q"]
    st, grf, strength, limit = guard(state), guard(c["grf"]), guard(c["strength"]), guard(c["limit"])
    out, tau_cmd, tau = guard(np.full((B, 12), -5.0, np.float32)), guard(np.full((12, B), -5.0)), guard(np.full((12, B), -5.0))
    motor_abi.motor_apply(handle, st, grf, strength, limit, out, tau_cmd, tau)
    got, got_cmd, got_tau = out.cpu().numpy(), tau_cmd.cpu().numpy(), tau.cpu().numpy()
    assert guard.intact()
    # what is only read stays as it was
    for t, want in ((st, state), (grf, c["grf"]), (strength, c["strength"]), (limit, c["limit"])):
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(want).tobytes()
    passed = np.repeat(~c["sat"].T, 3, axis=1)                       # [B, 12]: the floats of the legs that pass through
    assert got[passed].tobytes() == c["grf"][passed].tobytes() == c["out"][passed].tobytes()
    assert within_ulp(got[~passed], c["out"][~passed].astype(np.float64)).all()
    assert passed.any() or B == 1
    assert (~passed).any() or B == 1
    for g, w in ((got_cmd, c["tau_cmd"]), (got_tau, c["tau"])):
        assert (np.abs(g - w) <= REL_TOL * np.maximum(1.0, np.abs(w))).all(), float(np.abs(g - w).max())
    worst = float(np.abs(got.astype(np.float64) - c["out"]).max())
    print(robot, B, "saturated legs", int(c["sat"].sum()), "of", 4 * B, "largest |grf_out - model|", worst)
    # in place equals out of place
    inplace = guard(c["grf"])
    motor_abi.motor_apply(handle, st, inplace, strength, limit, inplace, tau_cmd, tau)
    assert inplace.cpu().numpy().tobytes() == got.tobytes() and tau.cpu().numpy().tobytes() == got_tau.tobytes()
    # NULL tau_cmd and tau_out are accepted, and the force is the same
    again = guard(np.full((B, 12), -5.0, np.float32))
    tau_cmd.fill_(-5.0)
    tau.fill_(-5.0)
    motor_abi.motor_apply(handle, st, grf, strength, limit, again)
    assert again.cpu().numpy().tobytes() == got.tobytes() and bool((tau_cmd == -5.0).all()) and bool((tau == -5.0).all())
    assert guard.intact()
    handle.close()


def test_a_nan_force_gives_nan_on_its_leg_only_and_bad_arguments_are_refused_by_name(dev):
    import ctypes as C
    c = MF.make_case("ghost", 17)
    handle = srb_abi.SrbHandle(c["cfg"], 17, dev)
    guard = Guarded(dev)
    state = np.zeros((M.STATE_ROWS, 17))
    state[M.ROW_Q:M.ROW_Q + 12] = c["q"]
    g = c["grf"].copy()
    g[16, 10] = np.nan
    limit = c["limit"].copy()
    limit[9:12, 16] = 3.0                                            # a finite limit does not turn it into a number
    want, _, want_tau, _ = MM.apply(M.Chain(c["cfg"]), c["q"], g, c["strength"], limit)
    st, grf, strength, lim = guard(state), guard(g), guard(c["strength"]), guard(limit)
    out, tau = guard(np.zeros((17, 12), np.float32)), guard(np.zeros((12, 17)))
    motor_abi.motor_apply(handle, st, grf, strength, lim, out, None, tau)
    got = out.cpu().numpy()
    assert np.isnan(got[16, 9:12]).all() and np.isnan(want[16, 9:12]).all() and np.isnan(tau.cpu().numpy()[9:12, 16]).all()
    rest = np.ones((17, 12), dtype=bool)
    rest[16, 9:12] = False
    assert np.isfinite(got[rest]).all() and within_ulp(got[rest], want[rest].astype(np.float64)).all() and guard.intact()
    lib, h = motor_abi.load_library(), handle._h
    p = dict(state=st, grf=grf, strength=strength, torque_limit=lim, grf_out=out)
    for name in p:
        a = {k: (None if k == name else v.data_ptr()) for k, v in p.items()}
        rc = lib.rg_srb_motor_apply(h, a["state"], a["grf"], a["strength"], a["torque_limit"], a["grf_out"], None, None, None)
        assert rc == -1 and f"motor_apply: null {name}".encode() in lib.rg_srb_last_error(h), name
    with pytest.raises(ValueError, match="motor_apply: strength"):
        motor_abi.motor_apply(handle, st, grf, strength.cpu(), lim, out)
    with pytest.raises(ValueError, match="motor_apply: tau_out"):
        motor_abi.motor_apply(handle, st, grf, strength, lim, out, None, tau.t())
    assert C.sizeof(C.c_void_p) == 8 and guard.intact()
    handle.close()


# ---- 2. the closed loop ----------------------------------------------------------------------------------------------------

def _pair(robot, batch, dev, motors=None, **sim_kw):
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.sim import BatchedSRBSim
    cfg = MPCConfig.for_robot(robot)
    return cfg, BatchedMPCController(batch, cfg, device=dev), BatchedSRBSim(batch, cfg, device=dev, motors=motors, **sim_kw)


def _start(ctl, sim, cmd, hs):
    sim.reset(height=sim.cfg.body_height * np.asarray(hs))
    ctl.reset()
    ctl.set_raw_command(torch.as_tensor(np.ascontiguousarray(np.asarray(cmd, dtype=np.float32).T), device=sim.device))


def _snap(sim):
    return [sim.state.clone()] + [sim.obs[k].clone() for k in sorted(sim.obs)] + [sim.touch.clone()] + ([] if sim.slip is None else [sim.slip.clone()])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_tau_cmd_is_the_controllers_own_tau_stance(robot, dev):
    """The convention cross-check: the torque the rule derives from grf and the simulator's angles is the torque the controller
    itself reports, within the project's parity bar, 1e-4 of max(|tau|, 1 N m)."""
    from robot_gym_amd.sim import MotorModel
    cmd, hs = F.tiled_cases(robot, 65)
    cfg, ctl, sim = _pair(robot, 65, dev, motors=MotorModel())
    _start(ctl, sim, cmd, hs)
    worst, largest = 0.0, 0.0
    for k in range(60):
        ctl.get_action(0.0, sim.obs)
        sim.step(ctl)
        want = ctl.extra["tau_stance"].t().to(torch.float64)
        got = sim.motors.tau_cmd
        rel = ((got - want).abs() / want.abs().clamp(min=1.0)).max()
        worst, largest = max(worst, float(rel)), max(largest, float(want.abs().max()))
        assert float(rel) <= 1e-4, (k, float(rel))
        assert torch.equal(sim.motors.tau, sim.motors.tau_cmd) and torch.equal(sim.motors.grf, ctl.extra["grf"])
    print(robot, "largest |tau_cmd - tau_stance| / max(|tau|, 1)", worst, "largest |tau_stance|", largest)
    assert largest > 5.0 and int(sim.fallen().sum()) == 0
    ctl.close()
    sim.close()


def _configurations():
    from robot_gym_amd.sim.terrain import RandomTerrain
    return dict(schedule_plane=lambda: dict(), measured_terrain=lambda: dict(contact="measured", terrain=RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED)),
                friction=lambda: dict(friction=0.3))


@pytest.mark.parametrize("name", ["schedule_plane", "measured_terrain", "friction"])
def test_the_default_model_is_bit_identical_to_no_model(name, dev):
    from robot_gym_amd.sim import MotorModel
    cmd, hs = F.tiled_cases("ghost", 65)
    runs = []
    for motors in (None, MotorModel()):
        cfg, ctl, sim = _pair("ghost", 65, dev, motors=motors, **_configurations()[name]())
        assert (sim.motors is None) == (motors is None)
        _start(ctl, sim, cmd, hs)
        snaps = []
        for k in range(50):
            ctl.get_action(0.0, sim.obs)
            sim.step(ctl)
            snaps.append(_snap(sim))
        runs.append(snaps)
        assert int(sim.fallen().sum()) == 0
        ctl.close()
        sim.close()
    for k, (a, b) in enumerate(zip(*runs)):
        assert _same(a, b), (name, k)
    assert not _same(runs[0][0], runs[0][-1])


def test_the_env_with_the_default_model_steps_bit_identically_under_auto_reset(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import MotorModel
    B, T = 65, 50
    rng = np.random.default_rng(2)
    actions = torch.as_tensor(rng.uniform([0.1, -0.3], [0.4, 0.3], (T, B, 2)).astype(np.float32), device=dev)
    runs, resets = [], 0
    for motors in (None, MotorModel()):
        env = BatchedGoEnv(B, device=dev, auto_reset=True, max_time=0.95, seed=3, motor_model=motors)   # the time limit ends every episode on tick 10
        assert (env.sim.motors is None) == (motors is None)
        env.reset()
        outs = []
        for t in range(T):
            env.step(actions[t])
            outs.append([env.obs.clone(), env.final_obs.clone(), env.reward.clone(), env.done.clone(), env.reset_mask.clone(), env.sim.state.clone()])
            resets += int((env.reset_mask != 0).sum())
        runs.append(outs)
        env.close()
    for t, (a, b) in enumerate(zip(*runs)):
        assert _same(a, b), t
    assert resets >= 2 * 4 * B


def _limited_loop(robot, dev, limit_rows):
    """400 ticks of the 32 cases on the plane with schedule contact.  limit_rows: [12, 32] or None (no model) -> (final state,
    saturated leg-ticks of running robots, fallen, worst |tau| per motor over running robots)."""
    from robot_gym_amd.sim import MotorModel
    cmd, hs = F.cases(robot)
    n = len(hs)
    cfg, ctl, sim = _pair(robot, n, dev, motors=None if limit_rows is None else MotorModel(torque_limit=limit_rows))
    _start(ctl, sim, cmd, hs)
    saturated = torch.zeros((), dtype=torch.int64, device=dev)
    worst = torch.zeros(12, dtype=torch.float64, device=dev)
    for k in range(F.TICKS):
        ctl.get_action(0.0, sim.obs)
        running = ~sim.fallen()
        sim.step(ctl)
        if sim.motors is not None:
            differs = (sim.motors.tau != sim.motors.tau_cmd).view(4, 3, n).any(1)
            saturated += (differs & running[None, :]).sum()
            worst = torch.maximum(worst, torch.where(running[None, :], sim.motors.tau.abs(), torch.zeros_like(sim.motors.tau)).amax(1))
    out = sim.state.clone(), int(saturated), int(sim.fallen().sum()), worst.cpu().numpy()
    ctl.close()
    sim.close()
    return out


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_closed_loop_under_a_torque_limit_stays_inside_the_cpu_band(robot, dev):
    """Every limit at LIMIT_FRACTION of the peak torque of the CPU loop without a model, 4 s at batch 32: legs saturate, no torque
    exceeds its limit, and the falls and the saturated leg-ticks are at most twice the CPU reference loop's.  Robots given +inf in
    the same batch walk exactly as without a model."""
    peak = np.asarray(MF.PEAK[robot])
    limit = MF.limit_rows(peak, MF.LIMIT_FRACTION, 32)
    _, saturated, fallen, worst = _limited_loop(robot, dev, limit)
    print(robot, "saturated leg-ticks", saturated, "band", MF.SATURATED_BAND[robot], "fallen", fallen, "band", MF.FALLEN_BAND[robot],
          "worst |tau| / limit", float((worst / limit[:, 0]).max()))
    assert (worst <= limit[:, 0]).all()
    assert 0 < saturated <= MF.SATURATED_BAND[robot] and fallen <= MF.FALLEN_BAND[robot]
    mixed = limit.copy()
    mixed[:, 1::2] = np.inf
    free, _, _, _ = _limited_loop(robot, dev, None)
    some, sat_some, _, _ = _limited_loop(robot, dev, mixed)
    assert sat_some > 0 and torch.equal(some[:, 1::2], free[:, 1::2]) and not torch.equal(some[:, 0::2], free[:, 0::2])


def test_a_cloned_robot_continues_bit_for_bit_with_its_motors(dev):
    from robot_gym_amd.sim import MotorModel, clone
    B = 64
    cmd, hs = F.tiled_cases("k3lso", B)
    rng = np.random.default_rng(9)
    strength = rng.uniform(0.7, 1.1, (12, B))
    limit = np.asarray(MF.PEAK["k3lso"])[:, None] * rng.uniform(0.7, 1.5, (12, B))
    limit[:, 48:] = np.inf
    cfg, ctl, sim = _pair("k3lso", B, dev, motors=MotorModel(strength=strength, torque_limit=torch.as_tensor(limit)))
    _start(ctl, sim, cmd, hs)
    for k in range(30):
        ctl.get_action(0.0, sim.obs)
        sim.step(ctl)
    src, dst = torch.arange(16, device=dev), torch.arange(16, device=dev) + 32          # dst = src modulo 16
    mot = sim.motors
    assert not torch.equal(sim.state[:, src], sim.state[:, dst]) and not torch.equal(mot.strength[:, src], mot.strength[:, dst])
    clone(ctl, sim, src, dst)
    assert torch.equal(mot.strength[:, src], mot.strength[:, dst]) and torch.equal(mot.torque_limit[:, src], mot.torque_limit[:, dst])
    assert mot.strength[:, :32].cpu().numpy().tobytes() == np.ascontiguousarray(strength[:, :32]).tobytes()
    saturated = 0
    for k in range(40):
        ctl.get_action(0.0, sim.obs)
        sim.step(ctl)
        assert torch.equal(sim.state[:, src], sim.state[:, dst]), k
        assert torch.equal(mot.tau[:, src], mot.tau[:, dst]) and torch.equal(mot.grf[src], mot.grf[dst]), k
        saturated += int((mot.tau[:, dst] != mot.tau_cmd[:, dst]).sum())
    assert saturated > 0
    # the setters write the robots named, and None is no limit
    mot.set_strength(0.5, idx=[3])
    mot.set_torque_limit(None, idx=torch.tensor([4], device=dev))
    mot.set_torque_limit(np.full((12, 2), 7.0), idx=[5, 6])
    assert bool((mot.strength[:, 3] == 0.5).all()) and bool(torch.isinf(mot.torque_limit[:, 4]).all()) and bool((mot.torque_limit[:, 5:7] == 7.0).all())
    assert float(mot.strength[0, 2]) == strength[0, 2]
    with pytest.raises(ValueError, match="set_strength: values"):
        mot.set_strength(np.ones((12, 3)), idx=[1, 2])
    ctl.close()
    sim.close()


# ---- 3. the draw and the randomiser ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_motor_draw_is_the_model_bit_for_bit(B, dev):
    handle = srb_abi.SrbHandle(MPCConfig.for_robot("ghost"), B, dev)
    rng = np.random.default_rng(B)
    key = rng.integers(-5000, 5000, B).astype(np.float64)
    draws = rng.integers(0, 40, B).astype(np.float64)
    seed, lo, hi = (1 << 63) + 977 * B, 0.7, 1.0
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    masks = dict(sparse=(rng.uniform(size=B) < 0.3).astype(np.int32), empty=np.zeros(B, np.int32), full=np.ones(B, np.int32))
    masks["sparse"][B - 1] = 1                                  # the last lane of the batch draws
    for name, mask in masks.items():
        guard = Guarded(dev)
        s = guard(np.full((12, B), -7.0))
        want = MM.draw(np.full((12, B), -7.0), mask, key, draws, seed, lo, hi)
        motor_abi.motor_draw(handle, t(mask), t(key), t(draws), seed, lo, hi, s)
        got = s.cpu().numpy()
        assert got.tobytes() == want.tobytes() and guard.intact(), name
        on = mask != 0
        assert (got[:, ~on] == -7.0).all() and (got[:, on] >= lo).all() and (got[:, on] <= hi).all()
    with pytest.raises(ValueError, match="motor_draw"):
        motor_abi.motor_draw(handle, t(masks["full"]), t(key), t(draws), seed, 0.9, 0.2, s)
    with pytest.raises(ValueError, match="motor_draw: strength"):
        motor_abi.motor_draw(handle, t(masks["full"]), t(key), t(draws), seed, lo, hi, s[:4])
    handle.close()


def test_the_randomiser_draws_the_models_strengths_at_every_reset(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import BatchedSRBSim, DomainRandomizer, MotorModel
    B, T, seed, lo, hi = 64, 35, 11, 0.7, 1.0
    dr = DomainRandomizer(motor_strength=(lo, hi), seed=seed)
    env = BatchedGoEnv(B, device=dev, randomizer=dr, motor_model=MotorModel(), auto_reset=True, max_time=0.95, seed=3)   # every episode ends on tick 10
    host = lambda x: x.cpu().numpy()
    mot = env.sim.motors
    key = host(dr.state[dr_abi.ROW_KEY]).copy()
    s = host(mot.strength).copy()
    assert (s == 1.0).all()
    env.reset()                                                 # the host reset draws for every robot, at draw count 0
    MM.draw(s, np.ones(B), key, np.zeros(B), seed, lo, hi)
    assert host(mot.strength).tobytes() == s.tobytes() and (s >= lo).all() and (s <= hi).all() and len(set(s.reshape(-1).tolist())) == 12 * B
    rng = np.random.default_rng(1)
    actions = torch.as_tensor(rng.uniform([0.1, -0.3], [0.4, 0.3], (T, B, 2)).astype(np.float32), device=dev)
    resets = 0
    for t in range(T):
        draws = host(dr.state[dr_abi.ROW_DRAWS]).copy()
        env.step(actions[t])
        mask = host(env.reset_mask) != 0
        MM.draw(s, mask, key, draws, seed, lo, hi)              # a robot that was reset drew at its key and draw count, the others keep theirs
        assert host(mot.strength).tobytes() == s.tobytes(), t
        assert (host(dr.state[dr_abi.ROW_DRAWS]) == draws + mask).all(), t
        resets += int(mask.sum())
    assert resets >= 3 * B and bool(torch.isinf(mot.torque_limit).all())
    env.close()
    # a simulator without a motor model has no rows for the draw
    plain = BatchedSRBSim(5, device=dev)
    assert plain.motors is None
    with pytest.raises(ValueError, match="needs a simulator built with a motor model"):
        DomainRandomizer(motor_strength=(lo, hi)).bind(plain)
    plain.close()


# ---- 4. non-identity motors in front of every tick ---------------------------------------------------------------------------

def _tick_sim_kw(name):
    from robot_gym_amd.sim.terrain import RandomTerrain
    terrain = lambda: RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED)
    return dict(plane_schedule=lambda: dict(), terrain_schedule=lambda: dict(terrain=terrain()),
                terrain_measured=lambda: dict(terrain=terrain(), contact="measured"),
                terrain_friction=lambda: dict(terrain=terrain(), contact="measured", friction=MF.TICK_MU))[name]()


def _tick_run(name, robot, dev, rows, model=False):
    """MF.TICK_T closed-loop ticks of MF.TICK_B robots in configuration `name`.  rows: (strength, limit) or None (motors=None).
    model: hold every tick to the numpy models, resynchronised at the start of the tick: motors.grf to motor_model.apply on the
    controller's grf and the angles before the tick, the tick to the configuration's model stepped on motors.grf.
    -> (the snapshots after every tick, figures of the run)."""
    from robot_gym_amd.sim import MotorModel
    from tests import terrain_model as TM
    B = MF.TICK_B
    cmd, hs = F.tiled_cases(robot, B)
    motors = None if rows is None else MotorModel(strength=rows[0], torque_limit=torch.as_tensor(rows[1]))
    cfg, ctl, sim = _pair(robot, B, dev, motors=motors, **_tick_sim_kw(name))
    _start(ctl, sim, cmd, hs)
    host = lambda t: t.cpu().numpy()
    if model:
        t = sim.terrain
        ground = None if t is None else TM.Random(t.amplitude, t.cell, t.seed, host(t.keys))
        m, step = MF.tick_model(name, cfg, B, ground)
        chain, cmp = M.Chain(cfg), S.Comparison()
    fig = dict(worst_grf=0.0, worst_tau=0.0, worst_slip=0.0, changed=0, clipped=0, slid=0, touched=0)
    snaps = []
    for k in range(MF.TICK_T):
        state0, obs0 = host(sim.state), {n: host(v) for n, v in sim.obs.items()}
        ctl.get_action(0.0, sim.obs)
        sim.step(ctl)
        snaps.append(_snap(sim))
        if not model:
            continue
        out = {n: host(ctl.extra[n]) for n in ("grf", "foot_target", "desired_state", "leg_state")}
        mot = sim.motors
        planned, delivered = out["grf"], host(mot.grf)
        want = MM.apply(chain, state0[M.ROW_Q:M.ROW_Q + 12], planned, rows[0], rows[1])
        bad, worst, worst_tau = MF.delivered_mismatches(planned, want, (delivered, host(mot.tau_cmd), host(mot.tau)))
        assert bad == [], (name, k, bad)
        fig["worst_grf"], fig["worst_tau"] = max(fig["worst_grf"], worst), max(fig["worst_tau"], worst_tau)
        changed = (delivered.view(np.int32) != planned.view(np.int32)).reshape(B, 4, 3).any(2)
        assert changed.any(), (name, k)                          # delivered != planned on some leg of every tick
        fig["changed"] += int(changed.sum())
        fig["clipped"] += int((np.abs(want[2]) == rows[1]).sum())
        # the tick, from the simulator's state and observation before it, on the DELIVERED force
        m.state[:] = state0
        for n in m.obs:
            m.obs[n][...] = obs0[n]
        step(m, delivered, out)
        cmp.check(host(sim.state), {n: host(v) for n, v in sim.obs.items()}, m.state, m.obs)
        assert cmp.clean(), (name, k, cmp.bad, cmp.worst)
        if hasattr(m, "touch"):
            assert (host(sim.touch) == m.touch).all(), (name, k)
            fig["touched"] += int(m.touch.sum())
        else:
            assert not bool(sim.touch.any()), (name, k)
        if hasattr(m, "slip"):
            got, w = host(sim.slip), m.slip
            rel = np.abs(got - w) / np.maximum(1.0, np.abs(w))
            fig["worst_slip"] = max(fig["worst_slip"], float(rel.max()))
            assert (rel <= S.REL_TOL).all(), (name, k, fig["worst_slip"])
            fig["slid"] += int((w > 0).sum())
        else:
            assert sim.slip is None
    if model:
        fig.update(cmp.worst)
    fig["fallen"] = int(sim.fallen().sum())
    ctl.close()
    sim.close()
    return snaps, fig


@pytest.mark.parametrize("name", MF.TICK_CONFIGS)
def test_non_identity_motors_stand_in_front_of_every_tick(name, dev):
    """Each of the four ticks BatchedSRBSim.step dispatches to, with every motor at its own strength and mixed limits: the force
    the tick integrates is the DELIVERED one (a tick handed the planned force fails the state comparison on its first tick), the
    delivered force is the model's, and it differs from the planned one on every tick.  Then even robots at strength 1 without a
    limit in the same batch walk bit for bit as in a run without motors."""
    robot = "ghost"
    _, fig = _tick_run(name, robot, dev, MF.tick_motors(robot, MF.TICK_B), model=True)
    print(name, fig)
    assert fig["changed"] > 0 and fig["clipped"] > 0 and fig["fallen"] == 0
    assert name != "terrain_friction" or fig["slid"] > 0
    mixed, _ = _tick_run(name, robot, dev, MF.tick_motors(robot, MF.TICK_B, identity_even=True))
    free, _ = _tick_run(name, robot, dev, None)
    cols = lambda snap, sl: [t[..., sl] for t in snap]
    for k, (a, b) in enumerate(zip(mixed, free)):
        assert _same(cols(a, slice(0, None, 2)), cols(b, slice(0, None, 2))), (name, k)
    assert not _same(cols(mixed[-1], slice(1, None, 2)), cols(free[-1], slice(1, None, 2)))


# ---- 5. the kernel's singular branch and the settings only the C ABI accepts ------------------------------------------------

@pytest.fixture(scope="module")
def edge_cases(cases):
    return dict(singular={robot: MF.singular_case(robot) for robot in F.ROBOTS}, abi=MF.abi_cases())


def _run_case(c, dev):
    """rg_srb_motor_apply on a case's raw tensors, guarded -> (grf_out, tau_cmd, tau_out) as numpy."""
    B = c["B"]
    handle = srb_abi.SrbHandle(c["cfg"], B, dev)
    guard = Guarded(dev)
    state = np.zeros((M.STATE_ROWS, B))
    state[M.ROW_Q:M.ROW_Q + 12] = c["q"]
    st, grf, strength, limit = guard(state), guard(c["grf"]), guard(c["strength"]), guard(c["limit"])
    out, tau_cmd, tau = guard(np.full((B, 12), -5.0, np.float32)), guard(np.full((12, B), -5.0)), guard(np.full((12, B), -5.0))
    motor_abi.motor_apply(handle, st, grf, strength, limit, out, tau_cmd, tau)
    got = out.cpu().numpy(), tau_cmd.cpu().numpy(), tau.cpu().numpy()
    assert guard.intact()
    handle.close()
    return got


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_a_leg_with_its_foot_on_the_knee_axis_takes_the_uniform_scale_on_the_device(robot, edge_cases, dev):
    """The `!solve3(...)` branch of the kernel: leg 0's floats are (float)(k * g), bit for bit with the model, which takes its fmin
    chain in the kernel's order; the other three legs take the solve and are held as in the regular test."""
    c = edge_cases["singular"][robot]
    got, got_cmd, got_tau = _run_case(c, dev)
    assert got[:, :3].tobytes() == c["out"][:, :3].tobytes()
    assert (got[:, :3] != c["grf"][:, :3]).all() and np.isfinite(got).all()
    assert (got_cmd[2] == 0.0).all() and (got_tau[2] == 0.0).all()                          # the knee moves nothing
    bad, worst, worst_tau = MF.delivered_mismatches(c["grf"], (c["out"], c["tau_cmd"], c["tau"], c["sat"]), (got, got_cmd, got_tau))
    print(robot, "singular leg: largest |grf_out - model|", worst, "largest torque deviation", worst_tau)
    assert bad == []


@pytest.mark.parametrize("name", ["strength_zero", "limit_zero", "limit_nan", "limit_negative", "strength_inf_on_a_swinging_leg",
                                  "negative_zero_and_denormal_force", "all_zero_force"])
def test_settings_only_the_c_abi_accepts_are_the_models(name, edge_cases, dev):
    """What MotorModel refuses and rg_srb_motor_apply takes, each held to the model (what the case is about is asserted on the
    model in motor_fixtures.abi_cases, and stated in rg_srb_motor.h): a NaN where the model has one and nowhere else, the floats
    of `exact` by bits, the rest within one ulp, the torques within the tolerance."""
    c = edge_cases["abi"][name]
    got, got_cmd, got_tau = _run_case(c, dev)
    want = c["out"]
    assert (np.isnan(got) == np.isnan(want)).all(), np.argwhere(np.isnan(got) != np.isnan(want))[:5]
    exact = c["exact"]
    assert got[exact].tobytes() == want[exact].tobytes(), np.argwhere((got.view(np.int32) != want.view(np.int32)) & exact)[:5]
    rest = ~exact & ~np.isnan(want)
    assert within_ulp(got[rest], want[rest].astype(np.float64)).all()
    for g, w in ((got_cmd, c["tau_cmd"]), (got_tau, c["tau"])):
        assert (np.isnan(g) == np.isnan(w)).all()
        ok = ~np.isnan(w)
        assert (np.abs(g[ok] - w[ok]) <= REL_TOL * np.maximum(1.0, np.abs(w[ok]))).all(), float(np.abs(g[ok] - w[ok]).max())
    assert exact.any() or np.isnan(want).any() or name == "limit_zero"
