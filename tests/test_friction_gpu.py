"""Coulomb friction at the stance feet on the GPU (include/rg_srb_friction.h, robot_gym_amd/csrc/rg_srb_friction.hip): the
kernel against tests/friction_model.py on recorded streams at batches 1, 3 and 67 on the flat, random and grid grounds in both
contact modes, with every mu = +inf rg_srb_step_friction against rg_srb_step / the terrain step / rg_srb_step_contact byte for
byte, rg_srb_friction_draw against the model bit for bit, the go-to env with a friction-drawing randomiser replayed into the
model with a clone in mid-slide, and the closed loop with the real controller on a slippery floor inside the band of the CPU
reference loop (tests/friction_fixtures.py).

Every model run is made before the GPU is opened (`dev` depends on `recordings`)."""
import numpy as np
import pytest
import torch

from robot_gym_amd.core import dr_abi, friction_abi
from robot_gym_amd.core.config import MPCConfig
from tests import contact_fixtures as CF
from tests import friction_fixtures as FF
from tests import friction_model as FM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
from tests import terrain_model as TM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recordings():
    out = {}
    for measured in (0, 1):
        for g, kind in enumerate(FF.GROUNDS):
            slip = stick = pulled = 0
            for n, B in enumerate(FF.BATCHES):
                rec = out[kind, B, measured] = FF.run_model(MPCConfig.for_robot(FF.STREAM_ROBOT[B]), B, FF.stream_seed(g, n, measured), kind, measured)
                slip, stick, pulled = slip + rec.slipping, stick + rec.sticking, pulled + rec.pulled
                # the run is the one described: the robot that loses its forces falls, the reset happened, a state was kept
                f = CF.faller(B)
                assert any(s[M.ROW_STATUS, f] == 1 for s in rec.states), (kind, B)
                assert (rec.states[FF.RESET_TICK + 1][M.ROW_STEPS, rec.resets[FF.RESET_TICK][0]] == 10).all()
                assert B < 3 or rec.kept >= 1, (kind, B, measured)
                assert B < 67 or int((rec.states[-1][M.ROW_STATUS] == 0).sum()) >= B - 4       # the faller and the poisoned robots
            # at least a quarter of the stance leg-ticks slip and at least a quarter stick
            assert 4 * slip >= slip + stick and 4 * stick >= slip + stick and slip + stick > 1000, (kind, measured, slip, stick)
            assert pulled > 100, (kind, measured, pulled)          # the ground is asked to pull, too
            # every mu = +inf over the same streams, batch 67: what the entries without friction compute
            out["grip", kind, measured] = FF.run_model(MPCConfig.for_robot("ghost"), 67, FF.stream_seed(g, 2, measured), kind, measured, mu=np.full(67, np.inf))
    return out


@pytest.fixture(scope="module")
def dev(recordings):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("measured", [0, 1], ids=["schedule", "measured"])
@pytest.mark.parametrize("B", FF.BATCHES)
@pytest.mark.parametrize("kind", FF.GROUNDS)
def test_kernel_against_the_friction_model(kind, B, measured, recordings, dev):
    """40 ticks of the friction streams: per-robot mu from +inf, NaN, -1, 0 and 0.05 .. 1.0, horizontal forces that make the feet
    slip and stick in like numbers, odd robots with their own true body, ext pushes, one reset at tick 32, one robot losing its
    forces at tick 10, non-finite forces.  srb_streams.Comparison with the simulator's tolerances (stance, status and steps
    exactly); touch exactly; slip within REL_TOL * max(1, |value|); sentinels around every buffer, mu, touch and slip included,
    after every tick."""
    rec = recordings[kind, B, measured]
    cmp = S.Comparison()
    raw, worst_slip = FF.replay(rec, dev, cmp=cmp)
    st, _ = raw.numpy()
    print(kind, B, measured, "largest deviations", cmp.worst, "slip", worst_slip, "leg-ticks slipping / sticking", rec.slipping, rec.sticking)
    assert np.isfinite(st).all()
    assert cmp.clean(), (cmp.bad, cmp.worst)
    assert (raw.mu.cpu().numpy().tobytes() == rec.mu.tobytes())          # mu is read, never written
    raw.close()


def test_null_outputs_are_accepted_and_bad_arguments_refused_by_name(dev):
    import ctypes as C
    cfg = MPCConfig.for_robot("ghost")
    raw = FF.RawFrictionSim(cfg, 3, dev, np.array([0.3, np.inf, 0.0]))
    raw.reset()
    lib, h = friction_abi.load_library(), raw.handle._h
    p = raw.state.data_ptr()
    z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
    g, ft, ls = z(3, 12), z(3, 12), torch.ones(3, 4, dtype=torch.int32, device=dev)
    before = raw.state.clone()
    friction_abi.step_friction(raw.handle, raw.state, g, ft, ls, 1, None, raw.ptrs, raw.mu)              # touch and slip NULL
    assert raw.guards_intact() and not torch.equal(before, raw.state)
    assert bool((raw.touch == -5).all()) and bool((raw.slip == -5.0).all())                                # neither was written
    for name in ("state", "grf", "foot_target", "leg_state", "mu"):
        a = dict(state=p, grf=g.data_ptr(), foot_target=ft.data_ptr(), leg_state=ls.data_ptr(), mu=raw.mu.data_ptr())
        a[name] = None
        rc = lib.rg_srb_step_friction(h, a["state"], a["grf"], a["foot_target"], a["leg_state"], 1, None, C.byref(raw.ptrs), a["mu"], 0.01, 1.0, None, None, None)
        assert rc == -1 and f"step_friction: null {name}".encode() in lib.rg_srb_last_error(h), name
    rc = lib.rg_srb_step_friction(h, p, g.data_ptr(), ft.data_ptr(), ls.data_ptr(), 2, None, C.byref(raw.ptrs), raw.mu.data_ptr(), 0.01, 1.0, None, None, None)
    assert rc == -1 and b"measured" in lib.rg_srb_last_error(h)
    with pytest.raises(ValueError, match="step_friction: mu"):
        friction_abi.step_friction(raw.handle, raw.state, g, ft, ls, 1, None, raw.ptrs, z(3, dt=torch.float64).cpu())
    with pytest.raises(ValueError, match="step_friction: slip"):
        friction_abi.step_friction(raw.handle, raw.state, g, ft, ls, 1, None, raw.ptrs, raw.mu, slip=z(3, 4, dt=torch.float64))
    with pytest.raises(ValueError, match="slip_gain"):
        friction_abi.step_friction(raw.handle, raw.state, g, ft, ls, 1, None, raw.ptrs, raw.mu, slip_gain=-1.0)
    assert raw.guards_intact()
    raw.close()


# ---- 2. every mu = +inf: the entries without friction, byte for byte ---------------------------------------------------------

def _snap(raw):
    return raw.state.cpu().numpy().tobytes() + b"".join(raw.obs[n].cpu().numpy().tobytes() for n in sorted(raw.obs)) + raw.touch.cpu().numpy().tobytes()


@pytest.mark.parametrize("measured", [0, 1], ids=["schedule", "measured"])
@pytest.mark.parametrize("kind", FF.GROUNDS)
def test_with_every_mu_infinite_the_friction_entry_is_the_entry_without_friction_byte_for_byte(kind, measured, recordings, dev):
    """rg_srb_step on a flat handle, the terrain step on a terrain handle (measured = 0), rg_srb_step_contact (measured = 1):
    state, observation and touch, over the streams of batch 67."""
    rec = recordings["grip", kind, measured]
    plain = FF.start(rec, dev)
    gripping = FF.start(rec, dev)
    plain.touch.zero_()
    gripping.touch.zero_()
    assert _snap(plain) == _snap(gripping)
    for k, (grf, ft, ls, ext) in enumerate(rec.inputs):
        if k in rec.resets:
            idx, xy, yaw, h = rec.resets[k]
            plain.reset(idx=idx, xy=xy, yaw=yaw, height=h)
            gripping.reset(idx=idx, xy=xy, yaw=yaw, height=h)
        if measured:
            plain.step_contact(grf, ft, ls, ext)
        else:
            plain.step(grf, ft, ls, ext)                       # rg_srb_step: the flat kernel on the plane, the terrain kernel on a terrain
        gripping.step_friction(grf, ft, ls, measured, ext)
        assert _snap(plain) == _snap(gripping), k
        assert bool((gripping.slip == 0.0).all()), k
        assert plain.guards_intact() and gripping.guards_intact()
    st = gripping.state.cpu().numpy()
    assert (st[M.ROW_STATUS] == 1).any() and (st[M.ROW_STATUS] == 0).sum() > 40
    assert measured == 0 or int(sum(t.sum() for t in rec.touches)) > 100
    plain.close()
    gripping.close()


# ---- 3. the draw -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_friction_draw_is_the_model_bit_for_bit(B, dev):
    from robot_gym_amd.core import srb_abi
    handle = srb_abi.SrbHandle(MPCConfig.for_robot("ghost"), B, dev)
    rng = np.random.default_rng(B)
    key = rng.integers(-5000, 5000, B).astype(np.float64)
    draws = rng.integers(0, 40, B).astype(np.float64)
    seed, lo, hi = (1 << 63) + 977 * B, 0.2, 0.9
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    masks = dict(sparse=(rng.uniform(size=B) < 0.3).astype(np.int32), empty=np.zeros(B, np.int32), full=np.ones(B, np.int32))
    masks["sparse"][B - 1] = 1                                  # the last lane of the batch draws
    perm = rng.permutation(B)
    for name, mask in masks.items():
        back = torch.full((B + 2 * S.PAD,), float(S.GUARD), dtype=torch.float64, device=dev)
        mu = back[S.PAD:S.PAD + B]
        mu.fill_(-7.0)
        want = FM.draw(np.full(B, -7.0), mask, key, draws, seed, lo, hi)
        friction_abi.friction_draw(handle, t(mask), t(key), t(draws), seed, lo, hi, mu)
        got = mu.cpu().numpy()
        assert got.tobytes() == want.tobytes(), name
        assert bool((back[:S.PAD] == S.GUARD).all()) and bool((back[-S.PAD:] == S.GUARD).all()), name
        on = mask != 0
        assert (got[~on] == -7.0).all() and (got[on] >= lo).all() and (got[on] <= hi).all()
        # permuted keys: the value follows the key
        again = torch.full((B,), -7.0, dtype=torch.float64, device=dev)
        friction_abi.friction_draw(handle, t(mask[perm]), t(key[perm]), t(draws[perm]), seed, lo, hi, again)
        assert again.cpu().numpy().tobytes() == got[perm].tobytes(), name
    with pytest.raises(ValueError, match="friction_draw"):
        friction_abi.friction_draw(handle, t(masks["full"]), t(key), t(draws), seed, 0.9, 0.2, again)
    with pytest.raises(ValueError, match="friction_draw: key"):
        friction_abi.friction_draw(handle, t(masks["full"]), t(key).to(torch.float32), t(draws), seed, lo, hi, again)
    handle.close()


# ---- 4. the env, replayed into the model -----------------------------------------------------------------------------------

def _columns(d, keep):
    return {k: (v[..., keep] if v.ndim else v) for k, v in d.items()}


def test_env_with_friction_is_the_model_on_every_tick_and_a_clone_in_mid_slide_continues_bit_identically(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain
    B, T, seed, lo, hi = 64, 60, 11, 0.2, 0.9
    dr = DomainRandomizer(friction=(lo, hi), seed=seed)
    env = BatchedGoEnv(B, device=dev, terrain=RandomTerrain(), contact="measured", friction=0.3, randomizer=dr, auto_reset=True, max_time=0.95,
                       seed=3)                                  # the time limit ends every episode on tick 10
    sim, cfg = env.sim, env.cfg
    assert bool((sim.mu == 0.3).all()) and tuple(sim.slip.shape) == (4, B) and sim.slip.dtype == torch.float64
    host = lambda t: t.cpu().numpy()
    key = host(dr.state[dr_abi.ROW_KEY]).copy()
    mu = host(sim.mu).copy()
    env.reset()                                                 # the host reset draws for every robot, at draw count 0
    FM.draw(mu, np.ones(B), key, np.zeros(B), seed, lo, hi)
    assert host(sim.mu).tobytes() == mu.tobytes() and (mu >= lo).all() and (mu <= hi).all() and len(set(mu.tolist())) == B
    assert (host(dr.state[dr_abi.ROW_DRAWS]) == 1).all()
    model = FM.FrictionSRBModel(B, cfg, TM.Random(sim.terrain.amplitude, sim.terrain.cell, sim.terrain.seed, host(sim.terrain.keys)), mu=mu)
    model.reset()
    rng = np.random.default_rng(1)
    actions = torch.as_tensor(rng.uniform([0.1, -0.3], [0.4, 0.3], (T, B, 2)).astype(np.float32), device=dev)
    cmp = S.Comparison()
    resets = slid = compared = 0
    worst_slip = 0.0
    for t in range(T):
        model.state[:] = host(sim.state)                        # the tick starts from the simulator's state, observation and floor
        for name in model.obs:
            model.obs[name][...] = host(sim.obs[name])
        model.mu[:] = mu
        draws = host(dr.state[dr_abi.ROW_DRAWS]).copy()
        env.step(actions[t])
        out = env.ctl.extra
        model.step_friction(host(out["grf"]), host(out["foot_target"]), host(out["leg_state"]), 1, None)
        mask = host(env.reset_mask) != 0
        keep = np.nonzero(~mask)[0]                             # a robot that was reset holds its new episode's first state
        if keep.size:
            cmp.check(host(sim.state)[:, keep], _columns({k: host(v) for k, v in sim.obs.items()}, keep), model.state[:, keep], _columns(model.obs, keep))
            assert (host(sim.touch)[:, keep] == model.touch[:, keep]).all(), t
            got, want = host(sim.slip)[:, keep], model.slip[:, keep]
            rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            worst_slip = max(worst_slip, float(rel.max(initial=0.0)))
            assert (rel <= S.REL_TOL).all(), (t, worst_slip)
            slid += int((want > 0).sum())
            compared += len(keep)
        # the floor: a robot that was reset drew at its key and draw count, the others keep theirs
        FM.draw(mu, mask, key, draws, seed, lo, hi)
        assert host(sim.mu).tobytes() == mu.tobytes(), t
        assert (host(dr.state[dr_abi.ROW_DRAWS]) == draws + mask).all(), t
        resets += int(mask.sum())
    print("largest deviations", cmp.worst, "slip", worst_slip, "resets", resets, "leg-ticks sliding", slid, "robot-ticks compared", compared)
    assert cmp.clean(), (cmp.bad, cmp.worst)
    assert resets >= 4 * B and slid > 0 and compared > T * B // 2

    # a clone in mid-slide: the floor, the slide and the draws go with the robot
    src, dst = torch.arange(16, device=dev), torch.arange(16, device=dev) + 32          # dst = src modulo 16
    sim.set_friction(0.2, idx=src)
    same = torch.as_tensor(np.tile(np.array([[0.35, 0.2]], dtype=np.float32), (B, 1)), device=dev)
    for _ in range(40):
        env.step(same)
        if bool((sim.slip[:, src] > 0).any()) and not bool((env.reset_mask != 0).any()):
            break
    assert bool((sim.slip[:, src] > 0).any()), "no source robot is sliding"
    assert not torch.equal(sim.state[:, src], sim.state[:, dst])
    env.clone(src, dst)
    assert torch.equal(sim.mu[src], sim.mu[dst]) and torch.equal(sim.slip[:, src], sim.slip[:, dst]) and bool((sim.mu[dst] == 0.2).all())
    slid_after = torch.zeros((), dtype=torch.float64, device=dev)
    for k in range(30):
        env.step(same)
        assert torch.equal(sim.state[:, src], sim.state[:, dst]), k
        assert torch.equal(sim.slip[:, src], sim.slip[:, dst]) and torch.equal(sim.mu[src], sim.mu[dst]), k
        assert torch.equal(sim.touch[:, src], sim.touch[:, dst]), k
        slid_after += sim.slip[:, dst].sum()
    assert float(slid_after) > 0.0 and bool(torch.isfinite(env.obs).all())
    env.close()


def test_the_python_layer_allocates_nothing_without_friction_and_sets_coefficients_with_it(dev):
    from robot_gym_amd.sim import BatchedSRBSim, DomainRandomizer
    cfg = MPCConfig.for_robot("ghost")
    plain = BatchedSRBSim(5, cfg, device=dev)
    assert plain.mu is None and plain.slip is None
    with pytest.raises(RuntimeError, match="built without friction"):
        plain.set_friction(0.3)
    with pytest.raises(ValueError, match="needs a simulator built with friction"):
        DomainRandomizer(friction=(0.2, 0.9)).bind(plain)
    plain.close()
    sim = BatchedSRBSim(5, cfg, device=dev, friction="inf", slip_gain=0.02, slip_speed_max=0.5)
    assert sim.mu.dtype == torch.float64 and tuple(sim.mu.shape) == (5,) and bool(torch.isinf(sim.mu).all()) and (sim.slip_gain, sim.slip_speed_max) == (0.02, 0.5)
    sim.set_friction([0.1, 0.2, 0.3, 0.4, 0.5])
    sim.set_friction(torch.tensor([0.9, float("nan")], dtype=torch.float64), idx=[4, 0])
    sim.set_friction("inf", idx=torch.tensor([2], device=dev))
    got = sim.mu.cpu().numpy()
    assert np.isnan(got[0]) and got[1:].tolist() == [0.2, np.inf, 0.4, 0.9]
    with pytest.raises(ValueError, match="set_friction"):
        sim.set_friction([0.1, 0.2])
    # schedule mode with friction steps on desired_state
    out = dict(grf=torch.zeros(5, 12, device=dev), foot_target=torch.zeros(5, 12, device=dev), leg_state=torch.ones(5, 4, dtype=torch.int32, device=dev))
    sim.reset()
    with pytest.raises(ValueError, match="desired_state"):
        sim.step(out)
    sim.step(dict(out, desired_state=out["leg_state"]))
    assert int(sim.fallen().sum()) == 0 and bool((sim.slip == 0).all())
    sim.copy_columns([1], [3])
    assert float(sim.mu[3]) == 0.2
    sim.close()


# ---- 5. the closed loop with the real controller ---------------------------------------------------------------------------

def _pair(robot, batch, dev, terrain, friction):
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.sim import BatchedSRBSim
    cfg = MPCConfig.for_robot(robot)
    return cfg, BatchedMPCController(batch, cfg, device=dev), BatchedSRBSim(batch, cfg, device=dev, terrain=terrain, contact="measured", friction=friction)


def _start(ctl, sim, cmd, hs):
    sim.reset(height=sim.cfg.body_height * np.asarray(hs))
    ctl.reset()
    ctl.set_raw_command(torch.as_tensor(np.ascontiguousarray(np.asarray(cmd, dtype=np.float32).T), device=sim.device))


def _closed_loop(robot, dev, friction):
    """The 32 cases, 400 ticks with measured contact on the reference's random terrain -> (worst band figures over the last 200
    ticks, slid [B]: the metres each robot's feet slid, fallen, solver failures)."""
    from robot_gym_amd.sim import rollout
    from robot_gym_amd.sim.terrain import RandomTerrain
    cmd, hs = F.cases(robot)
    n = len(hs)
    cfg, ctl, sim = _pair(robot, n, dev, RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED), friction)
    _start(ctl, sim, cmd, hs)
    slid = torch.zeros(n, dtype=torch.float64, device=dev)
    failures = [0]

    def watch(k):
        slid.add_(sim.slip.sum(0))
        failures[0] += ctl.solver_stats()["failures"]

    rollout(ctl, sim, None, F.TICKS - F.WINDOW, on_tick=watch)
    _, traj = rollout(ctl, sim, None, F.WINDOW, record_every=1, on_tick=watch)
    fallen = int(sim.fallen().sum())
    pxy = traj[:, M.ROW_P:M.ROW_P + 2, :].permute(0, 2, 1).reshape(-1, 2)
    who = torch.arange(n, device=dev, dtype=torch.int32).repeat(F.WINDOW)
    ground = sim.ground_height(pxy, who).reshape(F.WINDOW, n).cpu().numpy()
    fig = F.figures(traj.permute(1, 0, 2).cpu().numpy())
    fig["z"] = fig["z"] - ground
    worst = F.worst_in_window(fig, cmd, cfg.body_height)
    steps = sim.state[M.ROW_STEPS].cpu().numpy()
    ctl.close()
    sim.close()
    return worst, slid.cpu().numpy(), fallen, failures[0], steps


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_closed_loop_on_a_slippery_floor_stays_inside_the_cpu_band(robot, dev):
    """friction = 0.3 under a planner that believes 0.45: nobody falls, at least 16 of the 32 robots slide, and no robot's feet
    slide further than twice what the CPU reference loop's worst robot does."""
    worst, slid, fallen, failures, steps = _closed_loop(robot, dev, FF.MU_SLIPPERY)
    print(robot, "friction", FF.MU_SLIPPERY, "robots that slid", int((slid > 0).sum()), "worst slid", float(slid.max()), "band", FF.SLID_BAND[robot],
          {k: float(v.max()) for k, v in worst.items()})
    assert fallen == 0 and (steps == 10 * F.TICKS).all() and failures == 0
    assert int((slid > 0).sum()) >= FF.SLIDERS
    assert float(slid.max()) <= FF.SLID_BAND[robot], (float(slid.max()), FF.SLID_BAND[robot])


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_closed_loop_on_a_floor_that_grips_keeps_the_bands_of_measured_contact(robot, dev):
    """friction = 0.9, twice what the planner believes: nobody falls and the bands of contact_fixtures hold.  The worst slid
    distance is printed (profiles/srb_friction_tick.json and DESIGN.md record it), not bounded: it depends on how closely the ADMM lane keeps the cone, and the exact zero is
    the CPU loop's claim."""
    worst, slid, fallen, failures, steps = _closed_loop(robot, dev, 0.9)
    print(robot, "friction 0.9 robots that slid", int((slid > 0).sum()), "worst slid", float(slid.max()), {k: float(v.max()) for k, v in worst.items()})
    assert fallen == 0 and (steps == 10 * F.TICKS).all() and failures == 0
    assert not F.outside_bands(worst, CF.BANDS), F.outside_bands(worst, CF.BANDS)


def test_friction_none_and_friction_inf_give_the_same_state_bit_for_bit(dev):
    from robot_gym_amd.sim import rollout
    from robot_gym_amd.sim.terrain import RandomTerrain
    cmd, hs = F.cases("ghost")
    states = []
    for friction in (None, "inf"):
        cfg, ctl, sim = _pair("ghost", len(hs), dev, RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED), friction)
        _start(ctl, sim, cmd, hs)
        rollout(ctl, sim, None, 100)
        assert (sim.mu is None) == (friction is None)
        states.append((sim.state.cpu().numpy().tobytes(), {k: v.cpu().numpy().tobytes() for k, v in sim.obs.items()}, sim.touch.cpu().numpy().tobytes(),
                       int(sim.fallen().sum())))
        if friction is not None:
            assert bool((sim.slip == 0).all())
        ctl.close()
        sim.close()
    assert states[0] == states[1] and states[0][3] == 0
