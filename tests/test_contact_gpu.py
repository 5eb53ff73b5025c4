"""Measured foot contact on the GPU (include/rg_srb_contact.h, robot_gym_amd/csrc/rg_srb_contact.hip): the kernel against
tests/contact_model.py on recorded streams at batches 1, 3 and 67 on the flat, random and grid grounds, rg_srb_step_contact
against rg_srb_step byte for byte while nothing touches, the closed loop with the real controller inside the bands of the
CPU reference loop (tests/contact_fixtures.py) with the controller's EARLY_CONTACT branch entered, the step grid, clones, and
the go-to task with auto-reset in measured mode.

Every model run is made before the GPU is opened (`dev` depends on `recordings`)."""
import warnings

import numpy as np
import pytest
import torch

from robot_gym_amd.core.config import MPCConfig
from tests import contact_fixtures as CF
from tests import contact_model as CM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
from tests import terrain_fixtures as TF

pytestmark = pytest.mark.gpu

STREAM_ROBOT = {1: "ghost", 3: "k3lso", 67: "ghost"}


@pytest.fixture(scope="module")
def recordings():
    out = {}
    for g, kind in enumerate(CF.GROUNDS):
        touch = free = 0
        states = set()
        for n, B in enumerate(CF.BATCHES):
            rec = out[kind, B] = CF.run_model(MPCConfig.for_robot(STREAM_ROBOT[B]), B, 500 + 10 * g + n, kind)
            touch, free = touch + rec.swung_touch, free + rec.swung_free
            states |= set(np.unique(rec.s["leg_state"]).tolist())
            # the run is the one described: the robot that loses its forces falls, the others stand, the reset happened
            f = CF.faller(B)
            assert any(s[M.ROW_STATUS, f] == 1 for s in rec.states), (kind, B)
            others = np.delete(np.arange(B), f)
            assert all((s[M.ROW_STATUS, others] == 0).all() for s in rec.states), (kind, B)
            assert (rec.states[CF.RESET_TICK + 1][M.ROW_STEPS, rec.resets[CF.RESET_TICK][0]] == 10).all()
        assert states == {CM.SWING, CM.STANCE, CM.EARLY_CONTACT, CM.LOSE_CONTACT}
        # the targets are spread about the ground: at least a quarter of the swung leg-ticks touch, at least a quarter do not
        assert 4 * touch >= touch + free and 4 * free >= touch + free and touch + free > 300, (kind, touch, free)
    for kind in ("flat", "random"):
        out["same", kind] = CF.equivalence_recording(MPCConfig.for_robot("ghost"), 67, 40, 350, CF.stream_ground(kind, 67))
        assert out["same", kind].lowest > 0.0
    return out


@pytest.fixture(scope="module")
def dev(recordings):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_touch", [True, False], ids=["touch", "null"])
@pytest.mark.parametrize("B", CF.BATCHES)
@pytest.mark.parametrize("kind", CF.GROUNDS)
def test_kernel_against_the_contact_model(kind, B, with_touch, recordings, dev):
    """40 ticks of the contact streams: leg_state from all four values, odd robots with their own true body, ext pushes, one
    reset at tick 32, one robot losing its forces at tick 10.  srb_streams.Comparison with the simulator's tolerances
    (stance, status and steps exactly); touch exactly; sentinels around every buffer after every tick, around touch too, and
    with touch = NULL."""
    rec = recordings[kind, B]
    cmp = S.Comparison()
    raw = CF.replay(rec, dev, cmp=cmp, with_touch=with_touch)
    st, _ = raw.numpy()
    print(kind, B, "largest deviations", cmp.worst, "swung leg-ticks touching / free", rec.swung_touch, rec.swung_free)
    assert np.isfinite(st).all()
    assert cmp.clean(), (cmp.bad, cmp.worst)
    raw.close()


def test_null_arguments_are_refused_by_name(dev):
    import ctypes as C
    cfg = MPCConfig.for_robot("ghost")
    raw = CF.RawContactSim(cfg, 3, dev)
    lib, h = raw.handle._lib, raw.handle._h
    good = dict(state=raw.state.data_ptr(), grf=raw.state.data_ptr(), foot_target=raw.state.data_ptr(), leg_state=raw.state.data_ptr())
    for name in good:
        a = dict(good, **{name: None})
        rc = lib.rg_srb_step_contact(h, a["state"], a["grf"], a["foot_target"], a["leg_state"], None, C.byref(raw.ptrs), None, None)
        assert rc == -1 and f"step_contact: null {name}".encode() in lib.rg_srb_last_error(h), name
    assert lib.rg_srb_step_contact(h, good["state"], good["grf"], good["foot_target"], good["leg_state"], None, None, None, None) == -1
    assert b"step_contact: null obs" in lib.rg_srb_last_error(h)
    from robot_gym_amd.core import srb_abi
    hole = srb_abi.CObsPtrs()
    for name in srb_abi.OBS_FIELDS:
        setattr(hole, name, raw.obs[name].data_ptr())
    hole.jac = None
    assert lib.rg_srb_step_contact(h, good["state"], good["grf"], good["foot_target"], good["leg_state"], None, C.byref(hole), None, None) == -1
    assert b"obs" in lib.rg_srb_last_error(h)
    with pytest.raises(ValueError, match="step_contact: leg_state"):
        raw.handle.step_contact(raw.state, torch.zeros(3, 12, device=dev), torch.zeros(3, 12, device=dev), torch.zeros(3, 4, device=dev), None, raw.ptrs)
    with pytest.raises(ValueError, match="step_contact: touch"):
        raw.handle.step_contact(raw.state, torch.zeros(3, 12, device=dev), torch.zeros(3, 12, device=dev), torch.zeros(3, 4, dtype=torch.int32, device=dev),
                                None, raw.ptrs, torch.zeros(4, 3, dtype=torch.int32))
    assert raw.guards_intact()
    raw.close()


# ---- 2. while nothing touches, the schedule tick ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["flat", "random"])
def test_step_contact_is_rg_srb_step_byte_for_byte_while_nothing_touches(kind, recordings, dev):
    rec = recordings["same", kind]
    s = rec.s
    sims = []
    for contact in (False, True):
        raw = CF.RawContactSim(rec.cfg, rec.B, dev)
        TF.bind_ground(raw, rec.ground)
        raw.set_body(rec.body_idx, s["mass"][rec.body_idx], s["inertia"][:, rec.body_idx])
        raw.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
        sims.append(raw)
    plain, measured = sims
    snap = lambda raw: raw.state.cpu().numpy().tobytes() + b"".join(raw.obs[n].cpu().numpy().tobytes() for n in sorted(raw.obs))
    assert snap(plain) == snap(measured)
    for k, (grf, ft, d, ext) in enumerate(rec.inputs):
        plain.step(grf, ft, d, ext)
        measured.step_contact(grf, ft, d, ext)
        assert snap(plain) == snap(measured), k
        assert int(measured.touch.abs().sum()) == 0
        assert plain.guards_intact() and measured.guards_intact()
    assert int((plain.state[M.ROW_STANCE:M.ROW_STANCE + 4] == 0).sum()) > 0 and int(plain.state[M.ROW_STATUS].sum()) == 0
    plain.close()
    measured.close()


# ---- 3. the closed loop with the real controller ---------------------------------------------------------------------------

def _pair(robot, batch, dev, terrain):
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.sim import BatchedSRBSim
    cfg = MPCConfig.for_robot(robot)
    return cfg, BatchedMPCController(batch, cfg, device=dev), BatchedSRBSim(batch, cfg, device=dev, terrain=terrain, contact="measured")


def _start(ctl, sim, cmd, hs):
    sim.reset(height=sim.cfg.body_height * np.asarray(hs))
    ctl.reset()
    ctl.set_raw_command(torch.as_tensor(np.ascontiguousarray(np.asarray(cmd, dtype=np.float32).T), device=sim.device))


class _Watch:
    """Per tick, on the device: which robots were in EARLY_CONTACT / LOSE_CONTACT, how many feet touched; the solver's failures."""

    def __init__(self, ctl, sim):
        self.ctl, self.sim = ctl, sim
        self.early = torch.zeros(sim.batch, dtype=torch.bool, device=sim.device)
        self.lose = torch.zeros_like(self.early)
        self.touched = torch.zeros(sim.batch, dtype=torch.int64, device=sim.device)
        self.failures, self.ticks = 0, 0

    def __call__(self, k):
        ls = self.ctl.extra["leg_state"]
        self.early |= (ls == CM.EARLY_CONTACT).any(1)
        self.lose |= (ls == CM.LOSE_CONTACT).any(1)
        self.touched += self.sim.touch.sum(0)
        self.failures += self.ctl.solver_stats()["failures"]
        self.ticks += 1


@pytest.mark.parametrize("robot", F.ROBOTS)
def test_closed_loop_with_measured_contact_on_the_reference_terrain(robot, dev):
    """The 32 cases, 400 ticks at amplitude 0.06, one world per robot (keys arange(32), as the CPU loop): nobody falls, no
    solver failure, a clean audit, every robot inside contact_fixtures.BANDS over the last 200 ticks, and EARLY_CONTACT seen
    on at least half as many robots as the CPU reference loop saw it on."""
    from robot_gym_amd.sim import rollout
    from robot_gym_amd.sim.terrain import RandomTerrain
    cmd, hs = F.cases(robot)
    n = len(hs)
    cfg, ctl, sim = _pair(robot, n, dev, RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED))
    _start(ctl, sim, cmd, hs)
    watch = _Watch(ctl, sim)
    rollout(ctl, sim, None, F.TICKS - F.WINDOW, on_tick=watch)
    _, traj = rollout(ctl, sim, None, F.WINDOW, record_every=1, on_tick=watch)
    assert int(sim.fallen().sum()) == 0 and bool((sim.state[M.ROW_STEPS] == 10 * F.TICKS).all())
    pxy = traj[:, M.ROW_P:M.ROW_P + 2, :].permute(0, 2, 1).reshape(-1, 2)
    who = torch.arange(n, device=dev, dtype=torch.int32).repeat(F.WINDOW)
    ground = sim.ground_height(pxy, who).reshape(F.WINDOW, n).cpu().numpy()
    fig = F.figures(traj.permute(1, 0, 2).cpu().numpy())
    fig["z"] = fig["z"] - ground
    worst = F.worst_in_window(fig, cmd, cfg.body_height)
    early = int(watch.early.sum())
    print(robot, {k: float(v.max()) for k, v in worst.items()}, "robots in EARLY_CONTACT", early, "of", n, "(CPU loop:", CF.EARLY_ROBOTS[robot],
          ") touch-downs", int(watch.touched.sum()), "robots in LOSE_CONTACT", int(watch.lose.sum()))
    assert not F.outside_bands(worst, CF.BANDS), F.outside_bands(worst, CF.BANDS)
    assert 2 * early >= CF.EARLY_ROBOTS[robot], (early, CF.EARLY_ROBOTS[robot])
    audit = ctl.audit_stats()
    assert [watch.failures, watch.ticks] == [0, F.TICKS]
    assert audit["audit_over_tol"] == 0 and audit["audited"] > 0, audit
    ctl.close()
    sim.close()


def test_closed_loop_on_the_step_grid_every_robot_enters_early_contact(dev):
    from robot_gym_amd.sim import rollout
    from robot_gym_amd.sim.terrain import GridTerrain
    cfg, ctl, sim = _pair("ghost", 4, dev, GridTerrain(CF.step_heights(), CF.STEP_CELL, CF.STEP_ORIGIN))
    _start(ctl, sim, CF.STEP_CMD, CF.STEP_START)
    watch = _Watch(ctl, sim)
    rollout(ctl, sim, None, F.TICKS, on_tick=watch)
    print("EARLY_CONTACT", watch.early.tolist(), "touch-downs", watch.touched.tolist(), "x", sim.state[M.ROW_P].tolist())
    assert int(sim.fallen().sum()) == 0
    assert bool(watch.early.all()) and bool((watch.touched > 0).all())
    assert bool((sim.state[M.ROW_P].abs() > CF.STEP_AT).all())
    assert watch.failures == 0
    ctl.close()
    sim.close()


def test_measured_mode_needs_leg_state_and_schedule_mode_is_the_default(dev):
    from robot_gym_amd.sim import BatchedSRBSim
    cfg = MPCConfig.for_robot("ghost")
    sim = BatchedSRBSim(2, cfg, device=dev, contact="measured")
    assert sim.touch.dtype == torch.int32 and tuple(sim.touch.shape) == (4, 2) and sim.touch.device == sim.device
    out = dict(grf=torch.zeros(2, 12, device=dev), foot_target=torch.zeros(2, 12, device=dev), desired_state=torch.ones(2, 4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="leg_state"):
        sim.step(out)
    sim.reset()
    sim.step(dict(out, leg_state=out["desired_state"]))
    assert int(sim.fallen().sum()) == 0
    sim.close()
    plain = BatchedSRBSim(2, cfg, device=dev)
    assert plain.contact == "schedule"
    plain.reset()
    plain.step(out)                                        # no leg_state: schedule mode does not ask for it
    assert int(plain.touch.abs().sum()) == 0
    plain.close()


# ---- 4. clone ------------------------------------------------------------------------------------------------------------

def test_clone_in_measured_mode_is_bit_identical(dev):
    from robot_gym_amd.sim import clone, rollout
    from robot_gym_amd.sim.terrain import RandomTerrain
    n = 48
    terrain = RandomTerrain()
    cfg, ctl, sim = _pair("ghost", n, dev, terrain)
    cmd, hs = F.tiled_cases("ghost", n)
    src, dst = np.arange(16), np.arange(16) + 32                  # dst = src modulo 16
    cmd[dst] = cmd[src]
    _start(ctl, sim, cmd, hs)
    rollout(ctl, sim, None, 30)
    assert not bool((sim.state[:, src] == sim.state[:, dst]).all())
    s_t, d_t = torch.as_tensor(src, device=dev), torch.as_tensor(dst, device=dev)
    clone(ctl, sim, s_t, d_t)
    touched = torch.zeros((), dtype=torch.int64, device=dev)
    for k in range(50):
        ctl.get_action(0.0, sim.obs)
        sim.step(ctl)
        assert bool((sim.state[:, s_t] == sim.state[:, d_t]).all()), k
        assert bool((sim.touch[:, s_t] == sim.touch[:, d_t]).all()), k
        touched += sim.touch[:, s_t].sum()
    for name, t in sim.obs.items():
        assert bool((t[..., s_t] == t[..., d_t]).all()), name
    assert int(sim.fallen().sum()) == 0 and int(touched) > 0
    ctl.close()
    sim.close()


# ---- 5. the go-to task with auto-reset in measured mode ----------------------------------------------------------------------

def test_go_env_with_measured_contact_runs_without_a_host_read(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim.terrain import RandomTerrain
    B, STEPS = 64, 300
    env = BatchedGoEnv(B, device=dev, auto_reset=True, terrain=RandomTerrain(), contact="measured", max_time=0.95, seed=3)   # the time limit fires on tick 10
    sim = env.sim
    assert sim.contact == "measured"
    env.reset()
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    resets = torch.zeros((), dtype=torch.int64, device=dev)
    standing = torch.ones((), dtype=torch.bool, device=dev)
    finite = torch.ones((), dtype=torch.bool, device=dev)
    touched = torch.zeros((), dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(STEPS):
                obs, reward, done = env.step(action)
                r = env.reset_mask != 0
                resets += r.sum()
                on_four = (sim.state[M.ROW_STANCE:M.ROW_STANCE + 4] == 1).all(0) & (sim.obs["contact"] == 1).all(0) & (sim.state[M.ROW_STATUS] == 0)
                standing &= (on_four | ~r).all()
                finite &= torch.isfinite(obs).all() & torch.isfinite(reward).all() & torch.isfinite(sim.state).all()
                touched += sim.touch.sum()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert not [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]       # the loop issued no host read
    assert bool(finite) and bool(standing)
    assert int(resets) >= B and int(touched) > 0
    env.close()
