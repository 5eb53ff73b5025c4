"""What the friction tests share (include/rg_srb_friction.h): the band of the closed loop on a slippery floor, the CPU reference
loop (contact_fixtures.ContactCpuLoop with tests/friction_model.FrictionSRBModel), and the recorded streams for the kernel
with their replay on the GPU.

The band is TWICE the worst value the CPU reference loop itself produces on the 32 srb_fixtures.cases of each robot with
measured contact on the reference's random terrain at mu = MU_SLIPPERY (tests/test_friction_cpu.py recomputes it and fails if a
constant here is not twice its measurement): the convention of srb_fixtures.py.  The figure is, per robot, the distance its four
feet slid over the whole run, added up.
"""
import numpy as np

from tests import contact_fixtures as CF
from tests import friction_model as FM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
from tests import terrain_fixtures as TF

BELIEVED_MU = 0.45                               # MPCConfig.mu of both robots: what the planner's pyramid is built with
MU_GRIPS, MU_SLIPPERY, MU_ICE = 0.64, 0.3, 0.15  # above sqrt(2) * believed nothing slips; a centimetre of slide; everybody falls
SLIDERS = 16                                     # at MU_SLIPPERY at least this many of the 32 robots slide

#                band              measured worst slid distance of a robot, m (CPU loop, reference terrain, mu 0.3, 4 s)
SLID_BAND = dict(ghost=2 * 0.0107495,    # 0.0107495   (23 of the 32 robots slide; on the plane 0.0113747, 23 robots)
                 k3lso=2 * 0.0125028)    # 0.0125028   (25 robots; on the plane 0.0133920, 24 robots)


class FrictionCpuLoop(CF.ContactCpuLoop):
    """contact_fixtures.ContactCpuLoop on a floor with friction mu: the same oracle, the friction model stepped on the oracle's
    leg_state (measured contact).  slid [4, B]: the metres each foot has slid since the start."""

    def __init__(self, robot, cmd, height_scale, ground, mu, nthreads=0):
        super().__init__(robot, cmd, height_scale, ground, nthreads)
        self.model = FM.FrictionSRBModel(self.B, self.cfg, ground, mu=mu)
        self.model.reset(height=self.cfg.body_height * np.asarray(height_scale))
        self.slid = np.zeros((4, self.B))

    def tick(self, ext=None):
        m = self.model
        out = self.oracle.step(float(m.obs["t_robot"][0]), F.oracle_inputs(self.O, m.obs, self.cmd))
        self.last = out
        ls = np.asarray(out["leg_state"]).reshape(self.B, 4)
        m.step_friction(out["grf"].astype(np.float32), out["foot_target"].reshape(self.B, 12).astype(np.float32), ls, 1, ext)
        self.touched += m.touch.sum(0)
        self.slid += m.slip
        return TF.clearance_figures(m)


def run_cpu(robot, ground, mu, ticks=F.TICKS):
    """-> (trajectory dict of [ticks, B] arrays with z the clearance, the loop)."""
    cmd, hs = F.cases(robot)
    loop = FrictionCpuLoop(robot, cmd, hs, ground, mu)
    trajs = [loop.tick() for _ in range(ticks)]
    return F.stack(trajs), loop


def worst_slid(slid):
    """slid [4, B] -> [B]: the distance a robot's four feet slid, added up."""
    return np.asarray(slid).sum(0)


# ---- recorded streams for the kernel ----------------------------------------------------------------------------------

TICKS, FALL_TICK, RESET_TICK = CF.TICKS, CF.FALL_TICK, CF.RESET_TICK
BATCHES, GROUNDS = CF.BATCHES, CF.GROUNDS
STREAM_ROBOT = {1: "ghost", 3: "k3lso", 67: "ghost"}
# what a robot's mu is drawn from, by its index: the four values that grip, no friction at all, and 0.05 .. 1.0
MU_VALUES = (0.3, np.inf, 0.1, np.nan, 0.6, -1.0, 0.0, 0.05, 0.2, 0.45, 0.8, 1.0, 0.15)
# The streams' forces are the least-norm ones of a wrench, and one in ten of them pulls at the ground.  A floor with friction does
# not pull, which leaves a torque, and a body with the robot's own inertia (0.07 kg m2 in roll) is on its side within 0.2 s, its
# feet out of the legs' reach, where the leg IK amplifies a rounding error beyond any tolerance.  Every robot of these streams
# therefore carries SLOW times the inertia (the odd ones their own, as in srb_streams): the body turns slowly and the feet stay
# in reach.  What is compared is unchanged.
SLOW = 20.0
TANGENT = 0.3                                    # the horizontal force added at every foot, as a share of a quarter of the weight


def stream_seed(g, n, measured):
    """The seed of the recording on ground GROUNDS[g] at batch BATCHES[n]."""
    return 700 + 10 * g + n + 100 * int(measured)


def stream_mu(B):
    return np.array([MU_VALUES[b % len(MU_VALUES)] for b in range(B)], dtype=np.float64)


def poison(B):
    """{tick: (robot, leg, component, value)}: a non-finite force.  The robot keeps its last state on that tick and counts as
    fallen from then on (rg_srb.h), so each tick names another robot; the only robot of batch 1 is poisoned after its reset."""
    if B < 3:
        return {RESET_TICK + 4: (0, 1, 0, np.nan)}
    return {5: (0, 1, 0, np.nan), 21: (1, 2, 2, -np.inf)} if B == 3 else {5: (0, 1, 0, np.nan), 21: (4, 2, 2, -np.inf), 23: (3, 0, 1, np.nan)}


def run_model(cfg, B, seed, kind, measured, mu=None, T=TICKS):
    """The friction model over T ticks of contact_fixtures.contact_streams on the ground `kind` with per-robot mu (stream_mu, or
    the row `mu`): a true body on every robot (SLOW times the inertia; the odd robots their own mass and inertia), ext pushes, one reset before tick RESET_TICK, robot CF.faller(B) losing its
    forces at FALL_TICK, the non-finite forces of poison(B).  Horizontal forces of up
    to TANGENT times a quarter of the weight that squeeze the stance feet against each other are added, so that the feet slip
    and stick in like numbers.
    measured = 0 steps on the streams' desired_state (1 where the leg is not swung).  -> CF.ContactRecording with .ground, .mu,
    .measured, .touches, .slips and .slipping / .sticking / .pulled (stance leg-ticks of running robots the rule applies to)."""
    s = CF.contact_streams(cfg, B, T, seed)
    s["inertia"] = s["inertia"] * SLOW
    rec = CF.ContactRecording(cfg, B, s, {})
    rec.body_idx = np.arange(B)
    rec.ground, rec.measured = CF.stream_ground(kind, B), int(measured)
    rec.mu = stream_mu(B) if mu is None else np.asarray(mu, dtype=np.float64)
    model = FM.FrictionSRBModel(B, cfg, rec.ground, mu=rec.mu)
    if len(rec.body_idx):
        model.set_body(idx=rec.body_idx, mass=s["mass"][rec.body_idx], inertia=s["inertia"][:, rec.body_idx])
    rng = np.random.default_rng(seed + 1000)
    rec.start = (rng.uniform(-0.35, 0.35, (B, 2)), rng.uniform(-np.pi, np.pi, B), cfg.body_height * rng.uniform(0.9, 1.1, B))
    model.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
    rec.snap(model)
    idx = np.array([B - 1, 0, 17, 64, 33])
    idx = idx[idx < B] if B > 3 else np.array([B - 1])
    n = len(idx)
    rec.resets = {RESET_TICK: (idx, rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-np.pi, np.pi, n), cfg.body_height * rng.uniform(0.9, 1.1, n))}
    push, bad = np.random.default_rng([seed, 48]), poison(B)
    applies = (rec.mu >= 0.0) & (rec.mu < np.inf)
    rec.touches, rec.slips, rec.slipping, rec.sticking, rec.kept, rec.pulled = [], [], 0, 0, 0, 0
    for k in range(T):
        if k in rec.resets:
            i, xy, yaw, h = rec.resets[k]
            model.reset(idx=i, xy=xy, yaw=yaw, height=h)
        g = TF.stream_grf(model, cfg, s, k).reshape(B, 4, 3)
        # squeezing forces: drawn per foot, less their mean over the tick's stance feet, so they add no net force and, the feet
        # being level, no roll or pitch torque: the robots keep standing while their feet are asked for more than the floor holds
        on = (s["desired"][k] == 1)[:, :, None]
        t = np.where(on, TANGENT * 0.25 * cfg.mass * cfg.gravity * push.uniform(-1.0, 1.0, (B, 4, 2)), 0.0)
        t = np.where(on, t - t.sum(1, keepdims=True) / np.maximum(on.sum(1, keepdims=True), 1), 0.0)
        g[:, :, :2] += t.astype(np.float32)
        if k >= FALL_TICK:
            g[s["fall"]] = 0.0
        if k in bad:
            b, l, i, value = bad[k]
            g[b, l, i] = value
        g = np.ascontiguousarray(g.reshape(B, 12))
        ft = s["foot_target"][k].copy()
        ls = (s["leg_state"] if measured else s["desired"])[k].astype(np.int32).copy()
        ext = None if k % 3 == 0 else s["ext"][k].copy()
        before = model.state.copy()
        running = model.state[M.ROW_STATUS] == 0.0
        model.step_friction(g, ft, ls, rec.measured, ext)
        stored = running & (model.state[M.ROW_STEPS] != before[M.ROW_STEPS])
        on = (model.state[M.ROW_STANCE:M.ROW_STANCE + 4] == 1.0) & (stored & applies)[None, :]
        rec.slipping += int((on & (model.slip > 0.0)).sum())
        rec.sticking += int((on & (model.slip == 0.0)).sum())
        rec.kept += int((running & ~stored).sum())
        rec.pulled += int((on & (g.reshape(B, 4, 3)[:, :, 2].T > 0.0)).sum())        # the body being near level: asked to pull
        rec.inputs.append((g, ft, ls, ext))
        rec.touches.append(model.touch.copy())
        rec.slips.append(model.slip.copy())
        rec.snap(model)
    rec.model = model
    return rec


class RawFrictionSim(CF.RawContactSim):
    """contact_fixtures.RawContactSim stepping through rg_srb_step_friction, with guarded mu, touch and slip buffers."""

    def __init__(self, cfg, B, dev, mu, **sim_kw):
        super().__init__(cfg, B, dev, with_touch=True, **sim_kw)
        self.mu = self._guarded(1, self.torch.float64)[0]
        self.mu.copy_(self.torch.as_tensor(np.asarray(mu, dtype=np.float64), device=dev))
        self.slip = self._guarded(4, self.torch.float64)
        self.slip.fill_(-5.0)                # never a distance: every entry is written on every tick

    def step_friction(self, grf, foot_target, leg_state, measured, ext=None, slip_gain=FM.SLIP_GAIN, slip_speed_max=FM.SLIP_SPEED_MAX):
        from robot_gym_amd.core import friction_abi
        t = lambda a, dt: self.torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        self._held = (t(grf, np.float32), t(foot_target, np.float32), t(leg_state, np.int32), None if ext is None else t(ext, np.float64))
        g, f, d, e = self._held
        friction_abi.step_friction(self.handle, self.state, g, f, d, measured, e, self.ptrs, self.mu, slip_gain, slip_speed_max, self.touch, self.slip)


def start(rec, dev, mu=None):
    """A RawFrictionSim set up as the recording's model was: ground, bodies, start poses."""
    s = rec.s
    raw = RawFrictionSim(rec.cfg, rec.B, dev, rec.mu if mu is None else mu, **rec.sim_kw)
    TF.bind_ground(raw, rec.ground)
    raw.set_body(rec.body_idx, s["mass"][rec.body_idx], s["inertia"][:, rec.body_idx])
    raw.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
    return raw


def replay(rec, dev, cmp=None):
    """A run_model recording on the GPU through a RawFrictionSim.  cmp: a srb_streams.Comparison fed after the start and every
    tick.  The sentinels are asserted after every tick, touch is compared with the model's exactly and slip within
    REL_TOL * max(1, |value|).  -> (the RawFrictionSim, the largest slip deviation)."""
    raw = start(rec, dev)
    worst = 0.0

    def look(k):
        nonlocal worst
        if cmp is not None:
            st, obs = raw.numpy()
            cmp.check(st, obs, rec.states[k + 1], rec.obs[k + 1])
        if k >= 0:
            assert (raw.touch.cpu().numpy() == rec.touches[k]).all(), k
            got, want = raw.slip.cpu().numpy(), rec.slips[k]
            rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
            worst = max(worst, float(rel.max()))
            assert (rel <= S.REL_TOL).all(), (k, float(rel.max()))
        assert raw.guards_intact(), k

    look(-1)
    for k, (grf, ft, ls, ext) in enumerate(rec.inputs):
        if k in rec.resets:
            idx, xy, yaw, h = rec.resets[k]
            raw.reset(idx=idx, xy=xy, yaw=yaw, height=h)
        raw.step_friction(grf, ft, ls, rec.measured, ext)
        look(k)
    return raw, worst

