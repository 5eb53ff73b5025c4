"""What the measured-contact tests share (include/rg_srb_contact.h): the bands of the closed loop with measured contact on the
reference's random terrain, the CPU reference loop (srb_fixtures.CpuLoop with tests/contact_model.ContactSRBModel, stepped
on the oracle's leg_state), the step-grid case, and the recorded streams for the kernel with their replay on the GPU.

The bands are TWICE the worst value the CPU reference loop itself produces on the 32 srb_fixtures.cases of each robot at
amplitude AMPLITUDE with keys arange(32) (tests/test_contact_cpu.py recomputes them and fails if a constant here is not
twice its measurement): the convention of srb_fixtures.py.  The height band is taken on the clearance p.z - h(p.xy).
"""
import numpy as np

from tests import contact_model as CM
from tests import srb_fixtures as F
from tests import srb_model as M
from tests import srb_streams as S
from tests import terrain_fixtures as TF
from tests import terrain_model as TM

AMPLITUDE, CELL, SEED = TF.AMPLITUDE, TF.CELL, TF.SEED        # the reference's random terrain
WALKED = TF.WALKED

#                      band        measured worst (CPU reference loop with measured contact, 32 cases x 2 robots, last 2 s of 4)
BAND_HEIGHT = 2 * 0.19463     # |clearance - body_height| / body_height          0.19463     (ghost; k3lso 0.16767)
BAND_TILT = 2 * 0.0043047     # max(|roll|, |pitch|), rad                        0.0043047   (k3lso; ghost 0.0040911)
BAND_VX = 2 * 0.029890        # |mean body-frame vx - command|, m/s              0.029890    (ghost; k3lso 0.021995)
BAND_VY = 2 * 0.073843        # |mean body-frame vy - command|, m/s              0.073843    (ghost; k3lso 0.065869)
BAND_WZ = 2 * 0.00023289      # |mean body-frame yaw rate - command|, rad/s      0.00023289  (k3lso; ghost 0.00021499)
BANDS = dict(height=BAND_HEIGHT, tilt=BAND_TILT, vx=BAND_VX, vy=BAND_VY, wz=BAND_WZ)
# robots of the 32 that enter EARLY_CONTACT at least once in that run (a condition on the inputs: the branch is exercised);
# ghost spends 134 leg-ticks in it over 642 touch-downs, k3lso 92 over 653
EARLY_ROBOTS = dict(ghost=26, k3lso=24)


class ContactCpuLoop(F.CpuLoop):
    """F.CpuLoop with measured contact on a ground: the same oracle, the contact model stepped on the oracle's leg_state.
    early [B]: leg-ticks each robot spent in EARLY_CONTACT; lose: the same for LOSE_CONTACT; touched: touch-downs."""

    def __init__(self, robot, cmd, height_scale, ground, nthreads=0):
        super().__init__(robot, cmd, height_scale, nthreads)
        self.model = CM.ContactSRBModel(self.B, self.cfg, ground)
        self.model.reset(height=self.cfg.body_height * np.asarray(height_scale))
        self.early, self.lose, self.touched = np.zeros(self.B, int), np.zeros(self.B, int), np.zeros(self.B, int)

    def tick(self, ext=None):
        m = self.model
        out = self.oracle.step(float(m.obs["t_robot"][0]), F.oracle_inputs(self.O, m.obs, self.cmd))
        self.last = out
        ls = np.asarray(out["leg_state"]).reshape(self.B, 4)
        self.early += (ls == CM.EARLY_CONTACT).sum(1)
        self.lose += (ls == CM.LOSE_CONTACT).sum(1)
        m.step_contact(out["grf"].astype(np.float32), out["foot_target"].reshape(self.B, 12).astype(np.float32), ls, ext)
        self.touched += m.touch.sum(0)
        return TF.clearance_figures(m)


def run_cpu(robot, ground, ticks=F.TICKS, cmd=None, height_scale=None):
    """-> (trajectory dict of [ticks, B] arrays with z the clearance, the loop, path length [B] of the CoM in the plane)."""
    if cmd is None:
        cmd, height_scale = F.cases(robot)
    loop = ContactCpuLoop(robot, cmd, height_scale, ground)
    trajs, walked = [], np.zeros(loop.B)
    last = loop.model.state[M.ROW_P:M.ROW_P + 2].copy()
    for _ in range(ticks):
        trajs.append(loop.tick())
        now = loop.model.state[M.ROW_P:M.ROW_P + 2]
        walked += np.hypot(*(now - last))
        last = now.copy()
    return F.stack(trajs), loop, walked


def reference_ground(n=32):
    return TM.Random(AMPLITUDE, CELL, SEED, np.arange(n))


# The second, deterministic case: a 4 cm step up at |x| >= 0.5 m, the same for every y, and four ghost robots walking straight
# at it, forwards and backwards, fast and slowly.  Every one of them swings a foot into the rise.
STEP_HEIGHT, STEP_AT, STEP_CELL, STEP_ORIGIN = 0.04, 0.5, 0.05, (-3.0, -1.0)
STEP_CMD = np.array([[0.35, 0.0, 0.0], [-0.35, 0.0, 0.0], [0.2, 0.0, 0.0], [-0.2, 0.0, 0.0]], dtype=np.float32)
STEP_START = np.ones(4)            # start height / body_height


def step_heights():
    x = STEP_ORIGIN[0] + STEP_CELL * np.arange(121)
    return np.repeat(np.where(np.abs(x) >= STEP_AT - 1e-9, STEP_HEIGHT, 0.0)[:, None], 2, 1)


def step_ground():
    return TM.Grid(step_heights(), STEP_CELL, STEP_ORIGIN)


# ---- recorded streams for the kernel ----------------------------------------------------------------------------------

TICKS, FALL_TICK, RESET_TICK = 40, 10, 32
BATCHES = (1, 3, 67)               # 16 robots fill a wave and 64 a workgroup: 67 crosses both with a ragged tail
GROUNDS = ("flat", "random", "grid")
GRID_CELL, GRID_ORIGIN = 0.05, (-0.2, -0.15)


def stream_ground(kind, B):
    if kind == "flat":
        return TM.Flat()
    if kind == "random":
        keys = (np.arange(B, dtype=np.int64) * 7919 - 1000) % 4001 - 2000
        return TM.Random(0.06, 0.05, seed=777, keys=keys)
    return TM.Grid(np.random.default_rng(78).uniform(0.0, 0.06, (9, 7)), GRID_CELL, GRID_ORIGIN)


def faller(B):
    return min(63, B - 1)


def contact_streams(cfg, B, T, seed):
    """srb_streams.streams with leg_state [T,B,4] drawn from all four values (the crawl's schedule, with stance legs turned
    into EARLY_CONTACT, swing legs into LOSE_CONTACT and a few planted legs swung), `desired` replaced by what stream_grf needs
    (1 where the leg is not swung) and the targets' z spread about the ground: from 5 cm below the body's clearance height to
    6 cm above it."""
    fall = np.arange(B) == faller(B)
    s = S.streams(cfg, B, T, seed, fall, FALL_TICK)
    rng = np.random.default_rng([seed, 99])
    ls = s["desired"].copy()
    u = rng.uniform(size=ls.shape)
    ls = np.where((s["desired"] == 1) & (u < 0.15), CM.EARLY_CONTACT, ls)
    ls = np.where((s["desired"] == 1) & (u > 0.97), CM.LOSE_CONTACT, ls)
    ls = np.where((s["desired"] == 0) & (u < 0.3), CM.LOSE_CONTACT, ls)
    s["leg_state"] = ls.astype(np.int32)
    s["desired"] = ((ls == CM.STANCE) | (ls == CM.EARLY_CONTACT)).astype(np.int32)
    ft = s["foot_target"].reshape(T, B, 4, 3).copy()
    ft[..., 2] = (-cfg.body_height + rng.uniform(-0.05, 0.06, (T, B, 4))).astype(np.float32)
    s["foot_target"] = ft.reshape(T, B, 12)
    return s


class ContactRecording(S.Recording):
    """srb_streams.Recording of a ContactSRBModel run: inputs are (grf, foot_target, leg_state, ext), and touches[k] is the
    model's touch after tick k."""


def run_model(cfg, B, seed, kind, T=TICKS):
    """The contact model over T ticks of contact_streams on the ground `kind`: true bodies on the odd robots, ext pushes, one
    reset before tick RESET_TICK, robot faller(B) losing its forces at FALL_TICK.  -> ContactRecording with .ground, .touches,
    .swung_touch / .swung_free (leg-ticks of running robots)."""
    s = contact_streams(cfg, B, T, seed)
    rec = ContactRecording(cfg, B, s, {})
    rec.ground = stream_ground(kind, B)
    model = CM.ContactSRBModel(B, cfg, rec.ground)
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
    rec.touches, rec.swung_touch, rec.swung_free = [], 0, 0
    for k in range(T):
        if k in rec.resets:
            i, xy, yaw, h = rec.resets[k]
            model.reset(idx=i, xy=xy, yaw=yaw, height=h)
        g = TF.stream_grf(model, cfg, s, k)
        ft, ls = s["foot_target"][k].copy(), s["leg_state"][k].copy()
        ext = None if k % 3 == 0 else s["ext"][k].copy()
        running = model.state[M.ROW_STATUS] == 0.0
        model.step_contact(g, ft, ls, ext)
        swung = ((ls == CM.SWING) | (ls == CM.LOSE_CONTACT)) & running[:, None] & (model.state[M.ROW_STATUS] == 0.0)[:, None]
        rec.swung_touch += int((swung & (model.touch.T == 1)).sum())
        rec.swung_free += int((swung & (model.touch.T == 0)).sum())
        rec.inputs.append((g, ft, ls, ext))
        rec.touches.append(model.touch.copy())
        rec.snap(model)
    rec.model = model
    return rec


class RawContactSim(S.RawSim):
    """srb_streams.RawSim stepping through rg_srb_step_contact, with a guarded touch buffer (with_touch False: NULL)."""

    def __init__(self, cfg, B, dev, with_touch=True, **sim_kw):
        super().__init__(cfg, B, dev, **sim_kw)
        self.touch = self._guarded(4, self.torch.int32) if with_touch else None
        if with_touch:
            self.touch.fill_(-5)            # neither 0 nor 1: every entry is written on every tick

    def step_contact(self, grf, foot_target, leg_state, ext=None):
        t = lambda a, dt: self.torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        self._held = (t(grf, np.float32), t(foot_target, np.float32), t(leg_state, np.int32), None if ext is None else t(ext, np.float64))
        g, f, d, e = self._held
        self.handle.step_contact(self.state, g, f, d, e, self.ptrs, self.touch)


def replay(rec, dev, cmp=None, with_touch=True, after=None):
    """A ContactRecording on the GPU through a RawContactSim.  cmp: a srb_streams.Comparison fed after the start and every tick.
    The sentinels are asserted after every tick, and touch is compared with the model's exactly.  -> the RawContactSim."""
    s = rec.s
    raw = RawContactSim(rec.cfg, rec.B, dev, with_touch=with_touch, **rec.sim_kw)
    TF.bind_ground(raw, rec.ground)
    raw.set_body(rec.body_idx, s["mass"][rec.body_idx], s["inertia"][:, rec.body_idx])
    raw.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])

    def look(k):
        if cmp is not None:
            st, obs = raw.numpy()
            cmp.check(st, obs, rec.states[k + 1], rec.obs[k + 1])
        if with_touch and k >= 0:
            assert (raw.touch.cpu().numpy() == rec.touches[k]).all(), k
        assert raw.guards_intact(), k
        if after is not None:
            after(k, raw)

    look(-1)
    for k, (grf, ft, ls, ext) in enumerate(rec.inputs):
        if k in rec.resets:
            idx, xy, yaw, h = rec.resets[k]
            raw.reset(idx=idx, xy=xy, yaw=yaw, height=h)
        raw.step_contact(grf, ft, ls, ext)
        look(k)
    return raw


# ---- the equivalence stream: leg_state == desired_state and no swung target at or below the ground -------------------------

LIFT = 0.08        # more than the amplitude (0.06): the targets' z is shifted up by it


def equivalence_recording(cfg, B, T, seed, ground):
    """The SCHEDULE tick (TerrainSRBModel.step) on srb_streams.streams with the targets lifted by LIFT, so that no swung target
    comes to or below the ground; nobody loses their forces.  -> srb_streams.Recording with .ground; rec.inputs hold (grf,
    foot_target, desired_state, ext), and desired_state is the leg_state of the same run with measured contact."""
    s = S.streams(cfg, B, T, seed, np.zeros(B, bool))
    ft = s["foot_target"].reshape(T, B, 4, 3).copy()
    ft[..., 2] += np.float32(LIFT)
    s["foot_target"] = ft.reshape(T, B, 12)
    rec = S.Recording(cfg, B, s, {})
    rec.ground = ground
    model = TM.TerrainSRBModel(B, cfg, ground)
    if len(rec.body_idx):
        model.set_body(idx=rec.body_idx, mass=s["mass"][rec.body_idx], inertia=s["inertia"][:, rec.body_idx])
    rng = np.random.default_rng(seed + 1000)
    rec.start = (rng.uniform(-0.35, 0.35, (B, 2)), rng.uniform(-np.pi, np.pi, B), cfg.body_height * rng.uniform(0.9, 1.1, B))
    model.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
    rec.snap(model)
    rec.lowest = np.inf           # the least height of a swung target over the ground under it
    for k in range(T):
        g = TF.stream_grf(model, cfg, s, k)
        f, d = s["foot_target"][k].copy(), s["desired"][k].copy()
        ext = None if k % 3 == 0 else s["ext"][k].copy()
        st = model.state
        R = M.quat_rot([st[M.ROW_QUAT + i] for i in range(4)])
        for l in range(4):
            r = M.rot(R, [f[:, 3 * l + i].astype(np.float64) for i in range(3)])
            c = [st[M.ROW_P + i] + r[i] for i in range(3)]
            over = (c[2] - model.ground_height(c[0], c[1]))[(d[:, l] == 0) & (st[M.ROW_STATUS] == 0)]
            rec.lowest = min(rec.lowest, float(over.min())) if over.size else rec.lowest
        model.step(g, f, d, ext)
        rec.inputs.append((g, f, d, ext))
        rec.snap(model)
    rec.model = model
    return rec
