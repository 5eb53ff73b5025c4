"""Seeded input streams for the single-rigid-body simulator's kernel tests, the comparison of a kernel state with the float64
model (tests/srb_model.py), a model run recorded ahead of time, and a raw-buffer harness over srb_abi.SrbHandle.

The streams and the comparison are those of tests/test_srb_gpu.py::test_kernel_vs_model (same draws from the same seeds);
tests/test_srb_edges_gpu.py replays recorded model runs on the batches, settings and inputs of tests/srb_edges.py.  Nothing
here imports torch until a RawSim is made, so the CPU suite can run the model side of every seeded input.
"""
import numpy as np

from tests import srb_model as M
from tests.posctl_fixtures import REL_TOL, within_ulp
from tests.srb_fixtures import Q_TOL, Q_ULP

GUARD = 777           # the sentinel around every buffer of a RawSim: exact in float64, float32 and int32
PAD = 256             # sentinel elements on each side

INT_ROWS = list(range(M.ROW_STANCE, M.ROW_STANCE + 4)) + [M.ROW_STEPS, M.ROW_STATUS]
Q_ROWS = list(range(M.ROW_Q, M.ROW_Q + 12))
F_ROWS = [r for r in range(M.STATE_ROWS) if r not in INT_ROWS and r not in Q_ROWS]
OBS_NAMES = ("rpy", "rpy_rate", "v_world", "quat", "foot_pos", "q", "jac")


def streams(cfg, B, T, seed, fall=None, fall_tick=45):
    """What is drawn ahead of the run, one seeded stream per robot.  desired_state [T,B,4]: a crawl, one leg in swing at a time, with
    the robot's own period, duty and phase (both states, lift-off and touch-down, three- and four-leg ticks: the stance feet
    can then realise any wrench, which stream_grf needs); foot_target
    [T,B,12] float32: around the hips, lifted; force noise; ext [T,6,B] for the robots 0 and 1 mod 4; a true body for the
    odd robots (so a quarter of the batch has both, a quarter neither); robots 63 mod 64 (or the mask `fall`) lose their
    forces at tick `fall_tick` and fall."""
    rng = np.random.default_rng(seed)
    period = rng.integers(16, 48, B)
    duty = rng.uniform(0.76, 0.95, B)
    phase0 = rng.uniform(0, 1, B)
    k = np.arange(T)[:, None]
    ph = np.stack([(k / period + phase0 + off) % 1.0 for off in (0.0, 0.5, 0.75, 0.25)], 2)     # FR, FL, RR, RL
    desired = (ph < duty[None, :, None]).astype(np.int32)                                          # 1 STANCE, 0 SWING
    true_mass = np.full(B, cfg.mass)
    true_mass[1::2] *= rng.uniform(0.85, 1.15, B // 2)
    inertia = np.tile(np.asarray(cfg.inertia).reshape(9, 1), (1, B))
    scale = rng.uniform(0.8, 1.25, (3, B // 2))
    for a in range(3):
        inertia[4 * a, 1::2] *= scale[a]
    off = rng.uniform(-0.004, 0.004, B // 2)
    inertia[1, 1::2] = off
    inertia[3, 1::2] = off
    hip = np.asarray(cfg.hip).reshape(4, 3)
    ft = np.zeros((T, B, 4, 3))
    ft[..., 0] = hip[:, 0] + rng.uniform(-0.06, 0.06, (T, B, 4))
    ft[..., 1] = hip[:, 1] + rng.uniform(-0.04, 0.04, (T, B, 4))
    ft[..., 2] = -cfg.body_height + rng.uniform(0.0, 0.07, (T, B, 4))
    ext = np.zeros((T, 6, B))
    pushed = np.arange(B) % 4 < 2
    ext[:, :3, pushed] = rng.uniform(-4.0, 4.0, (T, 3, int(pushed.sum())))
    ext[:, 3:, pushed] = rng.uniform(-0.15, 0.15, (T, 3, int(pushed.sum())))
    return dict(desired=desired, foot_target=ft.reshape(T, B, 12).astype(np.float32), ext=ext, mass=true_mass, inertia=inertia,
                fall=np.arange(B) % 64 == 63 if fall is None else np.asarray(fall, dtype=bool), fall_tick=int(fall_tick),
                noise=rng.uniform(-1.0, 1.0, (T, B, 12)))


def stream_grf(model, cfg, s, k):
    """The grf row of tick k, float32 [B,12]: so that the streams keep the robots near their stance (feet the chain can
    reach) without a controller, the forces are the least-norm ones over the tick's stance feet of a wrench that holds the
    TRUE weight and damps height, tilt and velocities, computed from the MODEL's state before the tick, plus the stream's
    noise.  Deterministic given the seed; the kernels and the model are handed the same float32 values."""
    st, B = model.state, model.B
    R = np.stack(M.quat_rot([st[M.ROW_QUAT + i] for i in range(4)]), 1).reshape(B, 3, 3)
    p, v, w = st[M.ROW_P:M.ROW_P + 3].T, st[M.ROW_V:M.ROW_V + 3].T, st[M.ROW_W:M.ROW_W + 3].T
    wrench = np.zeros((B, 6))
    wrench[:, :3] = -8.0 * s["mass"][:, None] * v
    wrench[:, 2] += s["mass"] * (cfg.gravity + 60.0 * (cfg.body_height - p[:, 2]))
    tilt = np.stack([np.arctan2(R[:, 2, 1], R[:, 2, 2]), -np.arcsin(np.clip(R[:, 2, 0], -1, 1)), np.zeros(B)], 1)
    Idiag = np.asarray(cfg.inertia)[[0, 4, 8]]
    wrench[:, 3:] = np.einsum("bij,bj->bi", R, Idiag * (-80.0 * tilt - 12.0 * np.einsum("bji,bj->bi", R, w)))
    stance = s["desired"][k] == 1
    A = np.zeros((B, 6, 12))
    for l in range(4):
        r = st[M.ROW_FOOT + 3 * l:M.ROW_FOOT + 3 * l + 3].T - p
        # a swing foot that comes down this tick lands where it is, at z = 0
        r[:, 2] = np.where(stance[:, l] & (st[M.ROW_STANCE + l] == 0), -p[:, 2], r[:, 2])
        on = stance[:, l].astype(np.float64)
        for c in range(3):
            A[:, c, 3 * l + c] = on
        A[:, 3, 3 * l + 1], A[:, 3, 3 * l + 2] = -r[:, 2] * on, r[:, 1] * on
        A[:, 4, 3 * l], A[:, 4, 3 * l + 2] = r[:, 2] * on, -r[:, 0] * on
        A[:, 5, 3 * l], A[:, 5, 3 * l + 1] = -r[:, 1] * on, r[:, 0] * on
    ok = np.isfinite(A).all((1, 2)) & np.isfinite(wrench).all(1)
    f = np.zeros((B, 12))
    f[ok] = np.einsum("bij,bj->bi", np.linalg.pinv(A[ok], rcond=1e-6), wrench[ok])
    f = f.reshape(B, 4, 3) + 1.5 * s["noise"][k].reshape(B, 4, 3)
    grf = -np.einsum("bji,blj->bli", R, f)                # body frame, negated: what the controller's grf output holds
    grf[np.isfinite(grf) == False] = 0.0                 # noqa: E712
    if k >= s.get("fall_tick", 45):
        grf[s["fall"]] = 0.0
    return grf.reshape(B, 12).astype(np.float32)


def _within_ulps(got, want, n):
    want = np.asarray(want)
    return np.abs(np.asarray(got) - want) <= n * np.spacing(np.abs(want))


class Comparison:
    """The per-tick comparison of test_kernel_vs_model, added up over the ticks it is called on: integers and t_robot
    bit-exact; float64 state rows within REL_TOL * max(1, |value|); float32 observation rows within one float32 ulp of the
    model's rounded value; q state rows within Q_TOL and q / jac observation rows within Q_ULP ulp."""

    def __init__(self):
        self.worst = dict(state_rel=0.0, q_abs=0.0, obs_ulp=0.0, qjac_ulp=0.0)
        self.bad = dict(ints=0, t_robot=0, contact=0, state=0, q=0, obs=0, qjac=0)

    def check(self, st, obs, ms, mobs):
        """st [43,B] and obs (dict of arrays) of the kernels against the model's ms and mobs."""
        worst, bad = self.worst, self.bad
        bad["ints"] += int((st[INT_ROWS] != ms[INT_ROWS]).sum())
        bad["t_robot"] += int((obs["t_robot"] != mobs["t_robot"]).sum())
        bad["contact"] += int((obs["contact"] != mobs["contact"]).sum())
        rel = np.abs(st[F_ROWS] - ms[F_ROWS]) / np.maximum(1.0, np.abs(ms[F_ROWS]))
        worst["state_rel"] = max(worst["state_rel"], float(rel.max()))
        bad["state"] += int((~(rel <= REL_TOL)).sum())
        dq = np.abs(st[Q_ROWS] - ms[Q_ROWS])
        worst["q_abs"] = max(worst["q_abs"], float(dq.max()))
        bad["q"] += int((~(dq <= Q_TOL)).sum())
        for name in OBS_NAMES:
            want = mobs[name]
            ulps = np.abs(obs[name].astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
            key, n = ("qjac_ulp", Q_ULP) if name in ("q", "jac") else ("obs_ulp", 1)
            worst[key] = max(worst[key], float(ulps.max()))
            ok = _within_ulps(obs[name], want, n) if name in ("q", "jac") else within_ulp(obs[name], want)
            bad["qjac" if name in ("q", "jac") else "obs"] += int((~ok).sum())

    def clean(self):
        return all(v == 0 for v in self.bad.values())


# ---- a model run recorded ahead of time -----------------------------------------------------------------------------

class Recording:
    """One run of the model: what it was given (body, start, resets, per-tick inputs) and what it held after the start
    (states[0], obs[0]) and after every tick k (states[k + 1], obs[k + 1])."""

    def __init__(self, cfg, B, s, sim_kw):
        self.cfg, self.B, self.s, self.sim_kw = cfg, B, s, sim_kw
        self.body_idx = np.arange(1, B, 2)
        self.start, self.resets, self.inputs, self.states, self.obs = None, {}, [], [], []

    def snap(self, model):
        self.states.append(model.state.copy())
        self.obs.append({k: v.copy() for k, v in model.obs.items()})

    @property
    def ticks(self):
        return len(self.inputs)


def start_poses(cfg, B, rng, heights=(0.9, 1.1)):
    """(xy [n,2], yaw [n], height [n]) in the order test_kernel_vs_model draws them."""
    return rng.uniform(-2, 2, (B, 2)), rng.uniform(-np.pi, np.pi, B), cfg.body_height * rng.uniform(heights[0], heights[1], B)


def run_model(cfg, B, T, seed, resets=None, poison=None, no_ext=lambda k: k % 3 == 0, s=None, heights=(0.9, 1.1), fall=None,
              fall_tick=45, **sim_kw):
    """The model over T ticks of streams(cfg, B, T, seed) (or the prepared `s`), the odd robots with their true body, started
    from start_poses of seed + 1000.  resets: {tick: (idx, xy, yaw, height)} applied before that tick.  poison: a callable
    (k, grf, foot_target, desired, ext) that may change the tick's inputs in place (ext is None on the ticks no_ext names:
    the NULL path).  sim_kw: the simulator's settings.  -> Recording."""
    s = streams(cfg, B, T, seed, fall, fall_tick) if s is None else s
    rec = Recording(cfg, B, s, sim_kw)
    model = M.SRBModel(B, cfg, **sim_kw)
    assert model.fallen().all()                                   # nothing runs before its reset
    if len(rec.body_idx):
        model.set_body(idx=rec.body_idx, mass=s["mass"][rec.body_idx], inertia=s["inertia"][:, rec.body_idx])
    rec.start = start_poses(cfg, B, np.random.default_rng(seed + 1000), heights)
    model.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
    rec.snap(model)
    rec.resets = dict(resets or {})
    for k in range(T):
        if k in rec.resets:
            idx, xy, yaw, h = rec.resets[k]
            model.reset(idx=idx, xy=xy, yaw=yaw, height=h)
        grf = stream_grf(model, cfg, s, k)
        ft, d = s["foot_target"][k].copy(), s["desired"][k].copy()
        ext = None if no_ext(k) else s["ext"][k].copy()
        if poison is not None:
            poison(k, grf, ft, d, ext)
        model.step(grf, ft, d, ext)
        rec.inputs.append((grf, ft, d, ext))
        rec.snap(model)
    return rec


# ---- the kernels on caller-owned buffers ---------------------------------------------------------------------------

class RawSim:
    """srb_abi.SrbHandle with caller-owned state and observation tensors.  rg_srb.h lays every buffer out as [rows][B] with
    the row stride equal to B, so none may have guard columns of its own: each is a slice of one flat allocation with PAD
    elements of GUARD before and after it, so that a store past the last row -- where a lane past the batch would land -- or
    before the first hits a sentinel.  A store past the batch inside the buffer lands on another row's robot 0 .. and is
    seen by the comparison with the model."""

    def __init__(self, cfg, B, dev, **sim_kw):
        import torch
        from robot_gym_amd.controllers.mpc.batched import STATE_FIELDS
        from robot_gym_amd.core import srb_abi
        self.torch, self.dev, self.B = torch, dev, B
        self.handle = srb_abi.SrbHandle(cfg, B, dev, **sim_kw)
        self._backs = []
        self.state = self._guarded(srb_abi.STATE_ROWS, torch.float64)
        self.state[srb_abi.ROW_STATUS] = 1.0          # nothing runs before the first reset
        self.obs = {name: self._guarded(comps, dt) for name, comps, dt in STATE_FIELDS}
        self.obs["t_robot"] = self._guarded(1, torch.float64)[0]
        self.ptrs = srb_abi.CObsPtrs()
        for name in srb_abi.OBS_FIELDS:
            setattr(self.ptrs, name, self.obs[name].data_ptr())

    def _guarded(self, rows, dtype):
        back = self.torch.full((2 * PAD + rows * self.B,), GUARD, dtype=dtype, device=self.dev)
        view = back[PAD:PAD + rows * self.B].view(rows, self.B)
        view.zero_()
        self._backs.append(back)
        return view

    def guards_intact(self):
        return all(bool((b[:PAD] == GUARD).all()) and bool((b[-PAD:] == GUARD).all()) for b in self._backs)

    def set_body(self, idx, mass, inertia):
        if len(idx):
            self.handle.set_body(idx, mass, inertia)

    def reset(self, idx=None, xy=None, yaw=None, height=None):
        n = self.B if idx is None else len(idx)
        c = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))
        self.handle.reset(self.state.data_ptr(), self.ptrs, idx, None if xy is None else np.ascontiguousarray(np.asarray(xy, dtype=np.float64).T),
                          c(yaw), c(height))

    def step(self, grf, foot_target, desired, ext=None):
        """Host arrays: grf, foot_target [B,12] float32, desired [B,4] int32, ext [6,B] float64 or None."""
        t = lambda a, dt: self.torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=self.dev)
        self._held = (t(grf, np.float32), t(foot_target, np.float32), t(desired, np.int32), None if ext is None else t(ext, np.float64))
        g, f, d, e = self._held
        self.handle.step(self.state.data_ptr(), g.data_ptr(), f.data_ptr(), d.data_ptr(), None if e is None else e.data_ptr(), self.ptrs)

    def numpy(self):
        """(state [43,B], obs dict) on the host."""
        return self.state.cpu().numpy(), {k: v.cpu().numpy() for k, v in self.obs.items()}

    def close(self):
        self.handle.close()


def replay(rec, dev, cmp=None, after=None, guards_every_tick=True):
    """A Recording on the GPU through a RawSim: body, start, resets and every tick's inputs as the model had them.  cmp: a
    Comparison fed after the start and after every tick.  after: a callable (k, raw) after tick k (k = -1: after the
    start).  The sentinels are asserted after every tick.  -> the RawSim."""
    s = rec.s
    raw = RawSim(rec.cfg, rec.B, dev, **rec.sim_kw)
    raw.set_body(rec.body_idx, s["mass"][rec.body_idx], s["inertia"][:, rec.body_idx])
    raw.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])

    def look(k):
        if cmp is not None:
            st, obs = raw.numpy()
            cmp.check(st, obs, rec.states[k + 1], rec.obs[k + 1])
        if guards_every_tick:
            assert raw.guards_intact(), k
        if after is not None:
            after(k, raw)

    look(-1)
    for k, (grf, ft, d, ext) in enumerate(rec.inputs):
        if k in rec.resets:
            idx, xy, yaw, h = rec.resets[k]
            raw.reset(idx=idx, xy=xy, yaw=yaw, height=h)
        raw.step(grf, ft, d, ext)
        look(k)
    return raw
