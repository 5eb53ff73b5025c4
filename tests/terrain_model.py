"""The float64 statement of the terrain of include/rg_srb.h in numpy: the ground function h(x, y; robot) of both kinds, and
srb_model.SRBModel with the three rules a terrain changes (where a foot lands, the clearance of the fall test, settle after
a reset).  It restates robot_gym_amd/csrc/rg_srb_terrain.hip operation for operation -- the same divisions, the fmax / fmin
clamp (np.fmax / np.fmin: a NaN becomes the lower bound), floor, the 2 x 2 grouping by arithmetic shift, the hash words of
tests/stream_model.py's chain, and the two triangle formulas left to right -- so the ground is held to it BIT FOR BIT
(tests/test_terrain_gpu.py) and the kernels to it within the simulator's existing tolerances.
"""
import numpy as np

from tests import srb_model as M
from tests.stream_model import chain as hash_words, uniform as unit, vuniform     # over (key, I, J): ints of any sign

BOUND = 2.0 ** 40
MAX_DIM = 4096


def unit_vec(seed, key, I, J):
    """unit() over int64 arrays (key, I, J broadcast together): uint64 arithmetic wraps as the device's does."""
    return vuniform(seed, *(np.asarray(a, dtype=np.int64).astype(np.uint64) for a in (key, I, J)))


def _lattice(s):
    with np.errstate(invalid="ignore"):
        s = np.fmin(np.fmax(s, -BOUND), BOUND)
    f = np.floor(s)
    return f.astype(np.int64), s - f


def _interpolate(u, v, h00, h10, h01, h11):
    with np.errstate(invalid="ignore"):
        lower = h00 + u * (h10 - h00) + v * (h11 - h10)
        upper = h00 + u * (h11 - h01) + v * (h01 - h00)
    return np.where(u >= v, lower, upper)


class Flat:
    kind = 0

    def height(self, x, y, robot):
        return np.zeros(np.broadcast(x, y).shape)


class Random:
    kind = 1

    def __init__(self, amplitude=0.06, cell=0.05, seed=0, keys=None):
        """keys: int64 [B], or None: key 0 for every robot (the C-ABI's NULL)."""
        self.amplitude, self.cell, self.seed = float(amplitude), float(cell), int(seed)
        self.keys = None if keys is None else np.asarray(keys, dtype=np.int64)

    def vertex(self, key, i, j):
        return self.amplitude * unit_vec(self.seed, key, np.asarray(i, np.int64) >> 1, np.asarray(j, np.int64) >> 1)

    def height(self, x, y, robot):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        key = np.zeros(x.shape, np.int64) if self.keys is None else self.keys[np.asarray(robot)]
        with np.errstate(all="ignore"):
            i, u = _lattice(x / self.cell)
            j, v = _lattice(y / self.cell)
        return _interpolate(u, v, self.vertex(key, i, j), self.vertex(key, i + 1, j), self.vertex(key, i, j + 1), self.vertex(key, i + 1, j + 1))


class Grid:
    kind = 2

    def __init__(self, heights, cell, origin=(0.0, 0.0)):
        self.heights = np.asarray(heights, dtype=np.float64)
        self.cell, self.x0, self.y0 = float(cell), float(origin[0]), float(origin[1])

    def height(self, x, y, robot=None):
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        H = self.heights
        with np.errstate(all="ignore"):
            i, u = _lattice((x - self.x0) / self.cell)
            j, v = _lattice((y - self.y0) / self.cell)
        ci = lambda a: np.clip(a, 0, H.shape[0] - 1)
        cj = lambda a: np.clip(a, 0, H.shape[1] - 1)
        return _interpolate(u, v, H[ci(i), cj(j)], H[ci(i + 1), cj(j)], H[ci(i), cj(j + 1)], H[ci(i + 1), cj(j + 1)])


class TerrainSRBModel(M.SRBModel):
    """SRBModel on a ground (Flat, Random or Grid above).  step() is the parent's text with the two ground rules replaced;
    reset() is the parent's followed by settle()."""

    def __init__(self, batch, cfg, ground=None, **kw):
        super().__init__(batch, cfg, **kw)
        self.ground = ground or Flat()

    def ground_height(self, x, y, robot=None):
        robot = np.arange(len(np.atleast_1d(x))) if robot is None else robot
        return self.ground.height(x, y, robot)

    def settle(self, idx=None):
        """The robots idx (None: all) whose status is 0."""
        st = self.state
        idx = np.arange(self.B) if idx is None else np.asarray(idx, dtype=np.int64).reshape(-1)
        idx = idx[st[M.ROW_STATUS, idx] == 0.0]
        if idx.size == 0:
            return
        hs = []
        for l in range(4):
            h = self.ground.height(st[M.ROW_FOOT + 3 * l, idx], st[M.ROW_FOOT + 3 * l + 1, idx], idx)
            st[M.ROW_FOOT + 3 * l + 2, idx] = h
            hs.append(h)
        st[M.ROW_P + 2, idx] = st[M.ROW_P + 2, idx] + ((hs[0] + hs[1]) + (hs[2] + hs[3])) * 0.25
        self._observe(idx, M.RESET_IK_PASSES)

    def reset(self, idx=None, xy=None, yaw=None, height=None):
        super().reset(idx, xy, yaw, height)
        if self.ground.kind != 0:
            self.settle(idx)

    def step(self, grf, foot_target, desired_state, ext=None):
        B, st, dt = self.B, self.state, self.dt
        all_robots = np.arange(B)
        grf = np.asarray(grf).astype(np.float64).reshape(B, 4, 3)
        ft = np.asarray(foot_target).astype(np.float64).reshape(B, 4, 3)
        swing = np.asarray(desired_state).reshape(B, 4) == M.SWING
        ext = np.zeros((6, B)) if ext is None else np.asarray(ext, dtype=np.float64)
        running = st[M.ROW_STATUS] == 0.0
        p = [st[M.ROW_P + i].copy() for i in range(3)]
        qt = [st[M.ROW_QUAT + i].copy() for i in range(4)]
        v = [st[M.ROW_V + i].copy() for i in range(3)]
        w = [st[M.ROW_W + i].copy() for i in range(3)]
        foot = [[st[M.ROW_FOOT + 3 * l + i].copy() for i in range(3)] for l in range(4)]
        stance = [st[M.ROW_STANCE + l].copy() for l in range(4)]
        mass, I, Iinv = self.mass, list(self.I), list(self.Iinv)
        R = M.quat_rot(qt)
        rot, rot_t = M.rot, M.rot_t
        fbody = []
        with np.errstate(all="ignore"):
            # 1. feet
            for l in range(4):
                sw = swing[:, l]
                r = rot(R, [ft[:, l, k] for k in range(3)])
                land = ~sw & (stance[l] == 0.0)
                for i in range(3):
                    foot[l][i] = np.where(sw, p[i] + r[i], foot[l][i])
                foot[l][2] = np.where(land, self.ground.height(foot[l][0], foot[l][1], all_robots), foot[l][2])     # terrain rule 1
                stance[l] = np.where(sw, 0.0, 1.0)
                fbody.append([np.where(sw, 0.0, -grf[:, l, i]) for i in range(3)])
            wz = mass * -self.g
            # 2. sub-steps
            for _ in range(self.S):
                R = M.quat_rot(qt)
                f, tq = [], []
                for l in range(4):
                    fl = rot(R, fbody[l])
                    r = [foot[l][i] - p[i] for i in range(3)]
                    f.append(fl)
                    tq.append([r[1] * fl[2] - r[2] * fl[1], r[2] * fl[0] - r[0] * fl[2], r[0] * fl[1] - r[1] * fl[0]])
                F = [(f[0][i] + f[1][i]) + (f[2][i] + f[3][i]) for i in range(3)]
                T = [(tq[0][i] + tq[1][i]) + (tq[2][i] + tq[3][i]) for i in range(3)]
                F = [F[0] + ext[0], F[1] + ext[1], F[2] + wz + ext[2]]
                T = [T[0] + ext[3], T[1] + ext[4], T[2] + ext[5]]
                tb, wb = rot_t(R, T), rot_t(R, w)
                Iw = rot(I, wb)
                rhs = [tb[0] - (wb[1] * Iw[2] - wb[2] * Iw[1]), tb[1] - (wb[2] * Iw[0] - wb[0] * Iw[2]), tb[2] - (wb[0] * Iw[1] - wb[1] * Iw[0])]
                aw = rot(R, rot(Iinv, rhs))
                for i in range(3):
                    w[i] = w[i] + dt * aw[i]
                    v[i] = v[i] + dt * F[i] / mass
                    p[i] = p[i] + dt * v[i]
                ax, ay, az = 0.5 * dt * w[0], 0.5 * dt * w[1], 0.5 * dt * w[2]
                dx = ax * qt[3] + ay * qt[2] - az * qt[1]
                dy = ay * qt[3] + az * qt[0] - ax * qt[2]
                dz = az * qt[3] + ax * qt[1] - ay * qt[0]
                dw = -(ax * qt[0]) - ay * qt[1] - az * qt[2]
                qt = [qt[0] + dx, qt[1] + dy, qt[2] + dz, qt[3] + dw]
                nrm = np.sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3])
                qt = [qt[i] / nrm for i in range(4)]
            # 3. fall
            finite = np.ones(B, dtype=bool)
            for a in p + v + w + qt + [foot[l][i] for l in range(4) for i in range(3)]:
                finite &= np.isfinite(a)
            clearance = p[2] - self.ground.height(p[0], p[1], all_robots)                                             # terrain rule 2
            fallen = ~finite | (clearance < self.fall_z) | ((1 - 2 * (qt[0] * qt[0] + qt[1] * qt[1])) < self.cos_tilt)
        st[M.ROW_STATUS] = np.where(running, np.where(fallen, 1.0, 0.0), st[M.ROW_STATUS])
        store = running & finite
        idx = np.nonzero(store)[0]
        for i in range(3):
            st[M.ROW_P + i, idx], st[M.ROW_V + i, idx], st[M.ROW_W + i, idx] = p[i][idx], v[i][idx], w[i][idx]
        for i in range(4):
            st[M.ROW_QUAT + i, idx] = qt[i][idx]
        for l in range(4):
            for i in range(3):
                st[M.ROW_FOOT + 3 * l + i, idx] = foot[l][i][idx]
            st[M.ROW_STANCE + l, idx] = stance[l][idx]
        st[M.ROW_STEPS, idx] = st[M.ROW_STEPS, idx] + float(self.S)
        # 4. observation
        if idx.size:
            self._observe(idx, 1)
