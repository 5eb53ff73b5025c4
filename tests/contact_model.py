"""The float64 statement of the tick with measured foot contact of include/rg_srb_contact.h in numpy: terrain_model.
TerrainSRBModel with step_contact, which is its step() with step 1 (the feet) and the force rule in their second form and
otherwise its text.  It restates robot_gym_amd/csrc/rg_srb_contact.hip operation for operation: one ground evaluation per
leg, at the swing target or under the foot, chosen by a select.  `touch` [4, B] int32 holds the last tick's touch-downs.
"""
import numpy as np

from tests import srb_model as M
from tests import terrain_model as TM

SWING, STANCE, EARLY_CONTACT, LOSE_CONTACT = 0, 1, 2, 3


class ContactSRBModel(TM.TerrainSRBModel):
    def __init__(self, batch, cfg, ground=None, **kw):
        super().__init__(batch, cfg, ground, **kw)
        self.touch = np.zeros((4, self.B), dtype=np.int32)

    def step_contact(self, grf, foot_target, leg_state, ext=None):
        B, st, dt = self.B, self.state, self.dt
        all_robots = np.arange(B)
        grf = np.asarray(grf).astype(np.float64).reshape(B, 4, 3)
        ft = np.asarray(foot_target).astype(np.float64).reshape(B, 4, 3)
        ls = np.asarray(leg_state).reshape(B, 4)
        swung = (ls == SWING) | (ls == LOSE_CONTACT)
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
        fbody, touches = [], []
        with np.errstate(all="ignore"):
            # 1. feet
            for l in range(4):
                sw = swung[:, l]
                r = rot(R, [ft[:, l, k] for k in range(3)])
                c = [p[i] + r[i] for i in range(3)]
                gh = self.ground.height(np.where(sw, c[0], foot[l][0]), np.where(sw, c[1], foot[l][1]), all_robots)
                touch = sw & (c[2] <= gh)
                land = ~sw & (stance[l] == 0.0)
                foot[l][0] = np.where(sw, c[0], foot[l][0])
                foot[l][1] = np.where(sw, c[1], foot[l][1])
                foot[l][2] = np.where(sw, np.where(touch, gh, c[2]), np.where(land, gh, foot[l][2]))
                stance[l] = np.where(sw, np.where(touch, 1.0, 0.0), 1.0)
                touches.append(touch)
                # the ground pushes only through a foot that is on it
                fbody.append([np.where(stance[l] == 1.0, -grf[:, l, i], 0.0) for i in range(3)])
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
            clearance = p[2] - self.ground.height(p[0], p[1], all_robots)
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
            # touch is this tick's: a robot that is frozen, or keeps its last state, touched nothing
            self.touch[l] = (store & touches[l]).astype(np.int32)
        st[M.ROW_STEPS, idx] = st[M.ROW_STEPS, idx] + float(self.S)
        # 4. observation
        if idx.size:
            self._observe(idx, 1)
