"""Numpy model of the state estimator error model (include/rg_est.h), written from the header alone and vectorised over robots:
the stream in uint64 (the functions of tests/sensor_model.py), every real in float64 with each expression evaluated left to right
as the header writes it, float32 only where the header converts.  The legs are srb_model.Chain.fk, the restatement of the
controller's leg_fk that the simulator's rows are tested against.  Bit for bit but for the rows that go through sqrt, atan2, asin
and the kinematics' sin / cos (quat, rpy, foot_pos, jac), where numpy's functions stand against the device's.

A configuration is a dict of DEFAULTS' fields.  An observation is a dict of component-major arrays [c, B] under the names of
rg_srb_obs_ptrs (float32; contact int32; t_robot float64 [B])."""
import numpy as np

from tests import sensor_model as SM
from tests.srb_model import Chain, quat_rot

ROWS = 8
ROW_KEY, ROW_DRAWS, ROW_TICKS, ROW_RUN = 0, 1, 2, 3
BIAS, NOISE, MISS, GHOST = range(32, 36)
OBS_ROW_RPY, OBS_ROW_RPY_RATE, OBS_ROW_V_WORLD, OBS_ROW_Q, OBS_ROW_CONTACT = 0, 3, 6, 13, 73
RUN_MAX = 1 << 20
TRIPLES = ("imu_bias_half_width", "imu_noise_sigma", "gyro_bias_half_width", "gyro_noise_sigma", "velocity_bias_half_width", "velocity_noise_sigma")
SCALARS = ("encoder_bias_half_width", "encoder_noise_sigma", "encoder_quantum", "contact_miss_probability", "contact_ghost_probability")
DEFAULTS = dict(seed=0, contact_rise_ticks=0, **{name: (0.0, 0.0, 0.0) for name in TRIPLES}, **{name: 0.0 for name in SCALARS})
OBS_FIELDS = (("rpy", 3, np.float32), ("rpy_rate", 3, np.float32), ("v_world", 3, np.float32), ("quat", 4, np.float32), ("q", 12, np.float32),
              ("foot_pos", 12, np.float32), ("jac", 36, np.float32), ("contact", 4, np.int32))

U = np.uint64


def settings(**s):
    unknown = set(s) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown estimator setting(s) {sorted(unknown)}")
    cfg = {**DEFAULTS, **s}
    for name in TRIPLES:
        cfg[name] = tuple(float(x) for x in cfg[name])
    return cfg


def new_state(B, keys=None):
    st = np.zeros((ROWS, B))
    st[ROW_KEY] = np.arange(B) if keys is None else keys
    return st


def new_obs(B):
    out = {name: np.zeros((comps, B), dtype=dt) for name, comps, dt in OBS_FIELDS}
    out["t_robot"] = np.zeros(B)
    return out


def reset(mask, st):
    """rg_est_reset in place on st."""
    on = np.flatnonzero(np.asarray(mask) != 0)
    st[ROW_DRAWS, on] = st[ROW_DRAWS, on] + 1.0
    st[ROW_TICKS, on] = 0.0
    st[ROW_RUN:ROW_RUN + 4, on] = float(RUN_MAX)


def bias(cfg, key, d, w, row):
    return w * (2.0 * SM.vuniform(cfg["seed"], key, d, BIAS, U(row)) - 1.0)


def perturb(cfg, x, key, d, k, w, s, row):
    """x + bias(w, row) + noise(s, k, row), each term skipped where its amplitude is 0."""
    if w != 0.0:
        x = x + bias(cfg, key, d, w, row)
    if s != 0.0:
        x = x + s * SM.vnoise(cfg["seed"], key, d, NOISE, k, U(row))
    return x


def tilt_error(cfg, key, d, k):
    """e of the header, [3, B]."""
    return np.stack([perturb(cfg, np.zeros(key.shape[0]), key, d, k, cfg["imu_bias_half_width"][i], cfg["imu_noise_sigma"][i], OBS_ROW_RPY + i) for i in range(3)])


def estimate(cfg, chain, st, true):
    """rg_est_estimate: updates st in place and returns the estimated observation (new arrays).  chain: srb_model.Chain."""
    B = st.shape[1]
    k = SM.bounded(st[ROW_TICKS], 2.0 ** 52)
    key, d = SM.words(st[ROW_KEY]), SM.words(st[ROW_DRAWS] - 1.0)
    est = {name: np.array(v, copy=True) for name, v in true.items()}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for field, row0, wname, sname in (("rpy_rate", OBS_ROW_RPY_RATE, "gyro_bias_half_width", "gyro_noise_sigma"),
                                          ("v_world", OBS_ROW_V_WORLD, "velocity_bias_half_width", "velocity_noise_sigma")):
            for i in range(3):
                w, s = cfg[wname][i], cfg[sname][i]
                if w != 0.0 or s != 0.0:
                    est[field][i] = perturb(cfg, true[field][i].astype(np.float64), key, d, k, w, s, row0 + i).astype(np.float32)
        if any(v != 0.0 for v in cfg["imu_bias_half_width"] + cfg["imu_noise_sigma"]):
            e = tilt_error(cfg, key, d, k)
            dx, dy, dz = e[0] / 2.0, e[1] / 2.0, e[2] / 2.0
            qx, qy, qz, qw = (true["quat"][i].astype(np.float64) for i in range(4))
            x = ((qw * dx + qx) + qy * dz) - qz * dy
            y = ((qw * dy - qx * dz) + qy) + qz * dx
            z = ((qw * dz + qx * dy) - qy * dx) + qz
            w = ((qw - qx * dx) - qy * dy) - qz * dz
            s = np.sqrt(((x * x + y * y) + z * z) + w * w)
            qn = [x / s, y / s, z / s, w / s]
            for i in range(4):
                est["quat"][i] = qn[i].astype(np.float32)
            R = quat_rot(qn)
            sp = np.where(R[6] > 1.0, 1.0, np.where(R[6] < -1.0, -1.0, R[6]))
            est["rpy"][0] = np.arctan2(R[7], R[8]).astype(np.float32)
            est["rpy"][1] = (-np.arcsin(sp)).astype(np.float32)
            est["rpy"][2] = np.arctan2(R[3], R[0]).astype(np.float32)
        wq, sq, quantum = cfg["encoder_bias_half_width"], cfg["encoder_noise_sigma"], cfg["encoder_quantum"]
        if wq != 0.0 or sq != 0.0 or quantum != 0.0:
            for j in range(12):
                x = perturb(cfg, true["q"][j].astype(np.float64), key, d, k, wq, sq, OBS_ROW_Q + j)
                if quantum != 0.0:
                    x = quantum * np.rint(x / quantum)
                est["q"][j] = x.astype(np.float32)
            for leg in range(4):
                p, J = chain.fk(np.full(B, leg), [est["q"][3 * leg + i].astype(np.float64) for i in range(3)])
                for i in range(3):
                    est["foot_pos"][3 * leg + i] = p[i].astype(np.float32)
                for i in range(9):
                    est["jac"][9 * leg + i] = J[i].astype(np.float32)
    rise, pm, pg = int(cfg["contact_rise_ticks"]), cfg["contact_miss_probability"], cfg["contact_ghost_probability"]
    for leg in range(4):
        on = true["contact"][leg] != 0
        run = SM.bounded(st[ROW_RUN + leg], float(RUN_MAX))
        run = np.where(on, np.minimum(run + U(1), U(RUN_MAX)), U(0))
        st[ROW_RUN + leg] = run.astype(np.float64)
        if rise == 0 and pm == 0.0 and pg == 0.0:
            continue                                       # the int32 is copied as it is
        seen = on & (run > U(rise))
        index = (k << U(12)) | U((OBS_ROW_CONTACT + leg) << 2)
        out = seen.copy()
        if pm != 0.0:
            out = out & ~(seen & (SM.vuniform(cfg["seed"], key, d, MISS, index) < pm))
        if pg != 0.0:
            out = out | (~on & (SM.vuniform(cfg["seed"], key, d, GHOST, index) < pg))
        est["contact"][leg] = out.astype(np.int32)
    st[ROW_TICKS] = (k + U(1)).astype(np.float64)
    return est


def random_obs(rng, B, chain=None):
    """A plausible true observation of the simulator's ranges: tilts within 0.4 rad with a consistent unit quat, rates and
    velocities of order 1, joint angles about a standing pose; foot_pos and jac of those angles where a chain is given."""
    o = new_obs(B)
    rpy = np.stack([rng.uniform(-0.4, 0.4, B), rng.uniform(-0.4, 0.4, B), rng.uniform(-3.1, 3.1, B)])
    cr, sr, cp, sp, cy, sy = (f(0.5 * rpy[i]) for i in range(3) for f in (np.cos, np.sin))
    quat = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])
    o["rpy"][:], o["quat"][:] = rpy, quat
    o["rpy_rate"][:] = rng.normal(0.0, 1.0, (3, B))
    o["v_world"][:] = rng.normal(0.0, 0.5, (3, B))
    stand = np.tile(np.array([0.0, 0.9, -1.8]), 4)[:, None]
    o["q"][:] = stand + rng.uniform(-0.5, 0.5, (12, B))
    if chain is None:
        o["foot_pos"][:] = rng.normal(0.0, 0.2, (12, B))
        o["jac"][:] = rng.normal(0.0, 0.2, (36, B))
    else:
        for leg in range(4):
            p, J = chain.fk(np.full(B, leg), [o["q"][3 * leg + i].astype(np.float64) for i in range(3)])
            o["foot_pos"][3 * leg:3 * leg + 3] = np.stack(p)
            o["jac"][9 * leg:9 * leg + 9] = np.stack(J)
    o["contact"][:] = rng.integers(0, 2, (4, B))
    o["t_robot"][:] = rng.uniform(0.0, 10.0, B)
    return o
