"""Numpy model of the domain randomisation (include/rg_dr.h): the stream of tests/stream_model.py, every real in float64 with each
expression evaluated left to right as the header writes it, so that the device's outputs are compared bit for bit.  The
state is the header's [8, B] table; the body table is [19, B] (mass, I, I^-1)."""
import numpy as np

from tests.stream_model import GOLDEN, M64, mix64, uniform  # noqa: F401
from tests.stream_model import chain as hash4

ROWS, BODY_ROWS = 8, 19
ROW_KEY, ROW_DRAWS, ROW_MASS_SCALE, ROW_INERTIA_SCALE, ROW_WORLD = range(5)
MASS, INERTIA, WORLD, PUSH_START, PUSH_COMPONENT, PUSH_GATE = range(6)
STEPS_ROW = 41
DEFAULTS = dict(worlds=0, seed=0, mass_lo=1.0, mass_hi=1.0, inertia_lo=1.0, inertia_hi=1.0, push_interval=0, push_ticks=0, push_probability=0.0,
                push_force_xy=0.0, push_force_z=0.0, push_torque_xy=0.0, push_torque_z=0.0, substeps=10)


def word(v):
    """A state row's integer as the device reads it: through int64 to uint64."""
    return int(v) & M64


def settings(**s):
    unknown = set(s) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown randomiser setting(s) {sorted(unknown)}")
    return {**DEFAULTS, **s}


def new_state(B, keys=None, world=None):
    st = np.zeros((ROWS, B))
    st[ROW_KEY] = np.arange(B) if keys is None else keys
    st[ROW_MASS_SCALE] = st[ROW_INERTIA_SCALE] = 1.0
    if world is not None:
        st[ROW_WORLD] = world
    return st


def scaled_body(base, b, sm, si):
    """Column b of the body table: base scaled."""
    col = np.empty(BODY_ROWS)
    col[0] = base[0, b] * sm
    col[1:10] = base[1:10, b] * si
    col[10:19] = base[10:19, b] / si
    return col


def draw_scales(cfg, key, d):
    sm = cfg["mass_lo"] + (cfg["mass_hi"] - cfg["mass_lo"]) * uniform(cfg["seed"], key, d, MASS, 0)
    si = cfg["inertia_lo"] + (cfg["inertia_hi"] - cfg["inertia_lo"]) * uniform(cfg["seed"], key, d, INERTIA, 0)
    return sm, si


def reset(cfg, mask, st, base, body, terrain_key=None):
    """rg_dr_reset in place on st [8, B], body [19, B] and terrain_key int64 [B]."""
    for b in np.flatnonzero(np.asarray(mask) != 0):
        key, d = word(st[ROW_KEY, b]), word(st[ROW_DRAWS, b])
        sm, si = draw_scales(cfg, key, d)
        body[:, b] = scaled_body(base, b, sm, si)
        if cfg["worlds"]:
            w = hash4(cfg["seed"], key, d, WORLD, 0) >> 33
            terrain_key[b] = w
            st[ROW_WORLD, b] = float(w)
        st[ROW_MASS_SCALE, b], st[ROW_INERTIA_SCALE, b] = sm, si
        st[ROW_DRAWS, b] = st[ROW_DRAWS, b] + 1.0


def apply(mask, st, base, body):
    """rg_dr_apply in place on body; mask None: every robot."""
    B = st.shape[1]
    for b in (range(B) if mask is None else np.flatnonzero(np.asarray(mask) != 0)):
        sm, si = st[ROW_MASS_SCALE, b], st[ROW_INERTIA_SCALE, b]
        if 0.0 < sm < np.inf and 0.0 < si < np.inf:
            body[:, b] = scaled_body(base, b, sm, si)


def tick_of(steps, substeps):
    """k of rg_dr_push: fmin(fmax(steps, 0), 2^52) as uint64, over substeps; a NaN is 0."""
    s = 0.0 if np.isnan(steps) else min(max(float(steps), 0.0), 2.0 ** 52)
    return int(s) // int(substeps)


def push_window(cfg, key, d, win):
    """(start, pushes?) of window `win`."""
    n = cfg["push_interval"] - cfg["push_ticks"] + 1
    start = min(int(float(n) * uniform(cfg["seed"], key, d, PUSH_START, win)), n - 1)
    return start, uniform(cfg["seed"], key, d, PUSH_GATE, win) < cfg["push_probability"]


def amplitudes(cfg):
    return (cfg["push_force_xy"], cfg["push_force_xy"], cfg["push_force_z"], cfg["push_torque_xy"], cfg["push_torque_xy"], cfg["push_torque_z"])


def push_one(cfg, key, d, steps):
    """The six ext components of one robot."""
    k = tick_of(steps, cfg["substeps"])
    win, r = divmod(k, cfg["push_interval"])
    start, gate = push_window(cfg, key, d, win)
    if not (start <= r < start + cfg["push_ticks"] and gate):
        return np.zeros(6)
    return np.array([amp * (2.0 * uniform(cfg["seed"], key, d, PUSH_COMPONENT, 8 * win + a) - 1.0) for a, amp in enumerate(amplitudes(cfg))])


def push(cfg, sim_state, st):
    """rg_dr_push: ext [6, B]."""
    B = st.shape[1]
    return np.stack([push_one(cfg, word(st[ROW_KEY, b]), word(st[ROW_DRAWS, b]), sim_state[STEPS_ROW, b]) for b in range(B)], axis=1)
