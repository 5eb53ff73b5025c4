"""Numpy model of the sensor and actuator model (include/rg_sensor.h), written from the header alone: the stream in uint64,
every real in float64 with each expression evaluated left to right as the header writes it, float32 only where the header
converts, so that the device's outputs are compared bit for bit.  Arrays are vectorised over rows and robots.  The stream
is tests/stream_model.py's; its names are kept here (hash4 and vhash are its chain and vchain) for the tests that use them.

A configuration is a dict: DEFAULTS' fields; groups is a list of (begin, end, dict of GROUP_DEFAULTS' fields)."""
import numpy as np

from tests.stream_model import GOLDEN, M64, U, bounded, delay_draw, ix, mix64, noise, uniform, vmix, vnoise, vuniform, words  # noqa: F401
from tests.stream_model import chain as hash4, vchain as vhash  # noqa: F401

ROWS = 8
ROW_KEY, ROW_DRAWS, ROW_OBS_TICKS, ROW_ACT_TICKS, ROW_OBS_DELAY, ROW_ACT_DELAY = range(6)
OBS_DELAY, ACT_DELAY, BIAS, NOISE, DROPOUT, ACT_NOISE = range(16, 22)
GROUP_DEFAULTS = dict(noise_sigma=0.0, bias_half_width=0.0, dropout_probability=0.0, dropout_value=0.0, quantum=0.0)
DEFAULTS = dict(obs_dim=1, act_dim=1, seed=0, groups=(), obs_delay_min=0, obs_delay_max=0, act_delay_min=0, act_delay_max=0, act_noise_sigma=(), act_fill=())


# ---- configuration and buffers -------------------------------------------------------------------------------------------

def settings(**s):
    unknown = set(s) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown sensor setting(s) {sorted(unknown)}")
    cfg = {**DEFAULTS, **s}
    cfg["groups"] = [(int(b), int(e), {**GROUP_DEFAULTS, **g}) for b, e, g in cfg["groups"]]
    A = cfg["act_dim"]
    cfg["act_noise_sigma"] = list(cfg["act_noise_sigma"]) + [0.0] * (A - len(cfg["act_noise_sigma"]))
    cfg["act_fill"] = list(cfg["act_fill"]) + [0.0] * (A - len(cfg["act_fill"]))
    return cfg


def new_buffers(cfg, B, keys=None):
    """dict of state [8, B], obs_ring [Lo, D, B], obs_out [D, B], act_ring [La, A, B] as reset expects to find them."""
    D, A = cfg["obs_dim"], cfg["act_dim"]
    st = np.zeros((ROWS, B))
    st[ROW_KEY] = np.arange(B) if keys is None else keys
    return dict(state=st, obs_ring=np.zeros((cfg["obs_delay_max"] + 1, D, B), dtype=np.float32), obs_out=np.zeros((D, B), dtype=np.float32),
                act_ring=np.zeros((cfg["act_delay_max"] + 1, A, B), dtype=np.float32))


def measure(cfg, key, d, k, clean):
    """The measurement of clean float32 [D, n] for robots with words key, d, k (uint64 [n]): float32 [D, n]."""
    out = np.array(clean, dtype=np.float32, copy=True)
    for begin, end, g in cfg["groups"]:
        sigma, bias, prob, dropv, quantum = (g[f] for f in ("noise_sigma", "bias_half_width", "dropout_probability", "dropout_value", "quantum"))
        if sigma == 0.0 and bias == 0.0 and prob == 0.0 and quantum == 0.0:
            continue                                       # copied bit for bit
        rows = np.arange(begin, end, dtype=U)[:, None]
        seed = cfg["seed"]
        with np.errstate(invalid="ignore", over="ignore"):
            x = clean[begin:end].astype(np.float64)
            if bias != 0.0:
                x = x + bias * (2.0 * vuniform(seed, key[None, :], d[None, :], BIAS, rows) - 1.0)
            if sigma != 0.0:
                x = x + sigma * vnoise(seed, key[None, :], d[None, :], NOISE, k[None, :], rows)
            if quantum != 0.0:
                x = quantum * np.rint(x / quantum)
            if prob != 0.0:
                drop = vuniform(seed, key[None, :], d[None, :], DROPOUT, (k[None, :] << U(12)) | (rows << U(2))) < prob
                x = np.where(drop, dropv, x)
            out[begin:end] = x.astype(np.float32)
    return out


def reset(cfg, mask, buf, clean, prev=None):
    """rg_sensor_reset in place on buf (new_buffers) and prev [D, B]."""
    on = np.flatnonzero(np.asarray(mask) != 0)
    if on.size == 0:
        return
    st = buf["state"]
    if prev is not None:
        prev[:, on] = buf["obs_out"][:, on]
    key, d = words(st[ROW_KEY, on]), words(st[ROW_DRAWS, on])
    seed = cfg["seed"]
    for row, purpose, lo, hi in ((ROW_OBS_DELAY, OBS_DELAY, cfg["obs_delay_min"], cfg["obs_delay_max"]),
                                 (ROW_ACT_DELAY, ACT_DELAY, cfg["act_delay_min"], cfg["act_delay_max"])):
        v = (float(hi - lo + 1) * vuniform(seed, key, d, purpose, U(0))).astype(U)
        st[row, on] = (U(lo) + np.minimum(v, U(hi - lo))).astype(np.float64)
    m = measure(cfg, key, d, np.zeros(on.size, dtype=U), clean[:, on])
    buf["obs_ring"][:, :, on] = m[None]
    buf["obs_out"][:, on] = m
    buf["act_ring"][:, :, on] = np.asarray(cfg["act_fill"], dtype=np.float64).astype(np.float32)[None, :, None]
    st[ROW_OBS_TICKS, on] = 1.0
    st[ROW_ACT_TICKS, on] = 0.0
    st[ROW_DRAWS, on] = st[ROW_DRAWS, on] + 1.0


def observe(cfg, buf, clean):
    """rg_sensor_observe in place on buf."""
    st = buf["state"]
    B = st.shape[1]
    Lo = U(cfg["obs_delay_max"] + 1)
    k = bounded(st[ROW_OBS_TICKS], 2.0 ** 52)
    dl = bounded(st[ROW_OBS_DELAY], cfg["obs_delay_max"])
    key, d = words(st[ROW_KEY]), words(st[ROW_DRAWS] - 1.0)
    m = measure(cfg, key, d, k, clean)
    cols = np.arange(B)
    buf["obs_ring"][(k % Lo).astype(np.int64), :, cols] = m.T
    buf["obs_out"][:] = buf["obs_ring"][((k + Lo - dl) % Lo).astype(np.int64), :, cols].T
    st[ROW_OBS_TICKS] = (k + U(1)).astype(np.float64)


def act(cfg, buf, act_in):
    """rg_sensor_act in place on buf; act_in float32 [B, A]; returns act_out float32 [B, A]."""
    st = buf["state"]
    B, A = st.shape[1], cfg["act_dim"]
    La = U(cfg["act_delay_max"] + 1)
    k = bounded(st[ROW_ACT_TICKS], 2.0 ** 52)
    dl = bounded(st[ROW_ACT_DELAY], cfg["act_delay_max"])
    key, d = words(st[ROW_KEY]), words(st[ROW_DRAWS] - 1.0)
    v = np.array(act_in, dtype=np.float32, copy=True).T      # [A, B]
    for a in range(A):
        sigma = cfg["act_noise_sigma"][a]
        if sigma != 0.0:
            with np.errstate(invalid="ignore", over="ignore"):
                v[a] = (v[a].astype(np.float64) + sigma * vnoise(cfg["seed"], key, d, ACT_NOISE, k, U(a))).astype(np.float32)
    cols = np.arange(B)
    buf["act_ring"][(k % La).astype(np.int64), :, cols] = v.T
    st[ROW_ACT_TICKS] = (k + U(1)).astype(np.float64)
    return np.ascontiguousarray(buf["act_ring"][((k + La - dl) % La).astype(np.int64), :, cols])
