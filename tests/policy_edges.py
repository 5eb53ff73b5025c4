"""Seeded inputs of tests/test_policy_edges_gpu.py: network shapes that exercise the act kernel's control flow (no hidden
layer, one network deeper than the other, widths at the wave boundaries), act states with keys, counters and a seed beyond
32 bits, normaliser states at their edges (empty, one sample, a constant column) with and without clipping, and the inputs of
the record and returns edge runs.  Plain numpy; tests/test_policy_edges_cpu.py runs the model alone over every one of them.
"""
import functools
import math

import numpy as np

from tests import policy_model as PM

# ---- configurations ---------------------------------------------------------------------------------------------------

CONFIGS = {
    "head_only": dict(obs_dim=1, act_dim=1, policy_layers=(), value_layers=()),                          # no hidden layer in either network
    "policy_deeper": dict(obs_dim=5, act_dim=3, policy_layers=(9, 65, 3), value_layers=()),              # the value half idles, its result waits
    "value_deeper": dict(obs_dim=7, act_dim=2, policy_layers=(), value_layers=(64, 63, 255)),            # the policy half idles
    "wave_edges": dict(obs_dim=63, act_dim=4, policy_layers=(63, 64, 65), value_layers=(255, 256, 1)),   # widths at the wave boundaries
}
TRANSFORM = dict(obs_dim=64, act_dim=1, policy_layers=(), value_layers=())   # the value head reads one component: the transform, observable
TRANSFORM_BATCH = 13
BATCHES = {"head_only": (1, 13), "policy_deeper": (1, 13), "value_deeper": (1, 13), "wave_edges": (1, 13, 1037)}   # 13: a full tile and a ragged one
POOL = 1037
SEED = 2 ** 63 + 0x1234_5678_9ABC          # of the noise stream: its top bit is set
M32 = 0xFFFFFFFF


def config_of(name):
    return TRANSFORM if name == "transform" else CONFIGS[name]


@functools.lru_cache(maxsize=None)
def params(name):
    """(layout, policy_params, value_params) of a configuration: distinct random weights within the Glorot limit, non-zero
    biases, a distinct logstd per component."""
    cfg = config_of(name)
    rng = np.random.default_rng(700 + sorted(list(CONFIGS) + ["transform"]).index(name))
    lay = PM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["value_layers"])
    out = {}
    for net in ("policy", "value"):
        p = np.zeros(lay[net + "_count"], dtype=np.float32)
        for i, o, w, b in lay[net]:
            limit = math.sqrt(6.0 / (i + o))
            p[w:w + i * o] = rng.uniform(-limit, limit, i * o)
            p[b:b + o] = rng.normal(0.0, 0.1, o)
        out[net] = p
    out["policy"][lay["logstd_offset"]:] = -1.0 + 0.2 * np.arange(cfg["act_dim"]) + rng.normal(0.0, 0.05, cfg["act_dim"])
    return lay, out["policy"], out["value"]


# ---- act states -------------------------------------------------------------------------------------------------------

KEYS = (2 ** 32 + 5, -1, -2 ** 63, 2 ** 40, 2 ** 63 - 1, 3 * 2 ** 32, -2 ** 32 - 9)
COUNTERS = (2 ** 32 - 1, 2 ** 62, 2 ** 32, 2 ** 40 + 3, 0, 2 ** 33 + 1, 2 ** 62 + 2 ** 31)   # never 2^63 - 1: its increment overflows


def act_states(B):
    """(keys, counters) int64 [B]: the lists above first (so a batch of one has a wide key, and the counter whose increment
    crosses 32 bits), then keys spread over all 64 bits and counters above 2^32."""
    b = np.arange(B, dtype=np.uint64)
    keys = (b * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)).astype(np.int64)   # wraps modulo 2^64
    counters = ((b * np.uint64(0x2545F4914F6CDD1D)) >> np.uint64(2)).astype(np.int64)                # below 2^62
    keys[:len(KEYS)] = KEYS[:B]
    counters[:len(COUNTERS)] = COUNTERS[:B]
    return keys, counters


def truncations(v):
    """The values a 32-bit cast of the 64-bit word v can give: zero-extended and sign-extended."""
    lo = v & M32
    return lo, lo - (1 << 32) if lo >> 31 else lo


# ---- normaliser states and observations ----------------------------------------------------------------------------------

NORM_STATES = ("empty", "count1", "constant", "pool")
CLIPS = (5.0, 0.0)
CONSTANT_COL, CONSTANT_VALUE = 0, 0.75      # 50 * 0.75 and 37.5 / 50 are exact: the mean is 0.75 and var_sum 0 to the bit
FAR = 40.0                                  # observations out to 40 sigma


def _spread(d):
    rng = np.random.default_rng(710 + d)
    return rng.normal(0.3, 1.0, d), rng.uniform(0.2, 2.0, d)


@functools.lru_cache(maxsize=None)
def norm_state(kind, d):
    """norm_state [195] for obs_dim d.  empty: all zeros.  count1: one sample (a mean, no scale).  constant: one update of 50
    samples whose column 0 is 0.75 throughout (var_sum exactly 0, count > 1: the divisor is sqrt(1e-4) + 1e-8).  pool: three
    updates, non-trivial statistics everywhere."""
    centre, spread = _spread(d)
    rng = np.random.default_rng(720 + 10 * d + NORM_STATES.index(kind))
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    if kind == "count1":
        on.update(centre + spread * rng.normal(size=(1, d)))
        rn.update(rng.normal(0.0, 2.0, size=(1, 1)))
    elif kind == "constant":
        v = centre + spread * rng.normal(size=(50, d))
        v[:, CONSTANT_COL] = CONSTANT_VALUE
        on.update(v)
        rn.update(rng.normal(0.0, 2.0, size=(50, 1)))
    elif kind == "pool":
        for n in (1, 40, 300):
            on.update(centre + spread * rng.normal(size=(n, d)))
            rn.update(rng.normal(0.0, 2.0, size=(n, 1)))
    else:
        assert kind == "empty"
    s = PM.norm_state_of(on, rn)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def observations(d, B=POOL):
    """float32 [d, B]: 2.5 sigma around the centre the states were fed (a few percent beyond a clip of 5), one entry in 32 set
    to +-40 sigma, and column 0's first robots at the constant column's value, far out, and next to the constant."""
    centre, spread = _spread(d)
    rng = np.random.default_rng(730 + d)
    z = 2.5 * rng.normal(size=(d, B))
    far = rng.random((d, B)) < 1.0 / 32.0
    z[far] = FAR * rng.choice([-1.0, 1.0], size=int(far.sum()))
    obs = (centre[:, None] + spread[:, None] * z).astype(np.float32)
    obs[CONSTANT_COL, 0] = CONSTANT_VALUE              # x = 0 under the constant state
    if B > 1:
        obs[CONSTANT_COL, 1] = centre[CONSTANT_COL] + spread[CONSTANT_COL] * FAR   # the smallest configuration meets the clip too
    if B > 2:
        obs[CONSTANT_COL, 2] = CONSTANT_VALUE + 0.03   # 3 sigma of the floor sqrt(1e-4): inside the clip
    obs.setflags(write=False)
    return obs


def transform_x(kind, clip, d, B):
    """The model's normalised observation of observations(d)[:, :B]: (x float32 [B, d], v float64 [B, d] before the clip,
    scaled [d] bool: the columns that go through the division)."""
    s = norm_state(kind, d)
    on, _ = PM.normalizers_of(s, d, clip)
    v64 = (observations(d)[:, :B].T.astype(np.float64) - on.mean) / on.scale()
    x = on.transform(observations(d)[:, :B].T.astype(np.float64)).astype(np.float32)
    return x, v64, np.full(d, on.count > 1)


@functools.lru_cache(maxsize=None)
def act_case(name, B, kind="count1", clip=5.0):
    """The model over the first B robots of a configuration's pool under norm_state(kind) and obs_clip = clip: obs, state,
    keys, counters, the float64 and float32 models of PM.act (m64, m32), the exact float32 value (value_exact) and the exact
    float32 pre-activation of the mean head (pre_exact)."""
    cfg = config_of(name)
    lay, pp, vp = params(name)
    d = cfg["obs_dim"]
    obs = np.ascontiguousarray(observations(d)[:, :B])
    state = norm_state(kind, d)
    keys, counters = act_states(B)
    m64 = PM.act(obs, state, pp, vp, lay, keys, counters, SEED, obs_clip=clip)
    m32 = PM.act(obs, state, pp, vp, lay, keys, counters, SEED, obs_clip=clip, dtype=np.float32)
    value_exact = PM.forward_exact(m64["x"], PM.split(vp, lay["value"], np.float32), "linear")[:, 0]
    pre_exact = PM.forward_exact(m64["x"], PM.split(pp, lay["policy"], np.float32), "tanh")
    return dict(cfg=cfg, lay=lay, pp=pp, vp=vp, obs=obs, state=state, keys=keys, counters=counters, clip=clip, m64=m64, m32=m32,
                value_exact=value_exact, pre_exact=pre_exact)


# ---- record ---------------------------------------------------------------------------------------------------------

MASK_VALUES = (0, 1, -1, 2 ** 31 - 1, -2 ** 31, 0, 2, 0)     # everything but 0 selects
RECORD = {
    "obs64": dict(obs_dim=64, B=257, ticks=2, seed=741),       # the reward's workspace column and its norm_state column coincide
    "obs1_256": dict(obs_dim=1, B=256, ticks=2, seed=742), "obs1_257": dict(obs_dim=1, B=257, ticks=2, seed=743),
    "obs1_65536": dict(obs_dim=1, B=65536, ticks=2, seed=744), "obs1_65537": dict(obs_dim=1, B=65537, ticks=2, seed=745),   # robot 65536: the second trip of workgroup 0
    "count_2_40": dict(obs_dim=3, B=65, ticks=1, seed=746, count0=2 ** 40),
    "cancel": dict(obs_dim=3, B=257, ticks=1, seed=747, offset=1e4, spread=1e-2, masks=False),   # the real first tick under cancellation
}


def odd_mask(B, shift=0):
    """int32 [B]: MASK_VALUES in turn; the last robot (the one past a workgroup or stride boundary) is selected by -1."""
    m = np.array([MASK_VALUES[(b + shift) % len(MASK_VALUES)] for b in range(min(B, 64))], dtype=np.int64)
    m = np.resize(m, B).astype(np.int32)
    m[B - 1] = -1
    return m


@functools.lru_cache(maxsize=None)
def record_case(name):
    """dict(obs_dim, B, state0 [195], ticks = [(obs [obs_dim, B] f32, reward [B] f32, done [B] i32, mask [B] i32 or None)],
    n = [robots selected per tick], want [195]: the model's state after all ticks, states: after each)."""
    c = RECORD[name]
    d, B = c["obs_dim"], c["B"]
    rng = np.random.default_rng(c["seed"])
    on, rn = PM.Normalizer(d), PM.Normalizer(1, False)
    if "count0" in c:                       # statistics of 2^40 samples of mean ~0.5, variance ~1
        on.count = rn.count = c["count0"]
        on.mean, on.var_sum = 0.5 + 0.1 * np.arange(d), c["count0"] * rng.uniform(0.8, 1.2, d)
        rn.mean, rn.var_sum = np.array([-1.0]), c["count0"] * np.array([9.0])
    state0 = PM.norm_state_of(on, rn)
    centre = c.get("offset", 0.5) + 0.1 * np.arange(d)
    ticks, n, states = [], [], []
    for t in range(c["ticks"]):
        obs = (centre[:, None] + c.get("spread", 1.0) * rng.normal(size=(d, B))).astype(np.float32)
        reward = (c.get("offset", -1.0) + c.get("spread", 3.0) * rng.normal(size=B)).astype(np.float32)
        done = rng.integers(0, 2, B).astype(np.int32)
        mask = odd_mask(B, t) if c.get("masks", True) and t == 0 else None
        sel = np.ones(B, dtype=bool) if mask is None else mask != 0
        on.update(obs.T[sel])
        rn.update(reward[sel].reshape(-1, 1))
        ticks.append((obs, reward, done, mask))
        n.append(int(sel.sum()))
        states.append(PM.norm_state_of(on, rn))
    return dict(obs_dim=d, B=B, state0=state0, ticks=ticks, n=n, want=states[-1], states=states)


def cancel_bounds():
    """The first update from the empty state over values v of mean 1e4 and spread 1e-2, per column (observations, then the
    reward): the exact new var_sum sum(v (v - new_mean)) over the model's float64 new_mean in rational arithmetic, the
    order-independent bounds n 2^-53 sum|(v - mean)(v - new_mean)| on var_sum and n 2^-53 sum|v - mean| / n on the mean
    (mean = 0 before this update), and the model's new mean.  Every sum of n float32 values near 1e4 is exact in float64
    (multiples of 2^-10 below 2^53 of them), so the new mean is one correctly rounded division whatever the order."""
    from fractions import Fraction
    case = record_case("cancel")
    obs, reward, _, _ = case["ticks"][0]
    cols = [obs[i] for i in range(case["obs_dim"])] + [reward]
    want = case["want"].reshape(3, -1)
    idx = list(range(case["obs_dim"])) + [PM.NORM_REWARD]
    out = []
    for col, v in zip(idx, cols):
        v = v.astype(np.float64)
        n, nm = len(v), want[1, col]
        exact = sum(Fraction(float(a)) * (Fraction(float(a)) - Fraction(float(nm))) for a in v)
        exact_mean = sum(Fraction(float(a)) for a in v) / n
        bound_var = n * 2.0 ** -53 * float(np.sum(np.abs(v * (v - nm))))
        bound_mean = n * 2.0 ** -53 * float(np.sum(np.abs(v))) / n
        out.append(dict(col=col, n=n, mean=nm, exact_mean=float(exact_mean), exact_var=float(exact), model_var=want[2, col], bound_var=bound_var,
                        bound_mean=bound_mean))
    return out


# ---- returns ----------------------------------------------------------------------------------------------------------

RETURNS = {
    "t1_count0": dict(B=257, T=1, discount=0.0, lam=0.0, reward_clip=10.0, count=0, bootstrap=True, seed=761),
    "t300_count1_noclip": dict(B=1037, T=300, discount=1.0, lam=0.95, reward_clip=0.0, count=1, bootstrap=True, seed=762),
    "t300_half": dict(B=257, T=300, discount=0.5, lam=0.95, reward_clip=0.0, count=50, bootstrap=True, seed=763),
    "t1_one": dict(B=1037, T=1, discount=1.0, lam=0.0, reward_clip=10.0, count=50, bootstrap=True, seed=764),
    "t300_null_last": dict(B=257, T=300, discount=0.5, lam=0.0, reward_clip=10.0, count=1, bootstrap=False, seed=765),   # last_value NULL
    "t300_zero_discount": dict(B=1037, T=300, discount=0.0, lam=0.95, reward_clip=10.0, count=0, bootstrap=True, seed=766),
}
ALWAYS_DONE, NEVER_DONE = 0, 1             # robots (columns) done at every tick / at none


@functools.lru_cache(maxsize=None)
def returns_case(name):
    """dict of the settings, reward / value float32 [T, B], done int32 [T, B] holding 0, 1, 2 and -1 (column 0 done at every
    tick, column 1 never), last float32 [B], state [195], and the model's ret / adv float64 [T, B]."""
    c = dict(RETURNS[name])
    B, T = c["B"], c["T"]
    rng = np.random.default_rng(c["seed"])
    rn = PM.Normalizer(1, False, c["reward_clip"])
    if c["count"]:
        rn.update(rng.normal(0.0, 2.0, size=(c["count"], 1)))
    state = PM.norm_state_of(PM.Normalizer(1), rn)
    done = (rng.random((T, B)) < 0.05).astype(np.int32)
    done[done != 0] = rng.choice([1, 2, -1], size=int((done != 0).sum()))
    done[:, ALWAYS_DONE] = np.resize([1, 2, -1], T)
    done[:, NEVER_DONE] = 0
    done[T - 1, 2] = 2                      # a done that is not 1 at the last tick: it cuts the bootstrap off
    done[0, 3] = -1
    reward = rng.normal(0.0, 3.0, size=(T, B)).astype(np.float32)
    reward[rng.random((T, B)) < 0.1] = -100.0          # the task's limit reward: beyond a clip of 10
    value = rng.normal(0.0, 2.0, size=(T, B)).astype(np.float32)
    last = rng.normal(0.0, 2.0, size=B).astype(np.float32)
    ret, adv = PM.returns(reward, value, done, last, rn, c["discount"], c["lam"], c["bootstrap"])
    c.update(reward=reward, value=value, done=done, last=last, state=state, rn=rn, ret=ret, adv=adv)
    return c
