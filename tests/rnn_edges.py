"""The cases of tests/test_rnn_edges_gpu.py, built from the numpy models alone (tests/rnn_model.py, tests/bptt_model.py,
tests/policy_model.py) and tests/bptt_cases.py; tests/test_rnn_edges_cpu.py builds every one of them without a GPU, holds it to
the caps of tests/bptt_cases.py and asserts on the model what the case is about.  Nothing here comes from a kernel's output.

They go where tests/test_rnn_gpu.py and tests/test_bptt_gpu.py do not.  Acting (rg_rnn_act, rg_rnn_unroll): the batches at
which a tile of 8 robots is empty but for one, one short, full and one over; sequences of 33 and 257 ticks; saturated gates,
whose answers are known to the bit (u == 1 holds the state, r == u == 0 forgets it); a dead first layer; flag values that a
byte-wide or a sign test would misread; non-finite inputs; obs_clip 0 and 0.5; keys, counters and a seed beyond 32 bits.  The
update (rg_bptt.h): configurations at a wave's edge and at the row tile's edge of the weight kernel (bptt_cases.EDGE_CONFIGS),
batches of whole tiles and T * B of whole chunks, saturated gates in the backward pass, the same flag values.

Tolerances.  No new one: acting keeps the rule of tests/test_rnn_gpu.py (8 x the float32-numpy model's deviation from the float64
model over the case's own inputs and all its ticks, floor 1e-6), gradients keep the rule of tests/bptt_cases.py through
bptt_cases.case.  The caps are bptt_cases's; every acting bound is held to TOL_CAP too.

Relu of a NaN.  The kernels' relu is v > 0 ? v : 0 (rg_bptt.h, F), which sends a NaN to 0: a robot whose observation holds a
NaN leaves the dense layers with zeros, and so finite.  The models form relu the same way."""
import functools
import math

import numpy as np

from robot_gym_amd.core import bptt_abi
from tests import bptt_cases as BC
from tests import bptt_model as BM
from tests import policy_model as PM
from tests import rnn_model as RM

TILE, CHUNK = bptt_abi.TILE, BC.CHUNK
REDRAW_CAP, TOL_CAP, ULP_CAP = BC.REDRAW_CAP, BC.TOL_CAP, BC.ULP_CAP
FLOOR = 1e-6
SEED = 11
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
FLAGS = (256, 65536, INT_MIN, -1, INT_MAX)          # each is "set": a test of the low byte misreads the first two, a test of > 0 the next two

# ---- the acting configurations ------------------------------------------------------------------------------------------

ACT_CONFIGS = {
    "default": BC.CONFIGS["default"],
    "lopsided": BC.CONFIGS["lopsided"],
    "limits": BC.CONFIGS["limits"],
    "h65": dict(obs_dim=16, act_dim=2, policy_layers=(65,), gru_units=65, value_layers=(65,)),      # 2H = 130 gates: three waves; a dense layer of 65
}
ACT_SEEDS = {"default": 7301, "lopsided": 7302, "limits": 7303, "h65": 7304}


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def act_net(name):
    """dict(name, cfg, lay, pp, vp, state, centre, spread) of an acting configuration: weights within the Glorot limit, non-zero
    biases, the gates' biases spread between shut and open, a distinct logstd per component, a normaliser state with
    non-trivial statistics.  The arrays are read-only."""
    cfg = ACT_CONFIGS[name]
    rng = np.random.default_rng(ACT_SEEDS[name])
    lay = RM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["gru_units"], cfg["value_layers"])
    H = cfg["gru_units"]
    pp = np.zeros(lay["policy_count"], dtype=np.float32)
    for i, o, w, b in RM.blocks(lay):
        limit = math.sqrt(6.0 / (i + o))
        pp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        pp[b:b + o] = rng.normal(0.0, 0.1, o)
    b_ru = lay["w_ru"][3]
    pp[b_ru:b_ru + 2 * H] = rng.normal(0.0, 1.5, 2 * H)
    pp[lay["logstd_offset"]:] = -1.0 + 0.2 * np.arange(cfg["act_dim"]) + rng.normal(0.0, 0.05, cfg["act_dim"])
    vp = np.zeros(lay["value_count"], dtype=np.float32)
    for i, o, w, b in lay["value"]:
        limit = math.sqrt(6.0 / (i + o))
        vp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        vp[b:b + o] = rng.normal(0.0, 0.1, o)
    d = cfg["obs_dim"]
    centre, spread = rng.normal(0.3, 1.0, d), rng.uniform(0.2, 2.0, d)
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    for n in (1, 40, 300):
        on.update(centre + spread * rng.normal(size=(n, d)))
        rn.update(rng.normal(0.0, 2.0, size=(n, 1)))
    return dict(name=name, cfg=cfg, lay=lay, pp=_frozen(pp), vp=_frozen(vp), state=_frozen(PM.norm_state_of(on, rn)), centre=centre, spread=spread)


def dead_first_layer(pp, lay):
    """A copy of the policy buffer whose first dense layer has zero weights and negative biases: its output is exactly 0 for
    every finite observation."""
    i, o, w, b = lay["dense"][0]
    out = np.array(pp)
    out[w:w + i * o] = 0.0
    out[b:b + o] = -0.5 - np.abs(out[b:b + o])
    return out


@functools.lru_cache(maxsize=None)
def draw(name, T, B, seed, sigma=2.5):
    """dict(obs [T, obs_dim, B] out to a few `sigma`, hidden [B, H] in (-1, 1), keys, counters [B]), read-only, from `seed`."""
    n = act_net(name)
    d, H = n["cfg"]["obs_dim"], n["cfg"]["gru_units"]
    rng = np.random.default_rng(seed)
    obs = (n["centre"][None, :, None] + n["spread"][None, :, None] * rng.normal(size=(T, d, B)) * sigma).astype(np.float32)
    hidden = rng.uniform(-0.95, 0.95, size=(B, H)).astype(np.float32)
    keys = 1000 + 3 * np.arange(B, dtype=np.int64)
    counters = (np.arange(B, dtype=np.int64) * 7) % 5
    return dict(obs=_frozen(obs), hidden=_frozen(hidden), keys=_frozen(keys), counters=_frozen(counters))


def resets(T, B, flag=1):
    """reset int32 [T, B]: episodes that begin at tick 0, at a middle tick and at the last tick, each marked with `flag`; with one
    robot it is reset at the middle tick alone."""
    reset = np.zeros((T, B), dtype=np.int64)
    b = np.arange(B)
    reset[0, b % 3 == 0] = flag
    reset[T // 2, b % 5 == 1] = flag
    reset[T - 1, b % 7 == 2] = flag
    if B == 1:
        reset[:] = 0
        reset[T // 2, 0] = flag
    return reset.astype(np.int32)


# ---- the rule of tests/test_rnn_gpu.py --------------------------------------------------------------------------------------

def _dev(a32, a64):
    """max |a32 - a64| over the entries that are finite in the float64 model; the models must agree on which are not."""
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64)
    fin = np.isfinite(a64)
    assert np.array_equal(np.isfinite(a32), fin)
    return float(np.abs(a32[fin] - a64[fin]).max()) if fin.any() else 0.0


def act_rule(n, obs, hidden, reset, keys, counters, pp=None, seed=SEED, clip=5.0, sample=True):
    """rg_rnn_act's answers for one tick from the float64 model, the float32 model's deviation per output and the bound
    max(8 x deviation, 1e-6): dict(m64, dev, tol)."""
    pp = n["pp"] if pp is None else pp
    args = (obs, n["state"], pp, n["vp"], n["lay"], keys, counters, seed, hidden, reset)
    with np.errstate(invalid="ignore"):
        m64 = RM.act(*args, sample=sample, obs_clip=clip)
        m32 = RM.act(*args, sample=sample, obs_clip=clip, dtype=np.float32)
    dev = {k: _dev(m32[k], m64[k]) for k in ("mean", "value", "hidden")}
    return dict(m64=m64, m32=m32, dev=dev, tol={k: max(8.0 * v, FLOOR) for k, v in dev.items()})


def unroll_rule(n, obs, reset, h0, pp=None, clip=5.0):
    """rg_rnn_unroll's answers from the float64 model with the bound over all ticks, the state carried in each precision:
    dict(mean, hidden_seq, dev, tol)."""
    pp = n["pp"] if pp is None else pp
    m64, h64 = RM.unroll(obs, reset, h0, n["state"], pp, n["lay"], obs_clip=clip)
    m32, h32 = RM.unroll(obs, reset, h0, n["state"], pp, n["lay"], obs_clip=clip, dtype=np.float32)
    dev = dict(mean=_dev(m32, m64), hidden=_dev(h32, h64))
    return dict(mean=m64, hidden_seq=h64, mean32=m32, hidden32=h32, dev=dev, tol={k: max(8.0 * v, FLOOR) for k, v in dev.items()})


def carried(h0, reset):
    """[T, B, H]: the state a cell that holds it (u == 1) leaves after every tick: h0 through the resets, float32."""
    h = np.array(h0, dtype=np.float32)
    out = []
    for r in np.asarray(reset):
        h = np.where(r[:, None] != 0, np.float32(0), h)
        out.append(h)
    return np.stack(out)


# ---- A. memory and shapes ---------------------------------------------------------------------------------------------------

GUARD_BATCHES = (1, TILE - 1, TILE + 1, 257)
GUARD_T = (1, 3)
GUARD_CONFIGS = ("lopsided", "limits")
CHAIN_BATCHES = (1, TILE - 1, TILE)
CHAIN_T = (1, 2, 33)
STREAM_BATCHES = (TILE + 1, 257)
LONG_T, LONG_B = 257, TILE + 1
LONG_CONFIGS = ("lopsided", "h65")


@functools.lru_cache(maxsize=None)
def long_case(name):
    """T = 257 ticks of 9 robots with resets at tick 0, tick 128 and tick 256, and the model's answers with their bounds."""
    n = act_net(name)
    r = draw(name, LONG_T, LONG_B, 8100 + ACT_SEEDS[name])
    reset = resets(LONG_T, LONG_B)
    assert reset[0].any() and reset[LONG_T // 2].any() and reset[LONG_T - 1].any()
    return dict(n=n, obs=r["obs"], h0=r["hidden"], reset=reset, rule=unroll_rule(n, r["obs"], reset, r["hidden"]))


# ---- B. exact known answers -----------------------------------------------------------------------------------------------------

KNOWN_B = TILE + 5                   # a full tile and a ragged one
KNOWN_T = 4
KNOWN_CONFIGS = ("default", "h65")


@functools.lru_cache(maxsize=None)
def known_case(name, kind):
    """B = 13 robots, T = 4 ticks on parameters changed by `kind`: "hold" and "shut" (bptt_cases.saturate), "dead"
    (dead_first_layer), "plain" (unchanged).  dict(n, pp, obs [T, d, B], other_obs, hidden, other_hidden, reset [T, B], keys,
    counters, act: act_rule of tick 0, unroll: unroll_rule of the T ticks)."""
    n = act_net(name)
    lay = n["lay"]
    pp = dict(hold=lambda: BC.saturate(n["pp"], lay, "hold"), shut=lambda: BC.saturate(n["pp"], lay, "shut"), dead=lambda: dead_first_layer(n["pp"], lay),
              plain=lambda: n["pp"])[kind]()
    a, b = draw(name, KNOWN_T, KNOWN_B, 8200 + ACT_SEEDS[name]), draw(name, KNOWN_T, KNOWN_B, 8300 + ACT_SEEDS[name])
    reset = resets(KNOWN_T, KNOWN_B)
    assert 0 < (reset[0] != 0).sum() < KNOWN_B and (reset[0, :TILE] != 0).any() and (reset[0, TILE:] != 0).any()
    return dict(n=n, pp=pp, obs=a["obs"], other_obs=b["obs"], hidden=a["hidden"], other_hidden=b["hidden"], reset=reset, keys=a["keys"], counters=a["counters"],
                act=act_rule(n, a["obs"][0], a["hidden"], reset[0], a["keys"], a["counters"], pp=pp, sample=False),
                unroll=unroll_rule(n, a["obs"], reset, a["hidden"], pp=pp))


NAN_OBS_ROBOT, INF_OBS_ROBOT, NAN_HIDDEN_ROBOT = 2, 5, TILE + 3      # two in the full tile, one in the ragged one
SPOILT = (NAN_OBS_ROBOT, INF_OBS_ROBOT, NAN_HIDDEN_ROBOT)


@functools.lru_cache(maxsize=None)
def nonfinite_case(name):
    """One tick of 13 robots: robot 2 has a NaN observation component, robot 5 a +inf one (the normaliser clips it), robot 11 a
    NaN hidden row; no robot is reset.  dict(n, obs, clean_obs, hidden, clean_hidden, keys, counters, rule: act_rule of the
    spoilt inputs, clean: act_rule of the clean ones)."""
    n = act_net(name)
    r = draw(name, 1, KNOWN_B, 8400 + ACT_SEEDS[name])
    obs, hidden = np.array(r["obs"][0]), np.array(r["hidden"])
    obs[1 % obs.shape[0], NAN_OBS_ROBOT] = np.nan
    obs[0, INF_OBS_ROBOT] = np.inf
    hidden[NAN_HIDDEN_ROBOT] = np.nan
    reset = np.zeros(KNOWN_B, dtype=np.int32)
    return dict(n=n, obs=obs, clean_obs=r["obs"][0], hidden=hidden, clean_hidden=r["hidden"], reset=reset, keys=r["keys"], counters=r["counters"],
                rule=act_rule(n, obs, hidden, reset, r["keys"], r["counters"]), clean=act_rule(n, r["obs"][0], r["hidden"], reset, r["keys"], r["counters"]))


CLIPS = (0.0, 0.5)


@functools.lru_cache(maxsize=None)
def clip_case(name, clip):
    """One tick of 13 robots under obs_clip = clip; without clipping the observations reach out to 20 sigma."""
    n = act_net(name)
    r = draw(name, 1, KNOWN_B, 8500 + ACT_SEEDS[name], sigma=20.0 if clip == 0.0 else 2.5)
    reset = resets(1, KNOWN_B)[0]
    return dict(n=n, obs=r["obs"][0], hidden=r["hidden"], reset=reset, keys=r["keys"], counters=r["counters"],
                rule=act_rule(n, r["obs"][0], r["hidden"], reset, r["keys"], r["counters"], clip=clip, sample=False))


WIDE_SEED = 2 ** 63 + 0x1234567
WIDE_KEYS = (-1, -2 ** 63, 2 ** 40, 2 ** 40 + 5, 2 ** 62 + 3, -2 ** 40 - 7, 2 ** 32, 2 ** 32 + 1, 5, 2 ** 63 - 1, -2, 2 ** 48, 7)
WIDE_COUNTERS = (2 ** 32 - 1, 2 ** 32, 2 ** 63 - 2, 0, 2 ** 32 - 1, 2 ** 40, 2 ** 63 - 2, 1, 2 ** 32, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 33)
assert len(WIDE_KEYS) == len(WIDE_COUNTERS) == KNOWN_B


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """One sampling tick of 13 robots with negative keys, keys of 2^40 and more, counters 2^32 - 1, 2^32 and 2^63 - 2 and a seed
    above 2^63.  rule["m64"]["eps"] is PM.eps_batch's draw."""
    n = act_net(name)
    r = draw(name, 1, KNOWN_B, 8600 + ACT_SEEDS[name])
    keys, counters = np.array(WIDE_KEYS, dtype=np.int64), np.array(WIDE_COUNTERS, dtype=np.int64)
    reset = resets(1, KNOWN_B)[0]
    return dict(n=n, obs=r["obs"][0], hidden=r["hidden"], reset=reset, keys=keys, counters=counters,
                rule=act_rule(n, r["obs"][0], r["hidden"], reset, keys, counters, seed=WIDE_SEED))


# ---- C. the update ------------------------------------------------------------------------------------------------------------

EDGE_SHAPES = [(1, 1), (2, 9), (5, 37)]
EDGE_CASES = [(name, T, B) for name in BC.EDGE_CONFIGS for T, B in EDGE_SHAPES]
# no mirrored slot; T * B one chunk; one robot through 16 ticks; whole chunks of whole tiles; three full tiles
FULL_SHAPES = [(2, 8), (1, 16), (16, 1), (4, 16), (3, 24)]
FULL_CASES = [(name, T, B) for name in ("default", "two dense") for T, B in FULL_SHAPES]
assert any(B % TILE == 0 for _, B in FULL_SHAPES) and any(T * B == CHUNK for T, B in FULL_SHAPES)
assert any(T * B % CHUNK == 0 and T * B > CHUNK for T, B in FULL_SHAPES) and (16, 1) in FULL_SHAPES
# bptt_cases masks the last robot of every batch throughout, so what the delta pass leaves of it is all zeros and a workspace
# of zeros hides a last robot that was never visited: these run with mask "last" (the last robot valid at every tick, the
# first one masked), at full tiles, where no slot mirrors it, and at ragged ones, where the slots past the batch do
LAST_LIVE_CASES = [(name, T, B) for name, T, B in FULL_CASES if B % TILE == 0] + [("default", 2, 9), ("two dense", 5, 37), ("rows15", 2, 9)]
SATURATED_CASES = [(name, 5, 37) for name in ("default", "wave65")]
FLAG_CASE = ("rows15", 5, 37)
WORKSPACE_CASES = [("rows15", 2, 9), ("default", 4, 16)]
# tensors whose float64 gradient is about 1e-43 of the rest with both gates shut, where the kernel's is exactly 0: they are held
# to zero, not to a relative bound
SHUT_ZERO = ("W_ru", "b_ru")


def flagged(a, flag):
    """int32 array `a` with every 1 replaced by `flag`."""
    a = np.asarray(a)
    return np.where(a == 1, np.int32(flag), a).astype(np.int32)


def gate_tensors(lay):
    """The names of BM.tensors(lay) that a cell holding its state (u == 1) passes no gradient to: everything below the head."""
    return [k for k in BM.tensors(lay) if k not in ("W_head", "b_head", "logstd")]
