"""The cases of tests/test_ddpg_edges_gpu.py, built with the numpy model alone (tests/ddpg_model.py); tests/test_ddpg_edges_cpu.py
asserts what this builder promises.  They go where tests/ddpg_cases.py does not: layer widths at a wave's boundary, the widest
observation, act_dim 1, a hidden layer of one neuron, a deep network beside a head-only one, minibatches of exactly one tile, of
TILE * MAX_GROUPS and one more, and the API's largest; indices outside the ring; settings off their defaults; and a
known-answer probe of the window rule that needs no tolerance.  ddpg_cases derives its seeds from the position of a name in its
CONFIGS, so the configurations here live in their own dict with their own seeds and ddpg_cases stays as it is.

Tolerance of a gradient: the rule of tests/ddpg_cases.py, unchanged (its docstring; relu crossings are redrawn in the same way).
Where M > TILE * MAX_GROUPS a workgroup folds several tiles into its slab: there the float32 model that sums in numpy's order
overstates what float32 costs the kernel, and the yardstick is the float32 model summing in the header's order
(UM.tile_sum): the bound is max(8 x its deviation from float64, 1e-6).  Dropping one tile of 4096 moves a gradient by about
2.4e-4, far above every bound here.

The window probe (probe_walk): obs_dim 1, M = 1, gamma = 1, head-only critic and target critic.  Every observation in the ring
tensors -- the slots no store has written too -- is a small integer code, 1 .. base - 1.
  s1: the target critic's weights are 0 on the action rows and base^f on window element f, the online critic is zero and every
      reward is 0.  Q' is then an integer below 2^24, which the float32 fma chain forms exactly; y = nd Q', Q = 0, the critic's
      bias gradient is exactly -y and spells out s1 digit by digit (0 where done is set), and the loss is exactly 0.5 y^2.
  s0: both critics are zero and the probed transition's reward alone is -1: delta = 1 and the first layer's weight gradient is
      [action, s0] byte for byte, the bias gradient 1 and the loss 0.5."""
import functools
import math

import numpy as np

from tests import ddpg_cases as DC
from tests import ddpg_model as DM

TILE, MAX_GROUPS = DC.TILE, 256
FULL = TILE * MAX_GROUPS            # 4096: every workgroup walks one tile
MAX_MINIBATCH = 1 << 16
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
CONFIGS = {
    "head_only": dict(obs_dim=1, act_dim=1, window=1, actor_layers=(), critic_layers=()),
    "wave_edges": dict(obs_dim=63, act_dim=4, window=2, actor_layers=(63, 64, 65), critic_layers=(255, 256, 1)),      # the critic reads 130
    "obs64": dict(obs_dim=64, act_dim=1, window=2, actor_layers=(17,), critic_layers=(33,)),                            # 128 inputs, the critic 129
    "long_window": dict(obs_dim=1, act_dim=2, window=8, actor_layers=(9, 65, 3), critic_layers=()),
    "critic_deeper": dict(obs_dim=7, act_dim=2, window=3, actor_layers=(), critic_layers=(64, 63, 255)),
}
SEEDS = {"head_only": 9101, "wave_edges": 9102, "obs64": 9103, "long_window": 9104, "critic_deeper": 9105, "lopsided": 9106, "default": 9107,
         "limits": 9108}
# (configuration, B, capacity, ticks stored, M); "long_window" on capacity 2 has a window four times its ring; the last is the
# API's largest minibatch on the smallest networks of ddpg_cases
CASES = [("head_only", 1, 2, 2, 1), ("head_only", 17, 4, 3, 15), ("head_only", 16, 7, 9, FULL),
         ("wave_edges", 15, 4, 6, 17), ("wave_edges", 3, 7, 5, 100),
         ("obs64", 16, 7, 9, 16), ("obs64", 1, 4, 3, 100),
         ("long_window", 17, 2, 5, 15), ("long_window", 67, 7, 9, FULL + 1),
         ("critic_deeper", 15, 7, 10, 16), ("critic_deeper", 67, 4, 4, 1),
         ("lopsided", 67, 7, 9, MAX_MINIBATCH)]
ACT_CASES = [("head_only", 1, 2, 2, 1), ("head_only", 17, 4, 3, 15), ("wave_edges", 15, 4, 6, 17), ("obs64", 16, 7, 9, 16),
             ("long_window", 17, 2, 5, 15), ("long_window", 67, 7, 9, FULL + 1), ("critic_deeper", 15, 7, 10, 16)]
GAMMAS = (0.0, 0.5, 1.0)
GAMMA_CASE = ("critic_deeper", 15, 7, 10, 16)
SPOILT_CASE = ("wave_edges", 3, 7, 5, 100)


@functools.lru_cache(maxsize=None)
def net(name):
    """(cfg, layout, {net: float32 params}) as ddpg_cases.net draws them, from this module's seeds; a configuration of
    ddpg_cases is ddpg_cases's own."""
    if name in DC.CONFIGS:
        return DC.net(name)
    cfg = CONFIGS[name]
    rng = np.random.default_rng(SEEDS[name])
    lay = DM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["window"], cfg["actor_layers"], cfg["critic_layers"])
    params = {}
    for which in DC.NETS:
        kind = which.replace("target_", "")
        p = np.zeros(lay[kind + "_count"], dtype=np.float32)
        for i, o, w, b in lay[kind]:
            limit = math.sqrt(6.0 / (i + o))
            p[w:w + i * o] = rng.uniform(-limit, limit, i * o)
            p[b:b + o] = rng.normal(0.2, 0.1, o)
        params[which] = p
    return cfg, lay, params


def fill_ring(name, B, C, ticks, seed):
    """ddpg_cases.fill_ring for a configuration of either module."""
    cfg, _, _ = net(name)
    d, A = cfg["obs_dim"], cfg["act_dim"]
    rng = np.random.default_rng(seed)
    ring = DM.Ring(C, B, d, A)
    for t in range(ticks):
        done = rng.choice(np.array([0, 0, 0, 0, 1, -1, 2 ** 31 - 1], dtype=np.int64), size=B).astype(np.int32)
        if t == ticks - 3 and ticks >= 4:
            done[0] = 1
        ring.store(DC._draw_obs(rng, d, B).T, rng.uniform(-1, 1, size=(B, A)).astype(np.float32), rng.normal(0.5, 1.0, B).astype(np.float32), done)
    return ring, rng


def groups(M):
    return min(-(-M // TILE), MAX_GROUPS)


@functools.lru_cache(maxsize=None)
def case(name, B, C, ticks, M, gamma=DC.GAMMA):
    """ddpg_cases.case with gamma as a setting and, where M > TILE * MAX_GROUPS, the tile-ordered float32 model as the yardstick
    (`tiled`; dev32 is then that model's deviation and dev32_plain numpy's order)."""
    cfg, lay, params = net(name)
    W, d = cfg["window"], cfg["obs_dim"]
    ring, rng = fill_ring(name, B, C, ticks, SEEDS[name] * 1000 + 100 * M + 10 * B + C)
    idx = DC.given_indices(ring, M)
    margins, redraws = None, 0
    for _ in range(50):                                   # keep every differentiated hidden pre-activation away from 0 (ddpg_cases)
        pres = {}
        for dtype in (np.float64, np.float32):
            pc, pa, pq = [], [], []
            DM.critic_grad(ring, idx, params["critic"], params["target_actor"], params["target_critic"], lay, W, gamma, dtype, pre=pc)
            DM.actor_grad(ring, idx, params["actor"], params["critic"], lay, W, dtype, pre_actor=pa, pre_critic=pq)
            pres[dtype] = pc[:-1] + pa[:-1] + pq[:-1]
        if margins is None:
            margins = [8.0 * float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pres[np.float32], pres[np.float64])]
        near = np.zeros(M, dtype=bool)
        for y, m_ in zip(pres[np.float64], margins):
            near |= (np.abs(y) <= m_).any(axis=1)
        if not near.any():
            break
        cells = sorted({(ring.slot(int(a) + k), int(b)) for a, b in idx[near] for k in range(min(W, ring.count - int(a)))})
        for s, b in cells:
            ring.obs[s, :, b] = DC._draw_obs(rng, d, 1)[0]
        redraws += len(cells)
    assert not near.any()
    tiled = M > FULL
    c = dict(name=name, B=B, C=C, ticks=ticks, M=M, gamma=gamma, cfg=cfg, lay=lay, params=params, ring=ring, idx=idx, tiled=tiled,
             redrawn=redraws / (ring.count * B))
    small = M <= TILE + 1
    runs = dict(critic=lambda **kw: DM.critic_grad(ring, idx, params["critic"], params["target_actor"], params["target_critic"], lay, W, gamma, **kw),
                actor=lambda **kw: DM.actor_grad(ring, idx, params["actor"], params["critic"], lay, W, **kw))
    rel = lambda a, b: abs(a - b) / abs(b) if b != 0 else abs(a)
    for which, shift in (("critic", "q_shift"), ("actor", "mu_shift")):
        g64, g32 = runs[which](), runs[which](dtype=np.float32)
        names = DM.tensors(lay[which])
        plain = DC.deviation(g32["grad"], g64["grad"], names)
        if tiled:
            g32 = runs[which](dtype=np.float32, tiles=(TILE, MAX_GROUPS))
        dev32 = DC.deviation(g32["grad"], g64["grad"], names)
        if small:
            shifted = [runs[which](**{shift: s}) for s in (DC.FLOOR, -DC.FLOOR)]
            forward = [DC.deviation(s["grad"], g64["grad"], names) for s in shifted]
            mag, g = g64["mag"], g64["grad"]
            floor = {k: DC.FLOOR * (float(mag[s].max()) / float(np.abs(g[s]).max()) if np.abs(g[s]).max() > 0 else 0.0) + max(f[k] for f in forward)
                     for k, s in names.items()}
            loss_floor = DC.FLOOR + max(rel(s["loss"], g64["loss"]) for s in shifted)
        else:
            floor, loss_floor = dict.fromkeys(names, DC.PROJECT_FLOOR), DC.PROJECT_FLOOR
        c[which] = dict(m64=g64, m32=g32, names=names, dev32=dev32, dev32_plain=plain, floor=floor,
                        tol={k: max(8.0 * dev32[k], floor[k]) for k in names},
                        loss_dev32=rel(g32["loss"], g64["loss"]), loss_tol=max(8.0 * rel(g32["loss"], g64["loss"]), loss_floor))
    return c


# ---- indices outside the ring --------------------------------------------------------------------------------------------

def spoil(c, kind):
    """(idx int32 [M, 2], live bool [M]) from the indices of a case: `some` replaces single entries, and the whole of tile 2,
    by every kind of index that rg_ddpg.h says contributes exact zeros; `all` leaves no valid entry."""
    idx, count, B = c["idx"].copy(), c["ring"].count, c["B"]
    M = len(idx)
    a, b = int(idx[0, 0]), int(idx[0, 1])
    bad = [(0, b), (count, b), (-1, b), (INT_MIN, b), (a, B), (a, -1), (a, INT_MAX)]
    live = np.ones(M, dtype=bool)
    if kind == "some":
        assert M >= 3 * TILE + len(bad)
        where = [3, 5, 7, 11, 13, TILE + 4, 3 * TILE + 1] + list(range(2 * TILE, 3 * TILE))
    else:
        where = list(range(M))
    for n, m in enumerate(where):
        idx[m] = bad[n % len(bad)]
        live[m] = False
    return idx, live


def spoilt_model(c, kind):
    """{critic, actor: the float64 model with the spoilt samples contributing nothing while M stays M}, idx and live."""
    idx, live = spoil(c, kind)
    ring, lay, p, W = c["ring"], c["lay"], c["params"], c["cfg"]["window"]
    return dict(idx=idx, live=live,
                critic=DM.critic_grad(ring, idx, p["critic"], p["target_actor"], p["target_critic"], lay, W, c["gamma"], live=live),
                actor=DM.actor_grad(ring, idx, p["actor"], p["critic"], lay, W, live=live))


# ---- the window probe -----------------------------------------------------------------------------------------------------

PROBE_ACT = 2
# (window, base of the codes): 16^5 and 4^8 stay below 2^24
PROBE_WINDOWS = ((1, 16), (3, 16), (5, 16), (8, 4))
# name: (B, capacity, ticks stored, {(tick, robot): done}).  "unwrapped" has slots no store has written; "long" holds a whole
# window of 8.  The dones lie so that walking every (age, robot) puts one at the probed age, at age - 1, inside the window and
# just outside it, for every window here
PROBE_RINGS = {
    "two": (2, 2, 2, {(0, 1): 1}),
    "two_wrapped": (2, 2, 5, {(4, 0): -1, (3, 1): INT_MAX}),
    "seven_wrapped": (3, 7, 9, {(5, 1): -1, (7, 2): 1, (3, 2): INT_MAX}),
    "unwrapped": (3, 7, 4, {(1, 1): INT_MAX, (3, 2): -1}),
    "long": (3, 12, 15, {(9, 1): 1, (13, 2): -1, (5, 2): 1}),
}


def _code(t, b, base):
    return 1 + (t + 5 * b) % (base - 1)


def probe_ring(name, base):
    """The ring `name` with coded observations: tick t of robot b holds code 1 + (t + 5 b) mod (base - 1), distinct from tick to
    tick and robot to robot as far as base - 1 codes allow.  A slot no store has written holds a code too and no done, so that a read past
    `count` shows up as a digit.  Actions are distinct negative dyadic numbers."""
    B, C, ticks, dones = PROBE_RINGS[name]
    ring = DM.Ring(C, B, 1, PROBE_ACT)
    for s in range(C):                                   # what no store writes: codes, not zeros
        for b in range(B):
            ring.obs[s, 0, b] = _code(s + 3, b, base)
        ring.action[s] = -99.0
    for t in range(ticks):
        obs = np.array([[_code(t, b, base) for b in range(B)]], dtype=np.float32)
        action = np.array([[-(t + 1) - 0.25 * b - 0.125 * k for k in range(PROBE_ACT)] for b in range(B)], dtype=np.float32)
        done = np.array([dones.get((t, b), 0) for b in range(B)], dtype=np.int32)
        ring.store(obs, action, np.zeros(B, dtype=np.float32), done)
    return ring


def probe_walk(name, window, base):
    """Every (age, robot) of the ring: dict(age, robot, slot, s0, s1 (float32 [window], oldest first, DM.Ring.state's), done,
    kept0, kept1, cut0, cut1, y: the integer the s1 probe spells, action)."""
    ring = probe_ring(name, base)
    out = []
    for a in range(1, ring.count):
        for b in range(ring.B):
            s0, s1 = ring.state(a, b, window), ring.state(a - 1, b, window)
            done = int(ring.done[ring.slot(a), b])
            k0, k1 = ring.kept(a, b, window), ring.kept(a - 1, b, window)
            assert np.count_nonzero(s0) == k0 and np.count_nonzero(s1) == k1          # a code is never 0: the digits show what is kept
            y = 0 if done != 0 else int(sum(int(v) * base ** f for f, v in enumerate(s1)))
            out.append(dict(age=a, robot=b, slot=ring.slot(a), s0=s0, s1=s1, done=done, kept0=k0, kept1=k1, y=y,
                            cut0=_cut(ring, a, b, window, k0), cut1=_cut(ring, a - 1, b, window, k1), crosses0=_crosses(ring, a, k0),
                            action=ring.action[ring.slot(a), b].copy()))
    return ring, out


def _cut(ring, a, b, window, kept):
    """Why the window of the state ending at age a stops short: None (it does not), "done", "count" (the ring has not wrapped: the
    next slot was never written) or "wrap" (the ring has wrapped: the next slot back is the newest tick's)."""
    if kept == window:
        return None
    if a + kept >= ring.count:
        return "wrap" if ring.count == ring.C else "count"
    return "done"


def _crosses(ring, a, kept):
    """The kept elements run from slot 0 back to slot C - 1."""
    slots = [ring.slot(a + k) for k in range(kept)]
    return any(s == 0 and t == ring.C - 1 for s, t in zip(slots, slots[1:]))


def probe_weights(window, base):
    """The target critic of the s1 probe: float32 [PROBE_ACT + window + 1], 0 on the action rows, base^f on element f, bias 0."""
    p = np.zeros(PROBE_ACT + window + 1, dtype=np.float32)
    p[PROBE_ACT:PROBE_ACT + window] = [float(base ** f) for f in range(window)]
    return p


# ---- settings -------------------------------------------------------------------------------------------------------------

# Ornstein-Uhlenbeck settings off the defaults (0.5, 0.4, 0.3, 1e-2), one at a time and all four together
OU_SETTINGS = {
    "theta0": dict(ou_theta=0.0),
    "mu": dict(ou_mu=-0.7),
    "sigma0": dict(ou_sigma=0.0),
    "dt": dict(ou_dt=0.25),
    "all": dict(ou_theta=1.25, ou_mu=-0.7, ou_sigma=0.9, ou_dt=0.25),
}
# keys (row 0 of act_state) that are negative or above 2^40, and a counter of 2^40, beside small ones
OU_KEYS = (-1, INT_MIN, -2 ** 63, 2 ** 40 + 3, 2 ** 63 - 1, 5)
OU_COUNTERS = (2 ** 40, 0, 7, 2 ** 40, 2 ** 32, 2 ** 40)
ADAM_SETTINGS = {"beta1_0": dict(beta1=0.0), "beta2_0": dict(beta2=0.0), "eps_1e-3": dict(adam_eps=1e-3)}
# the sample stream: the largest seeds, update counts past 2^31, count - 1 = 7 and B = 67 coprime and no powers of two
SAMPLE_SEED = 2 ** 64 - 3
SAMPLE_UPDATES = (2 ** 31, 2 ** 40)
SAMPLE_SHAPE = dict(B=67, C=8, count=8, M=100)
