"""The cases of tests/test_ddpg_gpu.py, built with the numpy model alone (tests/ddpg_model.py): networks, a filled replay ring,
given minibatch indices, the float64 model's answers and the float32 model's deviations (the yardstick of a tolerance).
tests/test_ddpg_cpu.py builds every case too and asserts what the builder promises, so that is checked without a GPU.

Tolerance of a gradient: the rule of tests/test_ppo_update_gpu.py.  Per parameter tensor (each W, each b) the deviation is
max|g - g64| / max|g64| against the float64 model; the bound is max(8 x the float32 numpy model's deviation, 1e-6), formed from
the model alone.  Where M <= TILE + 1 the float32 model's deviation is one draw of a handful of rounding errors, not a measure;
there, and only there, the floor is instead 2^-22 of the largest sum of |terms| of the tensor's entries over its largest entry
plus what a forward pass off by 2^-22 (Q for the critic, the mean for the actor) does to the tensor in the float64 model.

Relu crossings: the ring's observations are drawn so that no hidden pre-activation of the float64 model -- of the critic on
[action, s0], of the actor on s0, of the critic on [mu, s0]: the passes that are differentiated -- lies within 8 x the largest
deviation of numpy's float32 pre-activations of that layer.  The observations of a sample that does are drawn again;
`redrawn` is their share of all the ring's observations, at most one in four (asserted by test_ddpg_cpu.py)."""
import functools
import math

import numpy as np

from tests import ddpg_model as DM

TILE = 16
FLOOR = 2.0 ** -22
PROJECT_FLOOR = 1e-6
CONFIGS = {
    "default": dict(obs_dim=16, act_dim=2, window=5, actor_layers=(128, 128, 64), critic_layers=(256, 256, 128)),
    "lopsided": dict(obs_dim=6, act_dim=3, window=3, actor_layers=(5,), critic_layers=(7, 3, 2)),
    "limits": dict(obs_dim=16, act_dim=4, window=8, actor_layers=(256, 256, 256), critic_layers=(256, 256, 256)),
    "flat": dict(obs_dim=16, act_dim=2, window=1, actor_layers=(), critic_layers=()),
}
BIG = 16 * 256 + 16 + 3       # one more tile than the 256 workgroups walk once, plus a ragged tail
# (configuration, B, capacity, ticks stored, M): B in {1, 3, 67}, capacity in {2, 4, 7}, wrapped (ticks > capacity) and not,
# M in {1, 5, 17, 100, BIG}; "limits" has a window longer than its ring
CASES = [("default", 3, 7, 5, 17), ("default", 67, 4, 6, 100), ("default", 1, 7, 9, 100),
         ("lopsided", 1, 2, 2, 1), ("lopsided", 3, 4, 6, 5), ("lopsided", 67, 7, 6, BIG),
         ("limits", 3, 7, 10, 17), ("limits", 67, 4, 3, 100),
         ("flat", 1, 2, 3, 1), ("flat", 3, 4, 4, 5), ("flat", 67, 7, 7, 100)]
NETS = ("actor", "critic", "target_actor", "target_critic")
GAMMA = 0.99


@functools.lru_cache(maxsize=None)
def net(name):
    """(cfg, layout, {net: float32 params}): weights uniform within the Glorot limit, biases around 0.2 (so that the
    narrow layers of "lopsided" keep live neurons at the smallest M); the targets differ from the
    online networks."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(700 + sorted(CONFIGS).index(name))
    lay = DM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["window"], cfg["actor_layers"], cfg["critic_layers"])
    params = {}
    for which in NETS:
        kind = which.replace("target_", "")
        p = np.zeros(lay[kind + "_count"], dtype=np.float32)
        for i, o, w, b in lay[kind]:
            limit = math.sqrt(6.0 / (i + o))
            p[w:w + i * o] = rng.uniform(-limit, limit, i * o)
            p[b:b + o] = rng.normal(0.2, 0.1, o)
        params[which] = p
    return cfg, lay, params


def given_indices(ring, M):
    """idx int32 [M, 2]: every age 1 .. count - 1 in turn (with a wrapped ring the windows cross the wrap) over the robots in
    turn, a repeated index, and, where the ring holds them, transitions whose done is set."""
    n = ring.count - 1
    idx = np.array([[1 + m % n, (m * 7 + m // n) % ring.B] for m in range(M)], dtype=np.int32)
    ends = [(a, b) for a in range(1, ring.count) for b in range(ring.B) if ring.done[ring.slot(a), b] != 0]
    for k, (a, b) in enumerate(ends[:max(0, min(3, M - 3))]):
        idx[M - 1 - k] = (a, b)
    if M > 1:
        idx[1] = idx[0]
    return idx


def deviation(g, g64, names):
    """{tensor: max|g - g64| / max|g64|}; a tensor whose float64 gradient is all zeros must be all zeros."""
    out = {}
    g = np.asarray(g, dtype=np.float64)
    for k, s in names.items():
        top = float(np.abs(g64[s]).max())
        out[k] = float(np.abs(g[s] - g64[s]).max()) / top if top > 0 else float(np.abs(g[s]).max())
    return out


def _draw_obs(rng, d, n):
    return (0.3 + rng.normal(size=(n, d))).astype(np.float32)


def fill_ring(name, B, C, ticks, seed):
    """A ring after `ticks` stores: random observations, actions in [-1, 1], rewards, and a done in about every fifth entry
    (any value but 0 counts), with one in the middle of the ring for robot 0 when there is room."""
    cfg, _, _ = net(name)
    d, A = cfg["obs_dim"], cfg["act_dim"]
    rng = np.random.default_rng(seed)
    ring = DM.Ring(C, B, d, A)
    for t in range(ticks):
        done = rng.choice(np.array([0, 0, 0, 0, 1, -1, 2 ** 31 - 1], dtype=np.int64), size=B).astype(np.int32)
        if t == ticks - 3 and ticks >= 4:
            done[0] = 1
        ring.store(_draw_obs(rng, d, B).T, rng.uniform(-1, 1, size=(B, A)).astype(np.float32), rng.normal(0.5, 1.0, B).astype(np.float32), done)
    return ring, rng


@functools.lru_cache(maxsize=None)
def case(name, B, C, ticks, M):
    cfg, lay, params = net(name)
    W, d = cfg["window"], cfg["obs_dim"]
    ring, rng = fill_ring(name, B, C, ticks, 1000 * M + 10 * B + C + 7 * sorted(CONFIGS).index(name))
    idx = given_indices(ring, M)
    margins, redraws = None, 0
    for _ in range(50):                                   # keep every differentiated hidden pre-activation away from 0 (module docstring)
        pres = {}
        for dtype in (np.float64, np.float32):
            pc, pa, pq = [], [], []
            DM.critic_grad(ring, idx, params["critic"], params["target_actor"], params["target_critic"], lay, W, GAMMA, dtype, pre=pc)
            DM.actor_grad(ring, idx, params["actor"], params["critic"], lay, W, dtype, pre_actor=pa, pre_critic=pq)
            pres[dtype] = pc[:-1] + pa[:-1] + pq[:-1]       # the hidden layers; the heads have no relu
        if margins is None:
            margins = [8.0 * float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pres[np.float32], pres[np.float64])]
        near = np.zeros(M, dtype=bool)
        for y, m_ in zip(pres[np.float64], margins):
            near |= (np.abs(y) <= m_).any(axis=1)
        if not near.any():
            break
        cells = sorted({(ring.slot(int(a) + k), int(b)) for a, b in idx[near] for k in range(min(W, ring.count - int(a)))})
        for s, b in cells:
            ring.obs[s, :, b] = _draw_obs(rng, d, 1)[0]
        redraws += len(cells)
    assert not near.any()
    c = dict(name=name, B=B, C=C, ticks=ticks, M=M, cfg=cfg, lay=lay, params=params, ring=ring, idx=idx, redrawn=redraws / (ring.count * B))
    small = M <= TILE + 1                                  # the derived floor is for these shapes alone (module docstring)
    runs = dict(critic=lambda **kw: DM.critic_grad(ring, idx, params["critic"], params["target_actor"], params["target_critic"], lay, W, GAMMA, **kw),
                actor=lambda **kw: DM.actor_grad(ring, idx, params["actor"], params["critic"], lay, W, **kw))
    rel = lambda a, b: abs(a - b) / abs(b) if b != 0 else abs(a)
    for which, shift in (("critic", "q_shift"), ("actor", "mu_shift")):
        g64, g32 = runs[which](), runs[which](dtype=np.float32)
        shifted = [runs[which](**{shift: s}) for s in (FLOOR, -FLOOR)]
        names = DM.tensors(lay[which])
        dev32 = deviation(g32["grad"], g64["grad"], names)
        forward = [deviation(s["grad"], g64["grad"], names) for s in shifted]
        mag, g = g64["mag"], g64["grad"]
        floor = {k: FLOOR * (float(mag[s].max()) / float(np.abs(g[s]).max()) if np.abs(g[s]).max() > 0 else 0.0) + max(f[k] for f in forward)
                 for k, s in names.items()}
        c[which] = dict(m64=g64, m32=g32, names=names, dev32=dev32, floor=floor,
                        tol={k: max(8.0 * dev32[k], floor[k] if small else PROJECT_FLOOR) for k in names},
                        loss_dev32=rel(g32["loss"], g64["loss"]),
                        loss_tol=max(8.0 * rel(g32["loss"], g64["loss"]),
                                     FLOOR + max(rel(s["loss"], g64["loss"]) for s in shifted) if small else PROJECT_FLOOR))
    return c
