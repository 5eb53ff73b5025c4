"""Numpy model of include/rg_ddpg.h: the replay ring with the window rule, the Ornstein-Uhlenbeck step on the noise stream of
tests/policy_model.py, the sample stream, both losses with their analytic gradients, the global-norm clip, Adam and the soft
update.  Float64 is the yardstick of the kernels and is itself checked against torch autograd (tests/test_ddpg_cpu.py).
dtype=np.float32 evaluates the networks' forward and backward passes in float32 (a neuron's sum sequentially, without fused
multiply-adds) with the heads in float64 as the kernels have them: its deviation from float64 measures what float32 costs at
the shapes of a test."""
import math

import numpy as np

from tests import policy_model as PM
from tests import ppo_update_model as UM
from tests.stream_model import chain as sample_hash     # over (updates, m, draw)

adam_step = UM.adam_step
tensors = UM.tensors


def layout(obs_dim, act_dim, window, actor_layers, critic_layers):
    """The layout rule of rg_ddpg.h: per network [(in, out, w_offset, b_offset), ...] with the head last; the critic's input is
    the action followed by the window."""
    out = {}
    for name, widths, first, head in (("actor", actor_layers, window * obs_dim, act_dim), ("critic", critic_layers, act_dim + window * obs_dim, 1)):
        layers, off, prev = [], 0, first
        for width in list(widths) + [head]:
            layers.append((prev, width, off, off + prev * width))
            off += prev * width + width
            prev = width
        out[name] = layers
        out[name + "_count"] = off
    return out


# ---- the ring ---------------------------------------------------------------------------------------------------------

class Ring:
    """The replay ring of rg_ddpg.h in numpy: the same arrays, head, count and updates."""

    def __init__(self, capacity, batch, obs_dim, act_dim):
        self.C, self.B, self.obs_dim, self.act_dim = capacity, batch, obs_dim, act_dim
        self.obs = np.zeros((capacity, obs_dim, batch), dtype=np.float32)
        self.action = np.zeros((capacity, batch, act_dim), dtype=np.float32)
        self.reward = np.zeros((capacity, batch), dtype=np.float32)
        self.done = np.zeros((capacity, batch), dtype=np.int32)
        self.head = self.count = self.updates = 0

    def store(self, obs_cm, action, reward, done):
        h = self.head
        self.obs[h], self.action[h], self.reward[h], self.done[h] = obs_cm, action, reward, done
        self.head, self.count = (h + 1) % self.C, min(self.count + 1, self.C)

    def slot(self, age):
        return (self.head - 1 - age) % self.C

    def kept(self, a, b, window):
        """How many elements (newest first) of the state of robot b ending at age a are kept; a = -1: the acting state."""
        k = 0
        while k < window:
            age = a + k
            if age >= self.count or (k > 0 and self.done[self.slot(age), b] != 0):
                break
            k += 1
        return k

    def state(self, a, b, window, cur=None):
        """float32 [window * obs_dim], oldest first; cur [obs_dim, B]: the current observation of an acting state (a = -1)."""
        x = np.zeros((window, self.obs_dim), dtype=np.float32)
        for k in range(self.kept(a, b, window)):
            x[window - 1 - k] = cur[:, b] if a + k < 0 else self.obs[self.slot(a + k), :, b]
        return x.reshape(-1)

    def states(self, ages, robots, window, cur=None):
        memo = {}
        for key in zip((int(a) for a in ages), (int(b) for b in robots)):
            if key not in memo:
                memo[key] = self.state(key[0], key[1], window, cur)
        return np.stack([memo[key] for key in zip((int(a) for a in ages), (int(b) for b in robots))])

    def state_array(self):
        return np.array([self.head, self.count, self.updates, 0], dtype=np.int64)


# ---- noise and sampling -------------------------------------------------------------------------------------------------

def ou_step(x, eps, theta=0.5, mu=0.4, sigma=0.3, dt=1e-2):
    """One Ornstein-Uhlenbeck step in float64 over float32 x and eps, rounded to float32 (rg_ddpg.h, rg_ddpg_act)."""
    x, eps = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(eps, dtype=np.float32).astype(np.float64)
    return ((x + (theta * (mu - x)) * dt) + (sigma * math.sqrt(dt)) * eps).astype(np.float32)


def sample(seed, updates, M, count, B):
    """idx int32 [M, 2] = (age, robot) of rg_ddpg_sample; None on a short ring."""
    if count < 2:
        return None
    return np.array([[1 + sample_hash(seed, updates, m, 0) % (count - 1), sample_hash(seed, updates, m, 1) % B] for m in range(M)], dtype=np.int32)


# ---- the losses -----------------------------------------------------------------------------------------------------------

def _f64(v):
    return np.asarray(v).astype(np.float64)


def _live(idx, live):
    """(idx with the dead samples pointed at transition (1, 0), which exists in every ring that holds one; live as float64)."""
    idx = np.asarray(idx)
    if live is None:
        return idx, np.ones(len(idx))
    live = np.asarray(live, dtype=bool)
    idx = idx.copy()
    idx[~live] = (1, 0)
    return idx, live.astype(np.float64)


def critic_grad(ring, idx, critic, target_actor, target_critic, lay, window, gamma=0.99, dtype=np.float64, q_shift=0.0, pre=None, live=None,
                tiles=None):
    """The critic's loss (sum 0.5 (y - Q)^2) / M over the transitions idx [M, 2] and its gradient with respect to the critic
    buffer.  q_shift is added to every Q after the forward pass; pre receives the critic's pre-activations on [action, s0].
    live (bool [M]): a sample whose entry is False contributes nothing to the loss or the gradient while M stays M (an index
    outside the ring, rg_ddpg.h); its index is not looked at.  tiles: UM.backward's.  Returns dict(grad, mag, loss, q, y)."""
    idx, lv = _live(idx, live)
    ages, robots = idx[:, 0], idx[:, 1]
    M = len(idx)
    s1, s0 = ring.states(ages - 1, robots, window), ring.states(ages, robots, window)
    slots = np.array([ring.slot(int(a)) for a in ages])
    a1 = UM.forward_all(s1, PM.split(target_actor, lay["actor"], dtype), "tanh", dtype)[-1]
    q1 = UM.forward_all(np.concatenate([a1, s1.astype(dtype)], axis=1), PM.split(target_critic, lay["critic"], dtype), "linear", dtype)[-1][:, 0]
    nd = 1.0 - (ring.done[slots, robots] != 0)
    y = _f64(ring.reward[slots, robots]) + (gamma * nd) * _f64(q1)
    layers = PM.split(critic, lay["critic"], dtype)
    acts = UM.forward_all(np.concatenate([ring.action[slots, robots].astype(dtype), s0.astype(dtype)], axis=1), layers, "linear", dtype, pre=pre)
    q = _f64(acts[-1][:, 0]) + q_shift
    e = (q - y) * lv
    mag = np.zeros(lay["critic_count"])
    grad = UM.backward(acts, layers, (e / M)[:, None].astype(dtype), lay["critic_count"], lay["critic"], dtype, mag, tiles)
    return dict(grad=_f64(grad), mag=mag, loss=float(np.sum(0.5 * e * e) / M), q=q, y=y)


def actor_grad(ring, idx, actor, critic, lay, window, dtype=np.float64, mu_shift=0.0, pre_actor=None, pre_critic=None, live=None, tiles=None):
    """The actor's loss -(sum Q([mu(s0), s0])) / M and its gradient with respect to the actor buffer: backward through the
    critic's inputs (relu gates on its hidden layers, none on the input), the action's components times (1 - mu^2) in float64,
    then through the actor.  mu_shift is added to every mean after the actor's forward pass.  live, tiles: critic_grad's.
    Returns dict(grad, mag, loss, mean_q, mu)."""
    idx, lv = _live(idx, live)
    ages, robots = idx[:, 0], idx[:, 1]
    M, A = len(idx), lay["actor"][-1][1]
    s0 = ring.states(ages, robots, window)
    la, lc = PM.split(actor, lay["actor"], dtype), PM.split(critic, lay["critic"], dtype)
    acts_a = UM.forward_all(s0, la, "tanh", dtype, pre=pre_actor)
    mu = _f64(acts_a[-1]) + mu_shift
    acts_c = UM.forward_all(np.concatenate([mu.astype(dtype), s0.astype(dtype)], axis=1), lc, "linear", dtype, pre=pre_critic)
    q = _f64(acts_c[-1][:, 0]) * lv
    d = (np.full((M, 1), dtype(-1.0 / M), dtype=dtype) * lv[:, None]).astype(dtype)
    for k in range(len(lc) - 1, -1, -1):
        d = d @ lc[k][0].T
        if k > 0:
            d = d * (acts_c[k] > 0)
    delta = (_f64(d[:, :A]) * (1.0 - mu * mu)).astype(dtype)
    mag = np.zeros(lay["actor_count"])
    grad = UM.backward(acts_a, la, delta, lay["actor_count"], lay["actor"], dtype, mag, tiles)
    return dict(grad=_f64(grad), mag=mag, loss=float(-np.sum(q) / M), mean_q=float(np.sum(q) / M), mu=acts_a[-1])


# ---- the optimiser ------------------------------------------------------------------------------------------------------

def clip(grad, clipnorm):
    """(grad after the global-norm clip as float32, the norm before it): float32 in, the norm in float64."""
    g = np.asarray(grad, dtype=np.float32)
    norm = math.sqrt(float(np.sum(g.astype(np.float64) ** 2)))
    if clipnorm > 0 and norm >= clipnorm:
        g = (g.astype(np.float64) * (clipnorm / norm)).astype(np.float32)
    return g, norm


def adam_header(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step of rg_ddpg_adam's formula with the header's roundings (rg_ddpg.h): float32 p, g, m, v; t is the step count before
    it.  m and v in float32 with one rounding per operation, p in float64 with one rounding.  Returns (p, m, v) as float32."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    f = np.float32
    t = float(t + 1)
    m = f(beta1) * m + f(1.0 - beta1) * g
    v = f(beta2) * v + f(1.0 - beta2) * (g * g)
    assert m.dtype == np.float32 and v.dtype == np.float32
    bc1, bc2s = 1.0 - math.pow(beta1, t), math.sqrt(1.0 - math.pow(beta2, t))
    denom = np.sqrt(v.astype(np.float64)) / bc2s + eps
    return (p.astype(np.float64) - (lr / bc1) * m.astype(np.float64) / denom).astype(np.float32), m, v


def soft_update(target, online, tau):
    t, o = np.asarray(target, dtype=np.float32).astype(np.float64), np.asarray(online, dtype=np.float32).astype(np.float64)
    return ((1.0 - tau) * t + tau * o).astype(np.float32)
