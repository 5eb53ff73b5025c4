"""Numpy model of include/rg_ppo.h: the advantage normalisation, both losses of PPO (robot_gym_amd/agents/ppo/algorithm.py) with
their analytic gradients through the two networks, Adam and the penalty rule.  Float64 is the yardstick of the kernels and is
itself checked against torch autograd (tests/test_ppo_update_cpu.py).  dtype=np.float32 evaluates the networks' forward and
backward passes in float32 (a neuron's sum sequentially, without fused multiply-adds; the products of the backward pass as
numpy forms them) with the head in float64 as the kernels have it: its deviation from float64 measures what float32 costs at
the shapes of a test."""
import numpy as np

from tests import policy_model as PM


def adv_stats(adv, mask):
    """(n clamped to 1, mean, std + 1e-8) of adv over the ticks with mask != 0, as PPO.batch forms them."""
    a = np.asarray(adv, dtype=np.float64)[np.asarray(mask) != 0]
    n = max(len(a), 1)
    m = float(np.sum(a)) / n
    return n, m, float(np.sqrt(np.sum((a - m) ** 2) / n)) + 1e-8


def normalized_obs(obs, norm_state, obs_clip=5.0):
    """obs float32 [T, obs_dim, B] through the observation normaliser in float64, rounded to float32: [T * B, obs_dim], sample
    n = t * B + b."""
    obs = np.asarray(obs)
    T, d, B = obs.shape
    on, _ = PM.normalizers_of(norm_state, d, obs_clip)
    return on.transform(obs.transpose(0, 2, 1).reshape(T * B, d).astype(np.float64)).astype(np.float32)


def forward_all(x, layers, head, dtype=np.float64, pre=None):
    """The activations of every layer, the input first: relu hidden layers, `head` in ("tanh", "linear").  pre: a list that
    receives every layer's pre-activations."""
    acts = [np.asarray(x, dtype=dtype)]
    for k, (W, b) in enumerate(layers):
        a = acts[-1]
        if dtype == np.float64:
            y = a @ W + b
        else:
            y = np.zeros((a.shape[0], W.shape[1]), dtype=np.float32)
            for i in range(W.shape[0]):
                y += a[:, i:i + 1] * W[i][None, :]
            y = y + b
        if pre is not None:
            pre.append(y)
        last = k == len(layers) - 1
        acts.append((np.tanh(y) if head == "tanh" else y) if last else np.where(y > 0, y, dtype(0)))
    return acts


def tile_sum(x, d, tile, groups):
    """x.T @ d for float32 x [M, in] and d [M, out] summed in the order of rg_ppo.h / rg_ddpg.h: a float32 chain over the `tile`
    samples of a tile in order (padded samples are zeros), a float32 running sum over the tiles g, g + groups, ... of a
    workgroup, a float64 sum over the workgroups in order, rounded to float32 once.  Products are rounded before they are added
    (no fused multiply-add), as everywhere in the float32 model."""
    x, d = np.asarray(x, dtype=np.float32), np.asarray(d, dtype=np.float32)
    M = x.shape[0]
    ntiles = -(-M // tile)
    pad = ntiles * tile - M
    xt = np.concatenate([x, np.zeros((pad, x.shape[1]), dtype=np.float32)]).reshape(ntiles, tile, -1)
    dt = np.concatenate([d, np.zeros((pad, d.shape[1]), dtype=np.float32)]).reshape(ntiles, tile, -1)
    t = np.zeros((ntiles, x.shape[1], d.shape[1]), dtype=np.float32)
    for s in range(tile):
        t += xt[:, s, :, None] * dt[:, s, None, :]
    G = min(ntiles, groups)
    slab = np.zeros((G,) + t.shape[1:], dtype=np.float32)
    for first in range(0, ntiles, G):
        n = min(G, ntiles - first)
        slab[:n] += t[first:first + n]
    total = np.zeros(t.shape[1:], dtype=np.float64)
    for g in range(G):
        total += slab[g]
    return total.astype(np.float32)


def backward(acts, layers, delta, count, spec, dtype=np.float64, mag=None, tiles=None):
    """The gradient of sum(delta * pre-activation of the head) with respect to every W and b, laid out as the buffer `spec`
    ([(in, out, w_offset, b_offset)]) of `count` entries.  relu'(0) = 0.  mag (an array of `count` entries) receives the sum of
    the absolute values of the terms each entry is the sum of: what a rounding error of that sum scales with.  tiles = (tile,
    groups), with dtype float32: the sums over the samples run in the kernels' order (tile_sum) instead of numpy's."""
    grad = np.zeros(count, dtype=dtype)
    d = np.asarray(delta, dtype=dtype)
    ordered = tiles is not None and dtype == np.float32
    for k in range(len(layers) - 1, -1, -1):
        i, o, w, b = spec[k]
        grad[w:w + i * o] = (tile_sum(acts[k], d, *tiles) if ordered else acts[k].T @ d).reshape(-1)
        grad[b:b + o] = tile_sum(np.ones((len(d), 1), dtype=np.float32), d, *tiles)[0] if ordered else d.sum(axis=0)
        if mag is not None:
            mag[w:w + i * o] = (np.abs(acts[k]).T @ np.abs(d)).reshape(-1)
            mag[b:b + o] = np.abs(d).sum(axis=0)
        if k > 0:
            d = (d @ layers[k][0].T) * (acts[k] > 0)
    return grad


def policy_head(mu, logstd, action, mean0, logstd0, advn, valid, T, B, penalty, kl_target=1e-2, kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0,
                conv="exact"):
    """The policy loss from the means mu [T * B, act_dim] on, in float64 (rg_ppo.h, Policy loss): dict(loss, kl [B], kl_sample,
    ratio, dmu: dL/dmu [T * B, act_dim], dlogstd [act_dim], over: kl > threshold [B])."""
    f = lambda v: np.asarray(v, dtype=np.float64)
    mu, ls, a, m0, ls0, advn = f(mu), f(logstd), f(action).reshape(T * B, -1), f(mean0).reshape(T * B, -1), f(logstd0), f(advn).reshape(T * B)
    valid = np.asarray(valid).reshape(T * B) != 0
    c = 1.0 if conv == "exact" else 0.5
    s1, s0 = np.exp(ls), np.exp(ls0)
    D, z, z0 = mu - m0, (a - mu) / s1, (a - m0) / s0
    q = (s0 * s0 + D * D) / (s1 * s1)
    kl_sample = np.where(valid, 0.5 * np.sum((q - 1.0) + 2.0 * (ls - ls0), axis=1), 0.0)
    ratio = np.exp(np.sum(-c * ls - 0.5 * z * z, axis=1) - np.sum(-c * ls0 - 0.5 * z0 * z0, axis=1))
    kl = kl_sample.reshape(T, B).sum(axis=0) / T
    thr = kl_target * kl_cutoff_factor
    over = kl > thr
    surrogate = np.where(valid, ratio * advn, 0.0)
    loss = -np.sum(surrogate) / (T * B) + np.sum(penalty * kl + kl_cutoff_coef * over * (kl - thr) ** 2) / B
    gb = np.tile(penalty + 2.0 * kl_cutoff_coef * over * (kl - thr), T)[:, None]
    w = (valid / (T * B))[:, None]
    ra = np.where(valid, ratio * advn, 0.0)[:, None]     # a masked tick carries nothing, whatever its ratio
    dmu = w * (-ra * z / s1 + gb * D / (s1 * s1))
    dlogstd = np.sum(w * (-ra * (z * z - c) + gb * (1.0 - q)), axis=0)
    return dict(loss=float(loss), kl=kl, kl_sample=kl_sample, ratio=ratio, dmu=dmu, dlogstd=dlogstd, over=over)


def policy_grad(x, policy_params, lay, action, mean0, logstd0, adv, mask, T, B, penalty, dtype=np.float64, stats=None, mean_shift=0.0, **settings):
    """PPO.policy_loss and its gradient with respect to the whole policy buffer (logstd last) for normalised observations
    x [T * B, obs_dim].  mean_shift is added to every mean after the forward pass (what an error of the forward pass does to
    the loss and the gradient).  Returns dict(grad [policy_count] float64, loss, kl [B], mean [T * B, act_dim], over)."""
    spec, lo = lay["policy"], lay["logstd_offset"]
    layers = PM.split(policy_params, spec, dtype)
    logstd = np.asarray(policy_params)[lo:lay["policy_count"]]
    acts = forward_all(x, layers, "tanh", dtype)
    mu = acts[-1].astype(np.float64) + mean_shift
    _, m, sd = adv_stats(adv, mask) if stats is None else stats
    advn = (np.asarray(adv, dtype=np.float64) - m) / sd
    h = policy_head(mu, logstd, action, mean0, logstd0, advn, mask, T, B, penalty, **settings)
    delta = h["dmu"] * (1.0 - mu * mu)
    grad, mag = np.zeros(lay["policy_count"]), np.zeros(lay["policy_count"])
    grad[:lo] = backward(acts, layers, delta.astype(dtype), lo, spec, dtype, mag)
    grad[lo:] = h["dlogstd"]
    mag[lo:] = np.abs(h["dlogstd"])
    return dict(grad=grad, mag=mag, loss=h["loss"], kl=h["kl"], mean=acts[-1], over=h["over"])


def value_grad(x, value_params, lay, ret, mask, T, B, dtype=np.float64, value_shift=0.0):
    """PPO.value_loss and its gradient with respect to the value buffer; value_shift is added to every value after the forward
    pass."""
    spec = lay["value"]
    layers = PM.split(value_params, spec, dtype)
    acts = forward_all(x, layers, "linear", dtype)
    V = acts[-1][:, 0].astype(np.float64) + value_shift
    valid = np.asarray(mask).reshape(T * B) != 0
    e = np.where(valid, np.asarray(ret, dtype=np.float64).reshape(T * B) - V, 0.0)
    loss = float(np.sum(0.5 * e * e) / (T * B))
    delta = (-e / (T * B))[:, None]
    mag = np.zeros(lay["value_count"])
    grad = backward(acts, layers, delta.astype(dtype), lay["value_count"], spec, dtype, mag).astype(np.float64)
    return dict(grad=grad, mag=mag, loss=loss, value=acts[-1][:, 0])


def tensors(spec, logstd_offset=None, count=None):
    """{name: slice} of the parameter tensors of a buffer: each W, each b, and logstd."""
    out = {}
    for k, (i, o, w, b) in enumerate(spec):
        out[f"W{k}"], out[f"b{k}"] = slice(w, w + i * o), slice(b, b + o)
    if logstd_offset is not None:
        out["logstd"] = slice(logstd_offset, count)
    return out


def adam_step(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """One step of torch.optim.Adam's formula; t is the step count before it.  Returns (p, m, v, t + 1)."""
    t = t + 1
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - lr / (1.0 - beta1 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - beta2 ** t) + eps)
    return p, m, v, t


def move_penalty(penalty, kl_change, kl_target):
    """x 1.5 above 1.3 x the target, / 1.5 below 0.7 x, else unchanged."""
    if kl_change > 1.3 * kl_target:
        return penalty * 1.5
    if kl_change < 0.7 * kl_target:
        return penalty / 1.5
    return penalty
