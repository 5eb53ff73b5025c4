"""Float64 numpy model of include/rg_policy.h, written from the formulas of the reference's agents/ppo (normalize.py,
utility.py, algorithm.py) and scripts/networks.py: the noise stream, the streaming normaliser, the two networks, the log
probability and the returns.  It is the yardstick of the kernels and of the torch update; TensorFlow's own arithmetic is
not pinned anywhere."""
import math

import numpy as np

from tests.stream_model import M64  # noqa: F401
from tests.stream_model import chain as noise_hash     # over (key, counter, axis, draw)

NORM_COLS, NORM_REWARD, NORM_ROWS = 65, 64, 195
LOG_2PI = 1.8378770664093453
TWO_PI = 6.283185307179586


# ---- the noise stream -------------------------------------------------------------------------------------------------

def uniforms(seed, key, counter, axis):
    """(u1, u2): u1 in (0, 1], u2 in [0, 1)."""
    return ((noise_hash(seed, key, counter, axis, 0) >> 11) + 1) * 2.0 ** -53, (noise_hash(seed, key, counter, axis, 1) >> 11) * 2.0 ** -53


def eps64(seed, key, counter, axis):
    u1, u2 = uniforms(seed, key, counter, axis)
    return math.sqrt(-2.0 * math.log(u1)) * math.cos(TWO_PI * u2)


def eps(seed, key, counter, axis):
    """The standard normal of (seed, key, counter, axis), rounded to float32 as the kernel rounds it."""
    return np.float32(eps64(seed, key, counter, axis))


def eps_batch(seed, keys, counters, act_dim):
    return np.array([[eps(seed, int(k), int(c), a) for a in range(act_dim)] for k, c in zip(keys, counters)], dtype=np.float32).reshape(-1, act_dim)


# ---- the normaliser ---------------------------------------------------------------------------------------------------

class Normalizer:
    """StreamingNormalize over `dim` components: count, mean [dim], var_sum [dim]."""

    def __init__(self, dim, center=True, clip=0.0):
        self.count, self.mean, self.var_sum = 0, np.zeros(dim), np.zeros(dim)
        self.center, self.clip = center, float(clip)

    def scale(self):
        return np.sqrt(self.var_sum / (self.count - 1) + 1e-4) + 1e-8 if self.count > 1 else np.ones_like(self.var_sum)

    def transform(self, value):
        v = np.asarray(value, dtype=np.float64)
        if self.center:
            v = v - self.mean
        v = v / self.scale()
        return np.clip(v, -self.clip, self.clip) if self.clip > 0 else v

    def update(self, values):
        """values [n, dim] (n = 0: nothing changes)."""
        v = np.asarray(values, dtype=np.float64).reshape(-1, len(self.mean))
        if len(v) == 0:
            return
        self.count += len(v)
        new_mean = self.mean + np.sum(v - self.mean, axis=0) / self.count if self.count > 1 else v[0].copy()
        self.var_sum = self.var_sum + np.sum((v - self.mean) * (v - new_mean), axis=0)
        self.mean = new_mean


def norm_state_of(obs_norm, reward_norm):
    """The kernel's norm_state [NORM_ROWS] from two Normalizers."""
    s = np.zeros((3, NORM_COLS))
    n = len(obs_norm.mean)
    s[0, :n], s[1, :n], s[2, :n] = obs_norm.count, obs_norm.mean, obs_norm.var_sum
    s[0, NORM_REWARD], s[1, NORM_REWARD], s[2, NORM_REWARD] = reward_norm.count, reward_norm.mean[0], reward_norm.var_sum[0]
    return s.reshape(-1)


def normalizers_of(state, obs_dim, obs_clip=5.0, reward_clip=10.0):
    s = np.asarray(state, dtype=np.float64).reshape(3, NORM_COLS)
    o, r = Normalizer(obs_dim, True, obs_clip), Normalizer(1, False, reward_clip)
    o.count, o.mean, o.var_sum = int(s[0, 0]), s[1, :obs_dim].copy(), s[2, :obs_dim].copy()
    r.count, r.mean, r.var_sum = int(s[0, NORM_REWARD]), s[1, NORM_REWARD:NORM_REWARD + 1].copy(), s[2, NORM_REWARD:NORM_REWARD + 1].copy()
    return o, r


# ---- the networks -----------------------------------------------------------------------------------------------------

def layout(obs_dim, act_dim, policy_layers, value_layers):
    """The layout rule of rg_policy.h: per network [(in, out, w_offset, b_offset), ...] with the head last."""
    out = {}
    for name, widths, head in (("policy", policy_layers, act_dim), ("value", value_layers, 1)):
        layers, off, prev = [], 0, obs_dim
        for width in list(widths) + [head]:
            layers.append((prev, width, off, off + prev * width))
            off += prev * width + width
            prev = width
        out[name] = layers
        out[name + "_count"] = off
    out["logstd_offset"] = out["policy_count"]
    out["policy_count"] += act_dim
    return out


def split(params, layers, dtype=np.float64):
    p = np.asarray(params)
    return [(p[w:w + i * o].reshape(i, o).astype(dtype), p[b:b + o].astype(dtype)) for i, o, w, b in layers]


def forward(x, layers, head, dtype=np.float64):
    """x [n, in] through [(W, b), ...]: relu hidden layers, `head` in ("tanh", "linear").  dtype float32 accumulates each
    neuron's sum sequentially in float32, without fused multiply-adds."""
    x = np.asarray(x, dtype=dtype)
    for k, (W, b) in enumerate(layers):
        if dtype == np.float64:
            y = x @ W + b
        else:
            y = np.zeros((x.shape[0], W.shape[1]), dtype=np.float32)
            for i in range(W.shape[0]):
                y += x[:, i:i + 1] * W[i][None, :]
            y = y + b
        x = (np.tanh(y) if head == "tanh" else y) if k == len(layers) - 1 else np.where(y > 0, y, dtype(0))   # the kernels' v > 0 ? v : 0: a NaN gives 0
    return x


def fma32(w, x, acc):
    """fmaf(w, x, acc) of float32 arrays (broadcast), correctly rounded, in numpy.  The product of two float32 values is exact
    in float64.  s = fl64(p + acc) and TwoSum's err (s + err = p + acc exactly) locate the true sum: no float32 rounding
    boundary lies strictly between s and s + err (the boundaries are float64 numbers), so rounding s to float32 is the answer
    unless s is itself a float32 midpoint and err != 0; then s moves one float64 ulp to err's side first."""
    w, x, acc = (np.asarray(v, dtype=np.float32) for v in (w, x, acc))
    p = w.astype(np.float64) * x.astype(np.float64)
    a = np.broadcast_to(acc.astype(np.float64), p.shape)
    s = np.atleast_1d(p + a)
    # candidates first, cheaply: a midpoint of two normal float32 values has the low 29 bits of its float64 mantissa equal to
    # 2^28; below the normal range every s is looked at.  The exact test then runs on the candidates alone.
    cand = np.flatnonzero((((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -125)).ravel())
    if len(cand):
        pc, ac, sc = np.atleast_1d(p).ravel()[cand], np.atleast_1d(a).ravel()[cand], s.ravel()[cand]
        t = sc - pc
        err = (pc - (sc - t)) + (ac - t)
        with np.errstate(over="ignore", invalid="ignore"):
            r = sc.astype(np.float32)
            other = np.nextafter(r, np.where(sc > r, np.inf, -np.inf).astype(np.float32))
            mid = np.isfinite(other) & (r.astype(np.float64) != sc) & ((r.astype(np.float64) + other.astype(np.float64)) * 0.5 == sc)   # the sum of two float32 neighbours is exact
        nudge = mid & (err != 0.0)
        s = s.copy().ravel()
        s[cand[nudge]] = np.nextafter(sc[nudge], np.where(err[nudge] > 0.0, np.inf, -np.inf))
    with np.errstate(over="ignore"):
        return s.reshape(p.shape).astype(np.float32)


def forward_exact(x, layers, head):
    """x float32 [n, in] through float32 [(W, b), ...] in the arithmetic rg_policy.h pins for a neuron: acc = 0, then
    acc = fma(W[i][j], x[i], acc) for i in order, then acc + b[j] in float32; relu as where(v > 0, v, 0).  head "linear": the
    float32 output; head "tanh": the float32 PRE-activation of the head (tanhf itself is the device's)."""
    assert head in ("tanh", "linear")
    x = np.asarray(x, dtype=np.float32)
    for k, (W, b) in enumerate(layers):
        W, b = np.asarray(W, dtype=np.float32), np.asarray(b, dtype=np.float32)
        acc = np.zeros((x.shape[0], W.shape[1]), dtype=np.float32)
        for i in range(W.shape[0]):
            acc = fma32(W[i][None, :], x[:, i:i + 1], acc)
        v = acc + b[None, :]
        assert v.dtype == np.float32
        x = v if k == len(layers) - 1 else np.where(v > 0, v, np.float32(0))
    return x


def logprob(eps_, logstd):
    """-0.5 sum eps^2 - sum logstd - 0.5 act_dim ln(2 pi), eps_ [n, act_dim]."""
    e, ls = np.asarray(eps_, dtype=np.float64), np.asarray(logstd, dtype=np.float64)
    return -0.5 * np.sum(e * e, axis=-1) - np.sum(ls) - 0.5 * len(ls) * LOG_2PI


def act(obs_cm, norm_state, policy_params, value_params, lay, keys, counters, seed, sample=True, obs_clip=5.0, dtype=np.float64):
    """rg_policy_act: obs_cm float32 [obs_dim, B].  Returns dict(x, mean, value, eps, action, logprob), mean / value in `dtype`,
    x the float32 normalised observation both precisions start from."""
    obs_cm = np.asarray(obs_cm)
    obs_dim, B = obs_cm.shape
    on, _ = normalizers_of(norm_state, obs_dim, obs_clip)
    x = on.transform(obs_cm.T.astype(np.float64)).astype(np.float32)
    act_dim = lay["policy"][-1][1]
    mean = forward(x, split(policy_params, lay["policy"], dtype), "tanh", dtype)
    value = forward(x, split(value_params, lay["value"], dtype), "linear", dtype)[:, 0]
    logstd = np.asarray(policy_params)[lay["logstd_offset"]:lay["logstd_offset"] + act_dim].astype(np.float32)
    e = eps_batch(seed, keys, counters, act_dim) if sample else np.zeros((B, act_dim), dtype=np.float32)
    action = mean.astype(np.float64) + np.exp(logstd.astype(np.float64)) * e
    return dict(x=x, mean=mean, value=value, eps=e, action=action, logprob=logprob(e, logstd), logstd=logstd)


# ---- returns ----------------------------------------------------------------------------------------------------------

def returns(reward, value, done, last_value, reward_norm, discount, lam, bootstrap):
    """rg_policy_returns: reward, value, done [T, B]; returns (ret, adv) float64 [T, B]."""
    reward, value = np.asarray(reward, dtype=np.float64), np.asarray(value, dtype=np.float64)
    T, B = reward.shape
    rp = reward_norm.transform(reward.reshape(-1, 1)).reshape(T, B)
    nd = 1.0 - (np.asarray(done) != 0)
    vnext = np.asarray(last_value, dtype=np.float64).copy() if bootstrap else np.zeros(B)
    anext = np.zeros(B)
    ret, adv = np.zeros((T, B)), np.zeros((T, B))
    for t in range(T - 1, -1, -1):
        delta = rp[t] + discount * nd[t] * vnext - value[t]
        a = delta + discount * lam * nd[t] * anext
        adv[t], ret[t] = a, a + value[t]
        vnext, anext = value[t], a
    return ret, adv


def discounted_return(reward, discount):
    """utility.discounted_return of one finished episode, summed directly: R_t = sum_k discount^k r_{t+k}."""
    r = np.asarray(reward, dtype=np.float64)
    return np.array([sum(discount ** k * r[t + k] for k in range(len(r) - t)) for t in range(len(r))])


# ---- the update's formulas ---------------------------------------------------------------------------------------------

def diag_normal_kl(mean0, logstd0, mean1, logstd1):
    l0, l1 = 2.0 * np.asarray(logstd0), 2.0 * np.asarray(logstd1)
    return 0.5 * (np.sum(np.exp(l0 - l1)) + np.sum((mean1 - mean0) ** 2 / np.exp(l1), axis=-1) + np.sum(l1) - np.sum(l0) - mean0.shape[-1])


def diag_normal_logpdf(mean, logstd, loc, conv):
    logstd = np.asarray(logstd)
    const = -0.5 * LOG_2PI - (logstd if conv == "exact" else 0.5 * logstd)
    return np.sum(const - 0.5 * ((loc - mean) / np.exp(logstd)) ** 2, axis=-1)
