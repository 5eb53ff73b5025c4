"""Numpy model of include/rg_bptt.h: RecurrentPPO.policy_loss and its gradient with respect to the whole policy buffer by a
hand-written back-propagation through time.  The forward pass is tests/rnn_model.py's tick, the head tests/ppo_update_model.py's
(policy_head, adv_stats; adam_step and move_penalty are used from there as they stand).  Float64 is the yardstick of the
kernels and is itself checked against torch autograd (tests/test_bptt_cpu.py).  dtype=np.float32 evaluates the networks'
forward and backward passes in float32 (a neuron's sum sequentially, without fused multiply-adds; the products and sums of
the backward pass as numpy forms them) with the head in float64, as the kernels have it: its deviation from float64 measures
what float32 costs at the shapes of a test."""
import numpy as np

from tests import policy_model as PM
from tests import ppo_update_model as UM
from tests import rnn_model as RM


def normalized_obs(obs, norm_state, obs_clip=5.0):
    """obs float32 [T, obs_dim, B] through the normaliser in float64, rounded to float32: [T, B, obs_dim]."""
    return np.stack([RM.normalised(o, norm_state, obs_clip) for o in np.asarray(obs)])


def dense_forward(x, policy_params, lay, dtype=np.float64, pre=None):
    """The activations of the dense relu layers for x [n, obs_dim], the input first; pre receives the pre-activations."""
    acts = [np.asarray(x, dtype=dtype)]
    for W, b in PM.split(policy_params, lay["dense"], dtype):
        y = RM._affine([acts[-1]], W, b, dtype)
        if pre is not None:
            pre.append(y)
        acts.append(np.where(y > 0, y, dtype(0)))
    return acts


def forward(x, reset, h0, policy_params, lay, dtype=np.float64):
    """The T ticks from h0 for normalised observations x [T, B, obs_dim]: dict(acts: the dense activations [T * B, width] each,
    the input first; h_in, r, u, c, hidden [T, B, H]; mean [T, B, act_dim]) in `dtype`."""
    x = np.asarray(x)
    T, B, _ = x.shape
    acts = dense_forward(x.reshape(T * B, -1), policy_params, lay, dtype)
    cell = dict(lay, dense=[])
    xc = acts[-1].reshape(T, B, -1)
    h = np.asarray(h0, dtype=dtype)
    out = {k: [] for k in ("h_in", "r", "u", "c", "hidden", "mean")}
    for t in range(T):
        o = RM.tick(xc[t], h, np.asarray(reset)[t], policy_params, cell, dtype)
        h = o["hidden"]
        for k in out:
            out[k].append(o[k])
    return dict(acts=acts, **{k: np.stack(v) for k, v in out.items()})


def policy_grad(x, reset, h0, policy_params, lay, action, mean0, logstd0, adv, mask, penalty, dtype=np.float64, stats=None, mean_shift=0.0, **settings):
    """RecurrentPPO.policy_loss and its gradient with respect to the whole policy buffer (logstd last) for normalised
    observations x [T, B, obs_dim], reset [T, B] and the state h0 [B, H] (a constant: nothing flows into it).  mean_shift is
    added to every mean after the forward pass.  Returns dict(grad [policy_count] float64, mag: per entry the sum of the
    absolute values of the terms it is the sum of, loss, kl [B], mean [T * B, act_dim], over)."""
    x, reset = np.asarray(x), np.asarray(reset)
    T, B, _ = x.shape
    H, n_x, lo, count = lay["gru_units"], lay["n_x"], lay["logstd_offset"], lay["policy_count"]
    f = forward(x, reset, h0, policy_params, lay, dtype)
    (W_ru, _), (W_c, _), (W_h, _) = PM.split(policy_params, [lay["w_ru"], lay["w_c"], lay["head"]], dtype)
    dense = PM.split(policy_params, lay["dense"], dtype)
    logstd = np.asarray(policy_params)[lo:count]
    mu = f["mean"].reshape(T * B, -1).astype(np.float64) + mean_shift
    _, m, sd = UM.adv_stats(adv, mask) if stats is None else stats
    advn = (np.asarray(adv, dtype=np.float64) - m) / sd
    head = UM.policy_head(mu, logstd, action, mean0, logstd0, advn, mask, T, B, penalty, **settings)
    d_mean = (head["dmu"] * (1.0 - mu * mu)).astype(dtype).reshape(T, B, -1)     # the one rounding into the backward pass
    one = dtype(1)
    d_ru, d_c, d_x = np.zeros((T, B, 2 * H), dtype=dtype), np.zeros((T, B, H), dtype=dtype), np.zeros((T, B, n_x), dtype=dtype)
    dh = np.zeros((B, H), dtype=dtype)
    for t in range(T - 1, -1, -1):
        h, r, u, c = f["h_in"][t], f["r"][t], f["u"][t], f["c"][t]
        dh = dh + d_mean[t] @ W_h.T
        dc, du, dh_prev = dh * (one - u), dh * (h - c), dh * u
        d_c[t] = dc * (one - c * c)
        drh = d_c[t] @ W_c[n_x:].T
        dh_prev = dh_prev + drh * r
        d_ru[t, :, :H] = (drh * h) * (r * (one - r))
        d_ru[t, :, H:] = du * (u * (one - u))
        dh_prev = dh_prev + d_ru[t] @ W_ru[n_x:].T
        d_x[t] = d_ru[t] @ W_ru[:n_x].T + d_c[t] @ W_c[:n_x].T
        dh = np.where(reset[t][:, None] != 0, dtype(0), dh_prev)                 # nothing crosses a reset; nothing flows into h0
    grad, mag = np.zeros(count), np.zeros(count)

    def block(spec, inp, delta):
        i, o, w, b = spec
        inp, delta = inp.reshape(T * B, -1), delta.reshape(T * B, -1)
        grad[w:w + i * o] = (inp.T @ delta).reshape(-1)
        grad[b:b + o] = delta.sum(axis=0)
        mag[w:w + i * o] = (np.abs(inp).T @ np.abs(delta)).reshape(-1)
        mag[b:b + o] = np.abs(delta).sum(axis=0)

    xc = f["acts"][-1].reshape(T, B, -1)
    block(lay["w_ru"], np.concatenate([xc, f["h_in"]], axis=2), d_ru)
    block(lay["w_c"], np.concatenate([xc, f["r"] * f["h_in"]], axis=2), d_c)
    block(lay["head"], f["hidden"], d_mean)
    d = d_x.reshape(T * B, -1)
    for k in range(len(dense) - 1, -1, -1):
        d = d * (f["acts"][k + 1] > 0)                                           # relu'(0) = 0
        block(lay["dense"][k], f["acts"][k], d)
        if k > 0:
            d = d @ dense[k][0].T
    grad[lo:] = head["dlogstd"]
    mag[lo:] = np.abs(head["dlogstd"])
    return dict(grad=grad, mag=mag, loss=head["loss"], kl=head["kl"], mean=f["mean"].reshape(T * B, -1), over=head["over"])


def tensors(lay):
    """{name: slice} of the parameter tensors of the policy buffer: W and b of every block, and logstd."""
    names = [f"dense{k}" for k in range(len(lay["dense"]))] + ["ru", "c", "head"]
    out = {}
    for name, (i, o, w, b) in zip(names, RM.blocks(lay)):
        out["W_" + name], out["b_" + name] = slice(w, w + i * o), slice(b, b + o)
    out["logstd"] = slice(lay["logstd_offset"], lay["policy_count"])
    return out


def h_rows(lay):
    """The slices of the policy buffer that hold the h rows of W_ru and of W_c."""
    out = []
    for name in ("w_ru", "w_c"):
        i, o, w, _ = lay[name]
        out.append(slice(w + lay["n_x"] * o, w + i * o))
    return out
