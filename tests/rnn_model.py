"""Numpy model of include/rg_rnn.h: the parameter layout, one tick of the recurrent Gaussian policy and the unroll, written
from the documented arithmetic of GRUBlockCell (r, u = sigmoid([x, h] W_ru + b_ru); c = tanh([x, r*h] W_c + b_c);
h' = u*h + (1 - u)*c) and the reference's scripts/networks.py (RecurrentGaussianPolicy).  The normaliser, the noise stream,
the value network and the log probability are tests/policy_model.py's.  dtype float64 is the yardstick; dtype float32 sums a
neuron's inputs in the kernel's order (the x inputs, then the h inputs) in float32 without fused multiply-adds, as
policy_model.forward does.  TensorFlow's own arithmetic is not pinned anywhere."""
import numpy as np

from tests import policy_model as PM


def layout(obs_dim, act_dim, policy_layers, gru_units, value_layers):
    """The layout rule of rg_rnn.h in the form of rnn_abi.param_layout."""
    H = int(gru_units)
    dense, off, prev = [], 0, obs_dim
    for width in policy_layers:
        dense.append((prev, width, off, off + prev * width))
        off += prev * width + width
        prev = width
    out = dict(dense=dense, n_x=prev, gru_units=H)
    for name, rows, cols in (("w_ru", prev + H, 2 * H), ("w_c", prev + H, H), ("head", H, act_dim)):
        out[name] = (rows, cols, off, off + rows * cols)
        off += rows * cols + cols
    out["logstd_offset"] = off
    out["policy_count"] = off + act_dim
    v = PM.layout(obs_dim, act_dim, (), value_layers)
    out["value"], out["value_count"] = v["value"], v["value_count"]
    return out


def blocks(lay):
    """Every (in, out, w_offset, b_offset) block of policy_params in the buffer's order."""
    return list(lay["dense"]) + [lay["w_ru"], lay["w_c"], lay["head"]]


def _affine(parts, W, b, dtype):
    """[parts...] W + b with the inputs of `parts` ([n, k] each) taken in order."""
    if dtype == np.float64:
        return np.concatenate(parts, axis=1) @ W + b
    y = np.zeros((parts[0].shape[0], W.shape[1]), dtype=np.float32)
    row = 0
    for p in parts:
        for i in range(p.shape[1]):
            y += p[:, i:i + 1] * W[row][None, :]
            row += 1
    return y + b


def _sigmoid(a, dtype):
    with np.errstate(over="ignore"):
        return dtype(1.0) / (dtype(1.0) + np.exp(-a))


def tick(x0, h, reset, policy_params, lay, dtype=np.float64):
    """One tick from the normalised observation x0 float32 [n, obs_dim] and the state h [n, H]; reset [n] or None.  Returns
    dict(x, h_in, r, u, c, hidden, mean) in `dtype`."""
    (W_ru, b_ru), (W_c, b_c), (W_h, b_h) = PM.split(policy_params, [lay["w_ru"], lay["w_c"], lay["head"]], dtype)
    x = np.asarray(x0, dtype=dtype)
    for W, b in PM.split(policy_params, lay["dense"], dtype):
        y = _affine([x], W, b, dtype)
        x = np.where(y > 0, y, dtype(0))           # rg_bptt.h, F: relu as v > 0 ? v : 0 (a NaN gives 0), as bptt_model.dense_forward
    h = np.asarray(h, dtype=dtype)
    if reset is not None:
        h = np.where(np.asarray(reset)[:, None] != 0, dtype(0), h)
    H = lay["gru_units"]
    ru = _sigmoid(_affine([x, h], W_ru, b_ru, dtype), dtype)
    r, u = ru[:, :H], ru[:, H:]
    c = np.tanh(_affine([x, r * h], W_c, b_c, dtype))
    if dtype == np.float64:
        hn = u * h + (c - u * c)
    else:
        hn = PM.fma32(u, h, PM.fma32(-u, c, c))   # rg_rnn.h: fmaf(u, h, fmaf(-u, c, c))
    mean = np.tanh(_affine([hn], W_h, b_h, dtype))
    return dict(x=x, h_in=h, r=r, u=u, c=c, hidden=hn, mean=mean)


def normalised(obs_cm, norm_state, obs_clip=5.0):
    """obs_cm float32 [obs_dim, n] through the normaliser: float32 [n, obs_dim]."""
    obs_cm = np.asarray(obs_cm)
    on, _ = PM.normalizers_of(norm_state, obs_cm.shape[0], obs_clip)
    return on.transform(obs_cm.T.astype(np.float64)).astype(np.float32)


def act(obs_cm, norm_state, policy_params, value_params, lay, keys, counters, seed, hidden, reset=None, sample=True, obs_clip=5.0, dtype=np.float64):
    """rg_rnn_act.  Returns dict(x, mean, value, hidden, eps, action, logprob, logstd, r, u, c)."""
    x0 = normalised(obs_cm, norm_state, obs_clip)
    B = x0.shape[0]
    t = tick(x0, hidden, reset, policy_params, lay, dtype)
    act_dim = lay["head"][1]
    value = PM.forward(x0, PM.split(value_params, lay["value"], dtype), "linear", dtype)[:, 0]
    off = lay["logstd_offset"]
    logstd = np.asarray(policy_params)[off:off + act_dim].astype(np.float32)
    e = PM.eps_batch(seed, keys, counters, act_dim) if sample else np.zeros((B, act_dim), dtype=np.float32)
    action = t["mean"].astype(np.float64) + np.exp(logstd.astype(np.float64)) * e
    return dict(x=x0, mean=t["mean"], value=value, hidden=t["hidden"], eps=e, action=action, logprob=PM.logprob(e, logstd), logstd=logstd,
                r=t["r"], u=t["u"], c=t["c"])


def unroll(obs, reset, h0, norm_state, policy_params, lay, obs_clip=5.0, dtype=np.float64):
    """rg_rnn_unroll: obs float32 [T, obs_dim, B], reset [T, B], h0 [B, H].  Returns (mean [T, B, act], hidden_seq [T, B, H]) in
    `dtype`; the state is carried in `dtype`."""
    h = np.asarray(h0, dtype=dtype)
    means, states = [], []
    for t in range(len(obs)):
        out = tick(normalised(obs[t], norm_state, obs_clip), h, reset[t], policy_params, lay, dtype)
        h = out["hidden"]
        means.append(out["mean"])
        states.append(h)
    return np.stack(means), np.stack(states)
