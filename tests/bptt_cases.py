"""The cases of tests/test_bptt_gpu.py, built from the numpy model (tests/bptt_model.py) alone: configurations, shapes, the
rollout of each (configuration, T, B) and the bounds its gradients are held to.  tests/test_bptt_cpu.py builds every one of
them without a GPU and checks the two caps below.

The bound of a gradient is the rule of tests/test_ppo_update_gpu.py, unchanged: per parameter tensor the deviation is
max|g - g64| / max|g64| against the float64 model, the bound max(8 x the float32 model's deviation, 1e-6), the loss relative
to |loss64|; at shapes of at most CHUNK + 1 samples the floor is instead 2^-22 of the tensor's largest sum of |terms| over its
largest entry plus what a forward pass off by +-2^-22 does to the tensor in the float64 model.  Nothing of it comes from a
kernel's output.

Relu crossings: the dense pre-activations depend on the tick's observation alone, so a sample whose float64 pre-activation of
a dense layer lies within 8 x the largest deviation of numpy's float32 pre-activations of that layer is drawn again.

One ulp of the forward pass.  The cutoff term turns an error e of a mean into a relative error of about 2 e / |mu - mu0| of
KL_b - threshold, and with it of the loss and of every tensor, since the robots above the cutoff carry nearly all of both.  A
float32 forward pass is free to be off by an ulp of a mean near 1/2, 2^-24, and free to be off to one side for every robot (a
rounding of the shared cell or head leaves the same trace in every mean).  With the robots above the cutoff a third of a
standard deviation (about 0.1) off the behaviour policy, as in tests/test_ppo_update_gpu.py, such an ulp moves the loss by
2.4e-6 and every tensor by about 2e-6 in the float64 model, at every configuration and shape: twice the 1e-6 floor, so a case
could be met only where numpy's float32 run happened to deviate by more than a quarter of that.  The robots above the
cutoff therefore lie OFF_POLICY = 1.5 standard deviations off, where the same ulp costs 4e-7 (7e-7 at most), and the model
says so for every case (c["ulp_cost"], ULP_CAP: below the floor).  At that distance the cutoff term outweighs the surrogate
by three to four orders of magnitude; the cases "no cutoff" (kl_cutoff_coef = 0, the surrogate and the penalty term of
comparable weight) hold the surrogate's path to the same rule.

Caps: at most one observation in four is ever redrawn (REDRAW_CAP); no tensor's bound exceeds 1e-4 (TOL_CAP); one ulp common
to the means moves no tensor and not the loss by more than the 1e-6 floor in the float64 model (ULP_CAP)."""
import functools
import math

import numpy as np

from robot_gym_amd.core import bptt_abi
from tests import bptt_model as BM
from tests import policy_model as PM
from tests import ppo_update_model as UM
from tests import rnn_model as RM

CHUNK = bptt_abi.CHUNK
FLOOR = 2.0 ** -22
PROJECT_FLOOR = 1e-6
REDRAW_CAP, TOL_CAP, ULP_CAP = 0.25, 1e-4, 1e-6
OFF_POLICY = 1.5            # standard deviations between the behaviour policy and the robots above the cutoff
ULP = 2.0 ** -24
CONFIGS = {      # "default", "lopsided", "limits" and the two-dense configuration of tests/test_rnn_cpu.py
    "default": dict(obs_dim=16, act_dim=2, policy_layers=(200,), gru_units=100, value_layers=(200, 100)),
    "lopsided": dict(obs_dim=6, act_dim=3, policy_layers=(), gru_units=5, value_layers=(7, 3, 2)),
    "two dense": dict(obs_dim=5, act_dim=2, policy_layers=(7, 4), gru_units=3, value_layers=(6,)),
    "limits": dict(obs_dim=64, act_dim=4, policy_layers=(256, 256), gru_units=128, value_layers=(256, 256, 256)),
}
# The configurations of tests/rnn_edges.py.  net() and case() seed a configuration of CONFIGS from its place in sorted(CONFIGS), so
# a new key there would redraw every case above: these have their own table and explicit seeds (EDGE_SEEDS: net, case).
EDGE_CONFIGS = {
    "wave63": dict(obs_dim=16, act_dim=2, policy_layers=(65,), gru_units=63, value_layers=(65,)),       # 2H = 126
    "wave64": dict(obs_dim=15, act_dim=1, policy_layers=(64,), gru_units=64, value_layers=(65,)),       # 2H = 128; 15 inputs: the bias closes the row tile
    "wave65": dict(obs_dim=1, act_dim=4, policy_layers=(63, 65), gru_units=65, value_layers=(65,)),     # 2H = 130: three waves; two dense layers
    "unit1": dict(obs_dim=16, act_dim=2, policy_layers=(65,), gru_units=1, value_layers=(65,)),         # H = 1
    "rows15": dict(obs_dim=15, act_dim=3, policy_layers=(31,), gru_units=16, value_layers=(65,)),       # blocks of 15, 47, 47 and 16 input rows
}
EDGE_SEEDS = {"wave63": (4101, 5101), "wave64": (4102, 5102), "wave65": (4103, 5103), "unit1": (4104, 5104), "rows15": (4105, 5105)}
assert not set(EDGE_CONFIGS) & set(CONFIGS) and set(EDGE_SEEDS) == set(EDGE_CONFIGS)
# one robot; below a tile; one robot past a tile; five tiles with a ragged one; 519 chunks: every group of the W phase folds
# more than one chunk and the last chunk is short
SHAPES = [(1, 1), (3, 5), (2, 9), (5, 37), (8, 1037)]
assert 8 * 1037 % CHUNK != 0 and -(-8 * 1037 // CHUNK) > 2 * bptt_abi.MAX_GROUPS and bptt_abi.groups(8, 1037) * 2 <= -(-8 * 1037 // CHUNK)
GRADIENT_CASES = [(name, T, B) for name in CONFIGS for T, B in SHAPES if name != "limits" or T * B <= 5 * 37]
NO_CUTOFF_CASES = [("default", 5, 37), ("default", 8, 1037), ("two dense", 8, 1037)]      # kl_cutoff_coef = 0 (module docstring)
PPO_KW = dict(kl_init_penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0)
MODEL_KW = dict(penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0)


@functools.lru_cache(maxsize=None)
def net(name):
    """(cfg, layout, policy_params, value_params, norm_state, centre, spread) of a configuration: weights within the Glorot
    limit, non-zero biases, a distinct logstd per component, a normaliser state with non-trivial statistics."""
    cfg = CONFIGS[name] if name in CONFIGS else EDGE_CONFIGS[name]
    rng = np.random.default_rng(1900 + sorted(CONFIGS).index(name) if name in CONFIGS else EDGE_SEEDS[name][0])
    lay = RM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["gru_units"], cfg["value_layers"])
    pp = np.zeros(lay["policy_count"], dtype=np.float32)
    for i, o, w, b in RM.blocks(lay):
        limit = math.sqrt(6.0 / (i + o))
        pp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        pp[b:b + o] = rng.normal(0.0, 0.1, o)
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
    return cfg, lay, pp, vp, PM.norm_state_of(on, rn), centre, spread


def deviation(g, g64, names):
    """{tensor: max|g - g64| / max|g64|}; a tensor whose float64 gradient is all zeros must be all zeros."""
    out = {}
    for k, s in names.items():
        top = float(np.abs(g64[s]).max())
        out[k] = float(np.abs(np.asarray(g, dtype=np.float64)[s] - g64[s]).max()) / top if top > 0 else float(np.abs(g[s]).max())
    return out


def resets(T, B, rng):
    """reset [T, B]: episodes that begin at tick 0, in the middle of the sequence and at its last tick; any non-zero value counts."""
    reset = np.zeros((T, B), dtype=np.int32)
    reset[0, ::2] = 1
    reset[T // 2, 1::3] = 5
    reset[T - 1, 2::5] = -1
    reset[rng.integers(0, T, size=B), np.arange(B)] |= (rng.random(B) < 0.2).astype(np.int32)
    return reset


def saturate(pp, lay, gates):
    """A copy of the policy buffer with the gates' biases moved to where float32 saturates: "hold": the u half of b_ru at +100
    (u == 1.0f, the cell holds its state); "shut": all of b_ru at -100 (expf overflows: r == u == 0.0f, h' = c); None: pp itself."""
    if gates is None:
        return pp
    H, b = lay["gru_units"], lay["w_ru"][3]
    out = np.array(pp)
    if gates == "hold":
        out[b + H:b + 2 * H] = 100.0
    else:
        assert gates == "shut"
        out[b:b + 2 * H] = -100.0
    return out


@functools.lru_cache(maxsize=None)
def case(name, T, B, mask_kind="some", cutoff=True, gates=None):
    """The rollout of (configuration, T, B) and the model's answers, once: inputs as float32 / int32 arrays, the float64 model,
    the float32 model's deviations and the bounds.  Every third robot lies off the behaviour policy by OFF_POLICY
    standard deviations (its KL is above the cutoff), the others by a hundredth.  mask "some": zeros in the mask and, where
    B > 1, the last robot masked throughout; "last": the first robot masked throughout and the last one valid at every tick (the
    last robot of a batch is the one a tile's slots past the batch mirror); "none": an all-zero mask.  cutoff=False: kl_cutoff_coef = 0 (c["ppo_kw"], c["model_kw"]
    are the settings of the case).  gates: saturate() applied to the configuration's parameters before anything is drawn from them."""
    MODEL_KW = dict(globals()["MODEL_KW"], kl_cutoff_coef=1000.0 if cutoff else 0.0)
    cfg, lay, pp, vp, state, centre, spread = net(name)
    pp = saturate(pp, lay, gates)
    d, A, H = cfg["obs_dim"], cfg["act_dim"], cfg["gru_units"]
    rng = np.random.default_rng(2000 * T + B + (7 * sorted(CONFIGS).index(name) if name in CONFIGS else EDGE_SEEDS[name][1]))
    obs = (centre[None, :, None] + spread[None, :, None] * rng.normal(size=(T, d, B)) * 2.5).astype(np.float32)
    margins, redrawn = None, np.zeros(T * B, dtype=bool)
    for _ in range(50):                                   # keep every dense pre-activation away from 0 (module docstring)
        x = BM.normalized_obs(obs, state)
        pre64, pre32 = [], []
        BM.dense_forward(x.reshape(T * B, d), pp, lay, pre=pre64)
        if margins is None:
            BM.dense_forward(x.reshape(T * B, d), pp, lay, np.float32, pre=pre32)
            margins = [8.0 * float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(pre32, pre64)]
        near = np.zeros(T * B, dtype=bool)
        for y, m_ in zip(pre64, margins):
            near |= (np.abs(y) <= m_).any(axis=1)
        if not near.any():
            break
        redrawn |= near
        t_, b_ = np.divmod(np.flatnonzero(near), B)
        obs[t_, :, b_] = (centre + spread * rng.normal(size=(len(t_), d)) * 2.5).astype(np.float32)
    assert not near.any()
    reset = resets(T, B, rng)
    h0 = rng.uniform(-0.9, 0.9, size=(B, H)).astype(np.float32)
    mu = BM.forward(x, reset, h0, pp, lay)["mean"]
    logstd = pp[lay["logstd_offset"]:].astype(np.float64)
    logstd0 = (logstd + rng.normal(0.0, 0.01, A)).astype(np.float32)
    off = 0.01 * rng.normal(size=(T, B, A))
    off[:, ::3] += OFF_POLICY * np.exp(logstd)
    if mask_kind == "last" and (B - 1) % 3 != 0:          # the last robot above the cutoff too: it carries a large part of every tensor
        off[:, B - 1] += OFF_POLICY * np.exp(logstd)
    mean0 = (mu + off).astype(np.float32)
    action = (mean0 + np.exp(logstd0) * rng.normal(size=(T, B, A))).astype(np.float32)
    adv = rng.normal(0.5, 2.0, size=(T, B)).astype(np.float32)
    ret = rng.normal(1.5, 2.0, size=(T, B)).astype(np.float32)
    if mask_kind == "none":
        mask = np.zeros((T, B), dtype=np.int32)
    else:
        mask = rng.choice(np.array([1, 1, 1, 0, -1, 2 ** 31 - 1], dtype=np.int64), size=(T, B)).astype(np.int32)   # everything but 0 selects
        mask[0, 0] = 1
        if B > 1:
            mask[:, B - 1] = 0
        if mask_kind == "last" and B > 1:                 # the first robot masked throughout instead, the last one valid at every tick
            mask[:, 0], mask[:, B - 1] = 0, 1
    c = dict(name=name, T=T, B=B, cfg=cfg, lay=lay, pp=pp, vp=vp, state=state, obs=obs, action=action, mean=mean0, logstd=logstd0, adv=adv, ret=ret,
             mask=mask, reset=reset, h0=h0, x=x, redrawn=float(redrawn.mean()), model_kw=MODEL_KW,
             ppo_kw=dict(PPO_KW, kl_cutoff_coef=MODEL_KW["kl_cutoff_coef"]))
    c["stats"] = UM.adv_stats(adv, mask)
    args = (x, reset, h0, pp, lay, action, mean0, logstd0, adv, mask)
    c["p64"] = BM.policy_grad(*args, **MODEL_KW)
    c["p32"] = BM.policy_grad(*args, dtype=np.float32, **MODEL_KW)
    names, g64, l64 = BM.tensors(lay), c["p64"]["grad"], c["p64"]["loss"]
    rel = lambda a, b: abs(a - b) / abs(b) if b != 0 else abs(a)
    small = T * B <= CHUNK + 1                            # the derived floor is for these shapes alone (module docstring)
    dev32 = deviation(c["p32"]["grad"], g64, names)
    c["p_dev32"], c["p_loss_dev32"] = dev32, rel(c["p32"]["loss"], l64)
    if small:
        shifted = [BM.policy_grad(*args, mean_shift=s, **MODEL_KW) for s in (FLOOR, -FLOOR)]
        forward = [deviation(s["grad"], g64, names) for s in shifted]
        mag = c["p64"]["mag"]
        floor = {k: FLOOR * (float(mag[s].max()) / float(np.abs(g64[s]).max()) if np.abs(g64[s]).max() > 0 else 0.0) + max(f[k] for f in forward)
                 for k, s in names.items()}
        loss_floor = FLOOR + max(rel(s["loss"], l64) for s in shifted)
    else:
        floor, loss_floor = {k: PROJECT_FLOOR for k in names}, PROJECT_FLOOR
    ulp = [BM.policy_grad(*args, mean_shift=s, **MODEL_KW) for s in (ULP, -ULP)]
    c["ulp_cost"] = max(max(max(deviation(s["grad"], g64, names).values()), rel(s["loss"], l64)) for s in ulp)
    c["p_tol"] = {k: max(8.0 * dev32[k], floor[k]) for k in names}
    c["p_loss_tol"] = max(8.0 * c["p_loss_dev32"], loss_floor)
    return c
