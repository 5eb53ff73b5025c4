"""The PPO update on the device (include/rg_ppo.h) on the GPU against the float64 numpy model of tests/ppo_update_model.py:
the gradients of both losses over seven configurations and shapes around the tile, the advantage scalars and the per-robot
KL, exactness where nothing has changed since the rollout, determinism and output bounds, Adam against torch.optim.Adam,
update against the single entries, the penalty's three branches, and two iterations of collect -> update in closed loop.

Tolerance of a gradient.  Per parameter tensor (each W, each b, logstd) the deviation is max|g - g64| / max|g64| against the
float64 model.  The model evaluated in numpy float32 (the networks' forward and backward passes in float32, a neuron's sum
in order without fused multiply-adds; the head in float64, as in the kernels) deviates from float64 by a figure that
measures what float32 costs at these shapes and weights.  The bound is the rule of tests/test_policy_gpu.py:
max(8 x that deviation, 1e-6), formed from the model alone, never from the kernel's output; the losses take it relative to
|loss64|.  That is the whole rule wherever a workgroup sees full tiles: (5, 1037) and (8, 4096).
At the shapes of at most TILE + 1 samples -- (1, 1), (3, 5), (1, 17) -- the float32 model's deviation is a single draw of a
handful of rounding errors, not a measure, and a fixed 1e-6 does not know how the cutoff term amplifies an error of the mean.
There, and only there, the floor is instead 2^-22 of the largest sum of |terms| of the tensor's entries over its largest
entry (the delta entering the backward pass, each product, each partial sum and the final rounding to float32 cost 2^-24 of
the terms' magnitudes: without cancellation this is 2^-22 of the largest entry) plus what a forward pass off by 2^-22 -- four
ulps of a mean or value of size 1 -- does to the tensor in the float64 model: the larger of the two deviations with every mean
(value) shifted by +2^-22 and by -2^-22.  Every figure is printed before it is asserted.

Conditioning.  The returns lie above the values on average (mean 1.5), as after a rollout with an untrained value network.
With returns centred on the values, the bias of a value head and the one weight behind a hidden layer of width 1 are sums of
thousands of terms that cancel to 1e-3 of one term's size; the relative deviation of such an entry measures the cancellation,
in numpy's float32 as in the kernel's, and not the arithmetic under test.

Relu crossings.  The gradient jumps where a hidden pre-activation crosses 0, and a float32 forward pass may land on either
side of a crossing that lies within its own error: one such sample moves a first-layer tensor by 1e-3 of its largest entry,
in numpy's float32 as much as in the kernel's, and says nothing about either.  The observations are therefore drawn so that
no hidden pre-activation of the float64 model lies within 8 x the largest deviation of numpy's float32 pre-activations of
that layer (the project's bound on a forward pass): samples that do are drawn again.  Every evaluation then has the float64
model's relu pattern, and the deviations measure rounding alone.  relu'(0) = 0 in the kernel has a test of its own below,
with a hidden neuron whose pre-activation is exactly 0."""
import functools
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import PPO, BatchedGaussianPolicy, DevicePPO, RolloutBuffer, collect
from robot_gym_amd.core import ppo_abi
from tests import policy_edges as E
from tests import policy_model as PM
from tests import ppo_update_model as UM

pytestmark = pytest.mark.gpu

TILE = ppo_abi.TILE
FLOOR = 2.0 ** -22
CONFIGS = {
    "default": dict(obs_dim=16, act_dim=2, policy_layers=(200, 100), value_layers=(200, 100)),
    "lopsided": dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2)),
    "limits": dict(obs_dim=64, act_dim=4, policy_layers=(256, 256, 256), value_layers=(256, 256, 256)),
    **E.CONFIGS,
}
# below one tile; one sample below and one above a tile; several workgroups with a ragged tail and more tiles (325) than the 256
# workgroups walk once
SHAPES = [(1, 1), (3, 5), (1, TILE + 1), (5, 1037)]
# 2048 tiles: every workgroup folds eight tiles into its slab in float32
LONG = [("lopsided", 8, 4096), ("policy_deeper", 8, 4096)]
PROJECT_FLOOR = 1e-6
assert 3 * 5 == TILE - 1 and -(-5 * 1037 // TILE) > ppo_abi.MAX_GROUPS
PPO_KW = dict(kl_init_penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0)
MODEL_KW = dict(penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2.0, kl_cutoff_coef=1000.0)
SLOTS = ("obs", "action", "mean", "logstd", "adv", "ret", "mask")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def net(name):
    """(cfg, layout, policy_params, value_params, norm_state, centre, spread) of a configuration: weights within the Glorot
    limit, non-zero biases, a distinct logstd per component, a normaliser state with non-trivial statistics."""
    cfg = CONFIGS[name]
    rng = np.random.default_rng(900 + sorted(CONFIGS).index(name))
    lay = PM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["value_layers"])
    out = {}
    for which in ("policy", "value"):
        p = np.zeros(lay[which + "_count"], dtype=np.float32)
        for i, o, w, b in lay[which]:
            limit = math.sqrt(6.0 / (i + o))
            p[w:w + i * o] = rng.uniform(-limit, limit, i * o)
            p[b:b + o] = rng.normal(0.0, 0.1, o)
        out[which] = p
    out["policy"][lay["logstd_offset"]:] = -1.0 + 0.2 * np.arange(cfg["act_dim"]) + rng.normal(0.0, 0.05, cfg["act_dim"])
    d = cfg["obs_dim"]
    centre, spread = rng.normal(0.3, 1.0, d), rng.uniform(0.2, 2.0, d)
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    for n in (1, 40, 300):
        on.update(centre + spread * rng.normal(size=(n, d)))
        rn.update(rng.normal(0.0, 2.0, size=(n, 1)))
    return cfg, lay, out["policy"], out["value"], PM.norm_state_of(on, rn), centre, spread


def _tensors(lay, which):
    return UM.tensors(lay["policy"], lay["logstd_offset"], lay["policy_count"]) if which == "policy" else UM.tensors(lay["value"])


def _deviation(g, g64, names):
    """{tensor: max|g - g64| / max|g64|}; a tensor whose float64 gradient is all zeros must be all zeros."""
    out = {}
    for k, s in names.items():
        top = float(np.abs(g64[s]).max())
        out[k] = float(np.abs(np.asarray(g, dtype=np.float64)[s] - g64[s]).max()) / top if top > 0 else float(np.abs(g[s]).max())
    return out


@functools.lru_cache(maxsize=None)
def case(name, T, B, mask_kind="some"):
    """The rollout of (configuration, T, B) and the model's answers, once: inputs as float32 / int32 arrays, the float64 model,
    and the float32 model's deviations (the yardstick).  Every third robot lies off the behaviour policy by about a third of a
    standard deviation (its KL is above the cutoff), the others by a hundredth.  mask "some": zeros in the mask and, where
    B > 1, the last robot masked throughout; "none": an all-zero mask."""
    cfg, lay, pp, vp, state, centre, spread = net(name)
    d, A = cfg["obs_dim"], cfg["act_dim"]
    rng = np.random.default_rng(1000 * T + B + 7 * sorted(CONFIGS).index(name))
    obs = (centre[None, :, None] + spread[None, :, None] * rng.normal(size=(T, d, B)) * 2.5).astype(np.float32)
    nets = [(PM.split(p, lay[w]), PM.split(p, lay[w], np.float32), h) for p, w, h in ((pp, "policy", "tanh"), (vp, "value", "linear"))]
    margins = None
    for _ in range(50):                                   # keep every hidden pre-activation away from 0 (module docstring)
        x = UM.normalized_obs(obs, state)
        pre64 = [[] for _ in nets]
        for (l64, _, head), out in zip(nets, pre64):
            UM.forward_all(x, l64, head, pre=out)
        if margins is None:
            margins = []
            for (_, l32, head), p64 in zip(nets, pre64):
                p32 = []
                UM.forward_all(x, l32, head, np.float32, pre=p32)
                margins.append([8.0 * float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(p32, p64)])
        near = np.zeros(T * B, dtype=bool)
        for p64, mg in zip(pre64, margins):
            for y, m_ in zip(p64[:-1], mg[:-1]):            # the hidden layers; the heads have no relu
                near |= (np.abs(y) <= m_).any(axis=1)
        if not near.any():
            break
        t_, b_ = np.divmod(np.flatnonzero(near), B)
        obs[t_, :, b_] = (centre + spread * rng.normal(size=(len(t_), d)) * 2.5).astype(np.float32)
    assert not near.any()
    mu = UM.forward_all(x, PM.split(pp, lay["policy"]), "tanh")[-1].reshape(T, B, A)
    logstd = pp[lay["logstd_offset"]:].astype(np.float64)
    logstd0 = (logstd + rng.normal(0.0, 0.01, A)).astype(np.float32)
    off = 0.01 * rng.normal(size=(T, B, A))
    off[:, ::3] += 0.3 * np.exp(logstd)
    mean0 = (mu + off).astype(np.float32)
    action = (mean0 + np.exp(logstd0) * rng.normal(size=(T, B, A))).astype(np.float32)
    adv = rng.normal(0.5, 2.0, size=(T, B)).astype(np.float32)
    ret = rng.normal(1.5, 2.0, size=(T, B)).astype(np.float32)        # above the values on average (module docstring)
    if mask_kind == "none":
        mask = np.zeros((T, B), dtype=np.int32)
    else:
        mask = rng.choice(np.array([1, 1, 1, 0, -1, 2 ** 31 - 1], dtype=np.int64), size=(T, B)).astype(np.int32)   # everything but 0 selects
        mask[0, 0] = 1
        if B > 1:
            mask[:, B - 1] = 0
    c = dict(name=name, T=T, B=B, cfg=cfg, lay=lay, pp=pp, vp=vp, state=state, obs=obs, action=action, mean=mean0, logstd=logstd0, adv=adv, ret=ret,
             mask=mask, x=x)
    c["stats"] = UM.adv_stats(adv, mask)
    for dtype, key in ((np.float64, "64"), (np.float32, "32")):
        c["p" + key] = UM.policy_grad(x, pp, lay, action, mean0, logstd0, adv, mask, T, B, dtype=dtype, **MODEL_KW)
        c["v" + key] = UM.value_grad(x, vp, lay, ret, mask, T, B, dtype=dtype)
    shifted = dict(p=[UM.policy_grad(x, pp, lay, action, mean0, logstd0, adv, mask, T, B, mean_shift=s, **MODEL_KW) for s in (FLOOR, -FLOOR)],
                   v=[UM.value_grad(x, vp, lay, ret, mask, T, B, value_shift=s) for s in (FLOOR, -FLOOR)])
    rel = lambda a, b: abs(a - b) / abs(b) if b != 0 else abs(a)
    small = T * B <= TILE + 1                             # the derived floor is for these shapes alone (module docstring)
    for which, key in (("policy", "p"), ("value", "v")):
        names, g64, l64 = _tensors(lay, which), c[key + "64"]["grad"], c[key + "64"]["loss"]
        dev32 = _deviation(c[key + "32"]["grad"], g64, names)
        forward = [_deviation(s["grad"], g64, names) for s in shifted[key]]
        c[key + "_dev32"] = dev32
        mag = c[key + "64"]["mag"]
        c[key + "_floor"] = {k: FLOOR * (float(mag[s].max()) / float(np.abs(g64[s]).max()) if np.abs(g64[s]).max() > 0 else 0.0) + max(f[k] for f in forward)
                             for k, s in names.items()}
        c[key + "_tol"] = {k: max(8.0 * dev32[k], c[key + "_floor"][k] if small else PROJECT_FLOOR) for k in names}
        c[key + "_loss_dev32"] = rel(c[key + "32"]["loss"], l64)
        c[key + "_loss_tol"] = max(8.0 * c[key + "_loss_dev32"], FLOOR + max(rel(s["loss"], l64) for s in shifted[key]) if small else PROJECT_FLOOR)
    return c


def _policy(dev, c):
    pol = BatchedGaussianPolicy(c["B"], seed=11, device=dev, **c["cfg"])
    assert pol.layout == c["lay"]
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(c["pp"]))
        pol.value_params.copy_(torch.as_tensor(c["vp"]))
    pol.norm_state.copy_(torch.as_tensor(c["state"]))
    return pol


def _rollout(dev, c):
    cfg = c["cfg"]
    ro = RolloutBuffer(c["T"], c["B"], cfg["obs_dim"], cfg["act_dim"], device=dev)
    for s in SLOTS:
        getattr(ro, s).copy_(torch.as_tensor(np.array(c[s])))
    return ro


def _kernel_means(pol, ro):
    """The float32 means of rg_policy_act over the rollout's observations: [T * B, act_dim]."""
    out = torch.zeros(ro.T, ro.batch, pol.act_dim, dtype=torch.float32, device=pol.device)
    scratch = torch.zeros(ro.batch, pol.act_dim, dtype=torch.float32, device=pol.device)
    for t in range(ro.T):
        pol.act(ro.obs[t], sample=False, out=dict(action=scratch, mean=out[t]))
    return out.cpu().numpy().reshape(ro.T * ro.batch, -1)


# ---- gradients, losses, KL and the advantage scalars against the model ---------------------------------------------------

@pytest.mark.parametrize("name,T,B", [(name, T, B) for name in CONFIGS for T, B in SHAPES] + LONG)
def test_gradients_match_the_model(dev, name, T, B):
    c = case(name, T, B)
    lay = c["lay"]
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DevicePPO(pol, T, **PPO_KW)
    upd.prepare(ro)
    n, m, sd = c["stats"]
    got = upd.adv_stats().cpu().numpy()
    assert got[0] == n and got[3] == int((c["mask"] != 0).sum())
    assert math.isclose(got[1], m, rel_tol=1e-12, abs_tol=1e-15) and math.isclose(got[2], sd, rel_tol=1e-12)
    grad, loss = upd.policy_grad(ro)
    grad, loss = grad.cpu().numpy(), float(loss)
    p64 = c["p64"]
    if B > 1:
        assert p64["over"].any() and not p64["over"].all() and p64["kl"][B - 1] == 0.0
    err = _deviation(grad, p64["grad"], _tensors(lay, "policy"))
    loss_err = abs(loss - p64["loss"]) / abs(p64["loss"])
    print(f"{name} T={T} B={B} policy: float32-numpy vs float64 {c['p_dev32']} loss {c['p_loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
          f"bounds {c['p_tol']} loss {c['p_loss_tol']:.3e}")
    for k, e in err.items():
        assert e <= c["p_tol"][k], (k, e, c["p_tol"][k])
    assert loss_err <= c["p_loss_tol"]
    # the per-robot KL in float64 from the kernel's own float32 means
    kl = upd.kl(ro).cpu().numpy()
    head = UM.policy_head(_kernel_means(pol, ro), c["pp"][lay["logstd_offset"]:], c["action"], c["mean"], c["logstd"],
                          (c["adv"].astype(np.float64) - m) / sd, c["mask"], T, B, **MODEL_KW)
    assert np.allclose(kl, head["kl"], rtol=1e-6, atol=0) and np.all(kl[head["kl"] == 0.0] == 0.0)
    assert math.isclose(loss, head["loss"], rel_tol=1e-9)                       # and the loss from those means: float64 sums, another order
    vgrad, vloss = upd.value_grad(ro)
    vgrad, vloss = vgrad.cpu().numpy(), float(vloss)
    v64 = c["v64"]
    verr = _deviation(vgrad, v64["grad"], _tensors(lay, "value"))
    vloss_err = abs(vloss - v64["loss"]) / abs(v64["loss"]) if v64["loss"] != 0 else abs(vloss)
    print(f"{name} T={T} B={B} value: float32-numpy vs float64 {c['v_dev32']} loss {c['v_loss_dev32']:.3e}; kernel vs float64 {verr} loss {vloss_err:.3e}; "
          f"bounds {c['v_tol']} loss {c['v_loss_tol']:.3e}")
    for k, e in verr.items():
        assert e <= c["v_tol"][k], (k, e, c["v_tol"][k])
    assert vloss_err <= c["v_loss_tol"]
    assert upd.steps.tolist() == [0, 0] and float(upd.penalty) == 0.7           # the gradient entries move no state
    upd.close(), pol.close()


DEAD = 2          # the hidden neuron of each network's first layer whose weights and bias are 0


def test_a_pre_activation_of_exactly_zero_passes_no_gradient(dev):
    """relu'(0) = 0 in the kernel: neuron DEAD of the first hidden layer of both networks has zero weights and a zero bias, so
    its pre-activation is exactly 0 for every sample.  Nothing may reach its weights, its bias or the row of the next layer it
    feeds -- a mask of x >= 0 instead of x > 0 would put the full delta on its bias; everything else is the model's."""
    c = dict(case("lopsided", 5, 1037))
    lay, T, B = c["lay"], c["T"], c["B"]
    params = {}
    for which, key in (("policy", "pp"), ("value", "vp")):
        p = c[key].copy()
        (i0, o0, w0, b0), (i1, o1, w1, _) = lay[which][0], lay[which][1]
        p[w0:w0 + i0 * o0].reshape(i0, o0)[:, DEAD] = 0.0
        p[b0 + DEAD] = 0.0
        params[which] = c[key] = p
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DevicePPO(pol, T, **PPO_KW)
    upd.prepare(ro)
    grads = dict(policy=upd.policy_grad(ro)[0].cpu().numpy(), value=upd.value_grad(ro)[0].cpu().numpy())
    want = dict(policy=UM.policy_grad(c["x"], params["policy"], lay, c["action"], c["mean"], c["logstd"], c["adv"], c["mask"], T, B, **MODEL_KW)["grad"],
                value=UM.value_grad(c["x"], params["value"], lay, c["ret"], c["mask"], T, B)["grad"])
    for which in ("policy", "value"):
        g, g64 = grads[which], want[which]
        (i0, o0, w0, b0), (i1, o1, w1, _) = lay[which][0], lay[which][1]
        for arr in (g, g64):
            W0, W1 = arr[w0:w0 + i0 * o0].reshape(i0, o0), arr[w1:w1 + i1 * o1].reshape(i1, o1)
            assert np.all(W0[:, DEAD] == 0.0) and arr[b0 + DEAD] == 0.0 and np.all(W1[DEAD] == 0.0), which
        live = np.delete(np.arange(o0), DEAD)
        assert np.all(np.abs(g[w0:w0 + i0 * o0].reshape(i0, o0)[:, live]).max(axis=0) > 0) and np.all(g[b0 + live] != 0.0)
        # the rest against the model: a sanity bound (the rule itself is test_gradients_match_the_model's), far below the
        # O(1) deviation a full delta on a dead neuron's bias would be
        names = _tensors(lay, which)
        err = _deviation(g, g64, names)
        print(f"dead neuron, {which}: kernel vs float64 {err}")
        assert max(err.values()) <= 1e-4
    upd.close(), pol.close()


@pytest.mark.parametrize("name,T,B", [("default", 3, 5), ("lopsided", 5, 1037), ("limits", 1, TILE + 1)])
def test_an_all_zero_mask_gives_exactly_zero_gradients(dev, name, T, B):
    c = case(name, T, B, "none")
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DevicePPO(pol, T, **PPO_KW)
    upd.prepare(ro)
    assert upd.adv_stats().cpu().tolist() == [1.0, 0.0, 1e-8, 0.0]               # n = 0: the count clamps to 1
    grad, loss = upd.policy_grad(ro)
    assert float(grad.abs().max()) == 0.0 and float(loss) == 0.0
    assert float(upd.kl(ro).abs().max()) == 0.0
    vgrad, vloss = upd.value_grad(ro)
    assert float(vgrad.abs().max()) == 0.0 and float(vloss) == 0.0
    assert c["p64"]["loss"] == 0.0 and np.abs(c["p64"]["grad"]).max() == 0.0 and np.abs(c["v64"]["grad"]).max() == 0.0
    upd.close(), pol.close()


# ---- exactness ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["default", "wave_edges"])
def test_nothing_changed_since_the_rollout_gives_ratio_one_and_kl_zero(dev, name):
    """The rollout's means come from rg_policy_act; parameters and normaliser are left as they were.  The update's forward pass
    then reproduces those means to the bit: the per-robot KL is exactly 0 and the ratio exactly 1, so the loss is
    -sum(advn * valid) / (T * B).  37 robots over 3 ticks put a robot at every place of a 16-sample tile."""
    T, B = 3, 37
    c = case(name, T, B)
    pol, ro = _policy(dev, c), _rollout(dev, c)
    for t in range(T):
        pol.act(ro.obs[t], sample=True, out=dict(action=ro.action[t], mean=ro.mean[t]))
    ro.logstd.copy_(pol.logstd.detach())
    upd = DevicePPO(pol, T, **PPO_KW)
    upd.prepare(ro)
    kl = upd.kl(ro).cpu().numpy()
    assert kl.shape == (B,) and np.all(kl == 0.0)
    _, loss = upd.policy_grad(ro)
    n, m, sd = c["stats"]
    advn = (c["adv"].astype(np.float64) - m) / sd
    head = UM.policy_head(ro.mean.cpu().numpy().reshape(T * B, -1), c["pp"][c["lay"]["logstd_offset"]:], ro.action.cpu().numpy(), ro.mean.cpu().numpy(),
                          ro.logstd.cpu().numpy(), advn, c["mask"], T, B, **MODEL_KW)
    valid = c["mask"] != 0
    assert np.all(head["ratio"] == 1.0) and np.all(head["kl"] == 0.0)
    want = -np.sum(advn[valid]) / (T * B)
    assert math.isclose(head["loss"], want, rel_tol=1e-13, abs_tol=1e-15)
    assert math.isclose(float(loss), want, rel_tol=1e-12, abs_tol=1e-15)
    upd.close(), pol.close()


# ---- determinism and bounds -------------------------------------------------------------------------------------------------

GUARD = 64
F_SENTINEL = -7.25


def _guarded(n, dtype, dev):
    big = torch.full((n + 2 * GUARD,), F_SENTINEL, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + n]


def _bands_intact(big):
    a = big.cpu().numpy()
    assert np.all(a[:GUARD] == F_SENTINEL) and np.all(a[-GUARD:] == F_SENTINEL)
    assert not np.any(a[GUARD:-GUARD] == F_SENTINEL)           # and the slice itself was filled


@pytest.mark.parametrize("name,T,B", [("lopsided", 3, 5), ("default", 5, 1037)])
def test_two_calls_and_another_stream_give_the_same_bytes_within_the_outputs(dev, name, T, B):
    c = case(name, T, B)
    lay = c["lay"]
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DevicePPO(pol, T, epochs_policy=2, epochs_value=2, **PPO_KW)
    f32, f64 = torch.float32, torch.float64

    def run():
        upd.prepare(ro)
        big_g, g = _guarded(lay["policy_count"], f32, dev)
        big_v, v = _guarded(lay["value_count"], f32, dev)
        big_k, k = _guarded(B, f64, dev)
        _, loss = upd.policy_grad(ro, out=g)
        loss = loss.clone()
        _, vloss = upd.value_grad(ro, out=v)
        upd.kl(ro, out=k)
        torch.cuda.synchronize()
        for big in (big_g, big_v, big_k):
            _bands_intact(big)
        return [t.cpu().numpy().tobytes() for t in (g, v, k, loss, vloss.clone())]

    first = run()
    assert run() == first
    upd.workspace.fill_(float("nan"))                              # nothing is carried in the workspace between calls
    assert run() == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert third == first
    # the whole update: stats within its bounds, the same bytes from the same start
    start = (pol.policy_params.detach().clone(), pol.value_params.detach().clone(), upd.opt_state.clone())
    results = []
    for _ in range(2):
        with torch.no_grad():
            pol.policy_params.copy_(start[0]), pol.value_params.copy_(start[1])
        upd.opt_state.copy_(start[2])
        big_s, upd.stats = _guarded(ppo_abi.STATS, f64, dev)
        upd.update(ro)
        torch.cuda.synchronize()
        _bands_intact(big_s)
        results.append([t.detach().cpu().numpy().tobytes() for t in (pol.policy_params, pol.value_params, upd.opt_state, upd.stats)])
    assert results[0] == results[1]
    assert upd.steps.tolist() == [2, 2]
    upd.close(), pol.close()


# ---- Adam ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 3])
def test_adam_agrees_with_torch_on_the_gpu(dev, steps):
    c = case("lopsided", 3, 5)
    pol = _policy(dev, c)
    upd = DevicePPO(pol, 3, policy_lr=1e-4, value_lr=3e-4)
    rng = np.random.default_rng(steps)
    for which, buf, lr in (("policy", pol.policy_params, 1e-4), ("value", pol.value_params, 3e-4)):
        n = buf.numel()
        twin = buf.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([twin], lr=lr)
        for k in range(steps):
            g = rng.normal(size=n) * np.logspace(-3, 1, n)
            g[::5] = 0.0
            g[1::5] = 1e-12 * np.sign(g[1::5])
            g = torch.as_tensor(g.astype(np.float32), device=dev)
            twin.grad = g.clone()
            opt.step()
            upd.adam(which, g)
        got, want = buf.detach().cpu().numpy().astype(np.float64), twin.detach().cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        bound = np.maximum(4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 1e-9)
        print(f"adam {which} {steps} step(s): worst |p - p_torch| {err.max():.3e}, worst ratio to its bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
        assert np.abs(got - c["pp" if which == "policy" else "vp"]).max() > 1e-5          # it stepped
    assert upd.steps.tolist() == [steps, steps]
    pc = c["lay"]["policy_count"]
    m = upd.moments[:pc].cpu().numpy()
    assert np.all(np.isfinite(upd.moments.cpu().numpy())) and np.abs(m).max() > 0
    upd.close(), pol.close()


# ---- update is the composition of the single entries ------------------------------------------------------------------------

def test_update_equals_the_single_entries_called_in_order(dev):
    c = case("lopsided", 5, 1037)
    T = c["T"]
    ro = _rollout(dev, c)
    pol_a, pol_b = _policy(dev, c), _policy(dev, c)
    kw = dict(epochs_policy=3, epochs_value=3, **PPO_KW)
    a, b = DevicePPO(pol_a, T, **kw), DevicePPO(pol_b, T, **kw)
    stats = a.update(ro).cpu().numpy()
    b.prepare(ro)
    losses = []
    for which, fn in (("policy", b.policy_grad), ("value", b.value_grad)):
        for _ in range(3):
            grad, loss = fn(ro)
            losses.append(float(loss))
            b.adam(which, grad)
    kl = b.kl(ro).cpu().numpy()
    assert torch.equal(pol_a.policy_params.detach(), pol_b.policy_params.detach()) and torch.equal(pol_a.value_params.detach(), pol_b.value_params.detach())
    assert not np.array_equal(pol_a.policy_params.detach().cpu().numpy(), c["pp"])
    assert a.steps.tolist() == b.steps.tolist() == [3, 3] and torch.equal(a.moments, b.moments)
    assert stats[:4].tolist() == [losses[0], losses[2], losses[3], losses[5]]
    assert math.isclose(stats[4], kl.mean(), rel_tol=1e-12)
    assert stats[5] == UM.move_penalty(0.7, stats[4], 1e-2) == float(a.penalty)
    assert a.stats_dict() == dict(zip(ppo_abi.STAT_NAMES, stats.tolist()))
    # save / restore copies into the same tensor
    state = a.state_dict()
    ptr = a.opt_state.data_ptr()
    a.opt_state.zero_()
    a.load_state_dict(state)
    assert a.opt_state.data_ptr() == ptr and a.steps.tolist() == [3, 3] and float(a.penalty) == stats[5]
    a.close(), b.close(), pol_a.close(), pol_b.close()


@pytest.mark.parametrize("scale,factor", [(0.5, 1.5), (2.0, 1 / 1.5), (1.0, 1.0)])
def test_penalty_moves_as_the_model_says(dev, scale, factor):
    """With no epochs the KL change is the rollout's own KL; kl_target = scale x that puts it above 1.3 x the target, below
    0.7 x, or between them."""
    c = case("default", 3, 5)
    pol, ro = _policy(dev, c), _rollout(dev, c)
    change = float(np.mean(c["p64"]["kl"]))
    assert change > 0
    upd = DevicePPO(pol, 3, epochs_policy=0, epochs_value=0, kl_target=scale * change, kl_init_penalty=2.0)
    out = upd.update(ro).cpu().numpy()
    assert math.isclose(out[4], change, rel_tol=1e-4)
    assert out[5] == UM.move_penalty(2.0, out[4], scale * change) == 2.0 * factor == float(upd.penalty)
    d = upd.stats_dict()
    assert d["policy_loss_first"] is None and d["value_loss_last"] is None and d["penalty"] == 2.0 * factor
    assert np.array_equal(pol.policy_params.detach().cpu().numpy(), c["pp"]) and upd.steps.tolist() == [0, 0]
    upd.close(), pol.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------

def test_two_iterations_of_collect_and_update(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    B, T = 64, 8
    env = BatchedGoEnv(B, device=dev, seed=5, auto_reset=True, max_time=0.45)
    env.reset()
    pol = BatchedGaussianPolicy(B, seed=11, device=dev)
    ro = RolloutBuffer(T, B, device=dev)
    upd = DevicePPO(pol, T, epochs_policy=10, epochs_value=10)
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    for it in range(2):
        collect(env, pol, ro)
        old = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
        obs = ro.obs[T - 1]
        f = dict(dtype=torch.float32, device=dev)
        before = pol.act(obs, sample=False, out=dict(action=torch.zeros(B, 2, **f), value=torch.zeros(B, **f)))
        stats = upd.update(ro)
        assert stats is upd.stats and stats.is_cuda
        d = upd.stats_dict()
        print(f"iteration {it}: {d}")
        assert all(math.isfinite(v) for v in d.values())
        assert d["value_loss_last"] < d["value_loss_first"]
        assert bool(torch.isfinite(pol.policy_params).all()) and bool(torch.isfinite(pol.value_params).all())
        assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
        assert not torch.equal(pol.policy_params.detach(), old[0]) and not torch.equal(pol.value_params.detach(), old[1])
        after = pol.act(obs, sample=False, out=dict(action=torch.zeros(B, 2, **f), value=torch.zeros(B, **f)))
        assert not torch.equal(after["value"], before["value"]) and not torch.equal(after["action"], before["action"])   # the new parameters, no copy
        assert upd.steps.tolist() == [10 * (it + 1)] * 2
    env.close(), upd.close(), pol.close()
