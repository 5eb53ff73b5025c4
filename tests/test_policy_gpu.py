"""The PPO agent's kernels (include/rg_policy.h) on the GPU against the float64 numpy model of tests/policy_model.py: act at
batches around the tile and over three configurations, position independence, the normalisers, the returns, the collector
in closed loop with BatchedGoEnv (with and without auto-reset), the update's parameters reaching the kernel with no copy,
and clones.

Tolerance of mean and value.  The kernel sums a neuron's inputs in order in float32 with fused multiply-adds; numpy's
float32 evaluation of the same inputs (PM.forward with dtype float32: the same order, no fusing) differs from the float64
model by a deviation that measures what float32 accumulation costs at these shapes and weights.  The bound is 8 x the
largest such deviation over the inputs of the test (floor 1e-6, a few float32 ulps of the O(1) outputs): it is formed from
the model alone, never from the kernel's output.  Both figures are printed."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import PPO, BatchedGaussianPolicy, RolloutBuffer, collect, play
from robot_gym_amd.core import policy_abi
from tests import policy_model as PM

pytestmark = pytest.mark.gpu

TILE = policy_abi.TILE
SEED = 11
CONFIGS = {
    "default": dict(obs_dim=16, act_dim=2, policy_layers=(200, 100), value_layers=(200, 100)),
    "lopsided": dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2)),      # tells nets, layers and heads apart
    "limits": dict(obs_dim=64, act_dim=4, policy_layers=(256, 256, 256), value_layers=(256, 256, 256)),
}
POOL = 1037   # an odd multi-workgroup batch; the smaller batches are its first robots


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _params(cfg, rng):
    lay = PM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["value_layers"])
    out = {}
    for name in ("policy", "value"):
        p = np.zeros(lay[name + "_count"], dtype=np.float32)
        for i, o, w, b in lay[name]:
            limit = math.sqrt(6.0 / (i + o))
            p[w:w + i * o] = rng.uniform(-limit, limit, i * o)
            p[b:b + o] = rng.normal(0.0, 0.1, o)
        out[name] = p
    out["policy"][lay["logstd_offset"]:] = rng.normal(-1.0, 0.3, cfg["act_dim"])
    return lay, out["policy"], out["value"]


_pools = {}


def pool(name):
    """Per configuration, once: POOL robots (observations with entries beyond the clip, keys, counters), parameters, a
    normaliser state with non-trivial statistics, and the model's answers in float64 and in float32."""
    if name in _pools:
        return _pools[name]
    cfg = CONFIGS[name]
    rng = np.random.default_rng(sorted(CONFIGS).index(name))
    lay, pp, vp = _params(cfg, rng)
    d = cfg["obs_dim"]
    centre, spread = rng.normal(0.3, 1.0, d), rng.uniform(0.2, 2.0, d)
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    for n in (1, 40, 300):
        on.update(centre + spread * rng.normal(size=(n, d)))
        rn.update(rng.normal(0.0, 2.0, size=(n, 1)))
    obs = (centre[:, None] + spread[:, None] * rng.normal(size=(d, POOL)) * 2.5).astype(np.float32)   # 2.5 sigma: a few percent clip
    keys = 1000 + 3 * np.arange(POOL, dtype=np.int64)
    counters = (np.arange(POOL, dtype=np.int64) * 7) % 5
    state = PM.norm_state_of(on, rn)
    m64 = PM.act(obs, state, pp, vp, lay, keys, counters, SEED)
    m32 = PM.act(obs, state, pp, vp, lay, keys, counters, SEED, dtype=np.float32)
    assert np.abs(m64["x"]).max() == 5.0 and (np.abs(m64["x"]) == 5.0).mean() < 0.2
    dev_mean = float(np.abs(m32["mean"].astype(np.float64) - m64["mean"]).max())
    dev_value = float(np.abs(m32["value"].astype(np.float64) - m64["value"]).max())
    _pools[name] = dict(cfg=cfg, lay=lay, pp=pp, vp=vp, state=state, obs=obs, keys=keys, counters=counters, m64=m64, dev_mean=dev_mean,
                        dev_value=dev_value, tol_mean=max(8.0 * dev_mean, 1e-6), tol_value=max(8.0 * dev_value, 1e-6))
    return _pools[name]


def _policy(dev, B, P, idx=None, seed=SEED, **extra):
    """A policy of batch B holding the pool's parameters and normaliser state and the act state of robots idx."""
    idx = np.arange(B) if idx is None else np.asarray(idx)
    pol = BatchedGaussianPolicy(B, seed=seed, device=dev, **P["cfg"], **extra)
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(P["pp"]))
        pol.value_params.copy_(torch.as_tensor(P["vp"]))
    pol.norm_state.copy_(torch.as_tensor(P["state"]))
    pol.act_state.copy_(torch.as_tensor(np.stack((P["keys"][idx], P["counters"][idx]))))
    return pol


def _outs(pol):
    B, A = pol.batch, pol.act_dim
    f = dict(dtype=torch.float32, device=pol.device)
    return dict(action=torch.full((B, A), 7.0, **f), mean=torch.full((B, A), 7.0, **f), value=torch.full((B,), 7.0, **f), logprob=torch.full((B,), 7.0, **f))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---- act against the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, TILE - 1, TILE, TILE + 1, POOL])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_act_matches_the_model(dev, name, B):
    P = pool(name)
    m = P["m64"]
    pol = _policy(dev, B, P)
    obs = torch.as_tensor(np.ascontiguousarray(P["obs"][:, :B]), device=dev)
    got = _np(pol.act(obs, sample=True, out=_outs(pol)))
    err_mean = float(np.abs(got["mean"] - m["mean"][:B]).max())
    err_value = float(np.abs(got["value"] - m["value"][:B]).max())
    print(f"{name} B={B}: float32-numpy vs float64 model mean {P['dev_mean']:.3e} value {P['dev_value']:.3e}; "
          f"kernel vs float64 model mean {err_mean:.3e} value {err_value:.3e}; bounds {P['tol_mean']:.3e} {P['tol_value']:.3e}")
    assert err_mean <= P["tol_mean"] and err_value <= P["tol_value"]
    # eps recovered from the kernel's own float32 outputs: action = fl(mean + fl(expf(logstd) * eps)).  Roundings: the sum
    # (2^-24 |action|), the product (2^-24), expf (two ulps: 2^-22), and the last float32 bit of eps itself where the device's
    # ln / cos round the other way (2^-23); 1 % on top for the second-order terms.
    std = np.exp(m["logstd"].astype(np.float64))
    e = m["eps"][:B].astype(np.float64)
    rec = (got["action"].astype(np.float64) - got["mean"].astype(np.float64)) / std
    bound = 1.01 * (np.abs(e) * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -22) + 2.0 ** -24 * np.abs(got["action"]) / std) + 1e-12
    assert np.all(np.abs(rec - e) <= bound), float(np.max(np.abs(rec - e) / bound))
    assert np.abs(got["logprob"] - m["logprob"][:B]).max() <= 1e-5
    state = pol.act_state.cpu().numpy()
    assert np.array_equal(state[0], P["keys"][:B]) and np.array_equal(state[1], P["counters"][:B] + 1)
    # MEAN mode: the mean itself, eps = 0, the counter untouched
    det = _np(pol.act(obs, sample=False, out=_outs(pol)))
    assert np.array_equal(det["action"], det["mean"]) and np.array_equal(det["mean"], got["mean"]) and np.array_equal(det["value"], got["value"])
    want = np.float32(-np.sum(m["logstd"].astype(np.float64)) - 0.5 * pol.act_dim * PM.LOG_2PI)
    assert np.abs(det["logprob"] - want).max() <= 1e-6
    assert np.array_equal(pol.act_state.cpu().numpy(), state)
    # optional outputs: action alone gives the same action for the same counter
    pol.act_state.copy_(torch.as_tensor(np.stack((P["keys"][:B], P["counters"][:B]))))
    alone = pol.act(obs, sample=True)["action"].cpu().numpy()
    assert np.array_equal(alone, got["action"])
    pol.close()


def test_act_does_not_depend_on_the_robots_place_in_the_batch(dev):
    P = pool("default")
    probe = 5                                  # the pool's robot 5: its observation column, key and counter
    rng = np.random.default_rng(9)
    results = []
    for B, places in ((1, (0,)), (65, (0, 7, 8, 64)), (1037, (0, 519, 1036))):
        for place in places:
            idx = rng.integers(0, POOL, B)     # who else is in the batch changes too
            idx[place] = probe
            pol = _policy(dev, B, P, idx)
            obs = torch.as_tensor(np.ascontiguousarray(P["obs"][:, idx]), device=dev)
            got = _np(pol.act(obs, sample=True, out=_outs(pol)))
            results.append({k: v[place].tobytes() for k, v in got.items()})
            pol.close()
    for r in results[1:]:
        assert r == results[0]


# ---- record against the model -----------------------------------------------------------------------------------------

def _record_run(dev, B, masks, seed, obs_dim=16):
    rng = np.random.default_rng(seed)
    pol = BatchedGaussianPolicy(B, obs_dim=obs_dim, device=dev)
    on, rn = PM.Normalizer(obs_dim), PM.Normalizer(1, False)
    centre = 0.5 + 0.1 * np.arange(obs_dim)
    f32 = dict(dtype=torch.float32, device=dev)
    for mask in masks:
        obs = (centre[:, None] + rng.normal(size=(obs_dim, B))).astype(np.float32)
        reward = rng.normal(-1.0, 3.0, B).astype(np.float32)
        done = rng.integers(0, 2, B).astype(np.int32)
        slots = torch.full((obs_dim, B), 7.0, **f32), torch.full((B,), 7.0, **f32), torch.full((B,), 7, dtype=torch.int32, device=dev)
        m = None if mask is None else torch.as_tensor(np.asarray(mask, dtype=np.int32), device=dev)
        pol.record(torch.as_tensor(obs, device=dev), torch.as_tensor(reward, device=dev), torch.as_tensor(done, device=dev), m, *slots)
        assert np.array_equal(slots[0].cpu().numpy(), obs) and np.array_equal(slots[1].cpu().numpy(), reward)
        assert np.array_equal(slots[2].cpu().numpy(), done)
        sel = np.ones(B, dtype=bool) if mask is None else np.asarray(mask) != 0
        on.update(obs.T[sel])
        rn.update(reward[sel].reshape(-1, 1))
    state = pol.norm_state.cpu().numpy()
    pol.close()
    return state, PM.norm_state_of(on, rn)


def _check_state(got, want):
    got, want = got.reshape(3, -1), want.reshape(3, -1)
    assert np.array_equal(got[0], want[0])                                   # the count is exact
    assert np.allclose(got[1], want[1], rtol=1e-12, atol=0) and np.allclose(got[2], want[2], rtol=1e-12, atol=0)


def test_record_five_ticks_with_changing_masks(dev):
    B = 65
    rng = np.random.default_rng(2)
    masks = [rng.integers(0, 2, B), np.zeros(B, dtype=int), rng.integers(0, 3, B), None, np.eye(1, B, 64, dtype=int)[0]]
    got, want = _record_run(dev, B, masks, seed=3)
    _check_state(got, want)
    assert want.reshape(3, -1)[0, 0] == sum(int((np.asarray(m) != 0).sum()) if m is not None else B for m in masks)
    again, _ = _record_run(dev, B, masks, seed=3)
    assert again.tobytes() == got.tobytes()                                  # two runs: bit-identical


def test_record_a_single_robot_from_the_empty_state(dev):
    got1, want1 = _record_run(dev, 1, [None], seed=4)                        # count becomes 1: the value itself, var_sum 0
    assert got1.reshape(3, -1)[0, 0] == 1 and np.array_equal(got1, want1)
    got2, want2 = _record_run(dev, 1, [None, None], seed=4)                  # count becomes 2
    assert got2.reshape(3, -1)[0, 0] == 2
    _check_state(got2, want2)
    got0, want0 = _record_run(dev, 1, [[0]], seed=4)                         # masked out: the empty state stays
    assert np.array_equal(got0, np.zeros_like(got0)) and np.array_equal(want0, got0)


@pytest.mark.parametrize("B", [1037, 70001])   # several workgroups per column; more robots than 256 workgroups take in one stride
def test_record_over_many_workgroups(dev, B):
    rng = np.random.default_rng(B)
    got, want = _record_run(dev, B, [rng.integers(0, 2, B), None], seed=5, obs_dim=3)
    _check_state(got, want)


# ---- returns against the model ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("bootstrap", [True, False])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
def test_returns_match_the_model(dev, lam, bootstrap):
    rng = np.random.default_rng(7)
    rn = PM.Normalizer(1, False, 10.0)
    rn.update(rng.normal(0.0, 2.0, size=(50, 1)))
    state = PM.norm_state_of(PM.Normalizer(16), rn)
    for B in (1, 65):
        pol = BatchedGaussianPolicy(B, device=dev, gae_lambda=lam)
        pol.norm_state.copy_(torch.as_tensor(state))
        for T in (1, 2, 7):
            patterns = []                       # never; at t = 0; at t = T - 1; twice in a row
            for p in range(4):
                d = np.zeros(T, dtype=np.int32)
                if p == 1:
                    d[0] = 1
                elif p == 2:
                    d[T - 1] = 1
                elif p == 3:
                    d[max(T - 3, 0):max(T - 3, 0) + 2] = 1
                patterns.append(d)
            for first in range(4 if B == 1 else 1):
                done = rng.integers(0, 2, size=(T, B)).astype(np.int32)
                for p in range(min(4, B)):
                    done[:, p] = patterns[(first + p) % 4]
                reward = rng.normal(0.0, 3.0, size=(T, B)).astype(np.float32)
                reward[rng.random((T, B)) < 0.1] = -100.0                    # the task's limit reward: beyond the clip
                value = rng.normal(0.0, 2.0, size=(T, B)).astype(np.float32)
                last = rng.normal(0.0, 2.0, size=B).astype(np.float32)
                ro = RolloutBuffer(T, B, device=dev)
                ro.reward.copy_(torch.as_tensor(reward)), ro.value.copy_(torch.as_tensor(value)), ro.done.copy_(torch.as_tensor(done))
                ro.last_value.copy_(torch.as_tensor(last))
                pol.returns(ro, bootstrap=bootstrap)
                ret, adv = PM.returns(reward, value, done, last, rn, 0.985, lam, bootstrap)
                for got, want in ((ro.ret.cpu().numpy(), ret), (ro.adv.cpu().numpy(), adv)):
                    assert np.all(np.abs(got - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)), (T, B, first)
        pol.close()


# ---- the collector in closed loop ---------------------------------------------------------------------------------------

def _env(dev, batch, **kw):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    return BatchedGoEnv(batch, device=dev, **kw)


def _check_rollout_against_model(pol, ro, state0, masks):
    """Replays the rollout through the model: slot t against the normaliser state of tick t, then the update of that tick."""
    cfg = CONFIGS["default"]
    lay = PM.layout(**cfg)
    pp, vp = pol.policy_params.detach().cpu().numpy(), pol.value_params.detach().cpu().numpy()
    on, rn = PM.normalizers_of(state0, 16)
    T, B = ro.T, ro.batch
    obs, reward, done = ro.obs.cpu().numpy(), ro.reward.cpu().numpy(), ro.done.cpu().numpy()
    got = {k: getattr(ro, k).cpu().numpy() for k in ("action", "mean", "value", "logprob", "ret", "adv", "last_value")}
    keys = np.arange(B)
    worst = dict(mean=0.0, value=0.0, dev_mean=0.0, dev_value=0.0)
    for t in range(T):
        state = PM.norm_state_of(on, rn)
        m64 = PM.act(obs[t], state, pp, vp, lay, keys, np.full(B, t), SEED)
        m32 = PM.act(obs[t], state, pp, vp, lay, keys, np.full(B, t), SEED, dtype=np.float32)
        dev_mean = float(np.abs(m32["mean"] - m64["mean"]).max())
        dev_value = float(np.abs(m32["value"] - m64["value"]).max())
        err_mean, err_value = float(np.abs(got["mean"][t] - m64["mean"]).max()), float(np.abs(got["value"][t] - m64["value"]).max())
        assert err_mean <= max(8 * dev_mean, 1e-6) and err_value <= max(8 * dev_value, 1e-6), (t, err_mean, dev_mean, err_value, dev_value)
        assert np.abs(got["logprob"][t] - m64["logprob"]).max() <= 1e-5
        std = np.exp(m64["logstd"].astype(np.float64))
        rec = (got["action"][t].astype(np.float64) - got["mean"][t]) / std
        e = m64["eps"].astype(np.float64)
        bound = 1.01 * (np.abs(e) * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -22) + 2.0 ** -24 * np.abs(got["action"][t]) / std) + 1e-12
        assert np.all(np.abs(rec - e) <= bound), t
        for k, v in (("mean", err_mean), ("value", err_value), ("dev_mean", dev_mean), ("dev_value", dev_value)):
            worst[k] = max(worst[k], v)
        sel = masks[t] != 0
        on.update(obs[t].T[sel])
        rn.update(reward[t][sel].reshape(-1, 1))
    print("collector: worst kernel error / float32-numpy deviation", worst)
    _check_state(pol.norm_state.cpu().numpy(), PM.norm_state_of(on, rn))
    assert np.array_equal(pol.act_state.cpu().numpy(), np.stack((keys, np.full(B, T))))
    ret, adv = PM.returns(reward, got["value"], done, got["last_value"], rn, 0.985, 1.0, True)
    for g, w in ((got["ret"], ret), (got["adv"], adv)):
        assert np.all(np.abs(g - w) <= 1e-6 * np.maximum(np.abs(w), 1.0))
    assert np.array_equal(ro.logstd.cpu().numpy(), pp[lay["logstd_offset"]:])
    return on, rn


@pytest.mark.parametrize("auto_reset", [True, False])
def test_collector_closed_loop_against_a_twin_and_the_model(dev, auto_reset):
    B, T = 64, 8
    task = dict(max_time=0.45)                   # 45 sub-steps: the time limit ends every episode on tick 5, inside the rollout
    env, twin = _env(dev, B, seed=3, auto_reset=auto_reset, **task), _env(dev, B, seed=3, auto_reset=auto_reset, **task)
    env.reset(), twin.reset()
    pol = BatchedGaussianPolicy(B, seed=SEED, device=dev)
    state0 = pol.norm_state.cpu().numpy().copy()
    ro = collect(env, pol, RolloutBuffer(T, B, device=dev))
    done = ro.done.cpu().numpy()
    assert done.sum() >= B                       # every robot finished inside the rollout
    if auto_reset:
        assert int(env.episode_count.sum()) >= B       # and went on with a new episode
        masks = np.ones((T, B), dtype=np.int32)
    else:
        frozen = np.cumsum(done, axis=0) - done > 0                           # done before the step
        assert frozen.any() and np.all(done[frozen] == 1)
        masks = (~frozen).astype(np.int32)
    assert np.array_equal(ro.mask.cpu().numpy(), masks)
    # the twin, stepped by hand with the recorded actions, reproduces the rollout bit for bit
    for t in range(T):
        assert torch.equal(twin.obs.t(), ro.obs[t]), t
        _, reward, d = twin.step(ro.action[t])
        assert torch.equal(reward, ro.reward[t]) and torch.equal(d, ro.done[t]), t
    assert torch.equal(twin.obs, env.obs)
    last = pol.act(env.obs.t().contiguous(), sample=False, out=dict(value=torch.zeros(B, device=dev)))["value"]
    assert torch.equal(last, ro.last_value)
    _check_rollout_against_model(pol, ro, state0, masks)
    env.close(), twin.close(), pol.close()


def test_update_reaches_the_kernel_with_no_copy(dev):
    B, T = 64, 8
    env = _env(dev, B, seed=5, auto_reset=True, max_time=0.45)
    env.reset()
    pol = BatchedGaussianPolicy(B, seed=SEED, device=dev)
    ro = collect(env, pol, RolloutBuffer(T, B, device=dev))
    obs = ro.obs[T - 1]
    before = _np(pol.act(obs, sample=False, out=_outs(pol)))
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    old = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
    out = PPO(pol, epochs_policy=3, epochs_value=3).update(ro)
    assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
    assert not torch.equal(pol.policy_params.detach(), old[0]) and not torch.equal(pol.value_params.detach(), old[1])
    assert math.isfinite(out["policy_loss_last"]) and math.isfinite(out["value_loss_last"])
    after = _np(pol.act(obs, sample=False, out=_outs(pol)))
    lay = PM.layout(**CONFIGS["default"])
    pp, vp = pol.policy_params.detach().cpu().numpy(), pol.value_params.detach().cpu().numpy()
    state = pol.norm_state.cpu().numpy()
    m64 = PM.act(obs.cpu().numpy(), state, pp, vp, lay, np.arange(B), np.zeros(B), SEED, sample=False)
    m32 = PM.act(obs.cpu().numpy(), state, pp, vp, lay, np.arange(B), np.zeros(B), SEED, sample=False, dtype=np.float32)
    tol_mean = max(8 * float(np.abs(m32["mean"] - m64["mean"]).max()), 1e-6)
    tol_value = max(8 * float(np.abs(m32["value"] - m64["value"]).max()), 1e-6)
    assert np.abs(after["mean"] - m64["mean"]).max() <= tol_mean and np.abs(after["value"] - m64["value"]).max() <= tol_value
    assert np.abs(after["value"] - before["value"]).max() > 10 * tol_value    # the new parameters, not the old ones
    assert np.abs(after["logprob"] - PM.logprob(np.zeros((B, 2)), m64["logstd"])).max() <= 1e-5   # the trained logstd too
    env.close(), pol.close()


def test_a_clone_acts_as_its_source(dev):
    B = 32
    env = _env(dev, B, seed=4, auto_reset=True, max_time=0.45)
    env.reset()
    pol = BatchedGaussianPolicy(B, seed=SEED, device=dev)
    collect(env, pol, RolloutBuffer(3, B, device=dev))
    src = np.arange(16)
    dst = src + 16                              # the same residue modulo 16: bit-identical continuations of the environment
    env.clone(src, dst)
    pol.clone(src, dst)
    assert torch.equal(pol.act_state[:, dst], pol.act_state[:, src]) and pol.act_state[0, dst].tolist() == list(range(16))
    ro = collect(env, pol, RolloutBuffer(3, B, device=dev))
    for name in ("action", "mean", "value", "logprob", "reward", "done"):
        ten = getattr(ro, name)
        assert torch.equal(ten[:, dst], ten[:, src]), name
    assert torch.equal(ro.obs[:, :, dst], ro.obs[:, :, src])
    assert int(ro.done.sum()) > 0               # through a reset
    assert not torch.equal(ro.action[:, :8], ro.action[:, 8:16])              # robots do differ
    env.close(), pol.close()


def test_the_player_is_deterministic_and_draws_no_noise(dev):
    B, TICKS = 16, 6
    totals = []
    for _ in range(2):
        env = _env(dev, B, seed=6, auto_reset=True, max_time=0.45)
        env.reset()
        pol = BatchedGaussianPolicy(B, seed=SEED, device=dev)
        twin = _env(dev, B, seed=6, auto_reset=True, max_time=0.45)
        twin.reset()
        want = torch.zeros(B, device=dev)
        for _ in range(TICKS):                      # by hand: action = mean of the current observation
            out = pol.act(twin.obs.t(), sample=False, out=_outs(pol))
            assert torch.equal(out["action"], out["mean"])
            want += twin.step(out["action"])[1]
        total = play(env, pol, TICKS)
        assert torch.equal(total, want) and torch.equal(env.obs, twin.obs)
        assert int(pol.act_state[1].sum()) == 0     # the counter of the noise stream is untouched
        totals.append(total.cpu().numpy())
        env.close(), twin.close(), pol.close()
    assert np.array_equal(totals[0], totals[1]) and np.abs(totals[0]).max() > 0
