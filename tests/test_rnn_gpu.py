"""The recurrent policy's kernels (include/rg_rnn.h) on the GPU against the numpy model of tests/rnn_model.py: act at batches
around the tile over the configurations, in place and out of place, the reset flag, position independence, the unroll
against a chain of acts, the collector in closed loop with BatchedGoEnv, the update's parameters reaching the kernel with
no copy, clones, checkpoints and the player.

Tolerance of mean, value and hidden (the rule of tests/test_policy_gpu.py).  The kernel sums a neuron's inputs in order in
float32 with fused multiply-adds; numpy's float32 evaluation of the same inputs (RM.tick with dtype float32: the same order,
no fusing) differs from the float64 model by a deviation that measures what float32 costs at these shapes and weights.  The
bound is 8 x the largest such deviation over the inputs of the test (for unroll: over all T ticks, the state carried in
each precision), floor 1e-6: it is formed from the model alone, never from the kernel's output.  Both figures are printed."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import (BatchedGaussianPolicy, RecurrentGaussianPolicy, RecurrentPPO, RecurrentRolloutBuffer, collect_recurrent,
                                      play_recurrent)
from robot_gym_amd.core import rnn_abi
from tests import policy_model as PM
from tests import rnn_model as RM

pytestmark = pytest.mark.gpu

TILE = rnn_abi.TILE
SEED = 11
CONFIGS = {
    "default": dict(obs_dim=16, act_dim=2, policy_layers=(200,), gru_units=100, value_layers=(200, 100)),
    "lopsided": dict(obs_dim=6, act_dim=3, policy_layers=(), gru_units=5, value_layers=(7, 3, 2)),      # tells nets, gates and heads apart
    "limits": dict(obs_dim=64, act_dim=4, policy_layers=(256, 256), gru_units=128, value_layers=(256, 256, 256)),
}
for _H in (1, 63, 64, 65):                                                                               # around a wave of gates
    CONFIGS[f"wave{_H}"] = dict(obs_dim=16, act_dim=2, policy_layers=(65,), gru_units=_H, value_layers=(65,))
POOL = 1037   # an odd multi-workgroup batch; the smaller batches are its first robots
T_SEQ = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _lay(cfg):
    return RM.layout(cfg["obs_dim"], cfg["act_dim"], cfg["policy_layers"], cfg["gru_units"], cfg["value_layers"])


def _params(cfg, rng):
    lay = _lay(cfg)
    pp = np.zeros(lay["policy_count"], dtype=np.float32)
    for i, o, w, b in RM.blocks(lay):
        limit = math.sqrt(6.0 / (i + o))
        pp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        pp[b:b + o] = rng.normal(0.0, 0.1, o)
    b_ru = lay["w_ru"][3]
    pp[b_ru:b_ru + 2 * lay["gru_units"]] = rng.normal(0.0, 1.5, 2 * lay["gru_units"])     # gates spread between shut and open
    pp[lay["logstd_offset"]:] = rng.normal(-1.0, 0.3, cfg["act_dim"])
    vp = np.zeros(lay["value_count"], dtype=np.float32)
    for i, o, w, b in lay["value"]:
        limit = math.sqrt(6.0 / (i + o))
        vp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        vp[b:b + o] = rng.normal(0.0, 0.1, o)
    return lay, pp, vp


_pools = {}


def pool(name):
    """Per configuration, once: POOL robots (T_SEQ observations each with entries beyond the clip, a hidden state in (-1, 1), a
    reset flag, keys, counters), parameters, a normaliser state with non-trivial statistics, and the model's answers for the
    first observation in float64 and in float32.  Nothing here is changed afterwards."""
    if name in _pools:
        return _pools[name]
    cfg = CONFIGS[name]
    rng = np.random.default_rng(sorted(CONFIGS).index(name))
    lay, pp, vp = _params(cfg, rng)
    d, H = cfg["obs_dim"], cfg["gru_units"]
    centre, spread = rng.normal(0.3, 1.0, d), rng.uniform(0.2, 2.0, d)
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    for n in (1, 40, 300):
        on.update(centre + spread * rng.normal(size=(n, d)))
        rn.update(rng.normal(0.0, 2.0, size=(n, 1)))
    obs_seq = (centre[None, :, None] + spread[None, :, None] * rng.normal(size=(T_SEQ, d, POOL)) * 2.5).astype(np.float32)   # 2.5 sigma: a few percent clip
    hidden = rng.uniform(-0.95, 0.95, size=(POOL, H)).astype(np.float32)
    reset = (rng.random(POOL) < 0.2).astype(np.int32)
    reset[:4] = (0, 1, 0, 3)                                   # both kinds in the smallest batches; any non-zero value resets
    keys = 1000 + 3 * np.arange(POOL, dtype=np.int64)
    counters = (np.arange(POOL, dtype=np.int64) * 7) % 5
    state = PM.norm_state_of(on, rn)
    obs = obs_seq[0]
    m64 = RM.act(obs, state, pp, vp, lay, keys, counters, SEED, hidden, reset)
    m32 = RM.act(obs, state, pp, vp, lay, keys, counters, SEED, hidden, reset, dtype=np.float32)
    assert np.abs(m64["x"]).max() == 5.0 and 0.0 < (np.abs(m64["x"]) == 5.0).mean() < 0.2
    assert np.abs(hidden).max() < 1.0
    gates = np.concatenate([m64["r"], m64["u"]], axis=1)       # neither all saturated nor all near 1/2
    assert gates.min() < 0.2 and gates.max() > 0.8 and gates.std() > 0.1 and ((gates < 0.01) | (gates > 0.99)).mean() < 0.5
    assert (np.abs(gates - 0.5) < 0.1).mean() < 0.5
    dev_ = {k: float(np.abs(m32[k].astype(np.float64) - m64[k]).max()) for k in ("mean", "value", "hidden")}
    _pools[name] = dict(cfg=cfg, lay=lay, pp=pp, vp=vp, state=state, obs=obs, obs_seq=obs_seq, hidden=hidden, reset=reset, keys=keys, counters=counters,
                        m64=m64, dev=dev_, tol={k: max(8.0 * v, 1e-6) for k, v in dev_.items()})
    return _pools[name]


def _policy(dev, B, P, idx=None, seed=SEED):
    """A policy of batch B holding the pool's parameters and normaliser state, and the act state, hidden rows and reset flags of
    robots idx."""
    idx = np.arange(B) if idx is None else np.asarray(idx)
    pol = RecurrentGaussianPolicy(B, seed=seed, device=dev, **P["cfg"])
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(P["pp"]))
        pol.value_params.copy_(torch.as_tensor(P["vp"]))
    pol.norm_state.copy_(torch.as_tensor(P["state"]))
    pol.act_state.copy_(torch.as_tensor(np.stack((P["keys"][idx], P["counters"][idx]))))
    pol.hidden.copy_(torch.as_tensor(P["hidden"][idx]))
    pol.pending_reset.copy_(torch.as_tensor(P["reset"][idx]))
    return pol


def _outs(pol):
    B, A = pol.batch, pol.act_dim
    f = dict(dtype=torch.float32, device=pol.device)
    return dict(action=torch.full((B, A), 7.0, **f), mean=torch.full((B, A), 7.0, **f), value=torch.full((B,), 7.0, **f), logprob=torch.full((B,), 7.0, **f))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _raw_act(pol, obs, hidden_in, hidden_out, reset, sample, out):
    """rg_rnn_act through the handle, with the state tensors and the reset flags (or None: a NULL pointer) given."""
    pol._rnn.act(obs.data_ptr(), pol.norm_state.data_ptr(), pol.policy_params.data_ptr(), pol.value_params.data_ptr(), pol.act_state.data_ptr(),
                 None if reset is None else reset.data_ptr(), hidden_in.data_ptr(), hidden_out.data_ptr(),
                 rnn_abi.MODE_SAMPLE if sample else rnn_abi.MODE_MEAN, out["action"].data_ptr(), out["mean"].data_ptr(), out["value"].data_ptr(),
                 out["logprob"].data_ptr())
    return out


# ---- act against the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, TILE - 1, TILE, TILE + 1, POOL])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_act_matches_the_model(dev, name, B):
    P = pool(name)
    m = P["m64"]
    pol = _policy(dev, B, P)
    obs = torch.as_tensor(np.ascontiguousarray(P["obs"][:, :B]), device=dev)
    h_in = pol.hidden.clone()
    got = _np(pol.act(obs, sample=True, out=_outs(pol)))
    hidden = pol.hidden.cpu().numpy()
    err = dict(mean=float(np.abs(got["mean"] - m["mean"][:B]).max()), value=float(np.abs(got["value"] - m["value"][:B]).max()),
               hidden=float(np.abs(hidden - m["hidden"][:B]).max()))
    print(f"{name} B={B}: float32-numpy vs float64 model {P['dev']}; kernel vs float64 model {err}; bounds {P['tol']}")
    for k in ("mean", "value", "hidden"):
        assert err[k] <= P["tol"][k], (k, err[k], P["tol"][k])
    assert pol.pending_reset.cpu().numpy().tolist() == [0] * B                 # consumed
    # eps, logprob and the counter, as test_policy_gpu.test_act_matches_the_model holds them
    std = np.exp(m["logstd"].astype(np.float64))
    e = m["eps"][:B].astype(np.float64)
    rec = (got["action"].astype(np.float64) - got["mean"].astype(np.float64)) / std
    bound = 1.01 * (np.abs(e) * (2.0 ** -24 + 2.0 ** -23 + 2.0 ** -22) + 2.0 ** -24 * np.abs(got["action"]) / std) + 1e-12
    assert np.all(np.abs(rec - e) <= bound), float(np.max(np.abs(rec - e) / bound))
    assert np.abs(got["logprob"] - m["logprob"][:B]).max() <= 1e-5
    state = pol.act_state.cpu().numpy()
    assert np.array_equal(state[0], P["keys"][:B]) and np.array_equal(state[1], P["counters"][:B] + 1)
    # out of place from the same inputs: the same bytes as in place, and the input state untouched
    reset = torch.as_tensor(P["reset"][:B], device=dev)
    h_out = torch.full_like(h_in, 7.0)
    keep = h_in.clone()
    pol.act_state.copy_(torch.as_tensor(np.stack((P["keys"][:B], P["counters"][:B]))))
    oop = _np(_raw_act(pol, obs, h_in, h_out, reset, True, _outs(pol)))
    assert torch.equal(h_in, keep) and h_out.cpu().numpy().tobytes() == hidden.tobytes()
    for k in got:
        assert oop[k].tobytes() == got[k].tobytes(), k
    # MEAN mode: the mean itself, eps = 0, the counter untouched
    state = pol.act_state.cpu().numpy()
    det = _np(_raw_act(pol, obs, h_in, h_out, reset, False, _outs(pol)))
    assert np.array_equal(det["action"], det["mean"]) and np.array_equal(det["mean"], got["mean"]) and np.array_equal(det["value"], got["value"])
    want = np.float32(-np.sum(m["logstd"].astype(np.float64)) - 0.5 * pol.act_dim * PM.LOG_2PI)
    assert np.abs(det["logprob"] - want).max() <= 1e-6
    assert np.array_equal(pol.act_state.cpu().numpy(), state)
    # the value is rg_policy_act's bit for bit, on the same value buffer and observations
    cfg = P["cfg"]
    ff = BatchedGaussianPolicy(B, obs_dim=cfg["obs_dim"], act_dim=cfg["act_dim"], policy_layers=(), value_layers=cfg["value_layers"], seed=SEED, device=dev)
    with torch.no_grad():
        ff.value_params.copy_(pol.value_params)
    ff.norm_state.copy_(pol.norm_state)
    v = ff.act(obs, sample=False, out=dict(value=torch.full((B,), 7.0, device=dev)))["value"].cpu().numpy()
    assert v.tobytes() == got["value"].tobytes()
    # optional outputs: action alone gives the same action for the same counter, and advance=False leaves the state alone
    pol.act_state.copy_(torch.as_tensor(np.stack((P["keys"][:B], P["counters"][:B]))))
    pol.hidden.copy_(h_in), pol.pending_reset.copy_(reset)
    alone = pol.act(obs, sample=True, advance=False)["action"].cpu().numpy()
    assert np.array_equal(alone, got["action"]) and torch.equal(pol.hidden, h_in) and torch.equal(pol.pending_reset, reset)
    ff.close(), pol.close()


def test_reset_reads_a_zero_state_and_null_is_no_reset(dev):
    P = pool("default")
    B = 65
    pol = _policy(dev, B, P)
    obs = torch.as_tensor(np.ascontiguousarray(P["obs"][:, :B]), device=dev)
    reset = torch.as_tensor(P["reset"][:B], device=dev)
    assert 0 < int((reset != 0).sum()) < B
    h_in = pol.hidden.clone()

    def run(h, r):
        h_out = torch.full_like(h, 7.0)
        out = _np(_raw_act(pol, obs, h, h_out, r, False, _outs(pol)))
        return dict(out, hidden=h_out.cpu().numpy())
    flagged = run(h_in, reset)
    zeroed = run(torch.where(reset[:, None] != 0, torch.zeros_like(h_in), h_in), torch.zeros_like(reset))
    null = run(h_in, None)
    zeros = run(h_in, torch.zeros_like(reset))
    for k in flagged:
        assert flagged[k].tobytes() == zeroed[k].tobytes(), k
        assert null[k].tobytes() == zeros[k].tobytes(), k
    sel = (reset != 0).cpu().numpy()
    assert np.all(np.abs(flagged["hidden"][sel] - null["hidden"][sel]).max(axis=1) > 0)          # the flag matters where it is set
    assert flagged["hidden"][~sel].tobytes() == null["hidden"][~sel].tobytes()                  # and nowhere else
    pol.close()


def test_act_does_not_depend_on_the_robots_place_in_the_batch(dev):
    P = pool("default")
    probe = 5                                  # the pool's robot 5: its observation column, state, key and counter
    rng = np.random.default_rng(9)
    results = []
    for B, places in ((1, (0,)), (65, (0, 7, 8, 64)), (1037, (0, 519, 1036))):
        for place in places:
            idx = rng.integers(0, POOL, B)     # who else is in the batch changes too
            idx[place] = probe
            pol = _policy(dev, B, P, idx)
            obs = torch.as_tensor(np.ascontiguousarray(P["obs"][:, idx]), device=dev)
            got = _np(pol.act(obs, sample=True, out=_outs(pol)))
            got["hidden"] = pol.hidden.cpu().numpy()
            results.append({k: v[place].tobytes() for k, v in got.items()})
            pol.close()
    assert len(results) == 8
    for r in results[1:]:
        assert r == results[0]


# ---- unroll against a chain of acts -------------------------------------------------------------------------------------

def _sequence(P, B):
    reset = np.zeros((T_SEQ, B), dtype=np.int32)
    b = np.arange(B)
    reset[0, b % 3 == 0] = 1
    reset[2, b % 5 == 1] = 1
    reset[4, b % 7 == 2] = 2
    return np.ascontiguousarray(P["obs_seq"][:, :, :B]), reset


@pytest.mark.parametrize("B", [TILE + 1, POOL])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_unroll_equals_a_chain_of_acts_bit_for_bit(dev, name, B):
    P = pool(name)
    cfg = P["cfg"]
    obs_np, reset_np = _sequence(P, B)
    pol = _policy(dev, B, P)
    ro = RecurrentRolloutBuffer(T_SEQ, B, cfg["obs_dim"], cfg["act_dim"], cfg["gru_units"], device=dev)
    ro.obs.copy_(torch.as_tensor(obs_np)), ro.reset.copy_(torch.as_tensor(reset_np)), ro.h0.copy_(pol.hidden)
    h = pol.hidden.clone()
    means, states = [], []
    for t in range(T_SEQ):                                                    # in place, tick after tick
        out = _raw_act(pol, ro.obs[t], h, h, ro.reset[t], False, _outs(pol))
        means.append(out["mean"].clone()), states.append(h.clone())
    A, H = cfg["act_dim"], cfg["gru_units"]
    full = dict(mean=torch.full((T_SEQ, B, A), 7.0, device=dev), hidden_seq=torch.full((T_SEQ, B, H), 7.0, device=dev),
                hidden_last=torch.full((B, H), 7.0, device=dev))
    pol.unroll(ro, out=full)
    assert torch.equal(full["mean"], torch.stack(means)) and torch.equal(full["hidden_seq"], torch.stack(states))
    assert torch.equal(full["hidden_last"], states[-1]) and torch.equal(ro.h0, pol.hidden)
    # within the bound of the float64 model, the deviation taken over all ticks
    m64, h64 = RM.unroll(obs_np, reset_np, P["hidden"][:B], P["state"], P["pp"], P["lay"])
    m32, h32 = RM.unroll(obs_np, reset_np, P["hidden"][:B], P["state"], P["pp"], P["lay"], dtype=np.float32)
    dev_mean, dev_hidden = float(np.abs(m32 - m64).max()), float(np.abs(h32 - h64).max())
    err_mean, err_hidden = float(np.abs(full["mean"].cpu().numpy() - m64).max()), float(np.abs(full["hidden_seq"].cpu().numpy() - h64).max())
    print(f"{name} B={B} T={T_SEQ}: float32-numpy vs float64 model mean {dev_mean:.3e} hidden {dev_hidden:.3e}; kernel vs float64 model mean "
          f"{err_mean:.3e} hidden {err_hidden:.3e}")
    assert err_mean <= max(8.0 * dev_mean, 1e-6) and err_hidden <= max(8.0 * dev_hidden, 1e-6)
    # the optional outputs are optional: the mean alone, and hidden_last written over h0 itself
    alone = pol.unroll(ro)["mean"]
    assert torch.equal(alone, full["mean"])
    last_only = dict(mean=torch.full((T_SEQ, B, A), 7.0, device=dev), hidden_last=ro.h0)
    pol.unroll(ro, out=last_only)
    assert torch.equal(last_only["mean"], full["mean"]) and torch.equal(ro.h0, states[-1])
    # T = 1
    ro.h0.copy_(pol.hidden)
    one = RecurrentRolloutBuffer(1, B, cfg["obs_dim"], cfg["act_dim"], cfg["gru_units"], device=dev)
    one.obs.copy_(ro.obs[:1]), one.reset.copy_(ro.reset[:1]), one.h0.copy_(ro.h0)
    got = pol.unroll(one, out=dict(hidden_seq=torch.full((1, B, H), 7.0, device=dev)))
    assert torch.equal(got["mean"][0], means[0]) and torch.equal(got["hidden_seq"][0], states[0])
    pol.close()


# ---- the collector in closed loop ---------------------------------------------------------------------------------------

def _env(dev, batch, **kw):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    return BatchedGoEnv(batch, device=dev, **kw)


@pytest.mark.parametrize("auto_reset", [True, False])
def test_collector_closed_loop_against_a_twin(dev, auto_reset):
    B, T = 64, 8
    task = dict(max_time=0.45)                   # 45 sub-steps: the time limit ends every episode on tick 5, inside the rollout
    env, twin = _env(dev, B, seed=3, auto_reset=auto_reset, **task), _env(dev, B, seed=3, auto_reset=auto_reset, **task)
    env.reset(), twin.reset()
    state = torch.as_tensor(pool("default")["state"], device=dev)           # non-trivial statistics, held still (see collect_recurrent)
    pol, pol2 = RecurrentGaussianPolicy(B, seed=SEED, device=dev), RecurrentGaussianPolicy(B, seed=SEED, device=dev)
    pol.norm_state.copy_(state), pol2.norm_state.copy_(state)
    H = pol.gru_units
    first = collect_recurrent(env, pol, RecurrentRolloutBuffer(T, B, device=dev), update_normalizers=False)
    h_after_first = pol.hidden.clone()
    second = collect_recurrent(env, pol, RecurrentRolloutBuffer(T, B, device=dev), update_normalizers=False)
    assert torch.equal(pol.norm_state, state)
    ended = int(first.done.sum())                # counted on the device results
    assert ended >= B, ended                     # every robot's episode ended inside the first rollout
    if auto_reset:
        assert int(env.episode_count.sum()) >= B
        assert int(first.mask.min()) == 1
    else:
        frozen = (torch.cumsum(first.done, 0) - first.done) > 0
        assert bool(frozen.any()) and torch.equal(first.mask, (~frozen).to(torch.int32))
    # the reset contract
    assert torch.equal(first.reset[0], torch.ones(B, dtype=torch.int32, device=dev))          # after env.reset: every robot begins
    assert torch.equal(first.h0, torch.zeros(B, H, device=dev))
    for ro in (first, second):
        assert torch.equal(ro.reset[1:], ro.done[:-1])
    assert torch.equal(second.reset[0], first.done[-1]) and torch.equal(pol.pending_reset, second.done[-1])
    # sequence evaluation reproduces what acting computed, and the second rollout continues the first
    for ro, h_end in ((first, h_after_first), (second, pol.hidden)):
        out = pol.unroll(ro, out=dict(hidden_last=torch.full((B, H), 7.0, device=dev)))
        assert torch.equal(out["mean"], ro.mean) and torch.equal(out["hidden_last"], h_end)
    assert torch.equal(second.h0, h_after_first) and float(second.h0.abs().max()) > 0
    # the bootstrap is a value-only look: the state it leaves is the last tick's (checked above), its value that of the last observation
    last = pol.act(env.obs.t().contiguous(), sample=False, out=dict(value=torch.zeros(B, device=dev)), advance=False)["value"]
    assert torch.equal(last, second.last_value)
    # the twin: the environment stepped by hand with the recorded actions, a second policy acting on the recorded slots
    for ro in (first, second):
        for t in range(T):
            assert torch.equal(twin.obs.t(), ro.obs[t]), t
            pol2.pending_reset.copy_(ro.reset[t])
            out = pol2.act(ro.obs[t], sample=True, out=_outs(pol2))
            for k in ("action", "mean", "value", "logprob"):
                assert torch.equal(out[k], getattr(ro, k)[t]), (k, t)
            _, reward, d = twin.step(ro.action[t])
            assert torch.equal(reward, ro.reward[t]) and torch.equal(d, ro.done[t]), t
    assert torch.equal(twin.obs, env.obs) and torch.equal(pol2.hidden, pol.hidden) and torch.equal(pol2.act_state, pol.act_state)
    assert int(pol.act_state[1].min()) == int(pol.act_state[1].max()) == 2 * T
    env.close(), twin.close(), pol.close(), pol2.close()


def test_update_reaches_the_kernel_with_no_copy(dev):
    B, T = 16, 4
    env = _env(dev, B, seed=5, auto_reset=True, max_time=0.45)
    env.reset()
    pol = RecurrentGaussianPolicy(B, seed=SEED, device=dev)
    ro = collect_recurrent(env, pol, RecurrentRolloutBuffer(T, B, device=dev))
    assert float(pol.norm_state[0]) == T * B                                  # the default: the normalisers follow the rollout
    obs = ro.obs[T - 1]
    h_in = pol.hidden.clone()
    reset = torch.zeros(B, dtype=torch.int32, device=dev)
    before = _np(_raw_act(pol, obs, h_in, torch.empty_like(h_in), reset, False, _outs(pol)))
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    old = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
    out = RecurrentPPO(pol, epochs_policy=2, epochs_value=2).update(ro)
    assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
    changed = pol.policy_params.detach() != old[0]
    for i, o, w, b in RM.blocks(pol.layout):                                  # the cell's blocks too: the gradient went through time
        assert bool(changed[w:w + i * o].any()), (i, o)
    assert not torch.equal(pol.value_params.detach(), old[1])
    assert math.isfinite(out["policy_loss_last"]) and math.isfinite(out["value_loss_last"]) and math.isfinite(out["kl_change"])
    h_out = torch.empty_like(h_in)
    after = _np(_raw_act(pol, obs, h_in, h_out, reset, False, _outs(pol)))
    lay = _lay(CONFIGS["default"])
    pp, vp = pol.policy_params.detach().cpu().numpy(), pol.value_params.detach().cpu().numpy()
    args = (obs.cpu().numpy(), pol.norm_state.cpu().numpy(), pp, vp, lay, np.arange(B), np.zeros(B), SEED, h_in.cpu().numpy(), reset.cpu().numpy())
    m64, m32 = RM.act(*args, sample=False), RM.act(*args, sample=False, dtype=np.float32)
    got = dict(after, hidden=h_out.cpu().numpy())
    for k in ("mean", "value", "hidden"):
        tol = max(8.0 * float(np.abs(m32[k] - m64[k]).max()), 1e-6)
        assert np.abs(got[k] - m64[k]).max() <= tol, k
    tol_value = max(8.0 * float(np.abs(m32["value"] - m64["value"]).max()), 1e-6)
    assert np.abs(after["value"] - before["value"]).max() > 10 * tol_value    # the new parameters, not the old ones
    assert np.abs(after["logprob"] - PM.logprob(np.zeros((B, 2)), m64["logstd"])).max() <= 1e-5   # the trained logstd too
    env.close(), pol.close()


def test_a_clone_acts_as_its_source_and_a_checkpoint_restores_the_next_tick(dev):
    B = 32
    env = _env(dev, B, seed=4, auto_reset=True, max_time=0.45)
    env.reset()
    pol = RecurrentGaussianPolicy(B, seed=SEED, device=dev)
    collect_recurrent(env, pol, RecurrentRolloutBuffer(3, B, device=dev))
    src = np.arange(16)
    dst = src + 16                              # the same residue modulo 16: bit-identical continuations of the environment
    assert not torch.equal(pol.hidden[dst], pol.hidden[src])
    env.clone(src, dst)
    pol.clone(src, dst)
    assert torch.equal(pol.act_state[:, dst], pol.act_state[:, src]) and pol.act_state[0, dst].tolist() == list(range(16))
    assert torch.equal(pol.hidden[dst], pol.hidden[src]) and torch.equal(pol.pending_reset[dst], pol.pending_reset[src])
    ro = collect_recurrent(env, pol, RecurrentRolloutBuffer(3, B, device=dev))
    for name in ("action", "mean", "value", "logprob", "reward", "done", "reset"):
        ten = getattr(ro, name)
        assert torch.equal(ten[:, dst], ten[:, src]), name
    assert torch.equal(ro.obs[:, :, dst], ro.obs[:, :, src]) and torch.equal(pol.hidden[dst], pol.hidden[src])
    assert int(ro.done.sum()) > 0               # through a reset
    assert not torch.equal(ro.action[:, :8], ro.action[:, 8:16])              # robots do differ
    # checkpoint: a second object loaded from the state gives the same next tick
    with torch.no_grad():
        pol.policy_params.mul_(1.03), pol.value_params.mul_(0.97)            # no longer what a fresh object of this seed holds
    other = RecurrentGaussianPolicy(B, seed=SEED, device=dev)                 # the seed of the noise stream is configuration, not state
    assert not torch.equal(other.policy_params, pol.policy_params)
    other.load_state_dict(pol.state_dict())
    obs = env.obs.t().contiguous()
    a, b = pol.act(obs, sample=True, out=_outs(pol)), other.act(obs, sample=True, out=_outs(other))
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(pol.hidden, other.hidden) and torch.equal(pol.act_state, other.act_state)
    assert float(a["action"].abs().max()) > 0 and float(pol.hidden.abs().max()) > 0
    env.close(), pol.close(), other.close()


def test_the_player_is_deterministic_and_draws_no_noise(dev):
    B, TICKS = 16, 6
    totals = []
    for _ in range(2):
        env = _env(dev, B, seed=6, auto_reset=True, max_time=0.45)
        env.reset()
        pol = RecurrentGaussianPolicy(B, seed=SEED, device=dev)
        twin = _env(dev, B, seed=6, auto_reset=True, max_time=0.45)
        twin.reset()
        want = torch.zeros(B, device=dev)
        h = torch.zeros(B, pol.gru_units, device=dev)
        reset = torch.ones(B, dtype=torch.int32, device=dev)
        ends = 0
        for _ in range(TICKS):                      # by hand: action = mean of the current observation, the state reset after a done
            out = _raw_act(pol, twin.obs.t().contiguous(), h, h, reset, False, _outs(pol))
            assert torch.equal(out["action"], out["mean"])
            _, reward, done = twin.step(out["action"])
            reset.copy_(done)
            ends += int(done.sum())
            want += reward
        assert ends > 0                             # the player went through a reset
        total = play_recurrent(env, pol, TICKS)
        assert torch.equal(total, want) and torch.equal(env.obs, twin.obs) and torch.equal(pol.hidden, h)
        assert int(pol.act_state[1].sum()) == 0     # the counter of the noise stream is untouched
        totals.append(total.cpu().numpy())
        env.close(), twin.close(), pol.close()
    assert np.array_equal(totals[0], totals[1]) and np.abs(totals[0]).max() > 0
