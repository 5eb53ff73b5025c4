"""The DDPG agent on the device (include/rg_ddpg.h) on the GPU against the numpy model of tests/ddpg_model.py: acting (the mean,
the zero padding, the Ornstein-Uhlenbeck state), the replay ring across a wrap, the sample stream, both gradients over the
cases of tests/ddpg_cases.py (its docstring has the tolerance rule and how relu crossings are kept out), relu'(0) = 0, the
action path, the clip, Adam, the soft update, update against its single entries, determinism and output bounds, a short ring,
and collect in closed loop.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ddpg import BatchedDDPGAgent, collect
from robot_gym_amd.core import ddpg_abi
from tests import ddpg_cases as DC
from tests import ddpg_model as DM
from tests import policy_model as PM
from tests import ppo_update_model as UM

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25
RINGS = ("ring_obs", "ring_action", "ring_reward", "ring_done")
ID = lambda cs: "-".join(str(v) for v in cs)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _load_ring(a, ring):
    for name, arr in (("ring_obs", ring.obs), ("ring_action", ring.action), ("ring_reward", ring.reward), ("ring_done", ring.done)):
        getattr(a, name).copy_(torch.as_tensor(arr))
    a.ring_state.copy_(torch.as_tensor(ring.state_array()))


def _agent(dev, c, **kw):
    a = BatchedDDPGAgent(c["B"], c["C"], device=dev, **{**dict(minibatch=c["M"], seed=11, **c["cfg"]), **kw})
    assert a.layout == c["lay"]
    for name in DC.NETS:
        getattr(a, name + "_params").copy_(torch.as_tensor(c["params"][name]))
    _load_ring(a, c["ring"])
    return a


def _sentinel(dtype):
    return SENTINEL if dtype.is_floating_point else -7


def _guarded(shape, dtype, dev, fill=None):
    n = int(np.prod(shape))
    big = torch.full((n + 2 * GUARD,), _sentinel(dtype), dtype=dtype, device=dev)
    view = big[GUARD:GUARD + n].view(*shape)
    if fill is not None:
        view.fill_(fill)
    return big, view


def _bands_intact(big):
    a, v = big.cpu().numpy(), _sentinel(big.dtype)
    assert np.all(a[:GUARD] == v) and np.all(a[-GUARD:] == v)


def _idx(dev, c):
    return torch.as_tensor(c["idx"], device=dev).contiguous()


# ---- act --------------------------------------------------------------------------------------------------------------

ACT_CASES = [("default", 67, 4, 6, 100), ("lopsided", 3, 4, 6, 5), ("limits", 3, 7, 10, 17), ("flat", 1, 2, 3, 1), ("lopsided", 67, 7, 6, DC.BIG)]


@pytest.mark.parametrize("cs", ACT_CASES, ids=ID)
def test_act_mean_padding_ou_state_and_counters(dev, cs):
    c = DC.case(*cs)
    cfg, lay, ring, B = c["cfg"], c["lay"], c["ring"], c["B"]
    W, A, d = cfg["window"], cfg["act_dim"], cfg["obs_dim"]
    a = _agent(dev, c)
    rng = np.random.default_rng(B + W)
    cur = (0.3 + rng.normal(size=(d, B))).astype(np.float32)
    obs = torch.as_tensor(cur, device=dev)
    x = ring.states([-1] * B, range(B), W, cur)
    m64 = UM.forward_all(x, PM.split(c["params"]["actor"], lay["actor"]), "tanh")[-1]
    m32 = UM.forward_all(x, PM.split(c["params"]["actor"], lay["actor"], np.float32), "tanh", np.float32)[-1]
    tol = max(8.0 * float(np.abs(m32 - m64).max()), 1e-6)
    f32 = dict(dtype=torch.float32, device=dev)
    big_a, action = _guarded((B, A), torch.float32, dev)
    big_m, mean = _guarded((B, A), torch.float32, dev)
    a.ou_state.copy_(torch.as_tensor(rng.normal(0.4, 0.1, size=(B, A)).astype(np.float32)))
    ou0, st0 = a.ou_state.cpu().numpy().copy(), a.act_state.cpu().numpy().copy()
    # MEAN mode: the mean, and no state moves
    a.act(obs, noise=False, out=dict(action=action, mean=mean))
    got = mean.cpu().numpy()
    err = float(np.abs(got - m64).max())
    print(f"{cs} act: float32-numpy vs float64 {np.abs(m32 - m64).max():.3e}; kernel vs float64 {err:.3e}; bound {tol:.3e}")
    assert err <= tol
    assert action.cpu().numpy().tobytes() == got.tobytes()
    assert a.ou_state.cpu().numpy().tobytes() == ou0.tobytes() and a.act_state.cpu().numpy().tobytes() == st0.tobytes()
    # the zero padding is exact zeros' effect: whatever lies in the masked observations, the bytes are the same
    kept = [ring.kept(-1, b, W) for b in range(B)]
    if ring.count > 0 and any(k < W for k in kept):
        spoilt = ring.obs.copy()
        for b, k in enumerate(kept):
            for age in range(max(k - 1, 0), ring.count):          # element k is age k - 1: from age kept - 1 on nothing is read
                spoilt[ring.slot(age), :, b] = np.nan
        a.ring_obs.copy_(torch.as_tensor(spoilt))
        mean2 = torch.zeros(B, A, **f32)
        a.act(obs, noise=False, out=dict(mean=mean2))
        assert mean2.cpu().numpy().tobytes() == got.tobytes()
        a.ring_obs.copy_(torch.as_tensor(ring.obs))
    # SAMPLE mode, twice: the OU state against the model on the stream of rg_policy.h
    x_model = ou0
    for step in range(2):
        a.act(obs, noise=True, out=dict(action=action, mean=mean))
        eps = PM.eps_batch(11, st0[0], st0[1] + step, A)
        want = DM.ou_step(x_model, eps, cfg.get("ou_theta", 0.5), 0.4, 0.3, 1e-2)
        ou = a.ou_state.cpu().numpy()
        # eps is the device's ln and cos: it may differ from numpy's in its last float32 bit, which moves x by sigma sqrt(dt) ulp(eps)
        bound = 0.3 * 0.1 * np.spacing(np.abs(eps)) + np.spacing(np.abs(want))
        print(f"{cs} act step {step}: worst |x - x_model| / bound {np.max(np.abs(ou.astype(np.float64) - want) / bound):.3f}")
        assert np.all(np.abs(ou.astype(np.float64) - want) <= bound)
        assert mean.cpu().numpy().tobytes() == got.tobytes()
        assert np.array_equal(action.cpu().numpy(), got + ou)                      # action = mean + x in float32
        x_model = ou
    st = a.act_state.cpu().numpy()
    assert np.array_equal(st[0], st0[0]) and np.array_equal(st[1], st0[1] + 2)
    _bands_intact(big_a), _bands_intact(big_m)
    a.close()


# ---- store and sample -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C", [(1, 2), (3, 4), (67, 7)])
def test_store_fills_the_slot_wraps_and_zeroes_ou_rows_of_done_robots(dev, B, C):
    cfg = DC.CONFIGS["lopsided"]
    d, A = cfg["obs_dim"], cfg["act_dim"]
    a = BatchedDDPGAgent(B, C, device=dev, minibatch=5, **cfg)
    bigs = {}
    for name in RINGS:
        t = getattr(a, name)
        bigs[name], view = _guarded(tuple(t.shape), t.dtype, dev, fill=0)
        setattr(a, name, view)
    bigs["ou"], a.ou_state = _guarded((B, A), torch.float32, dev, fill=0)
    bigs["state"], a.ring_state = _guarded((4,), torch.int64, dev, fill=0)
    ring = DM.Ring(C, B, d, A)
    rng = np.random.default_rng(C)
    for t in range(C + 2):
        obs, act = rng.normal(size=(d, B)).astype(np.float32), rng.uniform(-1, 1, size=(B, A)).astype(np.float32)
        rew, done = rng.normal(size=B).astype(np.float32), rng.choice(np.array([0, 0, 1, -3], dtype=np.int32), size=B)
        ou = rng.normal(0.4, 0.1, size=(B, A)).astype(np.float32)
        a.ou_state.copy_(torch.as_tensor(ou))
        a.store(*(torch.as_tensor(v, device=dev) for v in (obs, act, rew, done)))
        ring.store(obs, act, rew, done)
        for name, arr in (("ring_obs", ring.obs), ("ring_action", ring.action), ("ring_reward", ring.reward), ("ring_done", ring.done)):
            assert getattr(a, name).cpu().numpy().tobytes() == arr.tobytes(), (t, name)       # the slot written, every other byte as it was
        assert a.ring_state.cpu().tolist() == ring.state_array().tolist(), t
        ou[done != 0] = 0.0
        assert a.ou_state.cpu().numpy().tobytes() == ou.tobytes()
    assert ring.count == C and ring.head == (C + 2) % C and a.ticks_stored == C + 2
    for big in bigs.values():
        _bands_intact(big)
    a.close()


@pytest.mark.parametrize("B,C,ticks,M", [(1, 2, 2, 1), (3, 4, 3, 17), (67, 7, 9, DC.BIG)])
def test_sample_is_the_numpy_stream_and_a_short_ring_writes_nothing(dev, B, C, ticks, M):
    a = BatchedDDPGAgent(B, C, device=dev, minibatch=M, seed=77, **DC.CONFIGS["flat"])
    count = min(ticks, C)
    big, idx = _guarded((M, 2), torch.int32, dev)
    for updates in (0, 5):
        a.ring_state.copy_(torch.tensor([ticks % C, count, updates, 0]))
        a.sample(out=idx)
        got = idx.cpu().numpy()
        assert got.tobytes() == DM.sample(77, updates, M, count, B).tobytes()
        assert got[:, 0].min() >= 1 and got[:, 0].max() <= count - 1 and got[:, 1].min() >= 0 and got[:, 1].max() < B
    assert a.ring_state.cpu().tolist() == [ticks % C, count, 5, 0]                   # sample moves no state
    for short in (0, 1):
        idx.fill_(-9)
        a.ring_state.copy_(torch.tensor([short, short, 0, 0]))
        a.sample(out=idx)
        assert bool((idx == -9).all())
    _bands_intact(big)
    a.close()


# ---- gradients against the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", DC.CASES, ids=ID)
def test_gradients_match_the_model(dev, cs):
    c = DC.case(*cs)
    a = _agent(dev, c)
    idx = _idx(dev, c)
    start = {name: getattr(a, name).clone() for name in a._STATE}
    got = dict(critic=a.critic_grad(idx), actor=a.actor_grad(idx))
    for which in ("critic", "actor"):
        r = c[which]
        grad, loss = got[which][0].cpu().numpy(), float(got[which][1])
        err = DC.deviation(grad, r["m64"]["grad"], r["names"])
        l64 = r["m64"]["loss"]
        loss_err = abs(loss - l64) / abs(l64) if l64 != 0 else abs(loss)
        print(f"{cs} {which}: float32-numpy vs float64 {r['dev32']} loss {r['loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
              f"bounds {r['tol']} loss {r['loss_tol']:.3e}")
        for k, e in err.items():
            assert e <= r["tol"][k], (which, k, e, r["tol"][k])
        assert loss_err <= r["loss_tol"], (which, loss_err, r["loss_tol"])
    for name in a._STATE:                                                            # the gradient entries move no state
        assert torch.equal(getattr(a, name), start[name]), name
    a.close()


DEAD = 2          # the hidden neuron of each network's first layer whose weights and bias are 0


def test_a_pre_activation_of_exactly_zero_passes_no_gradient(dev):
    """relu'(0) = 0 in the kernel: neuron DEAD of the first hidden layer of the critic and of the actor has zero weights and a zero
    bias, so its pre-activation is exactly 0 for every sample.  Nothing may reach its weights, its bias or the row of the next
    layer it feeds -- a mask of x >= 0 instead of x > 0 would put the full delta on its bias."""
    c = dict(DC.case("default", 67, 4, 6, 100))
    lay, W = c["lay"], c["cfg"]["window"]
    params = dict(c["params"])
    for which in ("critic", "actor"):
        p = params[which].copy()
        i0, o0, w0, b0 = lay[which][0]
        p[w0:w0 + i0 * o0].reshape(i0, o0)[:, DEAD] = 0.0
        p[b0 + DEAD] = 0.0
        params[which] = p
    c["params"] = params
    a = _agent(dev, c)
    idx = _idx(dev, c)
    got = dict(critic=a.critic_grad(idx)[0].cpu().numpy(), actor=a.actor_grad(idx)[0].cpu().numpy())
    want = dict(critic=DM.critic_grad(c["ring"], c["idx"], params["critic"], params["target_actor"], params["target_critic"], lay, W, DC.GAMMA)["grad"],
                actor=DM.actor_grad(c["ring"], c["idx"], params["actor"], params["critic"], lay, W)["grad"])
    for which in ("critic", "actor"):
        g, g64 = got[which], want[which]
        (i0, o0, w0, b0), (i1, o1, w1, _) = lay[which][0], lay[which][1]
        for arr in (g, g64):
            W0, W1 = arr[w0:w0 + i0 * o0].reshape(i0, o0), arr[w1:w1 + i1 * o1].reshape(i1, o1)
            assert np.all(W0[:, DEAD] == 0.0) and arr[b0 + DEAD] == 0.0 and np.all(W1[DEAD] == 0.0), which
        assert np.abs(g[b0:b0 + o0]).max() > 0
        # the rest against the model: a sanity bound (the rule itself is test_gradients_match_the_model's), far below the O(1)
        # deviation a full delta on a dead neuron's bias would be
        err = DC.deviation(g, g64, DM.tensors(lay[which]))
        print(f"dead neuron, {which}: kernel vs float64 {err}")
        assert max(err.values()) <= 1e-4
    a.close()


@pytest.mark.parametrize("cs", [("default", 3, 7, 5, 17), ("lopsided", 67, 7, 6, DC.BIG)], ids=ID)
def test_a_critic_that_ignores_the_action_gives_an_actor_gradient_of_exactly_zero(dev, cs):
    c = dict(DC.case(*cs))
    lay, A = c["lay"], c["cfg"]["act_dim"]
    p = c["params"]["critic"].copy()
    i0, o0, w0, _ = lay["critic"][0]
    p[w0:w0 + i0 * o0].reshape(i0, o0)[:A] = 0.0                                     # the action's rows of the first layer
    c["params"] = dict(c["params"], critic=p)
    a = _agent(dev, c)
    grad, loss = a.actor_grad(_idx(dev, c))
    assert float(grad.abs().max()) == 0.0 and math.isfinite(float(loss)) and float(loss) != 0.0
    cgrad, _ = a.critic_grad(_idx(dev, c))
    assert float(cgrad.abs().max()) > 0.0                                            # the critic itself still learns
    a.close()


# ---- the optimiser ----------------------------------------------------------------------------------------------------------

def test_clipnorm_leaves_a_small_gradient_alone_scales_a_large_one_and_zero_is_off(dev):
    c = DC.case("lopsided", 3, 4, 6, 5)
    rng = np.random.default_rng(8)
    for which in ("actor", "critic"):
        n = c["lay"][which + "_count"]
        g = rng.normal(size=n).astype(np.float32)
        small, large = (g * np.float32(0.5 / np.linalg.norm(g))), (g * np.float32(30.0))
        for clipnorm, grad_in in ((1.0, small), (1.0, large), (0.0, large), (2.0, large)):
            a = _agent(dev, c, clipnorm=clipnorm)
            grad = torch.as_tensor(grad_in.copy(), device=dev)
            a.adam(which, grad)
            want, norm = DM.clip(grad_in, clipnorm)
            got = grad.cpu().numpy()
            assert math.isclose(float(a.grad_norm), norm, rel_tol=1e-14)
            if clipnorm == 0.0 or norm < clipnorm:
                assert got.tobytes() == grad_in.tobytes()
            else:
                # the norm is a float64 sum in another order than numpy's: the scale agrees to 1e-15, a scaled entry to one float32 ulp
                assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))) and not np.array_equal(got, grad_in)
                assert math.isclose(math.sqrt(float(np.sum(got.astype(np.float64) ** 2))), clipnorm, rel_tol=1e-6)
            assert a.steps.tolist() == ([1, 0] if which == "actor" else [0, 1])
            a.close()


@pytest.mark.parametrize("steps", [1, 3])
def test_adam_agrees_with_torch_on_the_gpu(dev, steps):
    c = DC.case("lopsided", 3, 4, 6, 5)
    a = _agent(dev, c, clipnorm=0.0, actor_lr=1e-3, critic_lr=3e-4)
    rng = np.random.default_rng(steps)
    for which, buf, lr in (("actor", a.actor_params, 1e-3), ("critic", a.critic_params, 3e-4)):
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
            a.adam(which, g)
        got, want = buf.detach().cpu().numpy().astype(np.float64), twin.detach().cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        bound = np.maximum(4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 1e-9)
        print(f"adam {which} {steps} step(s): worst |p - p_torch| {err.max():.3e}, worst ratio to its bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
        assert np.abs(got - c["params"][which]).max() > 1e-5          # it stepped
    assert a.steps.tolist() == [steps, steps]
    assert torch.equal(a.target_actor_params.cpu(), torch.as_tensor(c["params"]["target_actor"]))      # Adam touches no target
    a.close()


@pytest.mark.parametrize("tau", [1e-3, 0.25, 1.0])
def test_soft_update_is_the_numpy_expression(dev, tau):
    c = DC.case("default", 3, 7, 5, 17)
    a = _agent(dev, c, tau=tau)
    for which in ("actor", "critic"):
        a.soft_update(which)
        want = DM.soft_update(c["params"]["target_" + which], c["params"][which], tau)
        assert getattr(a, f"target_{which}_params").cpu().numpy().tobytes() == want.tobytes()
        assert getattr(a, f"{which}_params").cpu().numpy().tobytes() == c["params"][which].tobytes()
        if tau == 1.0:
            assert want.tobytes() == c["params"][which].tobytes()
    a.hard_update()
    assert torch.equal(a.actor_params, a.target_actor_params) and torch.equal(a.critic_params, a.target_critic_params)
    a.close()


# ---- update -----------------------------------------------------------------------------------------------------------------

def _bytes(a):
    return {name: getattr(a, name).cpu().numpy().tobytes() for name in a._STATE}


@pytest.mark.parametrize("cs", [("lopsided", 67, 7, 6, DC.BIG), ("default", 67, 4, 6, 100)], ids=ID)
def test_update_equals_the_single_entries_called_in_order(dev, cs):
    c = DC.case(*cs)
    a, b = _agent(dev, c), _agent(dev, c)
    stats = a.update(3).cpu().numpy()
    losses, norms, idxs = [], [], []
    for u in range(3):
        idxs.append(b.sample().cpu().numpy().copy())
        assert idxs[-1].tobytes() == DM.sample(11, u, c["M"], c["ring"].count, c["B"]).tobytes()
        grad, loss = b.critic_grad()
        losses.append(float(loss))
        b.adam("critic", grad, gated=True)
        norms.append(float(b.grad_norm))
        grad, loss = b.actor_grad()
        losses.append(float(loss))
        b.adam("actor", grad, gated=True)
        b.soft_update("actor", gated=True), b.soft_update("critic", gated=True)
        b.advance()
    assert _bytes(a) == _bytes(b)
    assert a.ring_state.cpu().tolist() == c["ring"].state_array().tolist()[:2] + [3, 0] and a.steps.tolist() == [3, 3]
    assert not np.array_equal(a.actor_params.cpu().numpy(), c["params"]["actor"]) and not np.array_equal(a.target_critic_params.cpu().numpy(), c["params"]["target_critic"])
    assert stats.tolist() == [losses[0], losses[4], losses[1], losses[5], -losses[5], norms[2]]
    assert a.stats_dict() == dict(zip(ddpg_abi.STAT_NAMES, stats.tolist()))
    a.close(), b.close()


@pytest.mark.parametrize("cs", [("lopsided", 3, 4, 6, 5), ("default", 67, 4, 6, 100)], ids=ID)
def test_two_calls_and_another_stream_give_the_same_bytes_within_the_outputs(dev, cs):
    c = DC.case(*cs)
    a = _agent(dev, c)
    idx = _idx(dev, c)
    big_w, a.workspace = _guarded((a._handle.workspace_bytes // 8,), torch.float64, dev, fill=0)

    def run():
        big_c, gc = _guarded((c["lay"]["critic_count"],), torch.float32, dev)
        big_a, ga = _guarded((c["lay"]["actor_count"],), torch.float32, dev)
        _, lc = a.critic_grad(idx, out=gc)
        lc = lc.clone()
        _, la = a.actor_grad(idx, out=ga)
        torch.cuda.synchronize()
        for big, view in ((big_c, gc), (big_a, ga)):
            _bands_intact(big)
            assert not bool((view == SENTINEL).any())                               # and the slice itself was filled
        _bands_intact(big_w)
        return [t.cpu().numpy().tobytes() for t in (gc, ga, lc, la.clone())]

    first = run()
    assert run() == first
    a.workspace.fill_(float("nan"))                                                  # nothing is carried in the workspace between calls
    assert run() == first
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        third = run()
    side.synchronize()
    assert third == first
    # the whole update: stats within its bounds, the same bytes from the same start
    start = a.state_dict()
    results = []
    for _ in range(2):
        a.load_state_dict(start)
        big_s, a.stats = _guarded((ddpg_abi.STATS,), torch.float64, dev)
        a.update(2)
        torch.cuda.synchronize()
        _bands_intact(big_s), _bands_intact(big_w)
        assert all(math.isfinite(v) for v in a.stats.cpu().tolist())
        results.append((_bytes(a), a.stats.cpu().numpy().tobytes()))
    assert results[0] == results[1] and a.steps.tolist() == [2, 2]
    a.close()


@pytest.mark.parametrize("ticks", [0, 1])
def test_a_short_ring_moves_nothing(dev, ticks):
    cfg = DC.CONFIGS["lopsided"]
    a = BatchedDDPGAgent(3, 4, device=dev, minibatch=5, **cfg)
    f = dict(device=dev)
    for _ in range(ticks):
        a.store(torch.ones(6, 3, **f), torch.ones(3, 3, **f), torch.ones(3, **f), torch.zeros(3, dtype=torch.int32, **f))
    a.soft_update("actor")                                                           # something for a wrong update to undo
    before = _bytes(a)
    a.idx.fill_(-9)
    a._grad[ddpg_abi.CRITIC].fill_(SENTINEL), a._grad[ddpg_abi.ACTOR].fill_(SENTINEL), a._loss.fill_(SENTINEL)
    stats = a.update(2).cpu().numpy()
    assert np.all(np.isnan(stats)) and a.stats_dict() == dict.fromkeys(ddpg_abi.STAT_NAMES)
    a.sample(), a.critic_grad(), a.actor_grad(), a.advance()
    a.adam("critic", gated=True), a.adam("actor", gated=True), a.soft_update("critic", gated=True)
    assert _bytes(a) == before and a.ring_state.cpu().tolist() == [ticks, ticks, 0, 0] and a.steps.tolist() == [0, 0]
    assert bool((a.idx == -9).all()) and bool((a._loss == SENTINEL).all())
    assert all(bool((g == SENTINEL).all()) for g in a._grad.values())
    a.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------

def test_collect_in_closed_loop_and_a_clone_continues_identically(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    B = 64
    env = BatchedGoEnv(B, device=dev, seed=5, auto_reset=True, max_time=0.45)
    env.reset()
    agent = BatchedDDPGAgent(B, 64, device=dev, seed=3)
    start = {name: getattr(agent, name + "_params").clone() for name in DC.NETS}
    ptrs = {name: getattr(agent, name + "_params").data_ptr() for name in DC.NETS}
    stats = collect(env, agent, 30, updates_per_tick=2, warmup=5)
    assert stats is agent.stats and stats.is_cuda
    d = agent.stats_dict()
    print(f"closed loop: {d}")
    assert all(v is not None and math.isfinite(v) for v in d.values())
    assert agent.ring_state.cpu().tolist() == [30, 30, 2 * 26, 0] and agent.steps.tolist() == [52, 52] and agent.ticks_stored == 30
    moved = {}
    for name in DC.NETS:
        p = getattr(agent, name + "_params")
        assert bool(torch.isfinite(p).all()) and p.data_ptr() == ptrs[name] and not torch.equal(p, start[name])
        moved[name] = float((p - start[name]).abs().max())
    assert moved["target_actor"] < moved["actor"] and moved["target_critic"] < moved["critic"]
    # a clone continues as its source does: the same tick and the same updates on both
    twin = agent.clone()
    obs = env.obs.t().contiguous()
    f32 = dict(dtype=torch.float32, device=dev)
    reward, done = torch.rand(B, **f32), torch.zeros(B, dtype=torch.int32, device=dev)
    for ag in (agent, twin):
        out = ag.act(obs, noise=True)
        ag.store(obs, out["action"], reward, done)
        ag.update(2)
    assert _bytes(agent) == _bytes(twin) and agent.stats.cpu().numpy().tobytes() == twin.stats.cpu().numpy().tobytes()
    env.close(), agent.close(), twin.close()
