"""The recurrent PPO policy update on the device (include/rg_bptt.h, DeviceRecurrentPPO) on the GPU against the float64 numpy model
of tests/bptt_model.py: the gradient and the loss over four configurations and shapes around the tile of robots and the chunk
of samples, the forward pass to the bit of rg_rnn_unroll, exact zeros under resets and masks, relu'(0) = 0, determinism and
independence of a robot's place in the batch, Adam against torch.optim.Adam, the penalty's three branches, update against the
single entries, one epoch against RecurrentPPO, and two iterations of collect -> update in closed loop.

The cases, the bound of a gradient (the rule of tests/test_ppo_update_gpu.py) and the redraw of observations near a relu
crossing are tests/bptt_cases.py's, formed from the model alone; tests/test_bptt_cpu.py holds them to their caps.  Every
figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import DeviceRecurrentPPO, RecurrentGaussianPolicy, RecurrentPPO, RecurrentRolloutBuffer, collect_recurrent
from robot_gym_amd.core import bptt_abi, ppo_abi
from tests import bptt_cases as BC
from tests import bptt_model as BM
from tests import ppo_update_model as UM
from tests import rnn_model as RM

pytestmark = pytest.mark.gpu

PPO_KW, MODEL_KW = BC.PPO_KW, BC.MODEL_KW
SLOTS = ("obs", "action", "mean", "logstd", "adv", "ret", "mask", "reset", "h0")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _policy(dev, c, pp=None):
    pol = RecurrentGaussianPolicy(c["B"], seed=11, device=dev, **c["cfg"])
    assert pol.layout == c["lay"]
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(c["pp"] if pp is None else pp))
        pol.value_params.copy_(torch.as_tensor(c["vp"]))
    pol.norm_state.copy_(torch.as_tensor(c["state"]))
    return pol


def _rollout(dev, c, **replace):
    cfg = c["cfg"]
    ro = RecurrentRolloutBuffer(c["T"], c["B"], cfg["obs_dim"], cfg["act_dim"], cfg["gru_units"], device=dev)
    for s in SLOTS:
        getattr(ro, s).copy_(torch.as_tensor(np.array(replace.get(s, c[s]))))
    return ro


def _grad(upd, ro):
    upd.prepare(ro)
    grad, loss = upd.policy_grad(ro)
    return grad.cpu().numpy(), float(loss)


# ---- the gradient and the loss against the model ------------------------------------------------------------------------------

def _check_gradient(dev, c):
    name, T, B = c["name"], c["T"], c["B"]
    lay = c["lay"]
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DeviceRecurrentPPO(pol, T, **c["ppo_kw"])
    assert upd._handle.groups == bptt_abi.groups(T, B)
    upd.prepare(ro)
    n, m, sd = c["stats"]
    got = upd.adv_stats().cpu().numpy()
    assert got[0] == n and math.isclose(got[1], m, rel_tol=1e-12, abs_tol=1e-15) and math.isclose(got[2], sd, rel_tol=1e-12)
    grad, loss = upd.policy_grad(ro)
    grad, loss = grad.cpu().numpy(), float(loss)
    p64 = c["p64"]
    err = BC.deviation(grad, p64["grad"], BM.tensors(lay))
    loss_err = abs(loss - p64["loss"]) / abs(p64["loss"])
    print(f"{name} T={T} B={B} coef={c['model_kw']['kl_cutoff_coef']}: float32-numpy vs float64 {c['p_dev32']} loss {c['p_loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
          f"bounds {c['p_tol']} loss {c['p_loss_tol']:.3e}")
    for k, e in err.items():
        assert e <= c["p_tol"][k], (k, e, c["p_tol"][k])
    assert loss_err <= c["p_loss_tol"]
    # the per-robot KL and the loss in float64 from the float32 means of rg_rnn_unroll
    means = pol.unroll(ro)["mean"].cpu().numpy().reshape(T * B, -1)
    head = UM.policy_head(means, c["pp"][lay["logstd_offset"]:], c["action"], c["mean"], c["logstd"], (c["adv"].astype(np.float64) - m) / sd, c["mask"],
                          T, B, **c["model_kw"])
    kl = upd.kl(ro).cpu().numpy()
    assert np.allclose(kl, head["kl"], rtol=1e-6, atol=0) and np.all(kl[head["kl"] == 0.0] == 0.0)
    assert math.isclose(loss, head["loss"], rel_tol=1e-9)
    assert upd.steps().tolist() == [0, 0] and float(upd.penalty) == 0.7         # the gradient entries move no state
    upd.close(), pol.close()


@pytest.mark.parametrize("name,T,B", BC.GRADIENT_CASES)
def test_gradients_match_the_model(dev, name, T, B):
    _check_gradient(dev, BC.case(name, T, B))


@pytest.mark.parametrize("name,T,B", BC.NO_CUTOFF_CASES)
def test_gradients_without_the_cutoff_match_the_model(dev, name, T, B):
    """kl_cutoff_coef = 0: the surrogate and the penalty term carry the gradient in comparable parts (tests/bptt_cases.py)."""
    _check_gradient(dev, BC.case(name, T, B, cutoff=False))


# ---- the forward pass is rg_rnn_unroll's to the bit ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BC.CONFIGS))
def test_nothing_changed_since_the_rollout_gives_kl_zero_and_ratio_one(dev, name):
    """The rollout's means come from rg_rnn_unroll with the current parameters and normaliser; logstd is copied.  One ulp of
    difference in a mean gives kl > 0 in float64, so kl == 0.0 for every robot says that the update's forward pass is that
    kernel's to the bit: with resets, a non-zero h0 and 37 robots (a tile of five)."""
    T, B = 5, 37
    c = BC.case(name, T, B)
    pol, ro = _policy(dev, c), _rollout(dev, c)
    pol.unroll(ro, out=dict(mean=ro.mean))
    ro.logstd.copy_(pol.logstd.detach())
    assert float(ro.mean.abs().max()) > 0
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    kl = upd.kl(ro).cpu().numpy()
    assert kl.shape == (B,) and np.all(kl == 0.0)
    _, loss = _grad(upd, ro)
    n, m, sd = c["stats"]
    advn = (c["adv"].astype(np.float64) - m) / sd
    want = -np.sum(advn[c["mask"] != 0]) / (T * B)
    print(f"{name}: loss {loss!r}, minus the mean normalised advantage {want!r}")
    assert math.isclose(loss, want, rel_tol=1e-12, abs_tol=1e-15)
    upd.close(), pol.close()


# ---- resets and masks, exact ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T,B", [("default", 3, 5), ("two dense", 5, 37)])
def test_resets_everywhere_leave_the_h_rows_exactly_zero(dev, name, T, B):
    c = BC.case(name, T, B)
    pol, ro = _policy(dev, c), _rollout(dev, c, reset=np.ones((T, B), dtype=np.int32))
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    grad, _ = _grad(upd, ro)
    for s in BM.h_rows(c["lay"]):
        assert np.all(grad[s] == 0.0)
    for k, s in BM.tensors(c["lay"]).items():
        assert np.abs(grad[s]).max() > 0, k
    free, _ = _grad(upd, _rollout(dev, c))
    assert all(np.abs(free[s]).max() > 0 for s in BM.h_rows(c["lay"]))
    upd.close(), pol.close()


@pytest.mark.parametrize("name,T,B", [("default", 3, 5), ("lopsided", 8, 1037), ("limits", 2, 9)])
def test_an_all_zero_mask_gives_exactly_zero_gradients(dev, name, T, B):
    c = BC.case(name, T, B)
    pol, ro = _policy(dev, c), _rollout(dev, c, mask=np.zeros((T, B), dtype=np.int32))
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    upd.prepare(ro)
    assert upd.adv_stats().cpu().tolist() == [1.0, 0.0, 1e-8, 0.0]
    grad, loss = upd.policy_grad(ro)
    assert float(grad.abs().max()) == 0.0 and float(loss) == 0.0
    assert float(upd.kl(ro).abs().max()) == 0.0
    upd.close(), pol.close()


def test_observations_before_a_reset_do_not_reach_the_gradient(dev):
    """Every third robot from robot 1 is reset at tick T // 2 and its ticks before that are masked: what those robots saw before
    the reset changes no byte of the gradient.  Without those resets the same change moves it."""
    name, T, B = "default", 5, 37
    c = BC.case(name, T, B)
    cut, robots = T // 2, np.arange(1, B, 3)
    assert np.all(c["reset"][cut, robots] != 0)
    mask = c["mask"].copy()
    mask[:cut, robots] = 0
    obs = c["obs"].copy()
    obs[:cut, :, robots] += np.random.default_rng(3).normal(size=obs[:cut, :, robots].shape).astype(np.float32)
    pol = _policy(dev, c)
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    a, la = _grad(upd, _rollout(dev, c, mask=mask))
    b, lb = _grad(upd, _rollout(dev, c, mask=mask, obs=obs))
    assert a.tobytes() == b.tobytes() and la == lb and np.abs(a).max() > 0
    reset = c["reset"].copy()
    reset[cut, robots] = 0
    a, _ = _grad(upd, _rollout(dev, c, mask=mask, reset=reset))
    b, _ = _grad(upd, _rollout(dev, c, mask=mask, obs=obs, reset=reset))
    assert not np.array_equal(a, b)
    upd.close(), pol.close()


DEAD = 2          # the neuron of the first dense layer whose weights and bias are 0


@pytest.mark.parametrize("name,T,B", [("default", 5, 37), ("two dense", 5, 37)])
def test_a_pre_activation_of_exactly_zero_passes_no_gradient(dev, name, T, B):
    """relu'(0) = 0 in the kernel: neuron DEAD of the first dense layer has zero weights and a zero bias, so its pre-activation is
    exactly 0 for every sample.  Nothing may reach its weights, its bias or the rows it feeds in the next block -- a mask of
    x >= 0 instead of x > 0 would put the full delta on its bias; everything else is the model's."""
    c = BC.case(name, T, B)
    lay = c["lay"]
    pp = c["pp"].copy()
    i0, o0, w0, b0 = lay["dense"][0]
    pp[w0:w0 + i0 * o0].reshape(i0, o0)[:, DEAD] = 0.0
    pp[b0 + DEAD] = 0.0
    nxt = [lay["dense"][1]] if len(lay["dense"]) > 1 else [lay["w_ru"], lay["w_c"]]
    pol, ro = _policy(dev, c, pp), _rollout(dev, c)
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    g, _ = _grad(upd, ro)
    g64 = BM.policy_grad(c["x"], c["reset"], c["h0"], pp, lay, c["action"], c["mean"], c["logstd"], c["adv"], c["mask"], **MODEL_KW)["grad"]
    for arr in (g, g64):
        assert np.all(arr[w0:w0 + i0 * o0].reshape(i0, o0)[:, DEAD] == 0.0) and arr[b0 + DEAD] == 0.0
        for i1, o1, w1, _ in nxt:
            assert np.all(arr[w1:w1 + i1 * o1].reshape(i1, o1)[DEAD] == 0.0)
    live = np.delete(np.arange(o0), DEAD)
    assert np.all(np.abs(g[w0:w0 + i0 * o0].reshape(i0, o0)[:, live]).max(axis=0) > 0) and np.all(g[b0 + live] != 0.0)
    err = BC.deviation(g, g64, BM.tensors(lay))
    print(f"dead neuron, {name}: kernel vs float64 {err}")
    assert max(err.values()) <= 1e-4            # a sanity bound, far below the O(1) deviation a full delta on a dead bias would be
    upd.close(), pol.close()


# ---- determinism, bounds of the outputs, a robot's place in the batch ---------------------------------------------------------------

GUARD = 64
F_SENTINEL = -7.25


def _guarded(n, dtype, dev):
    big = torch.full((n + 2 * GUARD,), F_SENTINEL, dtype=dtype, device=dev)
    return big, big[GUARD:GUARD + n]


def _bands_intact(big):
    a = big.cpu().numpy()
    assert np.all(a[:GUARD] == F_SENTINEL) and np.all(a[-GUARD:] == F_SENTINEL)
    assert not np.any(a[GUARD:-GUARD] == F_SENTINEL)           # and the slice itself was filled


@pytest.mark.parametrize("name,T,B", [("two dense", 2, 9), ("default", 8, 1037)])
def test_two_calls_and_another_stream_give_the_same_bytes_within_the_outputs(dev, name, T, B):
    c = BC.case(name, T, B)
    lay = c["lay"]
    pol, ro = _policy(dev, c), _rollout(dev, c)
    upd = DeviceRecurrentPPO(pol, T, epochs_policy=2, epochs_value=2, **PPO_KW)

    def run():
        upd.prepare(ro)
        big_g, g = _guarded(lay["policy_count"], torch.float32, dev)
        big_k, k = _guarded(B, torch.float64, dev)
        _, loss = upd.policy_grad(ro, out=g)
        loss = loss.clone()
        upd.kl(ro, out=k)
        torch.cuda.synchronize()
        _bands_intact(big_g), _bands_intact(big_k)
        return [t.cpu().numpy().tobytes() for t in (g, k, loss)]

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
    start = (pol.policy_params.detach().clone(), pol.value_params.detach().clone(), upd.opt_state.clone(), upd.value_opt_state.clone())
    results = []
    for _ in range(2):
        with torch.no_grad():
            pol.policy_params.copy_(start[0]), pol.value_params.copy_(start[1])
        upd.opt_state.copy_(start[2]), upd.value_opt_state.copy_(start[3])
        big_s, upd.stats = _guarded(ppo_abi.STATS, torch.float64, dev)
        upd.update(ro)
        torch.cuda.synchronize()
        _bands_intact(big_s)
        results.append([t.detach().cpu().numpy().tobytes() for t in (pol.policy_params, pol.value_params, upd.opt_state, upd.value_opt_state, upd.stats)])
    assert results[0] == results[1]
    assert upd.steps().tolist() == [2, 2]
    upd.close(), pol.close()


def test_a_robots_kl_does_not_depend_on_its_place_in_the_batch(dev):
    name, T, B = "default", 5, 37
    c = BC.case(name, T, B)
    perm = np.random.default_rng(5).permutation(B)
    moved = dict(obs=c["obs"][:, :, perm], action=c["action"][:, perm], mean=c["mean"][:, perm], adv=c["adv"][:, perm], ret=c["ret"][:, perm],
                 mask=c["mask"][:, perm], reset=c["reset"][:, perm], h0=c["h0"][perm])
    pol = _policy(dev, c)
    upd = DeviceRecurrentPPO(pol, T, **PPO_KW)
    a = upd.kl(_rollout(dev, c)).cpu().numpy()
    b = upd.kl(_rollout(dev, c, **moved)).cpu().numpy()
    assert a[perm].tobytes() == b.tobytes() and np.abs(a).max() > 0 and len(set(a.tolist())) > B // 2
    upd.close(), pol.close()


# ---- Adam and the penalty ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("steps", [1, 3])
def test_adam_agrees_with_torch_on_the_gpu(dev, steps):
    c = BC.case("lopsided", 3, 5)
    pol = _policy(dev, c)
    upd = DeviceRecurrentPPO(pol, 3, policy_lr=1e-4, value_lr=3e-4)
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
    assert upd.steps().tolist() == [steps, steps]
    assert np.all(np.isfinite(upd.moments.cpu().numpy())) and float(upd.moments.abs().max()) > 0 and float(upd.value_moments.abs().max()) > 0
    upd.close(), pol.close()


@pytest.mark.parametrize("scale,factor", [(0.5, 1.5), (2.0, 1 / 1.5), (1.0, 1.0)])
def test_penalty_moves_as_the_model_says(dev, scale, factor):
    """With no epochs the KL change is the rollout's own KL; kl_target = scale x that puts it above 1.3 x the target, below
    0.7 x, or between them."""
    c = BC.case("default", 3, 5)
    pol, ro = _policy(dev, c), _rollout(dev, c)
    change = float(np.mean(c["p64"]["kl"]))
    assert change > 0
    upd = DeviceRecurrentPPO(pol, 3, epochs_policy=0, epochs_value=0, kl_target=scale * change, kl_init_penalty=2.0)
    out = upd.update(ro).cpu().numpy()
    assert math.isclose(out[4], change, rel_tol=1e-4)
    assert out[5] == UM.move_penalty(2.0, out[4], scale * change) == 2.0 * factor == float(upd.penalty)
    d = upd.stats_dict()
    assert d["policy_loss_first"] is None and d["policy_loss_last"] is None and d["value_loss_first"] is None and d["value_loss_last"] is None
    assert d["penalty"] == 2.0 * factor
    assert np.array_equal(pol.policy_params.detach().cpu().numpy(), c["pp"]) and upd.steps().tolist() == [0, 0]
    upd.close(), pol.close()


# ---- update is the composition of the single entries ----------------------------------------------------------------------------------

def test_update_equals_the_single_entries_called_in_order(dev):
    c = BC.case("default", 5, 37)
    T, B = c["T"], c["B"]
    ro = _rollout(dev, c)
    pol_a, pol_b = _policy(dev, c), _policy(dev, c)
    kw = dict(epochs_policy=3, epochs_value=3, **PPO_KW)
    a, b = DeviceRecurrentPPO(pol_a, T, **kw), DeviceRecurrentPPO(pol_b, T, **kw)
    stats = a.update(ro).cpu().numpy()
    b.prepare(ro)
    losses = []
    for _ in range(3):
        grad, loss = b.policy_grad(ro)
        losses.append(float(loss))
        b.adam("policy", grad)
    kl = b.kl(ro)
    moved = b.move_penalty(kl).cpu().numpy()
    for _ in range(3):
        grad, loss = b.value_grad(ro)
        losses.append(float(loss))
        b.adam("value", grad)
    assert torch.equal(pol_a.policy_params.detach(), pol_b.policy_params.detach()) and torch.equal(pol_a.value_params.detach(), pol_b.value_params.detach())
    assert not np.array_equal(pol_a.policy_params.detach().cpu().numpy(), c["pp"]) and not np.array_equal(pol_a.value_params.detach().cpu().numpy(), c["vp"])
    assert a.steps().tolist() == b.steps().tolist() == [3, 3]
    assert torch.equal(a.opt_state, b.opt_state) and torch.equal(a.value_opt_state, b.value_opt_state)
    assert stats[:4].tolist() == [losses[0], losses[2], losses[3], losses[5]]
    assert stats[4:].tolist() == moved.tolist()
    assert math.isclose(stats[4], float(kl.mean()), rel_tol=1e-12)
    assert stats[5] == UM.move_penalty(0.7, stats[4], 1e-2) == float(a.penalty)
    assert a.stats_dict() == dict(zip(ppo_abi.STAT_NAMES, stats.tolist()))
    a.close(), b.close(), pol_a.close(), pol_b.close()


def test_one_epoch_agrees_with_recurrent_ppo(dev):
    """From the same start, one policy epoch: the first loss within the case's loss bound of torch's float32 loss, and the KL
    change after the step to 1e-4 of torch's.  At the largest shape: there the float32 model's deviation, which the bound is
    formed from, is a measure (every group of the W phase sees whole chunks) and not a single draw."""
    c = BC.case("default", 8, 1037)
    T = c["T"]
    ro = _rollout(dev, c)
    pol_a, pol_b = _policy(dev, c), _policy(dev, c)
    kw = dict(epochs_policy=1, epochs_value=0, **PPO_KW)
    got = DeviceRecurrentPPO(pol_a, T, **kw)
    got.update(ro)
    got = got.stats_dict()
    want = RecurrentPPO(pol_b, **kw).update(ro)
    print(f"one epoch: device {got}; torch {want}; loss bound {c['p_loss_tol']:.3e}")
    assert abs(got["policy_loss_first"] - want["policy_loss_first"]) <= c["p_loss_tol"] * abs(want["policy_loss_first"])
    assert math.isclose(got["kl_change"], want["kl_change"], rel_tol=1e-4)
    assert got["penalty"] == want["penalty"] and got["value_loss_first"] is None and want["value_loss_first"] is None
    pol_a.close(), pol_b.close()


# ---- closed loop ------------------------------------------------------------------------------------------------------------------

def test_two_iterations_of_collect_and_update(dev):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    B, T = 64, 8
    env = BatchedGoEnv(B, device=dev, seed=5, auto_reset=True, max_time=0.45)
    env.reset()
    pol = RecurrentGaussianPolicy(B, seed=11, device=dev)
    ro = RecurrentRolloutBuffer(T, B, device=dev)
    upd = DeviceRecurrentPPO(pol, epochs_policy=2, epochs_value=2)
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    for it in range(2):
        collect_recurrent(env, pol, ro)
        old = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
        saved = (pol.state_dict(), upd.state_dict()) if it == 1 else None
        stats = upd.update(ro)
        assert stats is upd.stats and stats.is_cuda
        d = upd.stats_dict()
        print(f"iteration {it}: {d}")
        assert all(math.isfinite(v) for v in d.values())
        assert bool(torch.isfinite(pol.policy_params).all()) and bool(torch.isfinite(pol.value_params).all())
        assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
        moved = pol.policy_params.detach() != old[0]
        for i, o, w, b in RM.blocks(pol.layout):                   # back-propagation through time reaches every block
            assert bool(moved[w:w + i * o].any()) and bool(moved[b:b + o].any())
        assert bool(moved[pol.layout["logstd_offset"]:].any()) and not torch.equal(pol.value_params.detach(), old[1])
        assert upd.steps().tolist() == [2 * (it + 1)] * 2
    # the second update once more from the saved state: the same bytes
    after = [t.detach().clone() for t in (pol.policy_params, pol.value_params, upd.opt_state, upd.value_opt_state, upd.stats)]
    pol.load_state_dict(saved[0])
    upd.load_state_dict(saved[1])
    assert upd.steps().tolist() == [2, 2] and not torch.equal(pol.policy_params.detach(), after[0])
    upd.update(ro)
    again = (pol.policy_params, pol.value_params, upd.opt_state, upd.value_opt_state, upd.stats)
    assert all(torch.equal(x.detach(), y) for x, y in zip(again, after))
    assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
    env.close(), upd.close(), pol.close()
