"""The DDPG kernels (include/rg_ddpg.h) on the GPU at the edges tests/test_ddpg_gpu.py leaves out, over the cases of
tests/ddpg_edges.py (its docstring has the tolerance rule and the window probe): both gradients and the acting mean at widths on
a wave's boundary, the widest observation, one-neuron layers, minibatches of one tile, of TILE * MAX_GROUPS and one more, and
the API's largest; the gathered states s0 and s1 of every (age, robot) of small rings, exactly; indices outside the ring; gamma,
the Ornstein-Uhlenbeck constants and Adam's off their defaults, lr = 0, step counts of 10^6; the clip and Adam on buffers the
norm kernel walks in strides; the sample stream past 2^32; and a ring head outside the ring.  Every figure is printed before it
is asserted, beside its bound."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ddpg import BatchedDDPGAgent
from tests import ddpg_cases as DC
from tests import ddpg_edges as DE
from tests import ddpg_model as DM
from tests import policy_model as PM
from tests import ppo_update_model as UM

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.25
RINGS = ("ring_obs", "ring_action", "ring_reward", "ring_done")
ID = lambda cs: "-".join(str(v) for v in cs)
LOPSIDED = DC.CONFIGS["lopsided"]


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
    a = BatchedDDPGAgent(c["B"], c["C"], device=dev, **{**dict(minibatch=c["M"], seed=11, gamma=c["gamma"], **c["cfg"]), **kw})
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


def _guard_rings(a, dev):
    """Every ring tensor, the ring state and the workspace of the agent behind guard bands; returns the bands' owners."""
    bigs = []
    for name in RINGS + ("ring_state", "workspace"):
        t = getattr(a, name)
        big, view = _guarded(tuple(t.shape), t.dtype, dev)
        view.copy_(t)
        setattr(a, name, view)
        bigs.append(big)
    return bigs


def _check_gradients(cs, c, a, idx, want, dev):
    """Both gradient entries on idx into guarded outputs against want = {critic, actor: the float64 model}, under the bounds of
    the case c."""
    bigs = _guard_rings(a, dev)
    for which, entry in (("critic", a.critic_grad), ("actor", a.actor_grad)):
        r = c[which]
        big, out = _guarded((c["lay"][which + "_count"],), torch.float32, dev)
        bigs.append(big)
        grad, loss = entry(idx, out=out)
        grad, loss = grad.cpu().numpy(), float(loss)
        err = DC.deviation(grad, want[which]["grad"], r["names"])
        l64 = want[which]["loss"]
        loss_err = abs(loss - l64) / abs(l64) if l64 != 0 else abs(loss)
        yard = "float32-numpy in the header's order" if c["tiled"] else "float32-numpy"
        print(f"{cs} {which}: {yard} vs float64 {r['dev32']} loss {r['loss_dev32']:.3e}; kernel vs float64 {err} loss {loss_err:.3e}; "
              f"bounds {r['tol']} loss {r['loss_tol']:.3e}")
        for k, e in err.items():
            assert e <= r["tol"][k], (which, k, e, r["tol"][k])
        assert loss_err <= r["loss_tol"], (which, loss_err, r["loss_tol"])
    for big in bigs:
        _bands_intact(big)


# ---- widths, limits and minibatch sizes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", DE.CASES, ids=ID)
def test_gradients_match_the_model_at_the_edges(dev, cs):
    c = DE.case(*cs)
    a = _agent(dev, c)
    assert a._handle.groups == DE.groups(c["M"])
    start = {name: getattr(a, name).clone() for name in a._STATE}
    _check_gradients(cs, c, a, torch.as_tensor(c["idx"], device=dev).contiguous(), dict(critic=c["critic"]["m64"], actor=c["actor"]["m64"]), dev)
    for name in a._STATE:
        assert torch.equal(getattr(a, name), start[name]), name
    a.close()


@pytest.mark.parametrize("cs", DE.ACT_CASES, ids=ID)
def test_act_at_the_edges_mean_padding_and_one_noisy_step(dev, cs):
    c = DE.case(*cs)
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
    big_a, action = _guarded((B, A), torch.float32, dev)
    big_m, mean = _guarded((B, A), torch.float32, dev)
    big_o, a.ou_state = _guarded((B, A), torch.float32, dev, fill=0)
    big_s, a.act_state = _guarded((2, B), torch.int64, dev, fill=0)
    a.act_state[0] = torch.arange(B, device=dev)
    a.ou_state.copy_(torch.as_tensor(rng.normal(0.4, 0.1, size=(B, A)).astype(np.float32)))
    ou0, st0 = a.ou_state.cpu().numpy().copy(), a.act_state.cpu().numpy().copy()
    a.act(obs, noise=False, out=dict(action=action, mean=mean))
    got = mean.cpu().numpy()
    err = float(np.abs(got - m64).max())
    print(f"{cs} act: float32-numpy vs float64 {np.abs(m32 - m64).max():.3e}; kernel vs float64 {err:.3e}; bound {tol:.3e}")
    assert err <= tol
    assert action.cpu().numpy().tobytes() == got.tobytes()
    assert a.ou_state.cpu().numpy().tobytes() == ou0.tobytes() and a.act_state.cpu().numpy().tobytes() == st0.tobytes()
    # whatever lies in the observations the window rule masks, the bytes are the same
    kept = [ring.kept(-1, b, W) for b in range(B)]
    if any(k < W for k in kept):
        spoilt = ring.obs.copy()
        for b, k in enumerate(kept):
            for age in range(max(k - 1, 0), ring.count):
                spoilt[ring.slot(age), :, b] = np.nan
        a.ring_obs.copy_(torch.as_tensor(spoilt))
        mean2 = torch.zeros(B, A, dtype=torch.float32, device=dev)
        a.act(obs, noise=False, out=dict(mean=mean2))
        assert mean2.cpu().numpy().tobytes() == got.tobytes()
        a.ring_obs.copy_(torch.as_tensor(ring.obs))
    a.act(obs, noise=True, out=dict(action=action, mean=mean))
    eps = PM.eps_batch(11, st0[0], st0[1], A)
    want = DM.ou_step(ou0, eps)
    ou = a.ou_state.cpu().numpy()
    bound = 0.3 * 0.1 * np.spacing(np.abs(eps)) + np.spacing(np.abs(want))
    print(f"{cs} act, noisy step: worst |x - x_model| / bound {np.max(np.abs(ou.astype(np.float64) - want) / bound):.3f}")
    assert np.all(np.abs(ou.astype(np.float64) - want) <= bound)
    assert mean.cpu().numpy().tobytes() == got.tobytes() and np.array_equal(action.cpu().numpy(), got + ou)
    st = a.act_state.cpu().numpy()
    assert np.array_equal(st[0], st0[0]) and np.array_equal(st[1], st0[1] + 1)
    for big in (big_a, big_m, big_o, big_s):
        _bands_intact(big)
    a.close()


# ---- the window rule, exactly -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,base", DE.PROBE_WINDOWS)
def test_the_gathered_states_of_every_age_and_robot_are_exact(dev, window, base):
    """The probe of tests/ddpg_edges.py: s1 read digit by digit off the critic's bias gradient, s0 byte for byte off its weight
    gradient, for every (age, robot) of every probe ring.  No tolerance."""
    n_in = DE.PROBE_ACT + window
    for name, (B, C, _, _) in DE.PROBE_RINGS.items():
        ring, walk = DE.probe_walk(name, window, base)
        a = BatchedDDPGAgent(B, C, device=dev, minibatch=1, gamma=1.0, obs_dim=1, act_dim=DE.PROBE_ACT, window=window, actor_layers=(), critic_layers=())
        assert a.layout["critic"] == [(n_in, 1, 0, n_in)]
        _load_ring(a, ring)
        a.critic_params.zero_()
        idx = torch.as_tensor(np.array([[w["age"], w["robot"]] for w in walk], dtype=np.int32), device=dev)
        # s1: the target critic weighs element f by base^f
        a.target_critic_params.copy_(torch.as_tensor(DE.probe_weights(window, base)))
        grads, losses = [], []
        for n in range(len(walk)):
            g, l = a.critic_grad(idx[n:n + 1])
            grads.append(g.clone()), losses.append(l.clone())
        grads, losses = torch.stack(grads).cpu().numpy(), torch.stack(losses).cpu().numpy()
        for w, g, l in zip(walk, grads, losses):
            digits = [int(-g[-1]) // base ** f % base for f in range(window)]
            assert g[-1] == np.float32(-w["y"]) and l == 0.5 * float(w["y"]) ** 2, (name, w["age"], w["robot"], "s1 read as", digits, "is", w["s1"].tolist(), "done", w["done"])
        # s0: delta = 1 on the probed transition alone
        a.target_critic_params.zero_()
        grads, losses = [], []
        for n, w in enumerate(walk):
            a.ring_reward.zero_()
            a.ring_reward[w["slot"], w["robot"]] = -1.0
            g, l = a.critic_grad(idx[n:n + 1])
            grads.append(g.clone()), losses.append(l.clone())
        grads, losses = torch.stack(grads).cpu().numpy(), torch.stack(losses).cpu().numpy()
        for w, g, l in zip(walk, grads, losses):
            want = np.concatenate([w["action"], w["s0"], np.ones(1, dtype=np.float32)])
            assert g.tobytes() == want.tobytes() and l == 0.5, (name, w["age"], w["robot"], "[action, s0, 1] read as", g.tolist(), "is", want.tolist())
        a.close()
        print(f"window {window}, ring {name}: {len(walk)} transitions, s0 and s1 exact")


# ---- indices outside the ring -----------------------------------------------------------------------------------------------

def test_an_index_outside_the_ring_contributes_exact_zeros_while_m_stays_m(dev):
    c = DE.case(*DE.SPOILT_CASE)
    s = DE.spoilt_model(c, "some")
    a = _agent(dev, c)
    _check_gradients(DE.SPOILT_CASE + (f"{int((~s['live']).sum())} spoilt",), c, a, torch.as_tensor(s["idx"], device=dev).contiguous(), s, dev)
    a.close()


def test_a_minibatch_of_invalid_indices_gives_zero_bytes_and_zero_losses(dev):
    c = DE.case(*DE.SPOILT_CASE)
    idx, live = DE.spoil(c, "all")
    assert not live.any()
    a = _agent(dev, c)
    bigs = _guard_rings(a, dev)
    for which, entry in (("critic", a.critic_grad), ("actor", a.actor_grad)):
        big, out = _guarded((c["lay"][which + "_count"],), torch.float32, dev)
        grad, loss = entry(torch.as_tensor(idx, device=dev).contiguous(), out=out)
        assert grad.cpu().numpy().tobytes() == bytes(4 * grad.numel()), which
        assert float(loss) == 0.0, which
        bigs.append(big)
    for big in bigs:
        _bands_intact(big)
    a.close()


# ---- settings off their defaults ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gamma", DE.GAMMAS)
def test_gamma_off_its_default_matches_the_model(dev, gamma):
    cs = DE.GAMMA_CASE + (gamma,)
    c = DE.case(*cs)
    a = _agent(dev, c)
    idx = torch.as_tensor(c["idx"], device=dev).contiguous()
    _check_gradients(cs, c, a, idx, dict(critic=c["critic"]["m64"], actor=c["actor"]["m64"]), dev)
    other = DE.case(*DE.GAMMA_CASE)["critic"]["m64"]                  # the same ring and networks at 0.99: the test can tell
    moved = DC.deviation(c["critic"]["m64"]["grad"], other["grad"], c["critic"]["names"])
    print(f"gamma {gamma}: the model's critic gradient differs from gamma 0.99's by {moved}")
    assert min(moved.values()) > 10 * max(c["critic"]["tol"].values())
    if gamma == 0.0:                                                  # the targets' (finite) parameters do not matter at all
        first = a.critic_grad(idx)[0].cpu().numpy().tobytes()
        a.target_actor_params.mul_(-3.0), a.target_critic_params.add_(5.0)
        assert a.critic_grad(idx)[0].cpu().numpy().tobytes() == first
    a.close()


@pytest.mark.parametrize("name", sorted(DE.OU_SETTINGS))
def test_ornstein_uhlenbeck_settings_keys_and_counters(dev, name):
    settings = dict(ou_theta=0.5, ou_mu=0.4, ou_sigma=0.3, ou_dt=1e-2)
    settings.update(DE.OU_SETTINGS[name])
    B, A, d = len(DE.OU_KEYS), LOPSIDED["act_dim"], LOPSIDED["obs_dim"]
    a = BatchedDDPGAgent(B, 4, device=dev, minibatch=5, seed=11, **LOPSIDED, **DE.OU_SETTINGS[name])
    rng = np.random.default_rng(len(name))
    obs = torch.as_tensor(rng.normal(size=(d, B)).astype(np.float32), device=dev)
    a.act_state.copy_(torch.as_tensor(np.array([DE.OU_KEYS, DE.OU_COUNTERS], dtype=np.int64)))
    a.ou_state.copy_(torch.as_tensor(rng.normal(0.4, 0.5, size=(B, A)).astype(np.float32)))
    x = a.ou_state.cpu().numpy().copy()
    theta, mu, sigma, dt = (settings[k] for k in ("ou_theta", "ou_mu", "ou_sigma", "ou_dt"))
    for step in range(2):
        out = a.act(obs, noise=True)
        eps = PM.eps_batch(11, DE.OU_KEYS, [k + step for k in DE.OU_COUNTERS], A)
        want = DM.ou_step(x, eps, theta, mu, sigma, dt)
        got = a.ou_state.cpu().numpy()
        assert not np.array_equal(want, DM.ou_step(x, eps)) and np.isfinite(want).all()            # the defaults would give another x
        if sigma == 0.0:                                                                           # no eps enters
            assert got.tobytes() == want.tobytes()
            print(f"OU {name} step {step}: byte-exact")
        else:
            bound = sigma * math.sqrt(dt) * np.spacing(np.abs(eps)) + np.spacing(np.abs(want))
            err = np.abs(got.astype(np.float64) - want)
            print(f"OU {name} step {step}: worst |x - x_model| {err.max():.3e}, worst ratio to its bound {np.max(err / bound):.3f}")
            assert np.all(err <= bound)
        x = got
    assert a.act_state.cpu().numpy().tolist() == [list(DE.OU_KEYS), [k + 2 for k in DE.OU_COUNTERS]]
    assert out["action"].shape == (B, A)
    a.close()


def _torch_adam_rule(got, want):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = np.maximum(4.0 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64), 1e-9)
    return err, bound


@pytest.mark.parametrize("name", sorted(DE.ADAM_SETTINGS))
def test_adam_settings_agree_with_torch(dev, name):
    s = DE.ADAM_SETTINGS[name]
    c = DC.case("lopsided", 3, 4, 6, 5)
    a = BatchedDDPGAgent(3, 4, device=dev, minibatch=5, clipnorm=0.0, actor_lr=1e-3, critic_lr=3e-4, **LOPSIDED, **s)
    rng = np.random.default_rng(len(name))
    for which, buf, lr in (("actor", a.actor_params, 1e-3), ("critic", a.critic_params, 3e-4)):
        buf.copy_(torch.as_tensor(c["params"][which]))
        n = buf.numel()
        twin = buf.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([twin], lr=lr, betas=(s.get("beta1", 0.9), s.get("beta2", 0.999)), eps=s.get("adam_eps", 1e-8))
        plain = buf.detach().clone().requires_grad_(True)
        ref = torch.optim.Adam([plain], lr=lr)
        for k in range(3):
            g = rng.normal(size=n) * np.logspace(-3, 1, n)
            g[::5] = 0.0
            g[1::5] = 1e-12 * np.sign(g[1::5])
            g = torch.as_tensor(g.astype(np.float32), device=dev)
            twin.grad, plain.grad = g.clone(), g.clone()
            opt.step(), ref.step()
            a.adam(which, g)
        err, bound = _torch_adam_rule(buf.detach().cpu().numpy(), twin.detach().cpu().numpy())
        told = float((twin.detach() - plain.detach()).abs().max())
        print(f"adam {name} {which}: worst |p - p_torch| {err.max():.3e}, worst ratio to its bound {np.max(err / bound):.3f}; "
              f"torch at the defaults differs by {told:.3e}")
        assert np.all(err <= bound)
        assert told > 100 * 1e-9 and told > 100 * float(np.abs(err).max())            # the setting tells
    assert a.steps.tolist() == [3, 3]
    a.close()


def test_a_learning_rate_of_zero_moves_the_moments_and_the_count_but_no_parameter(dev):
    a = BatchedDDPGAgent(3, 4, device=dev, minibatch=5, actor_lr=0.0, **LOPSIDED)
    before = a.actor_params.cpu().numpy().tobytes()
    n = a.actor_params.numel()
    g = torch.as_tensor(np.random.default_rng(2).normal(size=n).astype(np.float32), device=dev)
    a.adam("actor", g)
    a.adam("actor", g)
    assert a.actor_params.cpu().numpy().tobytes() == before
    m, v = a.moments[:n].cpu().numpy(), a.moments[n:2 * n].cpu().numpy()
    assert np.all(m != 0) and np.all(v > 0) and a.steps.tolist() == [2, 0]
    assert not a.moments[2 * n:].any()                                                # the critic's are untouched
    a.close()


def test_adam_after_a_million_steps_is_the_headers_formula(dev):
    """pow(beta, t) has underflowed to 0 for both betas: the bias corrections are exactly 1.  m and v are float32 with one rounding
    per operation and must agree to the byte; p is rounded once from float64, where the device's pow and sqrt may differ from
    numpy's in the last bit: one float32 ulp."""
    T = 10 ** 6
    a = BatchedDDPGAgent(3, 4, device=dev, minibatch=5, clipnorm=0.0, actor_lr=1e-3, critic_lr=3e-4, **LOPSIDED)
    rng = np.random.default_rng(12)
    na, nc = a.actor_params.numel(), a.critic_params.numel()
    a.steps.fill_(T)
    a.moments.copy_(torch.as_tensor(np.concatenate([0.1 * rng.normal(size=na), rng.uniform(0, 1, na) ** 4, 0.1 * rng.normal(size=nc),
                                                    rng.uniform(0, 1, nc) ** 4]).astype(np.float32)))
    mom = a.moments.cpu().numpy().copy()
    for which, buf, lr, n, off in (("actor", a.actor_params, 1e-3, na, 0), ("critic", a.critic_params, 3e-4, nc, 2 * na)):
        p0 = buf.cpu().numpy().copy()
        g = (rng.normal(size=n) * np.logspace(-3, 1, n)).astype(np.float32)
        a.adam(which, torch.as_tensor(g, device=dev))
        p, m, v = DM.adam_header(p0, g, mom[off:off + n], mom[off + n:off + 2 * n], T, lr)
        got = a.moments.cpu().numpy()
        assert got[off:off + n].tobytes() == m.tobytes() and got[off + n:off + 2 * n].tobytes() == v.tobytes(), which
        err = np.abs(buf.cpu().numpy().astype(np.float64) - p.astype(np.float64))
        print(f"adam at step 10^6 + 1, {which}: m and v byte-exact; worst |p - p_header| in ulps {np.max(err / np.spacing(np.abs(p))):.3f}, bound 1; "
              f"moved by {np.abs(p - p0).max():.3e}")
        assert np.all(err <= np.spacing(np.abs(p))) and np.abs(p - p0).max() > 1e-5
    assert a.steps.tolist() == [T + 1, T + 1]
    a.close()


@pytest.mark.parametrize("name", ["default", "limits"])
def test_the_clip_and_adam_on_buffers_the_norm_kernel_walks_in_strides(dev, name):
    cfg = DC.CONFIGS[name]
    a = BatchedDDPGAgent(1, 2, device=dev, minibatch=1, clipnorm=1.0, actor_lr=1e-3, critic_lr=3e-4, **cfg)
    rng = np.random.default_rng(len(name))
    strided = 0
    for which, buf, lr in (("actor", a.actor_params, 1e-3), ("critic", a.critic_params, 3e-4)):
        n = buf.numel()
        strided += n > 65536
        buf.copy_(torch.as_tensor(rng.normal(0.0, 0.1, n).astype(np.float32)))
        twin = buf.detach().clone().requires_grad_(True)
        opt = torch.optim.Adam([twin], lr=lr)
        # the tail of the buffer weighs as much as its head: a walk that stops after one stride is far off
        g_in = (rng.normal(size=n) * np.linspace(0.5, 2.0, n)).astype(np.float32)
        want, norm = DM.clip(g_in, 1.0)
        grad = torch.as_tensor(g_in.copy(), device=dev)
        a.adam(which, grad)
        got_norm = float(a.grad_norm)
        rel = abs(got_norm - norm) / norm
        print(f"{name} {which}, {n} floats: norm {got_norm:.17g} vs numpy {norm:.17g}, relative {rel:.3e}, bound {n * 2.0 ** -53:.3e}")
        assert rel <= n * 2.0 ** -53 and norm > 100.0
        got = grad.cpu().numpy()
        ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want))
        print(f"{name} {which}: worst clipped entry {ulps.max():.3f} ulp from the model, bound 1")
        assert np.all(ulps <= 1.0) and not np.array_equal(got, g_in)
        assert math.isclose(math.sqrt(float(np.sum(got.astype(np.float64) ** 2))), 1.0, rel_tol=1e-6)
        twin.grad = grad.clone()                                                      # torch steps with the gradient the kernel clipped
        opt.step()
        err, bound = _torch_adam_rule(buf.detach().cpu().numpy(), twin.detach().cpu().numpy())
        print(f"{name} {which}: adam worst |p - p_torch| {err.max():.3e}, worst ratio to its bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
    assert strided >= 1 and a.steps.tolist() == [1, 1]
    a.close()


def test_the_sample_stream_past_32_bits(dev):
    S = DE.SAMPLE_SHAPE
    a = BatchedDDPGAgent(S["B"], S["C"], device=dev, minibatch=S["M"], seed=DE.SAMPLE_SEED, **DC.CONFIGS["flat"])
    big, idx = _guarded((S["M"], 2), torch.int32, dev)
    for updates in DE.SAMPLE_UPDATES:
        a.ring_state.copy_(torch.tensor([0, S["count"], updates, 0]))
        a.sample(out=idx)
        got = idx.cpu().numpy()
        assert got.tobytes() == DM.sample(DE.SAMPLE_SEED, updates, S["M"], S["count"], S["B"]).tobytes(), updates
        assert got[:, 0].min() >= 1 and got[:, 0].max() <= S["count"] - 1 and got[:, 1].min() >= 0 and got[:, 1].max() < S["B"]
        assert a.ring_state.cpu().tolist() == [0, S["count"], updates, 0]
    _bands_intact(big)
    a.close()


# ---- a spoilt head ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,C", [(3, 4), (67, 7)])
@pytest.mark.parametrize("where", ["below", "above"])
def test_store_with_a_head_outside_the_ring_writes_the_nearest_slot_and_nothing_else(dev, B, C, where):
    """rg_ddpg.h: a head outside [0, C) is clamped, so that a ring state the caller spoilt sends no write outside the ring."""
    raw, slot = (-5, 0) if where == "below" else (C + 3, C - 1)
    d, A = LOPSIDED["obs_dim"], LOPSIDED["act_dim"]
    a = BatchedDDPGAgent(B, C, device=dev, minibatch=5, **LOPSIDED)
    rng = np.random.default_rng(C)
    ring = DM.Ring(C, B, d, A)
    ring.obs[:], ring.action[:], ring.reward[:] = rng.normal(size=ring.obs.shape), rng.normal(size=ring.action.shape), rng.normal(size=ring.reward.shape)
    ring.done[:] = rng.integers(-2, 3, size=ring.done.shape)
    _load_ring(a, ring)
    bigs = _guard_rings(a, dev)
    big_o, a.ou_state = _guarded((B, A), torch.float32, dev, fill=0.5)
    a.ring_state.copy_(torch.tensor([raw, 2, 9, 0]))
    obs, act = rng.normal(size=(d, B)).astype(np.float32), rng.uniform(-1, 1, size=(B, A)).astype(np.float32)
    rew, done = rng.normal(size=B).astype(np.float32), rng.choice(np.array([0, 0, 1, -3], dtype=np.int32), size=B)
    a.store(*(torch.as_tensor(v, device=dev) for v in (obs, act, rew, done)))
    ring.obs[slot], ring.action[slot], ring.reward[slot], ring.done[slot] = obs, act, rew, done
    for name, arr in (("ring_obs", ring.obs), ("ring_action", ring.action), ("ring_reward", ring.reward), ("ring_done", ring.done)):
        assert getattr(a, name).cpu().numpy().tobytes() == arr.tobytes(), name        # the clamped slot written, every other byte as it was
    assert a.ring_state.cpu().tolist() == [(slot + 1) % C, 3, 9, 0]
    ou = np.full((B, A), 0.5, dtype=np.float32)
    ou[done != 0] = 0.0
    assert a.ou_state.cpu().numpy().tobytes() == ou.tobytes()
    for big in bigs + [big_o]:
        _bands_intact(big)
    a.close()
