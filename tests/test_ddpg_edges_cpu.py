"""What tests/ddpg_edges.py promises, asserted on the numpy model alone (no GPU): every case builds within the redraw cap and with
bounds of at most 1e-3, the shapes the kernels branch on are there, the model's gradients on the two widest new configurations
equal torch autograd, the additions to the model (the live mask, the tile-ordered sum, the header's Adam) are what they claim,
the window probe's walk meets every way a window can be cut, the spoilt index lists hold every kind of bad index, and the
library accepts every configuration and setting used.  The figures are printed before they are asserted."""
import math

import numpy as np
import pytest
import torch

from robot_gym_amd.core import ddpg_abi
from tests import ddpg_cases as DC
from tests import ddpg_edges as DE
from tests import ddpg_model as DM
from tests import policy_model as PM
from tests import ppo_update_model as UM
from tests.test_ddpg_cpu import _torch_net

ID = lambda cs: "-".join(str(v) for v in cs)


# ---- the cases --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", DE.CASES + [DE.GAMMA_CASE + (g,) for g in DE.GAMMAS], ids=ID)
def test_every_edge_case_builds_within_the_redraw_cap_and_its_bounds_stay_small(cs):
    c = DE.case(*cs)
    ring, idx, M = c["ring"], c["idx"], c["M"]
    assert c["redrawn"] <= 0.25
    assert ring.count == min(c["ticks"], c["C"]) >= 2 and ring.head == c["ticks"] % c["C"]
    assert idx.shape == (M, 2) and idx[:, 0].min() >= 1 and idx[:, 0].max() <= ring.count - 1 and idx[:, 1].min() >= 0 and idx[:, 1].max() < c["B"]
    assert c["tiled"] == (M > ddpg_abi.TILE * ddpg_abi.MAX_GROUPS)
    for which in ("critic", "actor"):
        r = c[which]
        print(f"{cs} {which}: redrawn {c['redrawn']:.4f}; float32-numpy vs float64 {max(r['dev32_plain'].values()):.3e}"
              + (f", summed in the header's order {max(r['dev32'].values()):.3e}" if c["tiled"] else "") + f"; bounds {r['tol']} loss {r['loss_tol']:.3e}")
        assert all(math.isfinite(v) and v >= 0 for v in r["tol"].values()) and max(r["tol"].values()) <= 1e-3, (which, r["tol"])
        assert math.isfinite(r["loss_tol"]) and r["loss_tol"] <= 1e-3
        assert np.all(np.isfinite(r["m64"]["grad"])) and math.isfinite(r["m64"]["loss"])
        for k, s in r["names"].items():                      # every tensor learns: the one-neuron layer is alive
            assert np.abs(r["m64"]["grad"][s]).max() > 0, (which, k)
        if c["tiled"]:
            # one tile of 16 samples is 16 / M of a gradient: the bound must stay clearly below a dropped tile
            assert max(r["tol"].values()) <= 0.1 * ddpg_abi.TILE / M
            assert max(r["dev32"].values()) <= max(r["dev32_plain"].values())


def test_the_cases_cover_the_shapes_the_issue_lists():
    Bs, Ms = ({cs[k] for cs in DE.CASES} for k in (1, 4))
    assert Bs >= {1, 15, 16, 17, 67} and Ms == {1, 15, 16, 17, 100, 4096, 4097, 65536}
    assert {cs[1] for cs in DE.ACT_CASES} >= {1, 15, 16, 17, 67} and set(DE.ACT_CASES) <= set(DE.CASES)
    assert {cs[0] for cs in DE.CASES} == set(DE.CONFIGS) | {"lopsided"} and ("lopsided", 67, 7, 9, 65536) in DE.CASES
    assert any(cs[3] > cs[2] for cs in DE.CASES) and any(cs[3] <= cs[2] for cs in DE.CASES)          # wrapped and not
    assert DE.FULL == ddpg_abi.TILE * ddpg_abi.MAX_GROUPS == 4096 and DE.MAX_GROUPS == ddpg_abi.MAX_GROUPS and DE.MAX_MINIBATCH == 1 << 16
    assert not set(DE.CONFIGS) & set(DC.CONFIGS)
    C = DE.CONFIGS
    widths = {w for cfg in C.values() for w in cfg["actor_layers"] + cfg["critic_layers"]}
    assert widths >= {1, 63, 64, 65, 255, 256}
    assert C["obs64"]["obs_dim"] == ddpg_abi.MAX_OBS and C["obs64"]["obs_dim"] * C["obs64"]["window"] == ddpg_abi.MAX_INPUT
    assert {cfg["act_dim"] for cfg in C.values()} >= {1, 4}
    assert C["wave_edges"]["act_dim"] + C["wave_edges"]["obs_dim"] * C["wave_edges"]["window"] == 130
    assert C["long_window"]["window"] == ddpg_abi.MAX_WINDOW and ("long_window", 17, 2, 5, 15) in DE.CASES     # a window four times its ring
    assert C["critic_deeper"]["actor_layers"] == () and len(C["critic_deeper"]["critic_layers"]) == 3
    assert C["long_window"]["critic_layers"] == () and len(C["long_window"]["actor_layers"]) == 3
    assert C["head_only"] == dict(obs_dim=1, act_dim=1, window=1, actor_layers=(), critic_layers=())
    for name, cfg in C.items():
        assert ddpg_abi.param_layout(**cfg) == DM.layout(**cfg) == DE.net(name)[1], name
    for settings in list(DE.OU_SETTINGS.values()) + list(DE.ADAM_SETTINGS.values()) + [dict(gamma=g) for g in DE.GAMMAS] + \
            [dict(actor_lr=0.0), dict(seed=DE.SAMPLE_SEED), dict(minibatch=DE.MAX_MINIBATCH, **DC.CONFIGS["lopsided"])]:
        rc, msg = ddpg_abi.create_status(ddpg_abi.make_cconfig(**settings))
        assert rc == 0, (settings, msg)


@pytest.mark.parametrize("cs", [("wave_edges", 15, 4, 6, 17), ("critic_deeper", 15, 7, 10, 16)], ids=ID)
def test_the_model_on_the_new_configurations_equals_autograd(cs):
    c = DE.case(*cs)
    ring, idx, lay, W = c["ring"], c["idx"], c["lay"], c["cfg"]["window"]
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in c["params"].items()}
    ages, robots = idx[:, 0], idx[:, 1]
    slots = np.array([ring.slot(int(a)) for a in ages])
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    s0, s1 = t(ring.states(ages, robots, W)), t(ring.states(ages - 1, robots, W))
    action, reward, nd = t(ring.action[slots, robots]), t(ring.reward[slots, robots]), t(1.0 - (ring.done[slots, robots] != 0))
    with torch.no_grad():
        a1 = _torch_net(P["target_actor"], lay["actor"], s1, "tanh")
        y = reward + c["gamma"] * nd * _torch_net(P["target_critic"], lay["critic"], torch.cat([a1, s1], dim=1), "linear")[:, 0]
    q = _torch_net(P["critic"], lay["critic"], torch.cat([action, s0], dim=1), "linear")[:, 0]
    closs = (0.5 * (y - q) ** 2).sum() / len(q)
    closs.backward()
    want, got = P["critic"].grad.numpy().copy(), c["critic"]["m64"]
    assert math.isclose(got["loss"], float(closs.detach()), rel_tol=1e-12)
    assert np.abs(want).max() > 0 and np.allclose(got["grad"], want, rtol=1e-10, atol=1e-13 * np.abs(want).max())
    P["critic"].grad = None
    mu = _torch_net(P["actor"], lay["actor"], s0, "tanh")
    aloss = -_torch_net(P["critic"], lay["critic"], torch.cat([mu, s0], dim=1), "linear")[:, 0].sum() / len(idx)
    aloss.backward()
    want, got = P["actor"].grad.numpy(), c["actor"]["m64"]
    assert math.isclose(got["loss"], float(aloss.detach()), rel_tol=1e-12)
    assert np.abs(want).max() > 0 and np.allclose(got["grad"], want, rtol=1e-10, atol=1e-13 * np.abs(want).max())


# ---- the additions to the model -----------------------------------------------------------------------------------------------

def test_tile_sum_is_a_literal_loop_in_the_headers_order():
    rng = np.random.default_rng(4)
    M, tile, G = 83, 16, 2                                   # six tiles, the last ragged: workgroup 0 walks tiles 0, 2, 4
    x, d = rng.normal(size=(M, 3)).astype(np.float32), (rng.normal(size=(M, 2)) * np.logspace(-3, 3, M)[:, None]).astype(np.float32)
    got = UM.tile_sum(x, d, tile, G)
    f = np.float32
    want = np.zeros((3, 2), dtype=np.float32)
    for i in range(3):
        for j in range(2):
            slabs = [f(0.0)] * G
            for t in range(-(-M // tile)):
                v = f(0.0)
                for s in range(t * tile, min((t + 1) * tile, M)):
                    v = f(v + f(x[s, i] * d[s, j]))
                slabs[t % G] = f(slabs[t % G] + v)
            want[i, j] = f(float(slabs[0]) + float(slabs[1]))
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert not np.array_equal(got, x.T @ d)                  # the order matters at these magnitudes
    assert np.allclose(got, x.astype(np.float64).T @ d.astype(np.float64), rtol=0, atol=1e-3 * np.abs(d).max())
    # through backward: the float64 model ignores the option; the float32 model stays close to it
    c = DE.case("long_window", 17, 2, 5, 15)
    p, lay, W = c["params"], c["lay"], c["cfg"]["window"]
    run = lambda **kw: DM.actor_grad(c["ring"], c["idx"], p["actor"], p["critic"], lay, W, **kw)["grad"]
    assert np.array_equal(run(tiles=(16, 256)), run())
    assert np.allclose(run(dtype=np.float32, tiles=(16, 256)), run(), rtol=0, atol=1e-5 * np.abs(run()).max())


@pytest.mark.parametrize("kind", ["some", "all"])
def test_a_dead_sample_of_the_model_contributes_nothing_while_m_stays_m(kind):
    c = DE.case(*DE.SPOILT_CASE)
    s = DE.spoilt_model(c, kind)
    idx, live, M = s["idx"], s["live"], c["M"]
    count, B = c["ring"].count, c["B"]
    valid = (idx[:, 0] >= 1) & (idx[:, 0] < count) & (idx[:, 1] >= 0) & (idx[:, 1] < B)
    assert np.array_equal(valid, live)                                               # the mask is the header's rule
    bad = idx[~live]
    ages, robots = set(bad[:, 0].tolist()), set(bad[:, 1].tolist())
    assert {0, count, -1, DE.INT_MIN} <= ages and {B, -1, DE.INT_MAX} <= robots
    ring, lay, p, W = c["ring"], c["lay"], c["params"], c["cfg"]["window"]
    if kind == "all":
        assert not live.any()
        for which in ("critic", "actor"):
            assert not s[which]["grad"].any() and s[which]["loss"] == 0.0
        return
    assert not live[2 * DE.TILE:3 * DE.TILE].any() and live[:DE.TILE].any() and (~live[:DE.TILE]).any() and live[-1]    # a whole tile, and single entries
    sub, n = idx[live], int(live.sum())
    for which, run in (("critic", lambda i, **kw: DM.critic_grad(ring, i, p["critic"], p["target_actor"], p["target_critic"], lay, W, c["gamma"], **kw)),
                       ("actor", lambda i, **kw: DM.actor_grad(ring, i, p["actor"], p["critic"], lay, W, **kw))):
        alone = run(sub)                                                             # the live samples as a minibatch of their own: 1 / n in place of 1 / M
        assert math.isclose(s[which]["loss"], alone["loss"] * n / M, rel_tol=1e-12)
        assert np.allclose(s[which]["grad"], alone["grad"] * n / M, rtol=1e-10, atol=1e-14)
        full = c[which]["m64"]
        moved = DC.deviation(s[which]["grad"], full["grad"], c[which]["names"])
        print(f"{which}: dropping {M - n} of {M} samples moves the gradient by {moved}; bounds {c[which]['tol']}")
        assert min(moved.values()) > 100 * max(c[which]["tol"].values())            # the test can tell
        assert np.array_equal(run(c["idx"], live=np.ones(M, dtype=bool))["grad"], full["grad"])


def test_adam_header_is_the_formula_of_the_model_with_the_headers_roundings():
    rng = np.random.default_rng(6)
    n = 50
    p, g = rng.normal(size=n).astype(np.float32), (rng.normal(size=n) * np.logspace(-3, 1, n)).astype(np.float32)
    m, v = (0.1 * rng.normal(size=n)).astype(np.float32), (rng.uniform(0, 1, n) ** 2).astype(np.float32)
    for t, kw in ((0, {}), (4, dict(beta1=0.0)), (4, dict(beta2=0.0)), (4, dict(eps=1e-3)), (10 ** 6, {})):
        p1, m1, v1 = DM.adam_header(p, g, m, v, t, 1e-3, **kw)
        assert p1.dtype == m1.dtype == v1.dtype == np.float32
        q, mq, vq, _ = DM.adam_step(p.astype(np.float64), g.astype(np.float64), m.astype(np.float64), v.astype(np.float64), t, 1e-3, **kw)
        assert np.allclose(m1, mq, rtol=1e-6, atol=1e-12) and np.allclose(v1, vq, rtol=1e-6, atol=1e-12)
        # m and v carry float32's 2^-24 per operation into the step; p is rounded once
        assert np.all(np.abs(p1.astype(np.float64) - q) <= 1e-6 * np.abs(q - p) + np.spacing(np.abs(p1)))
    assert math.pow(0.9, 10 ** 6 + 1) == 0.0 and math.pow(0.999, 10 ** 6 + 1) == 0.0         # both bias corrections have underflowed to 1


# ---- the window probe -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window,base", DE.PROBE_WINDOWS)
def test_the_probe_walk_meets_every_kept_count_and_every_way_a_window_is_cut(window, base):
    """Over the rings of a window: s0 and s1 keep every count 1 .. W, the s1 probe spells every number of digits 0 .. W but 1
    (0: done is set at the probed age, nd = 0; with W > 1, s1 keeps one element exactly when that done is set, so a single digit
    is never spelt), a window is cut by a done, by `count` in a ring that has not wrapped, and by `count` in one
    that has (the next slot back is the newest tick's), a kept window crosses from slot 0 to slot C - 1, and a done lies at the
    probed age, at age - 1, inside the window and just outside it.  Done takes 1, -1 and 2^31 - 1."""
    assert base ** window <= 2 ** 24
    kept0, kept1, digits1, cuts, crossed, rel, dones = set(), set(), set(), set(), False, set(), set()
    for name, (B, C, ticks, marks) in DE.PROBE_RINGS.items():
        ring, walk = DE.probe_walk(name, window, base)
        assert (ring.head, ring.count) == (ticks % C, min(ticks, C)) and len(walk) == (ring.count - 1) * B
        codes = ring.obs.reshape(-1)
        assert codes.min() >= 1 and codes.max() <= base - 1 and np.all(codes == np.round(codes))
        dones |= set(marks.values())
        for w in walk:
            assert 0 <= w["y"] < 2 ** 24 and (w["y"] == 0) == (w["done"] != 0)
            kept0.add(w["kept0"])
            kept1.add(w["kept1"])
            digits1.add(0 if w["done"] else w["kept1"])
            cuts |= {(0, w["cut0"]), (1, w["cut1"])}
            crossed |= w["crosses0"]
            for a in range(ring.count):
                if ring.done[ring.slot(a), w["robot"]] != 0:
                    rel.add(a - w["age"])
    print(f"window {window}: s0 keeps {sorted(kept0)}, s1 spells {sorted(digits1)} digits, cuts {sorted(cuts, key=str)}, a done at {sorted(rel)} of the probed age")
    assert kept0 == kept1 == set(range(1, window + 1)) and digits1 == set(range(0, window + 1)) - ({1} if window > 1 else set())
    want = {(s, why) for s in (0, 1) for why in ((None,) if window == 1 else (None, "done", "count", "wrap"))}
    assert cuts >= want and (crossed or window == 1)
    assert {0, -1, window} <= rel and (window == 1 or any(0 < r < window for r in rel))
    assert dones == {1, -1, DE.INT_MAX}


def test_the_probe_expects_what_the_literal_known_answers_say():
    """DM.Ring.state's literal known answers are in tests/test_ddpg_cpu.py; here the probe's own numbers on the smallest ring,
    written out by hand: two robots, capacity 2, five ticks stored (ticks 3 and 4 are held, head 1)."""
    ring, walk = DE.probe_walk("two_wrapped", 3, 16)
    assert (ring.head, ring.count) == (1, 2) and len(walk) == 2
    w0, w1 = walk                                            # the transition at age 1 (tick 3) of robots 0 and 1
    # codes 1 + (t + 5 b) mod 15: tick 3 -> 4, 9; tick 4 -> 5, 10.  Robot 0's done at tick 4 (age 0) ends s1 itself and cuts nothing
    assert w0["s0"].tolist() == [0.0, 0.0, 4.0] and w0["s1"].tolist() == [0.0, 4.0, 5.0] and w0["y"] == 4 * 16 + 5 * 256 and w0["done"] == 0
    # robot 1's done at tick 3 (the probed age): nd = 0, and s1 does not look back across it
    assert w1["s0"].tolist() == [0.0, 0.0, 9.0] and w1["done"] == DE.INT_MAX and w1["y"] == 0 and w1["s1"].tolist() == [0.0, 0.0, 10.0]
    assert w0["action"].tolist() == [-4.0, -4.125] and w1["action"].tolist() == [-4.25, -4.375]
    assert DE.probe_weights(3, 16).tolist() == [0.0, 0.0, 1.0, 16.0, 256.0, 0.0]
    ring, walk = DE.probe_walk("unwrapped", 3, 16)
    assert ring.count == 4 and set(ring.obs[4:].reshape(-1).tolist()) <= set(range(1, 16)) and not ring.done[4:].any()   # codes where nothing was stored


def test_ou_settings_keys_and_the_sample_shape_are_what_the_gpu_tests_say():
    D = ddpg_abi.DEFAULTS
    for name, s in DE.OU_SETTINGS.items():
        assert all(v != D[k] for k, v in s.items()), name
    assert len(DE.OU_SETTINGS["all"]) == 4 and {k for s in DE.OU_SETTINGS.values() for k in s} == {"ou_theta", "ou_mu", "ou_sigma", "ou_dt"}
    assert any(k < 0 for k in DE.OU_KEYS) and any(k > 2 ** 40 for k in DE.OU_KEYS) and 2 ** 40 in DE.OU_COUNTERS and len(DE.OU_KEYS) == len(DE.OU_COUNTERS)
    e = [PM.eps(0, k, c, 0) for k, c in zip(DE.OU_KEYS, DE.OU_COUNTERS)]
    assert len(set(float(v) for v in e)) == len(e) and all(math.isfinite(float(v)) for v in e)
    assert PM.eps(0, -1, 2 ** 40, 0) == PM.eps(0, 2 ** 64 - 1, 2 ** 40, 0) != PM.eps(0, 2 ** 32 - 1, 2 ** 40, 0)     # a key is its 64 bits
    # sigma = 0: eps enters multiplied by exactly 0
    x = np.array([0.25, -3.0], dtype=np.float32)
    assert DM.ou_step(x, [5.0, -7.0], sigma=0.0).tobytes() == DM.ou_step(x, [0.0, 0.0], sigma=0.0).tobytes()
    S = DE.SAMPLE_SHAPE
    n, B = S["count"] - 1, S["B"]
    assert math.gcd(n, B) == 1 and all(v & (v - 1) for v in (n, B)) and S["count"] <= S["C"]
    for updates in DE.SAMPLE_UPDATES:
        idx = DM.sample(DE.SAMPLE_SEED, updates, S["M"], S["count"], B)
        # a hash cut to 32 bits before the modulo would give other indices
        cut = np.array([[1 + (DM.sample_hash(DE.SAMPLE_SEED, updates, m, 0) & 0xFFFFFFFF) % n, (DM.sample_hash(DE.SAMPLE_SEED, updates, m, 1) & 0xFFFFFFFF) % B]
                        for m in range(S["M"])])
        assert (idx != cut).mean() > 0.5
        if updates >> 32:
            assert not np.array_equal(idx, DM.sample(DE.SAMPLE_SEED, updates & 0xFFFFFFFF, S["M"], S["count"], B))  # nor is `updates` cut
        assert not np.array_equal(idx, DM.sample(DE.SAMPLE_SEED & 0xFFFFFFFF, updates, S["M"], S["count"], B))
