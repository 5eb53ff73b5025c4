"""Without a GPU: the exact float32 model of the networks (tests/policy_model.py: fma32, forward_exact) against the C
library's fmaf, the inputs of tests/test_policy_edges_gpu.py (tests/policy_edges.py) on the model alone, so that every case
is known to meet what it is there for before a GPU is used, and the argument checks of BatchedGaussianPolicy.record and
.returns on a host-only policy."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import BatchedGaussianPolicy, RolloutBuffer
from robot_gym_amd.core import policy_abi
from tests import policy_edges as E
from tests import policy_model as PM

f32 = np.float32


# ---- fma32 against fmaf -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fmaf():
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    libm.fmaf.restype = ctypes.c_float

    def call(w, x, acc):
        w, x, acc = (np.asarray(v, dtype=f32).ravel().tolist() for v in (w, x, acc))
        return np.array([libm.fmaf(a, b, c) for a, b, c in zip(w, x, acc)], dtype=f32)
    return call


def _bits(a):
    return np.asarray(a, dtype=f32).view(np.uint32)


def _naive(w, x, acc):
    """float32(float64(w) * x + acc): the sum is rounded twice."""
    return (np.asarray(w, f32).astype(np.float64) * np.asarray(x, f32).astype(np.float64) + np.asarray(acc, f32).astype(np.float64)).astype(f32)


def test_fma32_equals_fmaf_on_random_triples(fmaf):
    rng = np.random.default_rng(800)
    n = 120_000
    # the networks' magnitudes: Glorot weights, normalised observations clipped at 5 and relu activations (zeros among them),
    # partial sums of a few units
    w = rng.uniform(-0.6, 0.6, n).astype(f32)
    x = np.clip(rng.normal(0.0, 2.5, n), -5.0, 5.0).astype(f32)
    x[rng.random(n) < 0.2] = 0.0
    acc = rng.normal(0.0, 3.0, n).astype(f32)
    acc[rng.random(n) < 0.05] = 0.0
    # and exponents apart: unclipped observations, tiny weights, cancelling sums, partial sums far below the product
    m = 40_000
    w2 = (rng.uniform(-1, 1, m) * 2.0 ** rng.integers(-30, 8, m)).astype(f32)
    x2 = (rng.uniform(-1, 1, m) * 2.0 ** rng.integers(-20, 8, m)).astype(f32)
    acc2 = np.where(rng.random(m) < 0.5, -(w2.astype(np.float64) * x2).astype(f32) * f32(1 + 2.0 ** -20), rng.normal(size=m) * 2.0 ** rng.integers(-40, 10, m)).astype(f32)
    w, x, acc = np.concatenate((w, w2)), np.concatenate((x, x2)), np.concatenate((acc, acc2))
    assert len(w) >= 100_000
    got, want = PM.fma32(w, x, acc), fmaf(w, x, acc)
    assert got.dtype == f32 and np.array_equal(_bits(got), _bits(want))
    print(f"fma32 == fmaf on {len(w)} triples; the twice-rounded sum differs on {(_bits(_naive(w, x, acc)) != _bits(want)).sum()} of them")


def _round_to_f32(q):
    """The float32 nearest the rational q, ties to even, found among the neighbours of a first guess by exact comparison."""
    guess = f32(float(q))
    cands = sorted({float(np.nextafter(guess, f32(-np.inf))), float(guess), float(np.nextafter(guess, f32(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - q), int(_bits(c)) & 1))
    return f32(best)


def double_rounding_triples():
    """w x + acc whose float64-rounded sum is exactly a float32 midpoint while the true sum is not: |w x| = 2^-24 (1 - j^2 2^-46)
    lies j^2 2^-70 below half a float32 ulp of acc = +-(1 + k 2^-23).  Added to acc the true sum is just BELOW the midpoint
    above acc; subtracted it is just ABOVE the midpoint below acc.  Both for positive and negative acc, and for even and odd
    k, so that ties-to-even takes the wrong neighbour in half of them."""
    w, x, acc = [], [], []
    for j in (1, 2, 3, 7, 50, 200):            # j^2 2^-70 stays below half a float64 ulp of the sum
        a = j * 2.0 ** -23
        for k in (1, 2, 3, 4):
            for direction in (1.0, -1.0):
                for sign in (1.0, -1.0):
                    w.append(sign * direction * (1.0 + a))
                    x.append(2.0 ** -24 * (1.0 - a))
                    acc.append(sign * (1.0 + k * 2.0 ** -23))
    return np.array(w, dtype=f32), np.array(x, dtype=f32), np.array(acc, dtype=f32)


def test_fma32_on_constructed_double_rounding_triples(fmaf):
    w, x, acc = double_rounding_triples()
    assert np.array_equal(w.astype(np.float64), np.array(w, dtype=np.float64)) and len(w) == 96
    kinds = set()
    truth = []
    for a, b, c in zip(w.tolist(), x.tolist(), acc.tolist()):
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        s = a * b + c                                        # the product is exact, the sum rounded once
        lo, hi = f32(s), None
        assert float(lo) != s                                # not a float32 ...
        hi = np.nextafter(lo, f32(np.inf) if s > float(lo) else f32(-np.inf))
        assert (Fraction(float(lo)) + Fraction(float(hi))) / 2 == Fraction(s)    # ... but exactly between two
        assert exact != Fraction(s)                          # and the true sum is not
        kinds.add((exact > Fraction(s), c > 0))
        truth.append(_round_to_f32(exact))
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}   # both directions, both signs
    truth = np.array(truth, dtype=f32)
    want = fmaf(w, x, acc)
    assert np.array_equal(_bits(want), _bits(truth))         # the C library is right by exact rational arithmetic
    assert np.array_equal(_bits(PM.fma32(w, x, acc)), _bits(want))
    wrong = _bits(_naive(w, x, acc)) != _bits(want)
    print(f"the twice-rounded sum is wrong on {wrong.sum()} of {len(w)} constructed triples")
    assert wrong.sum() >= len(w) // 4                        # the construction bites: ties-to-even goes the wrong way


def test_fma32_broadcasts_and_keeps_exact_cases():
    z = PM.fma32(np.array([[1.5], [2.0]], dtype=f32), np.array([2.0, -4.0], dtype=f32), f32(0.25))
    assert z.shape == (2, 2) and z.tolist() == [[3.25, -5.75], [4.25, -7.75]]
    assert PM.fma32(f32(0.0), f32(5.0), f32(-3.0)) == f32(-3.0) and PM.fma32(f32(1.0), f32(7.0), f32(0.0)) == f32(7.0)
    big = f32(3e38)
    assert np.isinf(PM.fma32(big, f32(2.0), big)) and PM.fma32(big, f32(2.0), -big) == big   # no overflow of the exact product


# ---- forward_exact --------------------------------------------------------------------------------------------------

def test_forward_exact_hand_worked_layer():
    # one hidden neuron pair and a head: fma order, bias after the sum, relu as where(v > 0)
    W0 = np.array([[1.0, -1.0], [0.5, 0.25]], dtype=f32)
    b0 = np.array([0.5, -10.0], dtype=f32)
    W1 = np.array([[2.0], [3.0]], dtype=f32)
    b1 = np.array([-1.0], dtype=f32)
    x = np.array([[2.0, 4.0]], dtype=f32)
    assert PM.forward_exact(x, [(W0, b0), (W1, b1)], "linear").tolist() == [[2.0 * 4.5 + 0.0 - 1.0]]
    assert PM.forward_exact(x, [(W0, b0)], "tanh").tolist() == [[4.5, -11.0]]     # the head's pre-activation, no relu
    # fused: a^2 = 1 + 2^-11 + 2^-24 keeps its last bit inside the fma; rounded on its own it would lose it (a tie, to even)
    a = f32(1.0 + 2.0 ** -12)
    W = np.array([[-(1.0 + 2.0 ** -11)], [a]], dtype=f32)
    zero = np.zeros(1, dtype=f32)
    assert PM.forward_exact(np.array([[1.0, a]], dtype=f32), [(W, zero)], "linear")[0, 0] == f32(2.0 ** -24)
    assert PM.forward(np.array([[1.0, a]], dtype=f32), [(W, zero)], "linear", f32)[0, 0] == 0.0      # the unfused float32 model
    # in order: 2^-24 first, then 1 (the sum ties to even: 1), then -1 gives 0; the other order keeps 2^-24
    t = f32(2.0 ** -12)
    W = np.array([[t], [1.0], [-1.0]], dtype=f32)
    assert PM.forward_exact(np.array([[t, 1.0, 1.0]], dtype=f32), [(W, zero)], "linear")[0, 0] == 0.0
    assert PM.forward_exact(np.array([[1.0, 1.0, t]], dtype=f32), [(W[[1, 2, 0]], zero)], "linear")[0, 0] == f32(2.0 ** -24)
    # the bias comes after the sum: (2^-24 + 1) - 1 with the bias 1 added last is 0 + ... = 1 - 1
    W = np.array([[t], [-1.0]], dtype=f32)
    assert PM.forward_exact(np.array([[t, 1.0]], dtype=f32), [(W, np.ones(1, dtype=f32))], "linear")[0, 0] == f32(2.0 ** -24)   # bias first would give 0


def test_forward_exact_agrees_with_the_float64_model_within_the_8x_rule():
    for name, batches in E.BATCHES.items():
        c = E.act_case(name, 13)
        m64, m32 = c["m64"], c["m32"]
        dev_mean = float(np.abs(m32["mean"].astype(np.float64) - m64["mean"]).max())
        dev_value = float(np.abs(m32["value"].astype(np.float64) - m64["value"]).max())
        tol_mean, tol_value = max(8 * dev_mean, 1e-6), max(8 * dev_value, 1e-6)
        err_value = float(np.abs(c["value_exact"].astype(np.float64) - m64["value"]).max())
        err_mean = float(np.abs(np.tanh(c["pre_exact"].astype(np.float64)) - m64["mean"]).max())
        print(f"{name}: exact model vs float64 model: mean {err_mean:.3e} (bound {tol_mean:.3e}), value {err_value:.3e} (bound {tol_value:.3e})")
        assert c["value_exact"].dtype == f32 and c["pre_exact"].dtype == f32 and c["pre_exact"].shape == (13, c["cfg"]["act_dim"])
        assert err_mean <= tol_mean and err_value <= tol_value


# ---- the edge inputs on the model alone ---------------------------------------------------------------------------------

def test_configurations_are_what_the_table_says():
    n = {name: (len(c["policy_layers"]), len(c["value_layers"])) for name, c in E.CONFIGS.items()}
    assert n == {"head_only": (0, 0), "policy_deeper": (3, 0), "value_deeper": (0, 3), "wave_edges": (3, 3)}
    assert n["policy_deeper"][0] > n["policy_deeper"][1] and n["value_deeper"][1] > n["value_deeper"][0]   # the idle network has fewer layers
    w = E.CONFIGS["wave_edges"]
    assert set(w["policy_layers"] + w["value_layers"]) == {63, 64, 65, 255, 256, 1} and w["obs_dim"] == 63 and w["act_dim"] == 4
    assert (E.CONFIGS["head_only"]["obs_dim"], E.CONFIGS["head_only"]["act_dim"]) == (1, 1)
    assert all(b[:2] == (1, 13) for b in E.BATCHES.values()) and E.BATCHES["wave_edges"] == (1, 13, 1037)
    assert 13 % policy_abi.TILE != 0 and 13 > policy_abi.TILE and 1037 % policy_abi.TILE != 0
    for name in list(E.CONFIGS) + ["transform"]:
        lay, pp, vp = E.params(name)
        cfg = E.config_of(name)
        assert lay == policy_abi.param_layout(**cfg)
        for p, layers in ((pp, lay["policy"]), (vp, lay["value"])):
            for i, o, wo, bo in layers:
                assert len(np.unique(p[wo:wo + i * o])) > 0.99 * i * o and np.all(p[bo:bo + o] != 0)    # distinct weights (but for float32 collisions), non-zero biases
        logstd = pp[lay["logstd_offset"]:]
        assert len(logstd) == cfg["act_dim"] and len(np.unique(logstd)) == cfg["act_dim"]


def test_act_states_are_beyond_32_bits_and_a_truncated_draw_differs():
    assert {-1, -2 ** 63, 2 ** 32 + 5, 2 ** 40} <= set(E.KEYS) and {2 ** 32 - 1, 2 ** 62} <= set(E.COUNTERS)
    assert 2 ** 63 - 1 not in E.COUNTERS and E.SEED >= 2 ** 63
    keys, counters = E.act_states(E.POOL)
    assert keys.dtype == np.int64 and counters.dtype == np.int64 and keys[:len(E.KEYS)].tolist() == list(E.KEYS)
    assert counters[:len(E.COUNTERS)].tolist() == list(E.COUNTERS)
    assert counters.min() >= 0 and counters.max() < 2 ** 63 - 1 and len(np.unique(keys)) == E.POOL
    assert np.array_equal(E.act_states(13)[0], keys[:13]) and np.array_equal(E.act_states(1)[1], counters[:1])
    draw = lambda seed, k, c: tuple(PM.eps(seed, k, c, a) for a in range(4))
    for b in range(64):                   # every robot of the first tiles: its key and counter as they are against each 32-bit cast
        k, c = int(keys[b]), int(counters[b])
        full = draw(E.SEED, k, c)
        changed = 0
        for t in E.truncations(k & PM.M64):
            if t & PM.M64 != k & PM.M64:
                changed += 1
                assert draw(E.SEED, t, c) != full, (b, k)
        assert changed >= 1, k            # at least one kind of cast changes every key (-1 survives a sign-extending one only)
        for t in E.truncations(c):
            if t != c:
                assert draw(E.SEED, k, t) != full, (b, c)
        assert draw(E.SEED & E.M32, k, c) != full
        assert draw(E.SEED, k, c + 1) != draw(E.SEED, k, (c + 1) & E.M32) or c + 1 <= E.M32
    # each kind of cast is caught by a key of the FIRST robot already (a batch of one), and the crossing increment is seen
    assert all(t != E.KEYS[0] for t in E.truncations(E.KEYS[0]))
    assert E.COUNTERS[0] + 1 == 2 ** 32 and draw(E.SEED, E.KEYS[0], 2 ** 32) != draw(E.SEED, E.KEYS[0], 0)
    assert sum(1 for c in counters[:64] if c > E.M32) >= 32


@pytest.mark.parametrize("d", [1, 5, 7, 63, 64])
def test_normaliser_states_and_observations_meet_their_edges(d):
    empty, one, const, pool = (E.norm_state(k, d).reshape(3, -1) for k in E.NORM_STATES)
    assert not empty.any()
    assert np.all(one[0, :d] == 1) and one[0, PM.NORM_REWARD] == 1 and not one[2].any() and np.all(one[1, :d] != 0)
    assert const[0, 0] == 50 and const[1, E.CONSTANT_COL] == E.CONSTANT_VALUE and const[2, E.CONSTANT_COL] == 0.0
    assert d == 1 or np.all(const[2, 1:d] > 0)
    assert pool[0, 0] == 341 and np.all(pool[2, :d] > 0)
    B = 13 if d == 64 else E.POOL
    for kind in E.NORM_STATES:
        x5, v, scaled = E.transform_x(kind, 5.0, d, B)
        x0, _, _ = E.transform_x(kind, 0.0, d, B)
        assert scaled.all() == (kind in ("constant", "pool"))
        clipped = np.abs(v) >= 5.0
        assert clipped.any() and (~clipped).any()                              # both clipped and unclipped entries
        assert np.all(np.abs(x5[clipped]) == 5.0) and np.all(np.abs(x5[~clipped]) < 5.0 + 1e-6)
        assert np.array_equal(x0, v.astype(f32)) and np.abs(x0).max() > 5.0    # obs_clip = 0 passes the large values on
        if kind == "pool":
            assert np.abs(x0).max() > 30.0                                     # out to 40 sigma of the statistics
        if kind == "constant":
            assert x0[0, E.CONSTANT_COL] == 0.0 and (B < 3 or abs(x0[2, E.CONSTANT_COL] - 3.0) < 1e-2)   # 0.03 / (sqrt(1e-4) + 1e-8)


def test_act_cases_reach_the_clip_in_every_configuration():
    for name, batches in E.BATCHES.items():
        for B in batches:
            kind = "empty" if B == 1 else "count1"
            c = E.act_case(name, B, kind)
            assert c["m64"]["x"].shape == (B, c["cfg"]["obs_dim"]) and c["state"].reshape(3, -1)[0].max() <= 1
            assert np.isfinite(c["value_exact"]).all() and np.isfinite(c["pre_exact"]).all()
        x = E.act_case(name, batches[-1])["m64"]["x"]
        assert np.abs(x).max() == 5.0 and (np.abs(x) < 5.0).any()
    v = E.act_case("wave_edges", 1037)
    assert (v["pre_exact"] == 0).sum() == 0 and np.abs(np.tanh(v["pre_exact"].astype(np.float64))).max() > 0.5   # the tanh is not in its linear part only


@pytest.mark.parametrize("name", list(E.RECORD))
def test_record_cases_select_what_they_say(name):
    c = E.record_case(name)
    d, B = c["obs_dim"], c["B"]
    count0 = int(c["state0"][0])
    total = 0
    for (obs, reward, done, mask), n in zip(c["ticks"], c["n"]):
        assert obs.shape == (d, B) and obs.dtype == f32 and reward.dtype == f32 and done.dtype == np.int32
        want_n = B if mask is None else int(np.count_nonzero(mask))
        assert n == want_n
        total += n
        if mask is not None:
            assert mask.dtype == np.int32 and {-1, 2 ** 31 - 1, -2 ** 31, 0, 1, 2} <= set(mask.tolist()) and 0 < n < B
            assert mask[B - 1] == -1 and mask[0] == 0          # the robot past the boundary is selected, by a value that is not 1
    want = c["want"].reshape(3, -1)
    assert want[0, 0] == count0 + total and want[0, PM.NORM_REWARD] == count0 + total
    assert float(want[0, 0]).is_integer()
    if name == "obs64":
        assert np.all(want[0] == total) and np.all(want[2] > 0) and c["ticks"][0][3] is not None and c["ticks"][1][3] is None   # all 65 columns
    if name.startswith("obs1_"):
        assert d == 1 and B in (256, 257, 65536, 65537) and not want[0, 1:PM.NORM_REWARD].any()
    if name == "count_2_40":
        assert count0 == 2 ** 40 and 0 < total < 65 and int(want[0, 0]) == 2 ** 40 + total and want[0, 0] + 1.0 != want[0, 0]


def test_the_cancellation_case_is_beyond_the_relative_tolerance():
    c = E.record_case("cancel")
    assert not c["state0"].any() and c["ticks"][0][3] is None and c["n"] == [257]
    for r in E.cancel_bounds():
        assert abs(r["mean"] - 1e4) < 1.0 and 0.5 * 257 * 1e-4 < r["exact_var"] < 2.0 * 257 * 1e-4
        assert r["mean"] == r["exact_mean"]                                   # the sums of the mean are exact: one rounding
        assert r["bound_var"] > 1e3 * 1e-12 * r["exact_var"]                  # rtol = 1e-12 cannot be derived here
        err = abs(r["model_var"] - r["exact_var"])
        print(f"column {r['col']}: var_sum {r['exact_var']:.6e}, numpy model off by {err:.3e}, bound {r['bound_var']:.3e}, mean bound {r['bound_mean']:.3e}")
        assert err <= r["bound_var"]


def test_returns_cases_cover_the_settings_and_float32_rounding_stays_inside_the_bound():
    cases = {name: E.returns_case(name) for name in E.RETURNS}
    cover = lambda key: {c[key] for c in cases.values()}
    assert cover("B") == {257, 1037} and cover("T") == {1, 300} and cover("discount") == {0.0, 0.5, 1.0} and cover("lam") == {0.0, 0.95}
    assert 0.0 in cover("reward_clip") and {0, 1} <= cover("count") and False in cover("bootstrap")
    for name, c in cases.items():
        done, T = c["done"], c["T"]
        assert np.all(done[:, E.ALWAYS_DONE] != 0) and not done[:, E.NEVER_DONE].any()     # a column that is done at every tick
        assert {2, -1} <= set(done.ravel().tolist())
        assert c["rn"].count == c["count"] and c["state"].reshape(3, -1)[0, PM.NORM_REWARD] == c["count"]
        if c["count"] <= 1:
            assert c["rn"].scale()[0] == 1.0
        ret, adv = c["ret"], c["adv"]
        # the all-done column: every tick stands alone
        rp = c["rn"].transform(c["reward"][:, E.ALWAYS_DONE].reshape(-1, 1))[:, 0]
        assert np.array_equal(ret[:, E.ALWAYS_DONE], rp - c["value"][:, E.ALWAYS_DONE].astype(np.float64) + c["value"][:, E.ALWAYS_DONE])
        if c["reward_clip"] == 0:
            assert np.abs(rp).max() > 10.0                                                  # the limit reward passes
        for want in (ret, adv):
            assert np.all(np.abs(want.astype(f32).astype(np.float64) - want) <= 1e-6 * np.maximum(np.abs(want), 1.0)), name
        if T == 300 and c["discount"] == 1.0:
            assert np.abs(adv).max() > 50.0                                                 # long undiscounted sums


# ---- argument checks of record and returns -----------------------------------------------------------------------------

CFG = dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2))


def _record_args(B=4, d=6):
    return dict(obs_cm=torch.zeros(d, B), reward=torch.zeros(B), done=torch.zeros(B, dtype=torch.int32), mask=torch.ones(B, dtype=torch.int32),
                ro_obs=torch.zeros(d, B), ro_reward=torch.zeros(B), ro_done=torch.zeros(B, dtype=torch.int32))


def _no_device(call):
    with pytest.raises(policy_abi.RgPolicyError) as e:
        call()
    assert e.value.status == -3


def test_record_validates_every_tensor_before_the_library_sees_a_pointer():
    B = 4
    pol = BatchedGaussianPolicy(B, device="cpu", **CFG)
    _no_device(lambda: pol.record(**_record_args()))                             # valid: the library is reached
    a = _record_args()
    _no_device(lambda: pol.record(a["obs_cm"], a["reward"], a["done"]))          # every optional argument left out
    bad = {
        "done": [torch.zeros(B, dtype=torch.bool), torch.zeros(B, dtype=torch.int64), torch.zeros(B + 1, dtype=torch.int32), None],
        "reward": [torch.zeros(B, dtype=torch.float64), torch.zeros(B, 1), torch.zeros(2 * B)[::2], None],
        "obs_cm": [torch.zeros(B, 6).t(), torch.zeros(6, B + 1), torch.zeros(6, B, dtype=torch.float64), torch.zeros(6 * B), None],
        "mask": [torch.ones(B, dtype=torch.bool), torch.ones(B, dtype=torch.int64), torch.ones(B - 1, dtype=torch.int32)],
        "ro_obs": [torch.zeros(B, 6).t(), torch.zeros(5, B), torch.zeros(6, B, dtype=torch.float16)],
        "ro_reward": [torch.zeros(B, dtype=torch.float64), torch.zeros(B + 1)],
        "ro_done": [torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.bool), torch.zeros(B)],
    }
    for name, values in bad.items():
        for v in values:
            with pytest.raises(ValueError, match=rf"record: {name} "):
                pol.record(**dict(_record_args(), **{name: v}))
    with pytest.raises(ValueError, match="record: reward "):
        pol.record(**dict(_record_args(), reward=np.zeros(B, dtype=np.float32)))   # not a tensor
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="record: done "):
            pol.record(**dict(_record_args(), done=torch.zeros(B, dtype=torch.int32, device="cuda")))
    pol.close()


def test_returns_validates_the_rollout_before_the_library_sees_a_pointer():
    B, T = 4, 3
    pol = BatchedGaussianPolicy(B, device="cpu", **CFG)
    ro = lambda T=T, B=B: RolloutBuffer(T, B, 6, 3)
    _no_device(lambda: pol.returns(ro()))
    _no_device(lambda: pol.returns(ro(), bootstrap=False))
    r = ro()
    r.last_value = None
    _no_device(lambda: pol.returns(r, bootstrap=False))                          # no bootstrap: no last_value needed
    with pytest.raises(ValueError, match="returns: rollout.last_value "):
        pol.returns(r, bootstrap=True)
    with pytest.raises(ValueError, match="returns: rollout.batch "):
        pol.returns(ro(B=B + 1))                                                 # a buffer of another batch
    r = ro()
    r.T = T + 1                                                                  # a buffer whose tensors do not match its T
    with pytest.raises(ValueError, match="returns: rollout.reward "):
        pol.returns(r)
    r = ro()
    r.T = 0
    with pytest.raises(ValueError, match="returns: rollout.T "):
        pol.returns(r)
    bad = {
        "done": [torch.zeros(T, B, dtype=torch.bool), torch.zeros(T, B, dtype=torch.int64), torch.zeros(B, T, dtype=torch.int32).t()],
        "reward": [torch.zeros(T, B, dtype=torch.float64), torch.zeros(B, T).t(), torch.zeros(T, B + 1)],
        "value": [torch.zeros(T, B, dtype=torch.float64), torch.zeros(T + 1, B)],
        "ret": [torch.zeros(T - 1, B), torch.zeros(T, B, dtype=torch.float64)],
        "adv": [torch.zeros(T, 2 * B)[:, ::2], torch.zeros(T * B)],
        "last_value": [torch.zeros(B, dtype=torch.float64), torch.zeros(B + 1), torch.zeros(B, 1)],
    }
    for name, values in bad.items():
        for v in values:
            r = ro()
            setattr(r, name, v)
            with pytest.raises(ValueError, match=rf"returns: rollout.{name} "):
                pol.returns(r)
    r = RolloutBuffer(T, B, 6, 3, dtype=torch.float64)                            # the update's float64 buffers are not the kernels'
    with pytest.raises(ValueError, match="returns: rollout.reward "):
        pol.returns(r)
    pol.close()
