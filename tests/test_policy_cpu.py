"""The PPO agent's acting and collecting side (include/rg_policy.h) without a GPU: librg_mpc.so exports every rg_policy_*
entry, the ctypes binding matches the header, create validates its configuration (naming the field) before it looks for a
device, a host-only handle checks arguments and then returns NO_DEVICE, the layout rule; known answers of the numpy model
(tests/policy_model.py); the properties of the noise stream; the torch update on the CPU in float64 against numbers formed
in numpy from the formulas; and the kernels of rg_policy.hip cross-compile for gfx950 without scratch or spills, within
their LDS budget."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import PPO, BatchedGaussianPolicy, RolloutBuffer
from robot_gym_amd.core import policy_abi
from tests import kernel_checks
from tests import policy_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_policy.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI and configuration ------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = policy_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_policy_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 12
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(policy_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None or name.endswith(("_version", "_size", "_rows", "_tile")), name


def _struct_fields(name):
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", _header()))[name]
    sizes = {"int32_t": 4, "double": 8, "uint64_t": 8}
    want = []
    for line in re.findall(r"\b(int32_t|double|uint64_t)\s+([^;]+);", body):
        for n, dims in re.findall(r"([a-z_0-9]+)((?:\[\d+\])*)", line[1]):
            if not n or n.isdigit():
                continue
            count = 1
            for dim in re.findall(r"\[(\d+)\]", dims):
                count *= int(dim)
            want.append((n, sizes[line[0]] * count))
    return want


@pytest.mark.parametrize("name,struct", [("rg_policy_config", policy_abi.CConfig), ("rg_policy_layout", policy_abi.CLayout)])
def test_struct_layout_matches_header(name, struct):
    want = _struct_fields(name)
    got = struct._fields_
    assert [n for n, _ in want] == [n for n, _ in got]
    for (n, size), (_, tg) in zip(want, got):
        assert size == C.sizeof(tg), n
    assert sum(s for _, s in want) == C.sizeof(struct)   # no padding anywhere


def test_sizes_limits_and_defaults_match_header_and_binding():
    lib = policy_abi.load_library()
    assert lib.rg_policy_abi_version() == policy_abi.ABI_VERSION == 1
    assert lib.rg_policy_config_size() == C.sizeof(policy_abi.CConfig) == 88
    assert lib.rg_policy_layout_size() == C.sizeof(policy_abi.CLayout)
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_POLICY_\w+) (\d+)", _header())}
    assert lib.rg_policy_norm_rows() == defs["RG_POLICY_NORM_ROWS"] == policy_abi.NORM_ROWS == PM.NORM_ROWS == 3 * defs["RG_POLICY_NORM_COLS"]
    assert defs["RG_POLICY_NORM_COLS"] == policy_abi.NORM_COLS == PM.NORM_COLS and defs["RG_POLICY_NORM_REWARD"] == policy_abi.NORM_REWARD == PM.NORM_REWARD
    assert lib.rg_policy_tile() == defs["RG_POLICY_TILE"] == policy_abi.TILE
    assert (defs["RG_POLICY_MAX_OBS"], defs["RG_POLICY_MAX_ACT"], defs["RG_POLICY_MAX_LAYERS"], defs["RG_POLICY_MAX_WIDTH"]) == \
        (policy_abi.MAX_OBS, policy_abi.MAX_ACT, policy_abi.MAX_LAYERS, policy_abi.MAX_WIDTH) == (64, 4, 3, 256)
    assert (defs["RG_POLICY_MODE_SAMPLE"], defs["RG_POLICY_MODE_MEAN"]) == (policy_abi.MODE_SAMPLE, policy_abi.MODE_MEAN)
    D = policy_abi.DEFAULTS   # the reference's configs.py default() and networks.py
    assert (D["obs_dim"], D["act_dim"], D["policy_layers"], D["value_layers"]) == (16, 2, (200, 100), (200, 100))
    assert (D["obs_clip"], D["reward_clip"], D["discount"], D["gae_lambda"]) == (5.0, 10.0, 0.985, 1.0)
    cc = policy_abi.make_cconfig(policy_layers=(7,), seed=2 ** 63 + 5)
    assert (cc.n_policy_layers, list(cc.policy_layers), cc.n_value_layers, list(cc.value_layers), cc.seed) == (1, [7, 0, 0], 2, [200, 100, 0], 2 ** 63 + 5)
    with pytest.raises(TypeError):
        policy_abi.make_cconfig(gamma=0.9)
    with pytest.raises(ValueError):
        policy_abi.make_cconfig(value_layers=(1, 2, 3, 4))


def _set(cc, field, value):
    m = re.fullmatch(r"(\w+)\[(\d)\]", field)
    if m:
        getattr(cc, m.group(1))[int(m.group(2))] = value
    else:
        setattr(cc, field, value)


@pytest.mark.parametrize("field,value,text", [
    ("obs_dim", 0, "config.obs_dim"), ("obs_dim", 65, "config.obs_dim"), ("act_dim", 0, "config.act_dim"), ("act_dim", 5, "config.act_dim"),
    ("n_policy_layers", -1, "config.n_policy_layers"), ("n_policy_layers", 4, "config.n_policy_layers"), ("n_value_layers", 4, "config.n_value_layers"),
    ("policy_layers[0]", 0, "config.policy_layers[0]"), ("policy_layers[1]", 257, "config.policy_layers[1]"),
    ("policy_layers[2]", 5, "config.policy_layers[2]"), ("value_layers[1]", 0, "config.value_layers[1]"), ("value_layers[2]", 1, "config.value_layers[2]"),
    ("obs_clip", -1.0, "config.obs_clip"), ("obs_clip", NAN, "config.obs_clip"), ("reward_clip", INF, "config.reward_clip"),
    ("discount", 1.5, "config.discount"), ("discount", -0.1, "config.discount"), ("gae_lambda", 1.01, "config.gae_lambda"),
    ("gae_lambda", NAN, "config.gae_lambda"), ("abi_version", 2, "config.abi_version"), ("reserved0", 1, "config.reserved0"),
])
def test_create_rejects_a_bad_config_naming_the_field(field, value, text):
    cc = policy_abi.make_cconfig()
    _set(cc, field, value)
    for device in (0, policy_abi.DEVICE_NONE):
        rc, msg = policy_abi.create_status(cc, device=device)
        assert rc == -1 and text in msg, (rc, msg)
    lay = policy_abi.CLayout()
    assert policy_abi.load_library().rg_policy_param_layout(C.byref(cc), C.byref(lay)) == -1


def test_create_checks_batch_and_null_arguments():
    for batch in (0, -3, (1 << 24) + 1):
        rc, msg = policy_abi.create_status(batch=batch)
        assert rc == -1 and "batch" in msg
    lib = policy_abi.load_library()
    assert lib.rg_policy_create(None, 4, -1, C.byref(C.c_void_p())) == -1
    assert lib.rg_policy_param_layout(None, None) == -1
    for settings in (dict(), dict(obs_clip=0.0, reward_clip=0.0, discount=0.0, gae_lambda=0.0), dict(policy_layers=(), value_layers=())):
        rc, msg = policy_abi.create_status(policy_abi.make_cconfig(**settings))   # valid, host-only: a handle is made
        assert rc == 0, msg


def test_host_only_handle_checks_arguments_then_reports_no_device():
    h = policy_abi.PolicyHandle(4, policy_abi.DEVICE_NONE, seed=3)
    lib = policy_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p = dummy.ctypes.data
    last = lambda: lib.rg_policy_last_error(h._h).decode()
    good = [p, p, p, p, p, 0, p, p, p, p]
    assert lib.rg_policy_act(h._h, *good, None) == -3 and "host-only" in last()
    optional = list(good)
    optional[7] = optional[8] = optional[9] = None
    assert lib.rg_policy_act(h._h, *optional, None) == -3
    for k, name in enumerate(("obs", "norm_state", "policy_params", "value_params", "act_state", None, "action")):
        if name is None:
            continue
        a = list(good)
        a[k] = None
        assert lib.rg_policy_act(h._h, *a, None) == -1 and f"act: null {name}" in last(), last()
    a = list(good)
    a[4], a[5] = None, 1
    assert lib.rg_policy_act(h._h, *a, None) == -3     # MEAN mode needs no act state
    a[5] = 2
    assert lib.rg_policy_act(h._h, *a, None) == -1 and "mode" in last()
    good = [p, p, p, p, p, p, p, p]
    assert lib.rg_policy_record(h._h, *good, None) == -3
    assert lib.rg_policy_record(h._h, p, p, p, None, p, None, None, None, None) == -3
    for k, name in ((0, "obs"), (1, "reward"), (2, "done"), (4, "norm_state")):
        a = list(good)
        a[k] = None
        assert lib.rg_policy_record(h._h, *a, None) == -1 and f"record: null {name}" in last(), last()
    good = [p, p, p, p, p, 5, 1, p, p]
    assert lib.rg_policy_returns(h._h, *good, None) == -3
    for k, name in ((0, "reward"), (1, "value"), (2, "done"), (3, "last_value"), (4, "norm_state"), (7, "ret"), (8, "adv")):
        a = list(good)
        a[k] = None
        assert lib.rg_policy_returns(h._h, *a, None) == -1 and f"returns: null {name}" in last(), last()
    a = list(good)
    a[3], a[6] = None, 0
    assert lib.rg_policy_returns(h._h, *a, None) == -3   # no bootstrap: no last_value
    for T in (0, -1, (1 << 20) + 1):
        a = list(good)
        a[5] = T
        assert lib.rg_policy_returns(h._h, *a, None) == -1 and "returns: T" in last()
    assert lib.rg_policy_act(None, *([p] * 5), 0, *([p] * 4), None) == -1 and "null handle" in lib.rg_policy_last_error(None).decode()
    with pytest.raises(policy_abi.RgPolicyError) as e:
        h.record(p, p, p, None, p)
    assert e.value.status == -3
    h.close()


@pytest.mark.parametrize("settings", [
    dict(), dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2)), dict(obs_dim=64, act_dim=4, policy_layers=(), value_layers=()),
    dict(obs_dim=64, act_dim=4, policy_layers=(256, 256, 256), value_layers=(256, 256, 256)),
])
def test_param_layout_is_the_rule(settings):
    f = policy_abi.policy_fields(**settings)
    got = policy_abi.param_layout(**settings)
    want = PM.layout(f["obs_dim"], f["act_dim"], f["policy_layers"], f["value_layers"])
    assert got == want
    # buffers are dense: W then b of each layer, nothing between, logstd last
    for name in ("policy", "value"):
        end = 0
        for i, o, w, b in got[name]:
            assert (w, b) == (end, end + i * o)
            end = b + o
        assert end == (got["logstd_offset"] if name == "policy" else got["value_count"])
    assert got["policy_count"] == got["logstd_offset"] + f["act_dim"]


# ---- model known answers ----------------------------------------------------------------------------------------------

def test_normalizer_matches_numpy_mean_and_variance_over_several_batches():
    rng = np.random.default_rng(0)
    data = rng.normal(3.0, 2.0, size=(1 + 5 + 1 + 40 + 7, 3)) * np.array([1.0, 10.0, 0.01])
    n = PM.Normalizer(3)
    k = 0
    for size in (1, 5, 1, 0, 40, 7):   # a first batch of one sample; an empty one
        n.update(data[k:k + size])
        k += size
        if k == 1:
            assert n.count == 1 and np.array_equal(n.mean, data[0]) and np.array_equal(n.var_sum, np.zeros(3))
    assert n.count == len(data)
    assert np.allclose(n.mean, np.mean(data, axis=0), rtol=1e-13, atol=0)
    assert np.allclose(n.var_sum / (n.count - 1), np.var(data, axis=0, ddof=1), rtol=1e-12, atol=0)
    s = PM.norm_state_of(n, PM.Normalizer(1, False))
    o, r = PM.normalizers_of(s, 3)
    assert o.count == n.count and np.array_equal(o.mean, n.mean) and np.array_equal(o.var_sum, n.var_sum) and r.count == 0


def test_transform_with_count_at_most_one_only_centres_and_clips():
    n = PM.Normalizer(2, clip=5.0)
    v = np.array([[0.5, -7.0], [6.0, 2.0]])
    assert np.array_equal(n.transform(v), np.clip(v, -5, 5))             # empty: mean 0, divisor 1
    n.update([[1.0, -1.0]])
    assert n.count == 1
    assert np.array_equal(n.transform(v), np.clip(v - [1.0, -1.0], -5, 5))
    n.update([[3.0, -1.0]])                                                # count 2: var = (2, 0)
    want = (v - [2.0, -1.0]) / (np.sqrt(np.array([2.0, 0.0]) + 1e-4) + 1e-8)
    assert np.allclose(n.transform(v), np.clip(want, -5, 5), rtol=1e-15)
    r = PM.Normalizer(1, center=False, clip=10.0)                          # the reward: scale only
    r.update([[4.0]])
    r.update([[8.0]])
    assert np.allclose(r.transform([[6.0], [100.0]]), [[6.0 / (math.sqrt(8.0 + 1e-4) + 1e-8)], [10.0]], rtol=1e-15)
    assert np.array_equal(PM.Normalizer(1, clip=0.0).transform([[1e9]]), [[1e9]])   # clip 0: off


def test_returns_hand_worked_sequences():
    none = PM.Normalizer(1, False, 10.0)
    col = lambda *v: np.array(v, dtype=np.float64).reshape(-1, 1)
    # discount 0.5, lambda 1, values 0, done at the last step, no bootstrap: the discounted return
    ret, adv = PM.returns(col(1, 2, 4), col(0, 0, 0), col(0, 0, 1), [9.0], none, 0.5, 1.0, False)
    assert np.array_equal(ret[:, 0], [3.0, 4.0, 4.0]) and np.array_equal(adv, ret)
    ret_b, _ = PM.returns(col(1, 2, 4), col(0, 0, 0), col(0, 0, 1), [9.0], none, 0.5, 1.0, True)
    assert np.array_equal(ret_b, ret)                                      # a done at the last step cuts the bootstrap off
    # two dones in a row
    ret, _ = PM.returns(col(1, 2, 4), col(0, 0, 0), col(0, 1, 1), [9.0], none, 0.5, 1.0, True)
    assert np.array_equal(ret[:, 0], [2.0, 2.0, 4.0])
    # values, lambda 0.5, bootstrap 8:  d2 = 4 + 4 - 3 = 5; d1 = 2 + 1.5 - 2 = 1.5, A1 = 1.5 + 0.25 * 5; d0 = 1 + 1 - 1 = 1, A0 = 1 + 0.25 * 2.75
    ret, adv = PM.returns(col(1, 2, 4), col(1, 2, 3), col(0, 0, 0), [8.0], none, 0.5, 0.5, True)
    assert np.array_equal(adv[:, 0], [1.6875, 2.75, 5.0]) and np.array_equal(ret[:, 0], [2.6875, 4.75, 8.0])
    # lambda 0: one-step TD
    ret, adv = PM.returns(col(1, 2, 4), col(1, 2, 3), col(0, 1, 0), [8.0], none, 0.5, 0.0, True)
    assert np.array_equal(adv[:, 0], [1 + 1 - 1, 2 - 2, 4 + 4 - 3])
    # the reward goes through its normaliser: scaled by std + 1e-8, clipped
    r = PM.Normalizer(1, False, 1.5)
    r.update([[0.0], [2.0]])
    ret, _ = PM.returns(col(1, 100), col(0, 0), col(0, 1), [0.0], r, 0.0, 1.0, False)
    assert np.allclose(ret[:, 0], [1.0 / (math.sqrt(2.0 + 1e-4) + 1e-8), 1.5], rtol=1e-15)


def test_lambda_one_without_bootstrap_is_the_directly_summed_discounted_return():
    rng = np.random.default_rng(3)
    T = 9
    reward, value = rng.normal(size=(T, 1)), rng.normal(size=(T, 1))
    done = np.zeros((T, 1))
    done[-1] = 1
    ret, adv = PM.returns(reward, value, done, [5.0], PM.Normalizer(1, False, 10.0), 0.985, 1.0, False)
    assert np.allclose(ret[:, 0], PM.discounted_return(reward[:, 0], 0.985), rtol=1e-13, atol=1e-14)
    assert np.allclose(adv, ret - value, rtol=1e-13, atol=1e-14)


# ---- the noise stream -------------------------------------------------------------------------------------------------

def test_a_robots_draws_depend_on_seed_key_counter_and_axis_only():
    a = np.array([[[PM.eps64(5, k, c, ax) for ax in range(2)] for c in range(4)] for k in range(32)])
    b = np.array([[[PM.eps64(5, k, c, ax) for ax in range(2)] for c in (3, 0)] for k in (31, 7, 0)])   # another batch, another order
    assert np.array_equal(b, a[[31, 7, 0]][:, [3, 0]])
    assert len(np.unique(a)) == a.size                                        # key, counter and axis all matter
    assert PM.eps64(6, 0, 0, 0) != PM.eps64(5, 0, 0, 0)                       # and the seed
    assert PM.eps(5, 3, 2, 1) == np.float32(PM.eps64(5, 3, 2, 1))
    assert PM.noise_hash(0, 1, 2, 3, 0) != PM.noise_hash(0, 1, 2, 3, 1)
    assert PM.eps_batch(5, [7, 31], [0, 3], 2).tolist() == np.float32(a[[7, 31], [0, 3]]).tolist()


def test_noise_moments_are_within_four_sigma_and_u1_is_never_zero():
    N = 1 << 17
    e = np.array([PM.eps64(0, k, c, 0) for k in range(N // 8) for c in range(8)])
    assert abs(e.mean()) <= 4.0 / math.sqrt(N)                 # sd of the mean of N unit normals: 1 / sqrt(N)
    assert abs(e.var() - 1.0) <= 4.0 * math.sqrt(2.0 / N)      # sd of their variance: sqrt(2 / N)
    assert np.all(np.isfinite(e))
    u = np.array([PM.uniforms(1, k, 0, 1) for k in range(4096)])
    assert u[:, 0].min() > 0.0 and u[:, 0].max() <= 1.0 and u[:, 1].min() >= 0.0 and u[:, 1].max() < 1.0
    # the smallest u1 the formula can give is 2^-53, not 0: eps stays finite
    assert (0 + 1) * 2.0 ** -53 > 0.0 and math.isfinite(math.sqrt(-2.0 * math.log(2.0 ** -53)))


# ---- the update, torch on the CPU in float64 ----------------------------------------------------------------------------

CFG = dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2))


def _tiny(seed=0, T=3, B=4, mask_some=True):
    """A host-only float64 policy with random biases, logstd and normaliser state, and a synthetic rollout."""
    rng = np.random.default_rng(seed)
    pol = BatchedGaussianPolicy(B, device="cpu", dtype=torch.float64, seed=seed, **CFG)
    with torch.no_grad():
        for _, b in pol.policy_layers + pol.value_layers:
            b.copy_(torch.as_tensor(rng.normal(0, 0.3, size=b.shape)))
        pol.logstd.copy_(torch.as_tensor(rng.normal(-1, 0.2, size=3)))
    on, rn = PM.Normalizer(6, True, 5.0), PM.Normalizer(1, False, 10.0)
    on.update(rng.normal(0.2, 1.5, size=(30, 6)))
    rn.update(rng.normal(0.0, 3.0, size=(30, 1)))
    pol.norm_state.copy_(torch.as_tensor(PM.norm_state_of(on, rn)))
    ro = RolloutBuffer(T, B, 6, 3, dtype=torch.float64)
    ro.obs.copy_(torch.as_tensor(rng.normal(0.2, 3.0, size=(T, 6, B))))     # some components reach the clip
    ro.mean.copy_(torch.as_tensor(np.tanh(rng.normal(0, 0.5, size=(T, B, 3)))))
    ro.logstd.copy_(torch.as_tensor(rng.normal(-1, 0.2, size=3)))
    ro.action.copy_(ro.mean + torch.exp(ro.logstd) * torch.as_tensor(rng.normal(size=(T, B, 3))))
    ro.adv.copy_(torch.as_tensor(rng.normal(0.5, 2.0, size=(T, B))))
    ro.ret.copy_(torch.as_tensor(rng.normal(0.0, 2.0, size=(T, B))))
    if mask_some:
        ro.mask[2, 1] = 0
        ro.mask[1:, 3] = 0
    return pol, ro, on


def _model_forward(pol, ro, on):
    x = on.transform(ro.obs.numpy().transpose(0, 2, 1))
    lay = pol.layout
    pp, vp = pol.policy_params.detach().numpy(), pol.value_params.detach().numpy()
    T, B = ro.T, ro.batch
    mean = PM.forward(x.reshape(T * B, -1), PM.split(pp, lay["policy"]), "tanh").reshape(T, B, -1)
    value = PM.forward(x.reshape(T * B, -1), PM.split(vp, lay["value"]), "linear").reshape(T, B)
    return x, mean, value, pp[lay["logstd_offset"]:]


def test_evaluate_and_normalize_equal_the_model():
    pol, ro, on = _tiny()
    x, mean, value, logstd = _model_forward(pol, ro, on)
    assert np.abs(x).max() == 5.0                                            # the clip is exercised
    xt = pol.normalize_obs(ro.obs.permute(0, 2, 1))
    assert np.allclose(xt.numpy(), x, rtol=1e-14, atol=1e-15)
    m, v = pol.evaluate(xt)
    assert m.shape == (3, 4, 3) and v.shape == (3, 4)
    assert np.allclose(m.detach().numpy(), mean, rtol=1e-13, atol=1e-15) and np.allclose(v.detach().numpy(), value, rtol=1e-13, atol=1e-15)
    assert np.array_equal(pol.logstd.detach().numpy(), logstd)
    _, rn = PM.normalizers_of(pol.norm_state.numpy(), 6)
    r = np.array([0.3, -50.0, 2.0])
    assert np.allclose(pol.normalize_reward(torch.as_tensor(r)).numpy(), rn.transform(r.reshape(-1, 1))[:, 0], rtol=1e-15)
    empty = BatchedGaussianPolicy(2, device="cpu", dtype=torch.float64, **CFG)   # count 0: centre (mean 0) and clip only
    o = torch.tensor([[0.5, -7.0, 1.0, 2.0, 3.0, 9.0]], dtype=torch.float64)
    assert torch.equal(empty.normalize_obs(o), o.clamp(-5, 5))


@pytest.mark.parametrize("conv", ["exact", "reference"])
def test_losses_equal_the_formulas_in_numpy(conv):
    pol, ro, on = _tiny(seed=1)
    ppo = PPO(pol, kl_init_penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2, kl_cutoff_coef=1000, conv_logpdf=conv)
    b = ppo.batch(ro)
    x, mean, value, logstd = _model_forward(pol, ro, on)
    valid = (ro.mask.numpy() != 0).astype(np.float64)
    adv = ro.adv.numpy()
    sel = adv[valid != 0]
    adv_n = (adv - sel.mean()) / (sel.std() + 1e-8)
    assert np.allclose(b["adv"].numpy(), adv_n, rtol=1e-13, atol=1e-15)
    old_mean, old_logstd, action = ro.mean.numpy(), ro.logstd.numpy(), ro.action.numpy()
    kl = (PM.diag_normal_kl(old_mean, old_logstd, mean, logstd) * valid).mean(axis=0)           # per robot, over time
    ratio = np.exp(PM.diag_normal_logpdf(mean, logstd, action, conv) - PM.diag_normal_logpdf(old_mean, old_logstd, action, conv))
    surrogate = -(ratio * adv_n * valid).mean(axis=0)
    threshold = 2 * 1e-2
    assert (kl > threshold).any()                                              # the cutoff term is exercised
    want = np.mean(surrogate + 0.7 * kl + 1000 * (kl > threshold) * (kl - threshold) ** 2)
    assert math.isclose(float(ppo.policy_loss(b).detach()), want, rel_tol=1e-12)
    assert np.allclose(ppo.kl(b).detach().numpy(), kl, rtol=1e-12)
    want_v = np.mean(0.5 * (ro.ret.numpy() - value) ** 2 * valid)
    assert math.isclose(float(ppo.value_loss(b).detach()), want_v, rel_tol=1e-12)


def test_the_two_logpdf_conventions_differ_by_half_the_sum_of_logstd():
    from robot_gym_amd.agents.ppo import diag_normal_logpdf
    m, ls, a = torch.zeros(2, dtype=torch.float64), torch.tensor([-1.0, 0.5], dtype=torch.float64), torch.tensor([0.3, -0.2], dtype=torch.float64)
    exact, ref = diag_normal_logpdf(m, ls, a, "exact"), diag_normal_logpdf(m, ls, a, "reference")
    want = sum(-0.5 * math.log(2 * math.pi * math.exp(2 * s)) - 0.5 * (x / math.exp(s)) ** 2 for s, x in ((-1.0, 0.3), (0.5, -0.2)))
    assert math.isclose(float(exact), want, rel_tol=1e-14)                     # the density itself
    assert math.isclose(float(ref - exact), 0.5 * (-1.0 + 0.5), rel_tol=1e-13)
    with pytest.raises(ValueError):
        PPO(BatchedGaussianPolicy(1, device="cpu", **CFG), conv_logpdf="tf")


@pytest.mark.parametrize("kl,factor", [(0.02, 1.5), (0.0135, 1.5), (0.01, 1.0), (0.0125, 1.0), (0.0075, 1.0), (0.0065, 1 / 1.5), (0.001, 1 / 1.5)])
def test_penalty_moves_with_the_kl_change(kl, factor):
    pol, ro, on = _tiny(seed=2, mask_some=False)
    ppo = PPO(pol, epochs_policy=0, epochs_value=0, kl_target=1e-2, kl_init_penalty=2.0)
    with torch.no_grad():   # a behaviour policy at the same logstd, every mean off by d in one component: KL = 0.5 d^2 / std^2
        ro.logstd.copy_(pol.logstd)
        mean, _ = pol.evaluate(pol.normalize_obs(ro.obs.permute(0, 2, 1)))
        ro.mean.copy_(mean)
        ro.mean[..., 0] += math.sqrt(2.0 * kl) * torch.exp(pol.logstd[0])
    out = ppo.update(ro)
    assert math.isclose(out["kl_change"], kl, rel_tol=1e-9)
    assert math.isclose(ppo.penalty, 2.0 * factor, rel_tol=1e-15) and out["penalty"] == ppo.penalty


def test_update_steps_in_place_on_the_parameter_tensors():
    pol, ro, on = _tiny(seed=3)
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    before = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
    ppo = PPO(pol, epochs_policy=4, epochs_value=4)
    out = ppo.update(ro)
    assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
    assert not torch.equal(pol.policy_params.detach(), before[0]) and not torch.equal(pol.value_params.detach(), before[1])
    assert not torch.equal(pol.logstd.detach(), before[0][-3:])                  # logstd is trained with the policy
    assert out["value_loss_last"] < out["value_loss_first"] and out["policy_loss_last"] < out["policy_loss_first"]
    # save / restore copies into the same tensors
    state = pol.state_dict()
    with torch.no_grad():
        pol.policy_params.zero_()
        pol.act_state[1] += 5
    pol.load_state_dict(state)
    assert torch.equal(pol.policy_params.detach(), state["policy_params"]) and pol.policy_params.data_ptr() == ptrs[0]
    assert torch.equal(pol.act_state, state["act_state"]) and pol.act_state[0].tolist() == [0, 1, 2, 3]
    pol.clone([0], [2])
    assert pol.act_state[:, 2].tolist() == pol.act_state[:, 0].tolist()
    with pytest.raises(policy_abi.RgPolicyError) as e:                           # no CPU fallback
        pol.act(torch.zeros(6, 4))
    assert e.value.status == -3


def test_initialisation_follows_the_reference():
    pol = BatchedGaussianPolicy(1, device="cpu", seed=4)
    layers = [(W.detach(), b.detach()) for W, b in pol.policy_layers]
    for (W, b), (i, o) in zip(layers[:-1] + [(W.detach(), b.detach()) for W, b in pol.value_layers], ((16, 200), (200, 100), (16, 200), (200, 100), (100, 1))):
        limit = math.sqrt(6.0 / (i + o))
        assert tuple(W.shape) == (i, o) and float(W.abs().max()) <= limit and float(W.abs().max()) > 0.8 * limit and float(b.abs().max()) == 0.0
    W, b = layers[-1]
    std = math.sqrt(1.3 * 0.1 / 100)
    assert float(W.abs().max()) <= 2 * std + 1e-7 and 0.5 * std < float(W.std()) < std and float(b.abs().max()) == 0.0
    assert pol.logstd.tolist() == [-1.0, -1.0]
    again = BatchedGaussianPolicy(1, device="cpu", seed=4)
    assert torch.equal(again.policy_params, pol.policy_params) and torch.equal(again.value_params, pol.value_params)
    assert not torch.equal(BatchedGaussianPolicy(1, device="cpu", seed=5).policy_params, pol.policy_params)


# ---- resources of rg_policy.hip ---------------------------------------------------------------------------------------

KERNELS = {"rg_policy_act_kernel", "rg_policy_record_first_kernel", "rg_policy_record_second_kernel", "rg_policy_record_finish_kernel",
           "rg_policy_returns_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_policy.hip")


def test_every_policy_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_policy_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


# act kernel: 2 networks * 2 buffers * 256 inputs * 8 robots float32, and 8 * 4 float32 of noise.
# record kernels: one float64 per wave of the workgroup's sum.
LDS_BUDGET = {"rg_policy_act_kernel": 2 * 2 * 256 * 8 * 4 + 8 * 4 * 4, "rg_policy_record_first_kernel": 4 * 8, "rg_policy_record_second_kernel": 4 * 8,
              "rg_policy_record_finish_kernel": 4 * 8, "rg_policy_returns_kernel": 0}


def test_lds_is_within_the_budget(remarks):
    for name, budget in LDS_BUDGET.items():
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= budget, (name, remarks[name])


# What the device-only compile reports today (upper bounds; occupancy a lower bound).  The act kernel's workgroup is eight
# waves, two per SIMD: at four waves per SIMD two workgroups share a compute unit.
REGISTERS = {"rg_policy_act_kernel": dict(vgprs=100, agprs=0, occupancy=4), "rg_policy_record_first_kernel": dict(vgprs=26, agprs=0, occupancy=8),
             "rg_policy_record_second_kernel": dict(vgprs=29, agprs=0, occupancy=8), "rg_policy_record_finish_kernel": dict(vgprs=38, agprs=0, occupancy=8),
             "rg_policy_returns_kernel": dict(vgprs=26, agprs=0, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    own = open(os.path.join(SRC, "rg_policy.hip")).read()
    shared = [open(os.path.join(SRC, name)).read() for name in ("rg_host.h", "rg_agent_dev.inc", "rg_stream_dev.inc")]   # the agents' common code
    src = "\n".join([own] + shared)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    own_code = re.sub(r"//.*", "", own)
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index("__global__")
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index('#include "rg_agent_dev.inc"')
    assert re.findall(r'#include "([^"]+)"', own_code) == ["../../include/rg_policy.h", "rg_host.h", "rg_agent_dev.inc"]
    assert all("__global__" not in text for text in shared)
    assert [re.findall(r'#include "([^"]+)"', text) for text in shared] == [[], ["rg_stream_dev.inc"], []]     # the one stream, under the agents' noise
    import bench
    assert not any("rg_agent_" in rel or "rg_stream_" in rel or "rg_host" in rel for rel in bench.compiled_sources())     # the MPC hash behind profiles/ does not follow them
    assert "rg_policy" not in open(os.path.join(SRC, "rg_mpc.hip")).read()   # the source hash behind profiles/ does not move
    kernel_checks.assert_built_into_both("rg_policy.hip", header="rg_policy.h")
