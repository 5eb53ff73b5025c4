"""The recurrent Gaussian policy (include/rg_rnn.h) without a GPU: librg_mpc.so exports every rg_rnn_* entry, the ctypes
binding matches the header, create validates its configuration (naming the field) before it looks for a device, a host-only
handle checks arguments and then returns NO_DEVICE, the layout rule; known answers of the numpy model (tests/rnn_model.py);
the torch sequence evaluation and the update on the CPU in float64 against the model and against numbers formed in numpy
from the formulas; and the kernels of rg_rnn.hip cross-compile for gfx950 without scratch or spills, within their LDS
budget."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import RecurrentGaussianPolicy, RecurrentPPO, RecurrentRolloutBuffer
from robot_gym_amd.core import policy_abi, rnn_abi
from tests import kernel_checks
from tests import policy_model as PM
from tests import rnn_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_rnn.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")

CONFIGS = {
    "default": dict(),
    "lopsided": dict(obs_dim=6, act_dim=3, policy_layers=(), gru_units=5, value_layers=(7, 3, 2)),
    "limits": dict(obs_dim=64, act_dim=4, policy_layers=(256, 256), gru_units=128, value_layers=(256, 256, 256)),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI and configuration ------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = rnn_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_rnn_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 10
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(rnn_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None or name.endswith(("_version", "_size", "_tile")), name


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


@pytest.mark.parametrize("name,struct", [("rg_rnn_config", rnn_abi.CConfig), ("rg_rnn_layout", rnn_abi.CLayout)])
def test_struct_layout_matches_header(name, struct):
    want = _struct_fields(name)
    got = struct._fields_
    assert [n for n, _ in want] == [n for n, _ in got]
    for (n, size), (_, tg) in zip(want, got):
        assert size == C.sizeof(tg), n
    assert sum(s for _, s in want) == C.sizeof(struct)   # no padding anywhere


def test_sizes_limits_and_defaults_match_header_and_binding():
    lib = rnn_abi.load_library()
    assert lib.rg_rnn_abi_version() == rnn_abi.ABI_VERSION == 1
    assert lib.rg_rnn_config_size() == C.sizeof(rnn_abi.CConfig) == 64
    assert lib.rg_rnn_layout_size() == C.sizeof(rnn_abi.CLayout)
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_RNN_\w+) (\d+)", _header())}
    assert lib.rg_rnn_tile() == defs["RG_RNN_TILE"] == rnn_abi.TILE
    assert (defs["RG_RNN_MAX_OBS"], defs["RG_RNN_MAX_ACT"], defs["RG_RNN_MAX_DENSE"], defs["RG_RNN_MAX_VALUE_LAYERS"], defs["RG_RNN_MAX_WIDTH"],
            defs["RG_RNN_MAX_UNITS"]) == (rnn_abi.MAX_OBS, rnn_abi.MAX_ACT, rnn_abi.MAX_DENSE, rnn_abi.MAX_VALUE_LAYERS, rnn_abi.MAX_WIDTH,
                                         rnn_abi.MAX_UNITS) == (64, 4, 2, 3, 256, 128)
    assert (defs["RG_RNN_MODE_SAMPLE"], defs["RG_RNN_MODE_MEAN"]) == (rnn_abi.MODE_SAMPLE, rnn_abi.MODE_MEAN) == (policy_abi.MODE_SAMPLE, policy_abi.MODE_MEAN)
    assert "#define RG_RNN_MAX_T (1 << 16)" in _header() and rnn_abi.MAX_T == 1 << 16
    D = rnn_abi.DEFAULTS   # the reference's networks.py: policy_layers[:-1] of configs.py, GRUBlockCell(100)
    assert (D["obs_dim"], D["act_dim"], D["policy_layers"], D["gru_units"], D["value_layers"]) == (16, 2, (200,), 100, (200, 100))
    assert D["obs_clip"] == policy_abi.DEFAULTS["obs_clip"] == 5.0
    cc = rnn_abi.make_cconfig(policy_layers=(7, 9), gru_units=11, seed=2 ** 63 + 5)
    assert (cc.n_policy_layers, list(cc.policy_layers), cc.gru_units, cc.n_value_layers, list(cc.value_layers), cc.seed) == \
        (2, [7, 9], 11, 2, [200, 100, 0], 2 ** 63 + 5)
    with pytest.raises(TypeError):
        rnn_abi.make_cconfig(reward_clip=1.0)
    with pytest.raises(ValueError):
        rnn_abi.make_cconfig(policy_layers=(1, 2, 3))
    with pytest.raises(ValueError):
        rnn_abi.make_cconfig(value_layers=(1, 2, 3, 4))


def _set(cc, field, value):
    m = re.fullmatch(r"(\w+)\[(\d)\]", field)
    if m:
        getattr(cc, m.group(1))[int(m.group(2))] = value
    else:
        setattr(cc, field, value)


@pytest.mark.parametrize("field,value,text", [
    ("obs_dim", 0, "config.obs_dim"), ("obs_dim", 65, "config.obs_dim"), ("act_dim", 0, "config.act_dim"), ("act_dim", 5, "config.act_dim"),
    ("n_policy_layers", -1, "config.n_policy_layers"), ("n_policy_layers", 3, "config.n_policy_layers"),
    ("gru_units", 0, "config.gru_units"), ("gru_units", 129, "config.gru_units"),
    ("n_value_layers", -1, "config.n_value_layers"), ("n_value_layers", 4, "config.n_value_layers"),
    ("policy_layers[0]", 0, "config.policy_layers[0]"), ("policy_layers[0]", 257, "config.policy_layers[0]"),
    ("policy_layers[1]", 5, "config.policy_layers[1]"), ("value_layers[1]", 0, "config.value_layers[1]"), ("value_layers[0]", 257, "config.value_layers[0]"),
    ("value_layers[2]", 1, "config.value_layers[2]"), ("obs_clip", -1.0, "config.obs_clip"), ("obs_clip", NAN, "config.obs_clip"),
    ("obs_clip", INF, "config.obs_clip"), ("abi_version", 2, "config.abi_version"), ("reserved0", 1, "config.reserved0"),
])
def test_create_rejects_a_bad_config_naming_the_field(field, value, text):
    cc = rnn_abi.make_cconfig()
    _set(cc, field, value)
    for device in (0, rnn_abi.DEVICE_NONE):   # before it looks for a device: the same answer with and without one asked for
        rc, msg = rnn_abi.create_status(cc, device=device)
        assert rc == -1 and text in msg, (rc, msg)
    lay = rnn_abi.CLayout()
    assert rnn_abi.load_library().rg_rnn_param_layout(C.byref(cc), C.byref(lay)) == -1


def test_create_checks_batch_and_null_arguments():
    for batch in (0, -3, (1 << 24) + 1):
        for device in (0, rnn_abi.DEVICE_NONE):
            rc, msg = rnn_abi.create_status(batch=batch, device=device)
            assert rc == -1 and "batch" in msg
    lib = rnn_abi.load_library()
    assert lib.rg_rnn_create(None, 4, -1, C.byref(C.c_void_p())) == -1
    assert lib.rg_rnn_param_layout(None, None) == -1
    for settings in (dict(), dict(obs_clip=0.0), dict(policy_layers=(), value_layers=(), gru_units=1), CONFIGS["limits"]):
        rc, msg = rnn_abi.create_status(rnn_abi.make_cconfig(**settings))   # valid, host-only: a handle is made
        assert rc == 0, msg


def test_host_only_handle_checks_arguments_then_reports_no_device():
    h = rnn_abi.RnnHandle(4, rnn_abi.DEVICE_NONE, seed=3)
    lib = rnn_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p = dummy.ctypes.data
    last = lambda: lib.rg_rnn_last_error(h._h).decode()
    #        obs norm pp vp act_state reset hin hout mode action mean value logprob
    good = [p, p, p, p, p, p, p, p, 0, p, p, p, p]
    assert lib.rg_rnn_act(h._h, *good, None) == -3 and "host-only" in last()
    optional = list(good)
    optional[5] = optional[10] = optional[11] = optional[12] = None
    assert lib.rg_rnn_act(h._h, *optional, None) == -3
    same = list(good)
    same[7] = same[6]
    assert lib.rg_rnn_act(h._h, *same, None) == -3           # in place
    for k, name in ((0, "obs"), (1, "norm_state"), (2, "policy_params"), (3, "value_params"), (4, "act_state"), (6, "hidden_in"), (7, "hidden_out"),
                    (9, "action")):
        a = list(good)
        a[k] = None
        assert lib.rg_rnn_act(h._h, *a, None) == -1 and f"act: null {name}" in last(), last()
    a = list(good)
    a[4], a[8] = None, 1
    assert lib.rg_rnn_act(h._h, *a, None) == -3              # MEAN mode needs no act state
    for mode in (2, -1):
        a[8] = mode
        assert lib.rg_rnn_act(h._h, *a, None) == -1 and "mode" in last()
    #        obs reset h0 norm pp T mean hseq hlast
    good = [p, p, p, p, p, 5, p, p, p]
    assert lib.rg_rnn_unroll(h._h, *good, None) == -3 and "host-only" in last()
    a = list(good)
    a[7] = a[8] = None
    assert lib.rg_rnn_unroll(h._h, *a, None) == -3
    for k, name in ((0, "obs"), (1, "reset"), (2, "h0"), (3, "norm_state"), (4, "policy_params"), (6, "mean_out")):
        a = list(good)
        a[k] = None
        assert lib.rg_rnn_unroll(h._h, *a, None) == -1 and f"unroll: null {name}" in last(), last()
    for T in (0, -1, (1 << 16) + 1):
        a = list(good)
        a[5] = T
        assert lib.rg_rnn_unroll(h._h, *a, None) == -1 and "unroll: T" in last()
    for T in (1, 1 << 16):
        a = list(good)
        a[5] = T
        assert lib.rg_rnn_unroll(h._h, *a, None) == -3
    assert lib.rg_rnn_act(None, *([p] * 8), 0, *([p] * 4), None) == -1 and "null handle" in lib.rg_rnn_last_error(None).decode()
    assert lib.rg_rnn_unroll(None, *([p] * 5), 1, *([p] * 3), None) == -1 and "null handle" in lib.rg_rnn_last_error(None).decode()
    with pytest.raises(rnn_abi.RgRnnError) as e:
        h.unroll(p, p, p, p, p, 3, p)
    assert e.value.status == -3
    h.close()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_param_layout_is_the_rule(name):
    f = rnn_abi.rnn_fields(**CONFIGS[name])
    got = rnn_abi.param_layout(**CONFIGS[name])
    want = RM.layout(f["obs_dim"], f["act_dim"], f["policy_layers"], f["gru_units"], f["value_layers"])
    assert got == want
    H, n_x = f["gru_units"], (f["policy_layers"] or (f["obs_dim"],))[-1]
    assert got["n_x"] == n_x and got["w_ru"][:2] == (n_x + H, 2 * H) and got["w_c"][:2] == (n_x + H, H) and got["head"][:2] == (H, f["act_dim"])
    end = 0                                         # the policy buffer is dense: W then b of each block, logstd last
    for i, o, w, b in RM.blocks(got):
        assert (w, b) == (end, end + i * o)
        end = b + o
    assert end == got["logstd_offset"] and got["policy_count"] == end + f["act_dim"]
    assert got["value"] == policy_abi.param_layout(obs_dim=f["obs_dim"], act_dim=f["act_dim"], policy_layers=(), value_layers=f["value_layers"])["value"]


# ---- model known answers ----------------------------------------------------------------------------------------------

LOP = CONFIGS["lopsided"]


def _random_params(lay, rng, dtype=np.float32):
    pp = np.zeros(lay["policy_count"], dtype=dtype)
    for i, o, w, b in RM.blocks(lay):
        limit = math.sqrt(6.0 / (i + o))
        pp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        pp[b:b + o] = rng.normal(0.0, 0.5, o)
    pp[lay["logstd_offset"]:] = rng.normal(-1.0, 0.3, lay["policy_count"] - lay["logstd_offset"])
    vp = np.zeros(lay["value_count"], dtype=dtype)
    for i, o, w, b in lay["value"]:
        limit = math.sqrt(6.0 / (i + o))
        vp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        vp[b:b + o] = rng.normal(0.0, 0.1, o)
    return pp, vp


def _lop():
    rng = np.random.default_rng(0)
    lay = RM.layout(LOP["obs_dim"], LOP["act_dim"], LOP["policy_layers"], LOP["gru_units"], LOP["value_layers"])
    pp, _ = _random_params(lay, rng)
    x = rng.normal(size=(9, 6)).astype(np.float32)
    h = rng.uniform(-0.9, 0.9, size=(9, 5)).astype(np.float32)
    return lay, pp, x, h


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_update_gate_saturated_holds_the_state_or_takes_the_candidate_to_the_bit(dtype):
    lay, pp, x, h = _lop()
    H, b_ru = 5, lay["w_ru"][3]
    hold = pp.copy()
    hold[b_ru + H:b_ru + 2 * H] = 100.0
    out = RM.tick(x, h, None, hold, lay, dtype)
    assert np.all(out["u"] == 1.0) and out["hidden"].dtype == dtype and out["hidden"].tobytes() == h.astype(dtype).tobytes()
    take = pp.copy()
    take[b_ru + H:b_ru + 2 * H] = -100.0
    out = RM.tick(x, h, None, take, lay, dtype)
    assert np.all(out["u"] <= 1e-40) and out["hidden"].tobytes() == out["c"].tobytes() and np.abs(out["c"]).max() > 0.1
    if dtype == np.float32:
        assert np.all(out["u"] == 0.0)                        # expf overflows to inf: the gate is exactly shut
    free = RM.tick(x, h, None, pp, lay, dtype)                # neither: strictly between
    assert np.all((free["u"] > 0) & (free["u"] < 1)) and not np.array_equal(free["hidden"], free["c"])


def test_reset_gate_shut_makes_the_candidate_independent_of_the_state():
    lay, pp, x, h = _lop()
    shut = pp.copy()
    b_ru = lay["w_ru"][3]
    shut[b_ru:b_ru + 5] = -100.0
    for dtype in (np.float64, np.float32):
        a = RM.tick(x, h, None, shut, lay, dtype)
        b = RM.tick(x, -h[::-1], None, shut, lay, dtype)
        if dtype == np.float32:                               # expf overflows to inf: r is exactly 0
            assert np.all(a["r"] == 0.0) and a["c"].tobytes() == b["c"].tobytes()
        else:                                                 # r = 1 / (1 + e^100 ...): below 1e-40, nothing of h is left at 1e-15
            assert np.all(a["r"] <= 1e-40) and np.abs(a["c"] - b["c"]).max() <= 1e-15
        assert not np.array_equal(a["u"], b["u"])             # the update gate still sees h
        c, d = RM.tick(x, h, None, pp, lay, dtype), RM.tick(x, -h[::-1], None, pp, lay, dtype)
        assert not np.array_equal(c["c"], d["c"])


def test_reset_is_a_zero_state_and_the_unroll_is_a_chain_of_ticks():
    lay, pp, x, h = _lop()
    reset = np.array([1, 0, 0, 5, 0, 0, -1, 0, 1])
    for dtype in (np.float64, np.float32):
        got = RM.tick(x, h, reset, pp, lay, dtype)
        zeroed = RM.tick(x, np.where(reset[:, None] != 0, 0, h), None, pp, lay, dtype)
        for k in ("hidden", "mean", "u", "c"):
            assert got[k].tobytes() == zeroed[k].tobytes()
        assert not np.array_equal(got["hidden"], RM.tick(x, h, None, pp, lay, dtype)["hidden"])
    # the hand-written cell once more, from the formulas, in float64
    (W_ru, b_ru), (W_c, b_c), (W_h, b_h) = PM.split(pp, [lay["w_ru"], lay["w_c"], lay["head"]])
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    xh = np.concatenate([x, h], axis=1).astype(np.float64)
    r, u = np.split(sig(xh @ W_ru + b_ru), 2, axis=1)
    c = np.tanh(np.concatenate([x, r * h], axis=1) @ W_c + b_c)
    hn = u * h + (1 - u) * c
    out = RM.tick(x, h, None, pp, lay)
    assert np.allclose(out["hidden"], hn, rtol=1e-14, atol=1e-16) and np.allclose(out["mean"], np.tanh(hn @ W_h + b_h), rtol=1e-14, atol=1e-16)
    # unroll: a chain of ticks from h0, the state carried
    rng = np.random.default_rng(1)
    T, B = 4, 3
    obs = rng.normal(size=(T, 6, B)).astype(np.float32)
    rs = np.zeros((T, B), dtype=np.int32)
    rs[2, 1] = 1
    state = np.zeros(PM.NORM_ROWS)
    mean, hseq = RM.unroll(obs, rs, h[:B], state, pp, lay)
    hh = h[:B].astype(np.float64)
    for t in range(T):
        o = RM.tick(obs[t].T, hh, rs[t], pp, lay)
        hh = o["hidden"]
        assert np.array_equal(mean[t], o["mean"]) and np.array_equal(hseq[t], hh)


# ---- the host-only policy, torch on the CPU in float64 ----------------------------------------------------------------

def _tiny(seed=0, T=5, B=4, mask_some=True, cfg=LOP):
    """A host-only float64 policy with random parameters and normaliser state, and a synthetic rollout with resets in the
    middle of the sequence and a non-zero h0."""
    rng = np.random.default_rng(seed)
    pol = RecurrentGaussianPolicy(B, device="cpu", dtype=torch.float64, seed=seed, **cfg)
    d, A, H = pol.obs_dim, pol.act_dim, pol.gru_units
    pp, vp = _random_params(pol.layout, rng, np.float64)
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(pp))
        pol.value_params.copy_(torch.as_tensor(vp))
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    on.update(rng.normal(0.2, 1.5, size=(30, d)))
    rn.update(rng.normal(0.0, 3.0, size=(30, 1)))
    pol.norm_state.copy_(torch.as_tensor(PM.norm_state_of(on, rn)))
    ro = RecurrentRolloutBuffer(T, B, d, A, H, dtype=torch.float64)
    ro.obs.copy_(torch.as_tensor(rng.normal(0.2, 4.5, size=(T, d, B))))     # three sigma of the normaliser's data: some reach the clip
    ro.h0.copy_(torch.as_tensor(rng.uniform(-0.9, 0.9, size=(B, H))))
    ro.reset[0, 0] = 1
    ro.reset[min(2, T - 1), 1] = 1
    ro.reset[min(3, T - 1), 2 % B] = 1
    ro.mean.copy_(torch.as_tensor(np.tanh(rng.normal(0, 0.5, size=(T, B, A)))))
    ro.logstd.copy_(torch.as_tensor(rng.normal(-1, 0.2, size=A)))
    ro.action.copy_(ro.mean + torch.exp(ro.logstd) * torch.as_tensor(rng.normal(size=(T, B, A))))
    ro.adv.copy_(torch.as_tensor(rng.normal(0.5, 2.0, size=(T, B))))
    ro.ret.copy_(torch.as_tensor(rng.normal(0.0, 2.0, size=(T, B))))
    if mask_some:
        ro.mask[2, 1] = 0
        ro.mask[1:, 3] = 0
    return pol, ro, on


def _model_forward(pol, ro):
    """The float64 model on the float64 normalised observations (no rounding to float32 in between, as the torch ops)."""
    pp, vp = pol.policy_params.detach().numpy(), pol.value_params.detach().numpy()
    on, _ = PM.normalizers_of(pol.norm_state.numpy(), pol.obs_dim, pol.obs_clip)
    x = on.transform(ro.obs.numpy().transpose(0, 2, 1))
    h = ro.h0.numpy()
    means = []
    for t in range(ro.T):
        o = RM.tick(x[t], h, ro.reset.numpy()[t], pp, pol.layout)
        h = o["hidden"]
        means.append(o["mean"])
    value = PM.forward(x.reshape(ro.T * ro.batch, -1), PM.split(vp, pol.layout["value"]), "linear").reshape(ro.T, ro.batch)
    return x, np.stack(means), value, h, pp[pol.layout["logstd_offset"]:]


@pytest.mark.parametrize("cfg", [LOP, dict(obs_dim=5, act_dim=2, policy_layers=(7, 4), gru_units=3, value_layers=(6,))])
def test_evaluate_sequence_equals_the_models_unroll(cfg):
    pol, ro, on = _tiny(cfg=cfg)
    x, mean, value, h_last, _ = _model_forward(pol, ro)
    assert np.abs(x).max() == 5.0                                            # the clip is exercised
    xt = pol.normalize_obs(ro.obs.permute(0, 2, 1))
    m, v = pol.evaluate_sequence(xt, ro.reset, ro.h0)
    assert m.shape == (ro.T, ro.batch, pol.act_dim) and v.shape == (ro.T, ro.batch)
    assert np.abs(m.detach().numpy() - mean).max() <= 1e-12 and np.abs(v.detach().numpy() - value).max() <= 1e-12
    hs = pol.evaluate_hidden(xt, ro.reset, ro.h0)
    assert np.abs(hs[-1].detach().numpy() - h_last).max() <= 1e-12
    no_reset, _ = pol.evaluate_sequence(xt, torch.zeros_like(ro.reset), ro.h0)
    assert np.abs(no_reset.detach().numpy() - mean).max() > 1e-3             # the resets and h0 matter
    zero_h0, _ = pol.evaluate_sequence(xt, ro.reset, torch.zeros_like(ro.h0))
    assert np.abs(zero_h0.detach().numpy() - mean).max() > 1e-3
    with pytest.raises(TypeError):
        pol.evaluate(xt)


def test_evaluate_sequence_passes_gradcheck_and_takes_no_gradient_of_h0():
    pol, ro, on = _tiny(seed=4, T=3, B=2, mask_some=False, cfg=dict(obs_dim=3, act_dim=2, policy_layers=(4,), gru_units=3, value_layers=(3,)))
    x = pol.normalize_obs(ro.obs.permute(0, 2, 1)).detach()
    lay = pol.layout

    def f(pp, vp, xin):
        pol.policy_params, pol.value_params = pp, vp
        mean, value = pol.evaluate_sequence(xin, ro.reset, ro.h0)
        return mean, value
    pp = pol.policy_params.detach().clone().requires_grad_(True)
    vp = pol.value_params.detach().clone().requires_grad_(True)
    xin = x.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(f, (pp, vp, xin), eps=1e-6, atol=1e-7, rtol=1e-5)
    h0 = ro.h0.clone().requires_grad_(True)
    mean, _ = pol.evaluate_sequence(xin, ro.reset, h0)
    assert mean.requires_grad
    mean.sum().backward()
    assert h0.grad is None                                                   # h0 enters as a constant
    g = pp.grad
    assert g is not None and all(float(g[w:w + i * o].abs().max()) > 0 for i, o, w, b in RM.blocks(lay))


def test_a_reset_cuts_the_dependence_on_earlier_observations_to_exact_zeros():
    pol, ro, on = _tiny(seed=5)
    T, B = ro.T, ro.batch
    x = pol.normalize_obs(ro.obs.permute(0, 2, 1)).detach()
    x = x.clone().requires_grad_(True)                                       # a leaf: the Jacobian is taken with respect to it
    mean, _ = pol.evaluate_sequence(x, ro.reset, ro.h0)
    for b, t_reset in ((1, 2), (2, 3)):
        for t in range(T):
            grad, = torch.autograd.grad(mean[t, b].sum(), x, retain_graph=True)
            g = grad.abs().sum(-1)                                           # [T, B]: the mean of (t, b) with respect to every tick
            assert torch.all(g[:, [k for k in range(B) if k != b]] == 0)      # robots do not mix
            assert torch.all(g[t + 1:, b] == 0)                              # nothing from the future
            assert float(g[t, b]) > 0
            if t >= t_reset:
                assert torch.all(g[:t_reset, b] == 0), (b, t)              # exact zeros across the reset
                assert torch.all(g[t_reset:t + 1, b] > 0)
            else:
                assert torch.all(g[:t + 1, b] > 0), (b, t)                   # before it, every earlier tick reaches the mean
    grad, = torch.autograd.grad(mean[T - 1, 3].sum(), x)                     # a robot without a reset: the whole sequence
    assert torch.all(grad.abs().sum(-1)[:, 3] > 0)


@pytest.mark.parametrize("conv", ["exact", "reference"])
def test_losses_equal_the_formulas_in_numpy(conv):
    pol, ro, on = _tiny(seed=1)
    ppo = RecurrentPPO(pol, kl_init_penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2, kl_cutoff_coef=1000, conv_logpdf=conv)
    b = ppo.batch(ro)
    x, mean, value, _, logstd = _model_forward(pol, ro)
    valid = (ro.mask.numpy() != 0).astype(np.float64)
    adv = ro.adv.numpy()
    sel = adv[valid != 0]
    adv_n = (adv - sel.mean()) / (sel.std() + 1e-8)
    assert np.allclose(b["adv"].numpy(), adv_n, rtol=1e-13, atol=1e-15)
    old_mean, old_logstd, action = ro.mean.numpy(), ro.logstd.numpy(), ro.action.numpy()
    kl = (PM.diag_normal_kl(old_mean, old_logstd, mean, logstd) * valid).mean(axis=0)
    ratio = np.exp(PM.diag_normal_logpdf(mean, logstd, action, conv) - PM.diag_normal_logpdf(old_mean, old_logstd, action, conv))
    surrogate = -(ratio * adv_n * valid).mean(axis=0)
    threshold = 2 * 1e-2
    assert (kl > threshold).any()                                              # the cutoff term is exercised
    want = np.mean(surrogate + 0.7 * kl + 1000 * (kl > threshold) * (kl - threshold) ** 2)
    assert math.isclose(float(ppo.policy_loss(b).detach()), want, rel_tol=1e-12)
    assert np.allclose(ppo.kl(b).detach().numpy(), kl, rtol=1e-12)
    want_v = np.mean(0.5 * (ro.ret.numpy() - value) ** 2 * valid)
    assert math.isclose(float(ppo.value_loss(b).detach()), want_v, rel_tol=1e-12)


def test_an_unchanged_policy_gives_ratio_one_and_kl_zero_and_the_update_steps_in_place():
    pol, ro, on = _tiny(seed=2, mask_some=False)
    with torch.no_grad():   # the behaviour policy IS the current one
        ro.logstd.copy_(pol.logstd)
        mean, _ = pol.evaluate_sequence(pol.normalize_obs(ro.obs.permute(0, 2, 1)), ro.reset, ro.h0)
        ro.mean.copy_(mean)
        ro.action.copy_(mean + torch.exp(pol.logstd) * torch.as_tensor(np.random.default_rng(3).normal(size=tuple(mean.shape))))
    ppo = RecurrentPPO(pol, epochs_policy=0, epochs_value=0, kl_init_penalty=2.0)
    b = ppo.batch(ro)
    from robot_gym_amd.agents.ppo import diag_normal_logpdf
    m, _ = pol.evaluate_sequence(b["x"], b["reset"], b["h0"])
    ratio = torch.exp(diag_normal_logpdf(m, pol.logstd, b["action"]) - diag_normal_logpdf(b["old_mean"], b["old_logstd"], b["action"]))
    assert float((ratio - 1.0).abs().max().detach()) <= 1e-12 and float(ppo.kl(b).abs().max().detach()) <= 1e-12
    assert math.isclose(float(ppo.policy_loss(b).detach()), float(-(b["adv"]).mean()), rel_tol=1e-12, abs_tol=1e-12)   # ratio 1: minus the mean advantage
    out = ppo.update(ro)
    assert abs(out["kl_change"]) <= 1e-12 and math.isclose(ppo.penalty, 2.0 / 1.5, rel_tol=1e-15)
    ptrs = (pol.policy_params.data_ptr(), pol.value_params.data_ptr())
    before = (pol.policy_params.detach().clone(), pol.value_params.detach().clone())
    out = RecurrentPPO(pol, epochs_policy=4, epochs_value=4).update(ro)
    assert (pol.policy_params.data_ptr(), pol.value_params.data_ptr()) == ptrs
    changed = (pol.policy_params.detach() != before[0])
    for i, o, w, bb in RM.blocks(pol.layout):                                # back-propagation reaches every block, the cell's included
        assert bool(changed[w:w + i * o].any()) and bool(changed[bb:bb + o].any())
    assert not torch.equal(pol.value_params.detach(), before[1])
    assert out["value_loss_last"] < out["value_loss_first"] and out["policy_loss_last"] < out["policy_loss_first"]


def test_state_clone_and_initialisation():
    pol = RecurrentGaussianPolicy(4, device="cpu", seed=4)
    assert tuple(pol.hidden.shape) == (4, 100) and pol.hidden.dtype == torch.float32 and float(pol.hidden.abs().max()) == 0.0
    assert pol.pending_reset.dtype == torch.int32 and pol.pending_reset.tolist() == [1, 1, 1, 1]
    (W_ru, b_ru), (W_c, b_c) = pol.cell
    for W, (i, o) in ((W_ru, (300, 200)), (W_c, (300, 100)), (pol.dense_layers[0][0], (16, 200))):
        limit = math.sqrt(6.0 / (i + o))
        assert tuple(W.shape) == (i, o) and 0.8 * limit < float(W.detach().abs().max()) <= limit
    assert torch.all(b_ru == 1.0) and torch.all(b_c == 0.0) and float(pol.dense_layers[0][1].detach().abs().max()) == 0.0
    W, b = pol.head
    std = math.sqrt(1.3 * 0.1 / 100)
    assert tuple(W.shape) == (100, 2) and float(W.detach().abs().max()) <= 2 * std + 1e-7 and 0.5 * std < float(W.detach().std()) < std and float(b.detach().abs().max()) == 0.0
    assert pol.logstd.tolist() == [-1.0, -1.0]
    for (W, b), (i, o) in zip(pol.value_layers, ((16, 200), (200, 100), (100, 1))):
        assert tuple(W.shape) == (i, o) and float(W.detach().abs().max()) > 0 and float(b.detach().abs().max()) == 0.0
    again = RecurrentGaussianPolicy(4, device="cpu", seed=4)
    assert torch.equal(again.policy_params, pol.policy_params) and torch.equal(again.value_params, pol.value_params)
    assert not torch.equal(RecurrentGaussianPolicy(4, device="cpu", seed=5).policy_params, pol.policy_params)
    # the views alias the buffers
    with torch.no_grad():
        W_c[3, 7] = 9.0
    assert float(pol.policy_params.detach()[pol.layout["w_c"][2] + 3 * 100 + 7]) == 9.0
    # pending_reset, clone, state_dict
    pol.pending_reset.zero_()
    pol.begin_episodes(torch.tensor([0, 1, 0, 0], dtype=torch.int32))
    assert pol.pending_reset.tolist() == [0, 1, 0, 0]
    pol.hidden.copy_(torch.arange(400, dtype=torch.float32).view(4, 100))
    pol.act_state[1] = torch.tensor([5, 6, 7, 8])
    pol.clone([1, 0], [2, 3])
    assert torch.equal(pol.hidden[2], pol.hidden[1]) and torch.equal(pol.hidden[3], pol.hidden[0]) and pol.pending_reset.tolist() == [0, 1, 1, 0]
    assert pol.act_state[:, 2].tolist() == [1, 6] and pol.act_state[:, 3].tolist() == [0, 5]
    state = pol.state_dict()
    ptr = pol.hidden.data_ptr()
    pol.hidden.zero_()
    pol.begin_episodes()
    assert pol.pending_reset.tolist() == [1, 1, 1, 1]
    with torch.no_grad():
        pol.policy_params.zero_()
    pol.load_state_dict(state)
    assert torch.equal(pol.hidden, state["hidden"]) and pol.hidden.data_ptr() == ptr and pol.pending_reset.tolist() == [0, 1, 1, 0]
    assert torch.equal(pol.policy_params.detach(), state["policy_params"])
    with pytest.raises(ValueError):
        RecurrentGaussianPolicy(4, device="cpu", gru_units=7).load_state_dict(state)
    with pytest.raises(rnn_abi.RgRnnError) as e:                                 # no CPU fallback
        pol.act(torch.zeros(16, 4))
    assert e.value.status == -3
    with pytest.raises(rnn_abi.RgRnnError) as e:
        pol.unroll(RecurrentRolloutBuffer(3, 4))
    assert e.value.status == -3
    pol.close()


# ---- resources of rg_rnn.hip ------------------------------------------------------------------------------------------

KERNELS = {"rg_rnn_act_kernel", "rg_rnn_unroll_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_rnn.hip")


def test_every_rnn_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_rnn_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


# DESIGN.md section 7, in floats of the header's limits.  act: two x buffers for each of the two networks, h, r*h and u, and the
# noise of a tile.  unroll: the policy's two x buffers, h, r*h and u, and its copy of the descriptor (at most 256 bytes).
W_, H_, A_, T_ = rnn_abi.MAX_WIDTH, rnn_abi.MAX_UNITS, rnn_abi.MAX_ACT, rnn_abi.TILE
LDS_BUDGET = {"rg_rnn_act_kernel": (4 * W_ + 3 * H_ + A_) * T_ * 4, "rg_rnn_unroll_kernel": (2 * W_ + 3 * H_) * T_ * 4 + 256}


def test_lds_is_within_the_budget(remarks):
    assert LDS_BUDGET == {"rg_rnn_act_kernel": 45184, "rg_rnn_unroll_kernel": 28928}
    for name, budget in LDS_BUDGET.items():
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= budget <= 65536, (name, remarks[name])


# What the device-only compile reports today (upper bounds; occupancy a lower bound).  The act kernel's workgroup is eight
# waves, two per SIMD: at four waves per SIMD two workgroups share a compute unit.
REGISTERS = {"rg_rnn_act_kernel": dict(vgprs=110, agprs=0, occupancy=4), "rg_rnn_unroll_kernel": dict(vgprs=128, agprs=0, occupancy=4)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    own = open(os.path.join(SRC, "rg_rnn.hip")).read()
    code = re.sub(r"//.*", "", own)
    assert "asm" not in code and "atomic" not in own.lower()
    assert code.index("#pragma clang fp contract(off)") < code.index("__global__")
    assert code.index("#pragma clang fp contract(off)") < code.index("__device__")
    assert code.index("#pragma clang fp contract(off)") < code.index('#include "rg_agent_dev.inc"') < code.index('#include "rg_gru_dev.inc"')
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_policy.h", "../../include/rg_rnn.h", "rg_host.h", "rg_agent_dev.inc",
                                                      "rg_gru_dev.inc"]
    assert not re.search(r"\b(chain8|sigmoidf)\s*\([^;{]*\)\s*\{", code)         # the tick's device code is rg_gru_dev.inc's alone
    import bench
    assert not any("rg_rnn" in rel for rel in bench.compiled_sources())          # the MPC hash behind profiles/ does not follow it
    for other in ("rg_mpc.hip", "rg_policy.hip", "rg_ppo.hip", "rg_ddpg.hip"):
        assert "rg_rnn" not in open(os.path.join(SRC, other)).read(), other
    kernel_checks.assert_built_into_both("rg_rnn.hip", header="rg_rnn.h")
