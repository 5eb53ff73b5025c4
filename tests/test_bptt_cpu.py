"""The recurrent PPO policy update on the device (include/rg_bptt.h) without a GPU: librg_mpc.so exports every rg_bptt_* entry,
the ctypes binding matches the header, create validates both configurations, T, B and T * B (naming the field) before it
looks for a device, a host-only handle checks every pointer and then returns NO_DEVICE; the numpy model's float64 gradient
(tests/bptt_model.py) against torch autograd through RecurrentPPO.policy_loss, and its known answers; every case of
tests/test_bptt_gpu.py builds from the model within its caps; the kernels of rg_bptt.hip cross-compile for gfx950 without
scratch or spills, within their LDS budget."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import DeviceRecurrentPPO, RecurrentGaussianPolicy, RecurrentPPO, RecurrentRolloutBuffer
from robot_gym_amd.core import bptt_abi, ppo_abi, rnn_abi
from tests import bptt_cases as BC
from tests import bptt_model as BM
from tests import kernel_checks
from tests import policy_model as PM
from tests import rnn_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_bptt.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI and configuration ------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = bptt_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_bptt_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 13
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(bptt_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None, name
    for entry in ("create", "workspace_bytes", "opt_state_bytes", "groups", "policy_grad", "kl", "adam", "penalty", "update_policy"):
        assert entry in bptt_abi.SIGNATURES


def test_constants_match_header_and_binding():
    lib = bptt_abi.load_library()
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_BPTT_\w+) \(?(-?\d+)\)?", _header())}
    assert lib.rg_bptt_abi_version() == defs["RG_BPTT_ABI_VERSION"] == bptt_abi.ABI_VERSION == 1
    assert lib.rg_bptt_tile() == bptt_abi.TILE == rnn_abi.TILE
    assert (defs["RG_BPTT_CHUNK"], defs["RG_BPTT_ROWS"], defs["RG_BPTT_MAX_GROUPS"], defs["RG_BPTT_STATS"], defs["RG_BPTT_OPT_HEADER_BYTES"],
            defs["RG_BPTT_DEVICE_NONE"]) == (bptt_abi.CHUNK, bptt_abi.ROWS, bptt_abi.MAX_GROUPS, bptt_abi.STATS, bptt_abi.OPT_HEADER_BYTES,
                                             bptt_abi.DEVICE_NONE) == (16, 16, 64, 4, 16, -1)
    assert len(bptt_abi.STAT_NAMES) == bptt_abi.STATS and set(bptt_abi.STAT_NAMES) < set(ppo_abi.STAT_NAMES)
    assert '#include "rg_ppo.h"' in _header() and '#include "rg_rnn.h"' in _header()     # the structures are those two headers'
    with pytest.raises(TypeError):
        bptt_abi.BpttHandle(3, 4, bptt_abi.DEVICE_NONE, no_such_setting=1)


@pytest.mark.parametrize("name", list(BC.CONFIGS))
@pytest.mark.parametrize("T,B", [(1, 1), (3, 5), (8, 1037), (32, 4096)])
def test_sizes_of_a_handle(name, T, B):
    cfg = BC.CONFIGS[name]
    h = bptt_abi.BpttHandle(T, B, bptt_abi.DEVICE_NONE, rnn_settings=cfg)
    lay = rnn_abi.param_layout(**cfg)
    count, N, H, A = lay["policy_count"], T * B, cfg["gru_units"], cfg["act_dim"]
    assert h.opt_state_bytes == bptt_abi.OPT_HEADER_BYTES + 8 * count and h.opt_state_bytes % 8 == 0
    assert h.groups == bptt_abi.groups(T, B) <= bptt_abi.MAX_GROUPS
    per_sample = 4 * (cfg["obs_dim"] + 2 * sum(cfg["policy_layers"]) + 9 * H + 2 * A) + 8                    # rg_bptt.h, Workspace
    fixed = 8 * h.groups * count + 2 * 4 * count
    assert fixed + N * per_sample <= h.workspace_bytes <= fixed + N * per_sample + 65536 + 8 * B + 8 * 20 and h.workspace_bytes % 8 == 0
    h.close()


def _set(cc, field, value):
    m = re.fullmatch(r"(\w+)\[(\d)\]", field)
    if m:
        getattr(cc, m.group(1))[int(m.group(2))] = value
    else:
        setattr(cc, field, value)


@pytest.mark.parametrize("field,value", [
    ("obs_dim", 0), ("obs_dim", 65), ("act_dim", 0), ("act_dim", 5), ("n_policy_layers", -1), ("n_policy_layers", 3), ("gru_units", 0), ("gru_units", 129),
    ("n_value_layers", -1), ("n_value_layers", 4), ("policy_layers[0]", 0), ("policy_layers[0]", 257), ("policy_layers[1]", 5), ("value_layers[1]", 0),
    ("value_layers[0]", 257), ("value_layers[2]", 1), ("obs_clip", -1.0), ("obs_clip", NAN), ("obs_clip", INF), ("abi_version", 2), ("reserved0", 1),
])
def test_create_rejects_a_bad_rnn_config_naming_the_field(field, value):
    cc = rnn_abi.make_cconfig()
    _set(cc, field, value)
    for device in (0, bptt_abi.DEVICE_NONE):   # before it looks for a device: the same answer with and without one asked for
        rc, msg = bptt_abi.create_status(cc, device=device)
        assert rc == -1 and "rnn_cfg." + field in msg, (rc, msg)


@pytest.mark.parametrize("field,value", [
    ("abi_version", 0), ("epochs_policy", -1), ("epochs_policy", (1 << 20) + 1), ("epochs_value", -1), ("conv_logpdf", 2), ("conv_logpdf", -1),
    ("policy_lr", -1e-3), ("policy_lr", NAN), ("value_lr", INF), ("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", NAN), ("adam_eps", 0.0),
    ("adam_eps", -1e-8), ("kl_target", 0.0), ("kl_target", INF), ("kl_cutoff_factor", -1.0), ("kl_cutoff_coef", -1.0), ("kl_cutoff_coef", NAN),
])
def test_create_rejects_a_bad_ppo_config_naming_the_field(field, value):
    cc = ppo_abi.make_cconfig()
    setattr(cc, field, value)
    for device in (0, bptt_abi.DEVICE_NONE):
        rc, msg = bptt_abi.create_status(None, cc, device=device)
        assert rc == -1 and "ppo_cfg." + field in msg, (rc, msg)


def test_create_checks_T_B_their_product_and_null_arguments():
    for device in (0, bptt_abi.DEVICE_NONE):
        for T in (0, -1, bptt_abi.MAX_T + 1):
            rc, msg = bptt_abi.create_status(T=T, device=device)
            assert rc == -1 and msg.startswith("T:"), msg
        for B in (0, -2, bptt_abi.MAX_BATCH + 1):
            rc, msg = bptt_abi.create_status(B=B, device=device)
            assert rc == -1 and msg.startswith("B:"), msg
        rc, msg = bptt_abi.create_status(T=1 << 16, B=(1 << 14) + 1, device=device)
        assert rc == -1 and msg.startswith("T * B:"), msg
    rc, msg = bptt_abi.create_status(T=1 << 16, B=1 << 14)          # the most samples: a host-only handle is made
    assert rc == 0, msg
    lib = bptt_abi.load_library()
    rc_, cc, out = rnn_abi.make_cconfig(), ppo_abi.make_cconfig(), C.c_void_p()
    assert lib.rg_bptt_create(None, C.byref(cc), 4, 4, -1, C.byref(out)) == -1
    assert lib.rg_bptt_create(C.byref(rc_), None, 4, 4, -1, C.byref(out)) == -1
    assert lib.rg_bptt_create(C.byref(rc_), C.byref(cc), 4, 4, -1, None) == -1 and "null" in lib.rg_bptt_last_error(None).decode()
    assert lib.rg_bptt_workspace_bytes(None) == -1 and lib.rg_bptt_opt_state_bytes(None) == -1 and lib.rg_bptt_groups(None) == -1
    for name, cfg in BC.CONFIGS.items():
        rc, msg = bptt_abi.create_status(rnn_abi.make_cconfig(**cfg))
        assert rc == 0, (name, msg)


def test_host_only_handle_checks_every_pointer_then_reports_no_device():
    h = bptt_abi.BpttHandle(3, 4, bptt_abi.DEVICE_NONE)
    lib = bptt_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p = dummy.ctypes.data
    last = lambda: lib.rg_bptt_last_error(h._h).decode()
    slots = ("obs", "action", "mean", "logstd", "adv", "ret", "mask")
    full = lambda **kw: ppo_abi.make_crollout(**{**{s: p for s in slots}, **kw})
    entries = {
        "policy_grad": (lib.rg_bptt_policy_grad, ("obs", "action", "mean", "logstd", "adv", "mask"),
                        ("reset", "h0", "adv_stats", "norm_state", "policy_params", "opt_state", "workspace", "grad_out", "loss_out")),
        "kl": (lib.rg_bptt_kl, ("obs", "mean", "logstd", "mask"), ("reset", "h0", "norm_state", "policy_params", "workspace", "kl_out")),
        "update_policy": (lib.rg_bptt_update_policy, ("obs", "action", "mean", "logstd", "adv", "mask"),
                          ("reset", "h0", "adv_stats", "norm_state", "policy_params", "opt_state", "workspace", "stats")),
    }
    for call, (fn, read, names) in entries.items():
        good = [p] * len(names)
        assert fn(h._h, C.byref(full()), *good, None) == -3 and "host-only" in last(), call
        assert fn(h._h, C.byref(full(ret=None)), *good, None) == -3                       # ret is not read
        assert fn(h._h, None, *good, None) == -1 and f"{call}: null rollout" in last()
        for s in read:
            assert fn(h._h, C.byref(full(**{s: None})), *good, None) == -1 and f"{call}: null rollout.{s}" in last(), (call, s, last())
        for s in set(slots) - set(read):
            assert fn(h._h, C.byref(full(**{s: None})), *good, None) == -3, (call, s)      # slots the entry does not read
        for k, name in enumerate(names):
            a = list(good)
            a[k] = None
            assert fn(h._h, C.byref(full()), *a, None) == -1 and f"{call}: null {name}" in last(), (call, name, last())
        assert fn(None, C.byref(full()), *good, None) == -1 and "null handle" in lib.rg_bptt_last_error(None).decode()
    for call, fn, names in (("adam", lib.rg_bptt_adam, ("params", "grad", "opt_state")), ("penalty", lib.rg_bptt_penalty, ("kl", "opt_state", "stats"))):
        good = [p] * 3
        assert fn(h._h, *good, None) == -3 and "host-only" in last()
        for k, name in enumerate(names):
            a = list(good)
            a[k] = None
            assert fn(h._h, *a, None) == -1 and f"{call}: null {name}" in last(), (call, name, last())
        assert fn(None, *good, None) == -1 and "null handle" in lib.rg_bptt_last_error(None).decode()
    with pytest.raises(bptt_abi.RgBpttError) as e:
        h.adam(p, p, p)
    assert e.value.status == -3 and "NO_DEVICE" in str(e.value)
    h.close()


# ---- the model against torch autograd, float64 ----------------------------------------------------------------------------

TWO_DENSE = dict(obs_dim=5, act_dim=2, policy_layers=(7, 4), gru_units=3, value_layers=(6,))


def _random_params(lay, rng):
    pp = np.zeros(lay["policy_count"])
    for i, o, w, b in RM.blocks(lay):
        limit = math.sqrt(6.0 / (i + o))
        pp[w:w + i * o] = rng.uniform(-limit, limit, i * o)
        pp[b:b + o] = rng.normal(0.0, 0.5, o)
    pp[lay["logstd_offset"]:] = rng.normal(-1.0, 0.3, lay["policy_count"] - lay["logstd_offset"])
    return pp


def _tiny(cfg, seed=0, T=6, B=5):
    """A host-only float64 policy with random parameters and normaliser state, and a synthetic rollout with resets at tick 0, in
    the middle of the sequence and at the last tick, masked ticks and a non-zero h0."""
    rng = np.random.default_rng(seed)
    pol = RecurrentGaussianPolicy(B, device="cpu", dtype=torch.float64, seed=seed, **cfg)
    d, A, H = pol.obs_dim, pol.act_dim, pol.gru_units
    with torch.no_grad():
        pol.policy_params.copy_(torch.as_tensor(_random_params(pol.layout, rng)))
    on, rn = PM.Normalizer(d, True, 5.0), PM.Normalizer(1, False, 10.0)
    on.update(rng.normal(0.2, 1.5, size=(30, d)))
    rn.update(rng.normal(0.0, 3.0, size=(30, 1)))
    pol.norm_state.copy_(torch.as_tensor(PM.norm_state_of(on, rn)))
    ro = RecurrentRolloutBuffer(T, B, d, A, H, dtype=torch.float64)
    ro.obs.copy_(torch.as_tensor(rng.normal(0.2, 4.5, size=(T, d, B))))
    ro.h0.copy_(torch.as_tensor(rng.uniform(-0.9, 0.9, size=(B, H))))
    ro.reset[0, 0] = 1
    ro.reset[2, 1] = 1
    ro.reset[3, 2] = 7
    ro.reset[T - 1, 3] = -1
    ro.mean.copy_(torch.as_tensor(np.tanh(rng.normal(0, 0.5, size=(T, B, A)))))
    ro.logstd.copy_(torch.as_tensor(rng.normal(-1, 0.2, size=A)))
    ro.action.copy_(ro.mean + torch.exp(ro.logstd) * torch.as_tensor(rng.normal(size=(T, B, A))))
    ro.adv.copy_(torch.as_tensor(rng.normal(0.5, 2.0, size=(T, B))))
    ro.mask[2, 1] = 0
    ro.mask[:, 4] = 0          # a robot with no valid tick: its KL is 0, below the cutoff
    return pol, ro


def _model_args(pol, ro, x):
    return (x, ro.reset.numpy(), ro.h0.numpy(), pol.policy_params.detach().numpy(), pol.layout, ro.action.numpy(), ro.mean.numpy(), ro.logstd.numpy(),
            ro.adv.numpy(), ro.mask.numpy())


@pytest.mark.parametrize("conv", ["exact", "reference"])
@pytest.mark.parametrize("cfg", [BC.CONFIGS["lopsided"], TWO_DENSE], ids=["lopsided", "two dense"])
def test_the_models_gradient_is_torch_autograd_through_policy_loss(cfg, conv):
    pol, ro = _tiny(cfg, seed=3)
    kw = dict(kl_target=1e-2, kl_cutoff_factor=2, kl_cutoff_coef=1000)
    ppo = RecurrentPPO(pol, kl_init_penalty=0.7, conv_logpdf=conv, **kw)
    b = ppo.batch(ro)
    loss = ppo.policy_loss(b)
    loss.backward()
    want = pol.policy_params.grad.numpy()
    got = BM.policy_grad(*_model_args(pol, ro, b["x"].numpy()), penalty=0.7, conv=conv, **kw)
    assert got["over"].any() and not got["over"].all()                          # the cutoff term is active, and not for every robot
    assert math.isclose(got["loss"], float(loss.detach()), rel_tol=1e-12)
    assert np.allclose(got["kl"], ppo.kl(b).detach().numpy(), rtol=1e-12, atol=0)
    for name, s in BM.tensors(pol.layout).items():
        top = np.abs(want[s]).max()
        assert top > 0, name
        assert np.abs(got["grad"][s] - want[s]).max() <= 1e-9 * top, (name, np.abs(got["grad"][s] - want[s]).max() / top)
        assert np.all(got["mag"][s] >= np.abs(got["grad"][s]) * (1 - 1e-12))


def test_the_float32_model_is_close_to_the_float64_model_and_no_closer_than_float32():
    pol, ro = _tiny(BC.CONFIGS["lopsided"], seed=4)
    b = RecurrentPPO(pol).batch(ro)
    args = _model_args(pol, ro, b["x"].numpy().astype(np.float32))
    g64, g32 = BM.policy_grad(*args, penalty=0.7), BM.policy_grad(*args, penalty=0.7, dtype=np.float32)
    dev = BC.deviation(g32["grad"], g64["grad"], BM.tensors(pol.layout))
    assert all(1e-9 < v < 1e-5 for k, v in dev.items() if k != "logstd"), dev
    assert g32["mean"].dtype == np.float32


# ---- known answers of the model -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_resets_everywhere_leave_the_h_rows_exactly_zero(dtype):
    pol, ro = _tiny(TWO_DENSE, seed=5)
    x = RecurrentPPO(pol).batch(ro)["x"].numpy()
    args = list(_model_args(pol, ro, x))
    args[1] = np.ones_like(args[1])
    g = BM.policy_grad(*args, penalty=0.7, dtype=dtype)["grad"]
    for s in BM.h_rows(pol.layout):
        assert np.all(g[s] == 0.0)
    for name, s in BM.tensors(pol.layout).items():
        assert np.abs(g[s]).max() > 0, name                                      # the x rows, the biases and the rest are not
    free = BM.policy_grad(*_model_args(pol, ro, x), penalty=0.7, dtype=dtype)["grad"]
    assert all(np.abs(free[s]).max() > 0 for s in BM.h_rows(pol.layout))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_an_all_zero_mask_leaves_every_entry_exactly_zero(dtype):
    pol, ro = _tiny(TWO_DENSE, seed=6)
    x = RecurrentPPO(pol).batch(ro)["x"].numpy()
    args = list(_model_args(pol, ro, x))
    args[9] = np.zeros_like(args[9])
    out = BM.policy_grad(*args, penalty=0.7, dtype=dtype)
    assert np.all(out["grad"] == 0.0) and out["loss"] == 0.0 and np.all(out["kl"] == 0.0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_reset_makes_the_gradient_independent_of_the_observations_before_it(dtype):
    """Robot 2 is reset at tick 3 and its ticks before that are masked (they carry no loss of their own): what it saw before
    the reset reaches nothing.  Without the reset the same change moves the gradient."""
    pol, ro = _tiny(TWO_DENSE, seed=7)
    ro.mask[:3, 2] = 0
    x = RecurrentPPO(pol).batch(ro)["x"].numpy()
    moved = x.copy()
    moved[:3, 2] = np.random.default_rng(1).normal(size=moved[:3, 2].shape)
    a, b = (BM.policy_grad(*_model_args(pol, ro, v), penalty=0.7, dtype=dtype)["grad"] for v in (x, moved))
    assert a.tobytes() == b.tobytes()
    ro.reset[3, 2] = 0
    a, b = (BM.policy_grad(*_model_args(pol, ro, v), penalty=0.7, dtype=dtype)["grad"] for v in (x, moved))
    assert not np.array_equal(a, b)


# ---- the cases of the GPU tests -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,T,B,cutoff", [k + (True,) for k in BC.GRADIENT_CASES] + [k + (False,) for k in BC.NO_CUTOFF_CASES])
def test_every_gpu_case_builds_from_the_model_within_its_caps(name, T, B, cutoff):
    c = BC.case(name, T, B, cutoff=cutoff)
    print(f"{name} T={T} B={B} cutoff={cutoff}: redrawn {c['redrawn']:.3f}; one ulp of the means costs {c['ulp_cost']:.3e}; float32-numpy vs float64 {c['p_dev32']} loss {c['p_loss_dev32']:.3e}; "
          f"bounds {c['p_tol']} loss {c['p_loss_tol']:.3e}")
    assert c["redrawn"] <= BC.REDRAW_CAP
    assert c["ulp_cost"] <= BC.ULP_CAP
    assert c["model_kw"]["kl_cutoff_coef"] == (1000.0 if cutoff else 0.0) == c["ppo_kw"]["kl_cutoff_coef"]
    assert max(c["p_tol"].values()) <= BC.TOL_CAP and c["p_loss_tol"] <= BC.TOL_CAP
    p64 = c["p64"]
    assert all(np.abs(p64["grad"][s]).max() > 0 for s in BM.tensors(c["lay"]).values())
    assert (c["reset"][0] != 0).any() and (c["reset"][T - 1] != 0).any() and np.abs(c["h0"]).max() > 0
    if B >= 5:
        assert p64["over"].any() and not p64["over"].all() and p64["kl"][B - 1] == 0.0
        assert (c["reset"] == 0).all(axis=0).any()                               # and a robot that is never reset
    assert len([s for s in BC.SHAPES if name != "limits" or s[0] * s[1] <= 185]) >= 4


# ---- DeviceRecurrentPPO without a device ------------------------------------------------------------------------------------------

def test_a_host_only_policy_gives_host_only_handles_that_check_and_then_report_no_device():
    pol = RecurrentGaussianPolicy(4, device="cpu", **BC.CONFIGS["lopsided"])
    ro = RecurrentRolloutBuffer(3, 4, 6, 3, 5)
    upd = DeviceRecurrentPPO(pol, epochs_policy=2, epochs_value=2, kl_init_penalty=0.7)
    assert upd.T is None and float(upd.penalty) == 0.7 and int(upd.step) == 0
    with pytest.raises(ValueError):
        upd.adam("policy", None)
    for call in (upd.update, upd.prepare, upd.policy_grad, upd.value_grad, upd.kl):
        with pytest.raises((bptt_abi.RgBpttError, ppo_abi.RgPpoError)) as e:
            call(ro)
        assert e.value.status == -3
    assert upd.T == 3 and upd.steps().tolist() == [0, 0]
    assert upd.opt_state.numel() * 8 == upd._handle.opt_state_bytes and upd.moments.numel() == 2 * pol.layout["policy_count"]
    assert upd.value_moments.numel() == 2 * pol.layout["value_count"]
    for which in ("policy", "value"):
        with pytest.raises((bptt_abi.RgBpttError, ppo_abi.RgPpoError)) as e:
            upd.adam(which, None)
        assert e.value.status == -3
    with pytest.raises(ValueError):
        upd.adam("both", None)
    # every tensor is checked before its pointer crosses the ABI
    with pytest.raises(ValueError, match="rollout.T"):
        upd.policy_grad(RecurrentRolloutBuffer(4, 4, 6, 3, 5))
    with pytest.raises(ValueError, match="rollout.batch"):
        upd.policy_grad(RecurrentRolloutBuffer(3, 5, 6, 3, 5))
    for name, bad in (("reset", ro.reset.to(torch.int64)), ("h0", ro.h0[:, :4]), ("mask", ro.mask.to(torch.float32)), ("obs", ro.obs.permute(0, 2, 1)),
                      ("mean", ro.mean.double()), ("adv", ro.adv[:2])):
        good = getattr(ro, name)
        setattr(ro, name, bad)
        with pytest.raises(ValueError, match="rollout." + name):
            upd.update(ro)
        setattr(ro, name, good)
    with pytest.raises(ValueError, match="out"):
        upd.kl(ro, out=torch.zeros(4))
    with pytest.raises(ValueError, match="out"):
        upd.policy_grad(ro, out=torch.zeros(3))
    state = upd.state_dict()
    upd.load_state_dict(state)
    with pytest.raises(ValueError):
        DeviceRecurrentPPO(pol, epochs_policy=3).load_state_dict(state)
    with pytest.raises(ValueError):
        DeviceRecurrentPPO(pol, conv_logpdf="neither")
    upd.close(), pol.close()


# ---- resources of rg_bptt.hip ------------------------------------------------------------------------------------------

KERNELS = {f"rg_bptt_{k}_kernel" for k in ("describe", "forward", "sample_kl", "robot_kl", "head", "loss_finish", "transpose", "delta", "weight",
                                           "grad_finish", "adam", "adam_count", "penalty")}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_bptt.hip")


def test_every_bptt_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_bptt_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


# The file's header comment, in floats of the header limits.  forward: two x buffers, h, r*h and u; delta: two dense delta
# buffers, delta_c, delta_ru (2H) and delta_mean; each with its copy of the descriptor (at most 768 bytes).  weight: a chunk's
# inputs of a row tile.  The sums: four float64.
W_, H_, A_, T_ = rnn_abi.MAX_WIDTH, rnn_abi.MAX_UNITS, rnn_abi.MAX_ACT, rnn_abi.TILE
LDS_BUDGET = {"rg_bptt_forward_kernel": (2 * W_ + 3 * H_) * T_ * 4 + 768, "rg_bptt_delta_kernel": (2 * W_ + 3 * H_ + A_) * T_ * 4 + 768,
              "rg_bptt_weight_kernel": bptt_abi.CHUNK * bptt_abi.ROWS * 4, "rg_bptt_head_kernel": 32, "rg_bptt_loss_finish_kernel": 32,
              "rg_bptt_penalty_kernel": 32}


def test_lds_is_within_the_budget(remarks):
    assert LDS_BUDGET["rg_bptt_forward_kernel"] == 29440 and LDS_BUDGET["rg_bptt_delta_kernel"] == 29568 and LDS_BUDGET["rg_bptt_weight_kernel"] == 1024
    for name in KERNELS:
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= LDS_BUDGET.get(name, 0) <= 65536, (name, remarks[name])


# What the device-only compile reports today (upper bounds; occupancy a lower bound).
REGISTERS = {
    "rg_bptt_forward_kernel": dict(vgprs=128, agprs=0, occupancy=4), "rg_bptt_delta_kernel": dict(vgprs=110, agprs=0, occupancy=4),
    "rg_bptt_weight_kernel": dict(vgprs=82, agprs=0, occupancy=5), "rg_bptt_head_kernel": dict(vgprs=122, agprs=0, occupancy=4),
    "rg_bptt_sample_kl_kernel": dict(vgprs=24, agprs=0, occupancy=8), "rg_bptt_loss_finish_kernel": dict(vgprs=33, agprs=0, occupancy=8),
    "rg_bptt_adam_kernel": dict(vgprs=33, agprs=0, occupancy=8), "rg_bptt_robot_kl_kernel": dict(vgprs=14, agprs=0, occupancy=8),
    "rg_bptt_grad_finish_kernel": dict(vgprs=8, agprs=0, occupancy=8), "rg_bptt_transpose_kernel": dict(vgprs=9, agprs=0, occupancy=8),
    "rg_bptt_penalty_kernel": dict(vgprs=12, agprs=0, occupancy=8), "rg_bptt_describe_kernel": dict(vgprs=10, agprs=0, occupancy=8),
    "rg_bptt_adam_count_kernel": dict(vgprs=4, agprs=0, occupancy=8),
}


def test_register_use_is_pinned(remarks):
    assert set(REGISTERS) == KERNELS
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    own = open(os.path.join(SRC, "rg_bptt.hip")).read()
    code = re.sub(r"//.*", "", own)
    assert "asm" not in code and "atomic" not in own.lower()
    assert code.index("#pragma clang fp contract(off)") < code.index("__global__")
    assert code.index("#pragma clang fp contract(off)") < code.index("__device__")
    assert code.index("#pragma clang fp contract(off)") < code.index('#include "rg_agent_dev.inc"') < code.index('#include "rg_gru_dev.inc"')
    assert code.index('#include "rg_gru_dev.inc"') < code.index('#include "rg_ppo_dev.inc"')
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_policy.h", "../../include/rg_ppo.h", "../../include/rg_rnn.h",
                                                      "../../include/rg_bptt.h", "rg_host.h", "rg_agent_dev.inc", "rg_gru_dev.inc", "rg_ppo_dev.inc"]
    assert not re.search(r"\b(chain8|sigmoidf)\s*\([^;{]*\)\s*\{", code)         # the tick's device code is rg_gru_dev.inc's alone
    shared = [open(os.path.join(SRC, name)).read() for name in ("rg_agent_dev.inc", "rg_gru_dev.inc", "rg_ppo_dev.inc", "rg_stream_dev.inc")]
    for text in shared:
        assert "asm" not in re.sub(r"//.*", "", text) and "atomic" not in text.lower()
        assert "__global__" not in text
    assert [re.findall(r'#include "([^"]+)"', text) for text in shared] == [["rg_stream_dev.inc"], [], [], []]     # the one stream, under the agents' noise
    # the head's and Adam's arithmetic is the shared files' alone: no update writes an exp or a pow of its own
    for name in ("rg_ppo.hip", "rg_bptt.hip", "rg_ddpg.hip"):
        text = re.sub(r"//.*", "", open(os.path.join(SRC, name)).read())
        assert "pow(" not in text, name
        assert name == "rg_ddpg.hip" or "exp(" not in text, name
    assert "pow(" in re.sub(r"//.*", "", shared[0]) and "exp(" in re.sub(r"//.*", "", shared[2])
    assert len(re.findall(r"__global__", code)) == len(KERNELS)
    import bench
    assert not any("rg_bptt" in rel for rel in bench.compiled_sources())         # the MPC hash behind profiles/ does not follow it
    for other in sorted(os.listdir(SRC)):                                        # included from nowhere
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_bptt.hip":
            assert "rg_bptt" not in open(os.path.join(SRC, other)).read(), other
    kernel_checks.assert_built_into_both("rg_bptt.hip", header="rg_bptt.h")
