"""The PPO update on the device (include/rg_ppo.h) without a GPU: librg_mpc.so exports every rg_ppo_* entry, the ctypes binding
matches the header, create validates both configurations field by field (naming the field) before it looks for a device, a
host-only handle checks every pointer and then returns NO_DEVICE; the numpy model of the update (tests/ppo_update_model.py)
against torch autograd of PPO's losses in float64, its Adam against torch.optim.Adam, the penalty rule; the kernels of
rg_ppo.hip cross-compile for gfx950 without scratch or spills, within their LDS and register budgets; and DevicePPO rejects a
rollout it must not follow before the library sees a pointer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ppo import PPO, BatchedGaussianPolicy, DevicePPO, RolloutBuffer
from robot_gym_amd.core import policy_abi, ppo_abi
from tests import kernel_checks
from tests import policy_model as PM
from tests import ppo_update_model as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_ppo.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI and configuration ------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = ppo_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_ppo_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 17
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(ppo_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None, name


def test_struct_layouts_and_constants_match_the_header():
    lib = ppo_abi.load_library()
    structs = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", _header()))
    sizes = {"int32_t": 4, "double": 8}
    want = [(n, sizes[t]) for t, n in re.findall(r"\b(int32_t|double)\s+(\w+);", structs["rg_ppo_config"])]
    assert [n for n, _ in want] == [n for n, _ in ppo_abi.CConfig._fields_]
    for (n, size), (_, tg) in zip(want, ppo_abi.CConfig._fields_):
        assert size == C.sizeof(tg), n
    assert sum(s for _, s in want) == C.sizeof(ppo_abi.CConfig) == lib.rg_ppo_config_size() == 80   # no padding
    ptrs = re.findall(r"const (?:float|int32_t) \*(\w+);", structs["rg_ppo_rollout"])
    assert ptrs == [n for n, _ in ppo_abi.CRollout._fields_] == ["obs", "action", "mean", "logstd", "adv", "ret", "mask"]
    assert lib.rg_ppo_rollout_size() == C.sizeof(ppo_abi.CRollout) == 8 * len(ptrs)
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_PPO_\w+) (\d+)", _header())}
    assert lib.rg_ppo_abi_version() == defs["RG_PPO_ABI_VERSION"] == ppo_abi.ABI_VERSION == 1
    assert lib.rg_ppo_tile() == defs["RG_PPO_TILE"] == ppo_abi.TILE
    assert (defs["RG_PPO_MAX_GROUPS"], defs["RG_PPO_STATS"], defs["RG_PPO_OPT_HEADER_BYTES"]) == (ppo_abi.MAX_GROUPS, ppo_abi.STATS, ppo_abi.OPT_HEADER_BYTES)
    assert len(ppo_abi.STAT_NAMES) == ppo_abi.STATS
    assert (defs["RG_PPO_LOGPDF_EXACT"], defs["RG_PPO_LOGPDF_REFERENCE"]) == (ppo_abi.LOGPDF["exact"], ppo_abi.LOGPDF["reference"])
    assert (defs["RG_PPO_POLICY"], defs["RG_PPO_VALUE"]) == (ppo_abi.POLICY, ppo_abi.VALUE)


def test_defaults_are_those_of_the_torch_update():
    pol = BatchedGaussianPolicy(1, device="cpu", obs_dim=2, act_dim=1, policy_layers=(), value_layers=())
    ppo = PPO(pol)
    D = ppo_abi.DEFAULTS
    assert (D["epochs_policy"], D["epochs_value"], D["kl_target"], D["kl_cutoff_factor"], D["kl_cutoff_coef"], D["conv_logpdf"]) == \
        (ppo.epochs_policy, ppo.epochs_value, ppo.kl_target, ppo.kl_cutoff_factor, ppo.kl_cutoff_coef, ppo.conv_logpdf)
    g = ppo.policy_opt.param_groups[0]
    assert (D["policy_lr"], D["beta1"], D["beta2"], D["adam_eps"]) == (g["lr"], g["betas"][0], g["betas"][1], g["eps"])
    assert D["value_lr"] == ppo.value_opt.param_groups[0]["lr"]
    dev = DevicePPO(pol, 3)
    assert float(dev.penalty) == ppo.penalty == 1.0 and dev.fields == ppo_abi.ppo_fields()
    with pytest.raises(TypeError):
        ppo_abi.make_cconfig(gamma=0.9)
    with pytest.raises(ValueError):
        ppo_abi.make_cconfig(conv_logpdf="tf")


@pytest.mark.parametrize("field,value,text", [
    ("epochs_policy", -1, "ppo_cfg.epochs_policy"), ("epochs_value", (1 << 20) + 1, "ppo_cfg.epochs_value"), ("conv_logpdf", 2, "ppo_cfg.conv_logpdf"),
    ("conv_logpdf", -1, "ppo_cfg.conv_logpdf"), ("policy_lr", -1e-4, "ppo_cfg.policy_lr"), ("policy_lr", NAN, "ppo_cfg.policy_lr"),
    ("value_lr", INF, "ppo_cfg.value_lr"), ("beta1", 1.0, "ppo_cfg.beta1"), ("beta1", -0.1, "ppo_cfg.beta1"), ("beta2", 1.5, "ppo_cfg.beta2"),
    ("beta2", NAN, "ppo_cfg.beta2"), ("adam_eps", 0.0, "ppo_cfg.adam_eps"), ("adam_eps", -1e-8, "ppo_cfg.adam_eps"), ("kl_target", 0.0, "ppo_cfg.kl_target"),
    ("kl_target", INF, "ppo_cfg.kl_target"), ("kl_cutoff_factor", -1.0, "ppo_cfg.kl_cutoff_factor"), ("kl_cutoff_coef", NAN, "ppo_cfg.kl_cutoff_coef"),
    ("abi_version", 2, "ppo_cfg.abi_version"),
])
def test_create_rejects_a_bad_ppo_config_naming_the_field(field, value, text):
    cc = ppo_abi.make_cconfig()
    setattr(cc, field, value)
    for device in (0, ppo_abi.DEVICE_NONE):
        rc, msg = ppo_abi.create_status(None, cc, device=device)
        assert rc == -1 and text in msg, (rc, msg)


@pytest.mark.parametrize("field,value,text", [
    ("obs_dim", 65, "policy_cfg.obs_dim"), ("act_dim", 0, "policy_cfg.act_dim"), ("n_policy_layers", 4, "policy_cfg.n_policy_layers"),
    ("n_value_layers", -1, "policy_cfg.n_value_layers"), ("obs_clip", -1.0, "policy_cfg.obs_clip"), ("abi_version", 2, "policy_cfg.abi_version"),
    ("reserved0", 1, "policy_cfg.reserved0"),
])
def test_create_rejects_a_bad_policy_config_naming_the_field(field, value, text):
    pc = policy_abi.make_cconfig()
    setattr(pc, field, value)
    for device in (0, ppo_abi.DEVICE_NONE):
        rc, msg = ppo_abi.create_status(pc, device=device)
        assert rc == -1 and text in msg, (rc, msg)
    pc = policy_abi.make_cconfig()
    pc.policy_layers[1], pc.value_layers[2] = 257, 0
    rc, msg = ppo_abi.create_status(pc)
    assert rc == -1 and "policy_cfg.policy_layers[1]" in msg
    pc = policy_abi.make_cconfig()
    pc.value_layers[2] = 3
    rc, msg = ppo_abi.create_status(pc)
    assert rc == -1 and "policy_cfg.value_layers[2]" in msg


def test_create_checks_the_shape_and_null_arguments():
    for T, B, text in ((0, 4, "T:"), ((1 << 20) + 1, 1, "T:"), (4, 0, "B:"), (4, (1 << 24) + 1, "B:"), (1 << 10, 1 << 21, "T * B")):
        rc, msg = ppo_abi.create_status(T=T, B=B)
        assert rc == -1 and text in msg, (T, B, msg)
    lib = ppo_abi.load_library()
    pc, cc, h = policy_abi.make_cconfig(), ppo_abi.make_cconfig(), C.c_void_p()
    assert lib.rg_ppo_create(None, C.byref(cc), 4, 4, -1, C.byref(h)) == -1
    assert lib.rg_ppo_create(C.byref(pc), None, 4, 4, -1, C.byref(h)) == -1
    assert lib.rg_ppo_create(C.byref(pc), C.byref(cc), 4, 4, -1, None) == -1
    for settings in (dict(), dict(epochs_policy=0, epochs_value=0, policy_lr=0.0, kl_cutoff_factor=0.0, kl_cutoff_coef=0.0, conv_logpdf="reference")):
        rc, msg = ppo_abi.create_status(None, ppo_abi.make_cconfig(**settings))   # valid, host-only: a handle is made
        assert rc == 0, msg
    assert lib.rg_ppo_workspace_bytes(None) == -1 and lib.rg_ppo_opt_state_bytes(None) == -1 and lib.rg_ppo_groups(None) == -1


def test_sizes_of_a_handle_follow_the_header():
    for settings, T, B in ((dict(), 32, 64), (dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2)), 3, 5), (dict(), 5, 1037)):
        h = ppo_abi.PpoHandle(T, B, ppo_abi.DEVICE_NONE, policy_settings=settings)
        lay = policy_abi.param_layout(**settings)
        want = ppo_abi.OPT_HEADER_BYTES + 4 * 2 * (lay["policy_count"] + lay["value_count"])
        assert h.opt_state_bytes == (want + 7) // 8 * 8
        tiles = -(-T * B // ppo_abi.TILE)
        assert h.groups == min(tiles, ppo_abi.MAX_GROUPS)
        slabs = 4 * h.groups * max(lay["policy_count"], lay["value_count"])
        assert h.workspace_bytes % 8 == 0 and slabs + 8 * T * B <= h.workspace_bytes <= slabs + 8 * T * B + (1 << 20)
        assert 0 < h.scalars_offset < h.workspace_bytes and h.scalars_offset % 8 == 0
        h.close()


def test_host_only_handle_checks_every_pointer_then_reports_no_device():
    h = ppo_abi.PpoHandle(3, 4, ppo_abi.DEVICE_NONE)
    lib = ppo_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p = dummy.ctypes.data
    last = lambda: lib.rg_ppo_last_error(h._h).decode()
    slots = ("obs", "action", "mean", "logstd", "adv", "ret", "mask")
    full = lambda **kw: ppo_abi.make_crollout(**{**{s: p for s in slots}, **kw})
    calls = {
        "prepare": (lib.rg_ppo_prepare, ("adv", "mask"), ["workspace"]),
        "policy_grad": (lib.rg_ppo_policy_grad, ("obs", "action", "mean", "logstd", "adv", "mask"),
                        ["norm_state", "policy_params", "opt_state", "workspace", "grad_out", "loss_out"]),
        "value_grad": (lib.rg_ppo_value_grad, ("obs", "ret", "mask"), ["norm_state", "value_params", "workspace", "grad_out", "loss_out"]),
        "kl": (lib.rg_ppo_kl, ("obs", "mean", "logstd", "mask"), ["norm_state", "policy_params", "workspace", "kl_out"]),
        "update": (lib.rg_ppo_update, slots, ["norm_state", "policy_params", "value_params", "opt_state", "workspace", "stats"]),
    }
    for call, (fn, needs, args) in calls.items():
        good = [p] * len(args)
        assert fn(h._h, C.byref(full()), *good, None) == -3 and "host-only" in last(), call
        assert fn(h._h, C.byref(full(**{s: None for s in slots if s not in needs})), *good, None) == -3, call   # only what it reads
        assert fn(h._h, None, *good, None) == -1 and f"{call}: null rollout" in last()
        for s in needs:
            assert fn(h._h, C.byref(full(**{s: None})), *good, None) == -1 and f"{call}: null rollout.{s}" in last(), (call, s, last())
        for k, name in enumerate(args):
            a = list(good)
            a[k] = None
            assert fn(h._h, C.byref(full()), *a, None) == -1 and f"{call}: null {name}" in last(), (call, name, last())
        assert fn(None, C.byref(full()), *good, None) == -1 and "null handle" in lib.rg_ppo_last_error(None).decode()
    for which in (ppo_abi.POLICY, ppo_abi.VALUE):
        assert lib.rg_ppo_adam(h._h, which, p, p, p, None) == -3
    assert lib.rg_ppo_adam(h._h, 2, p, p, p, None) == -1 and "which" in last()
    for k, name in enumerate(("params", "grad", "opt_state")):
        a = [p, p, p]
        a[k] = None
        assert lib.rg_ppo_adam(h._h, 0, *a, None) == -1 and f"adam: null {name}" in last()
    with pytest.raises(ppo_abi.RgPpoError) as e:
        h.prepare(full(), p)
    assert e.value.status == -3
    h.close()


# ---- the model against autograd ---------------------------------------------------------------------------------------

CFG = dict(obs_dim=6, act_dim=3, policy_layers=(5,), value_layers=(7, 3, 2))
DEAD = 2          # the hidden neuron of the policy (and of the value network's first layer) whose pre-activation is exactly 0


def _tiny(seed=0, T=4, B=6):
    """A host-only float64 policy with random biases, logstd and normaliser state, one hidden neuron per network whose weights
    and bias are 0 (its pre-activation is exactly 0 for every sample), and a synthetic rollout: zeros in the mask, robot 3
    masked throughout, robots 0 and 1 far from the behaviour policy (their KL is above the cutoff), the others at it."""
    rng = np.random.default_rng(seed)
    pol = BatchedGaussianPolicy(B, device="cpu", dtype=torch.float64, seed=seed, **CFG)
    with torch.no_grad():
        for _, b in pol.policy_layers + pol.value_layers:
            b.copy_(torch.as_tensor(rng.normal(0, 0.3, size=b.shape)))
        for layers in (pol.policy_layers, pol.value_layers):
            layers[0][0][:, DEAD] = 0.0
            layers[0][1][DEAD] = 0.0
        pol.logstd.copy_(torch.as_tensor(rng.normal(-1, 0.2, size=3)))
    on, rn = PM.Normalizer(6, True, 5.0), PM.Normalizer(1, False, 10.0)
    on.update(rng.normal(0.2, 1.5, size=(30, 6)))
    rn.update(rng.normal(0.0, 3.0, size=(30, 1)))
    pol.norm_state.copy_(torch.as_tensor(PM.norm_state_of(on, rn)))
    ro = RolloutBuffer(T, B, 6, 3, dtype=torch.float64)
    ro.obs.copy_(torch.as_tensor(rng.normal(0.2, 3.0, size=(T, 6, B))))     # some components reach the clip
    with torch.no_grad():
        mean, _ = pol.evaluate(pol.normalize_obs(ro.obs.permute(0, 2, 1)))
    ro.logstd.copy_(pol.logstd.detach() + torch.as_tensor(rng.normal(0, 0.01, size=3)))
    off = 0.01 * rng.normal(size=(T, B, 3))
    off[:, :2] += 0.12                                                       # sigma ~ 0.37: KL ~ 0.5 * 3 * (0.12 / 0.37)^2 ~ 0.16 > 0.02
    ro.mean.copy_(mean + torch.as_tensor(off))
    ro.action.copy_(ro.mean + torch.exp(ro.logstd) * torch.as_tensor(rng.normal(size=(T, B, 3))))
    ro.adv.copy_(torch.as_tensor(rng.normal(0.5, 2.0, size=(T, B))))
    ro.ret.copy_(torch.as_tensor(rng.normal(0.0, 2.0, size=(T, B))))
    ro.mask[2, 1] = 0
    ro.mask[1, 4] = 0
    ro.mask[:, 3] = 0
    return pol, ro


def _model_inputs(pol, ro):
    x = pol.normalize_obs(ro.obs.permute(0, 2, 1)).reshape(ro.T * ro.batch, -1).numpy()
    return dict(x=x, action=ro.action.numpy(), mean0=ro.mean.numpy(), logstd0=ro.logstd.numpy(), adv=ro.adv.numpy(), mask=ro.mask.numpy(),
                T=ro.T, B=ro.batch)


@pytest.mark.parametrize("conv", ["exact", "reference"])
def test_policy_gradient_of_the_model_equals_autograd(conv):
    pol, ro = _tiny(seed=1)
    ppo = PPO(pol, kl_init_penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2, kl_cutoff_coef=1000, conv_logpdf=conv)
    b = ppo.batch(ro)
    loss = ppo.policy_loss(b)
    loss.backward()
    want = pol.policy_params.grad.numpy()
    got = UM.policy_grad(policy_params=pol.policy_params.detach().numpy(), lay=pol.layout, penalty=0.7, kl_target=1e-2, kl_cutoff_factor=2.0,
                         kl_cutoff_coef=1000.0, conv=conv, **_model_inputs(pol, ro))
    assert got["over"].any() and not got["over"].all() and got["over"][:2].all()       # the cutoff is on for some robots, off for others
    assert got["kl"][3] == 0.0 and (ro.mask.numpy() == 0).sum() > ro.T                 # a robot masked throughout, and single ticks
    assert math.isclose(got["loss"], float(loss.detach()), rel_tol=1e-12)
    assert np.allclose(got["kl"], ppo.kl(b).detach().numpy(), rtol=1e-10, atol=0)
    scale = np.abs(want).max()
    assert np.allclose(got["grad"], want, rtol=1e-10, atol=1e-10 * scale * 1e-3), float(np.abs(got["grad"] - want).max())
    names = UM.tensors(pol.layout["policy"], pol.layout["logstd_offset"], pol.layout["policy_count"])
    assert np.abs(want[names["logstd"]]).min() > 0 and np.abs(want[names["W1"]]).max() > 0
    # the neuron at exactly 0: relu'(0) = 0 in both, so nothing reaches its weights, its bias or what it feeds
    W0 = want[names["W0"]].reshape(6, 5)
    assert np.all(W0[:, DEAD] == 0) and want[names["b0"]][DEAD] == 0 and np.all(want[names["W1"]].reshape(5, 3)[DEAD] == 0)
    g0 = got["grad"][names["W0"]].reshape(6, 5)
    assert np.all(g0[:, DEAD] == 0) and got["grad"][names["b0"]][DEAD] == 0 and np.abs(g0).max() > 0


def test_value_gradient_of_the_model_equals_autograd():
    pol, ro = _tiny(seed=2)
    ppo = PPO(pol)
    loss = ppo.value_loss(ppo.batch(ro))
    loss.backward()
    want = pol.value_params.grad.numpy()
    m = _model_inputs(pol, ro)
    got = UM.value_grad(m["x"], pol.value_params.detach().numpy(), pol.layout, ro.ret.numpy(), m["mask"], ro.T, ro.batch)
    assert math.isclose(got["loss"], float(loss.detach()), rel_tol=1e-12)
    assert np.allclose(got["grad"], want, rtol=1e-10, atol=1e-13 * np.abs(want).max()), float(np.abs(got["grad"] - want).max())
    names = UM.tensors(pol.layout["value"])
    assert np.all(want[names["W0"]].reshape(6, 7)[:, DEAD] == 0) and np.all(got["grad"][names["W0"]].reshape(6, 7)[:, DEAD] == 0)
    assert all(np.abs(want[s]).max() > 0 for s in names.values())


def test_advantage_statistics_of_the_model_are_those_of_the_torch_batch():
    pol, ro = _tiny(seed=3)
    n, m, sd = UM.adv_stats(ro.adv.numpy(), ro.mask.numpy())
    b = PPO(pol).batch(ro)
    assert n == int((ro.mask != 0).sum())
    assert np.allclose(b["adv"].numpy(), (ro.adv.numpy() - m) / sd, rtol=1e-13, atol=1e-15)
    assert UM.adv_stats(ro.adv.numpy(), np.zeros_like(ro.mask.numpy())) == (1, 0.0, 1e-8)          # n = 0: the count clamps to 1


def test_float32_model_is_close_to_float64():
    pol, ro = _tiny(seed=4)
    m = _model_inputs(pol, ro)
    kw = dict(policy_params=pol.policy_params.detach().numpy(), lay=pol.layout, penalty=1.0, **m)
    g64, g32 = UM.policy_grad(**kw), UM.policy_grad(dtype=np.float32, **kw)
    assert 0 < np.abs(g32["grad"] - g64["grad"]).max() <= 1e-4 * np.abs(g64["grad"]).max()


# ---- Adam and the penalty -----------------------------------------------------------------------------------------------

def test_adam_of_the_model_equals_torch_over_five_steps():
    rng = np.random.default_rng(5)
    p0 = rng.normal(size=40)
    grads = rng.normal(size=(5, 40)) * np.logspace(-6, 1, 40)
    grads[:, 3] = 0.0
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t], lr=3e-4)
    p, m, v, step = p0.copy(), np.zeros(40), np.zeros(40), 0
    for g in grads:
        t.grad = torch.as_tensor(g.copy())
        opt.step()
        p, m, v, step = UM.adam_step(p, g, m, v, step, 3e-4)
        assert np.allclose(p, t.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert step == 5 and p[3] == p0[3]
    state = opt.state[t]
    assert np.allclose(m, state["exp_avg"].numpy(), rtol=1e-12, atol=1e-300) and np.allclose(v, state["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("kl,factor", [(0.02, 1.5), (0.0131, 1.5), (0.013, 1.0), (0.01, 1.0), (0.007, 1.0), (0.0069, 1 / 1.5), (0.0, 1 / 1.5)])
def test_penalty_rule_of_the_model_is_the_torch_rule(kl, factor):
    pol = BatchedGaussianPolicy(1, device="cpu", obs_dim=2, act_dim=1, policy_layers=(), value_layers=())
    ppo = PPO(pol, kl_target=1e-2, kl_init_penalty=2.0)
    assert UM.move_penalty(2.0, kl, 1e-2) == ppo.adjust_penalty(kl) == 2.0 * factor


# ---- resources of rg_ppo.hip ------------------------------------------------------------------------------------------

KERNELS = {"rg_ppo_prepare_first_kernel", "rg_ppo_prepare_second_kernel", "rg_ppo_prepare_finish_kernel", "rg_ppo_describe_kernel",
           "rg_ppo_transpose_kernel", "rg_ppo_policy_forward_kernel", "rg_ppo_policy_backward_kernel", "rg_ppo_value_backward_kernel",
           "rg_ppo_robot_kl_kernel", "rg_ppo_grad_finish_kernel", "rg_ppo_loss_finish_kernel", "rg_ppo_adam_kernel", "rg_ppo_adam_count_kernel",
           "rg_ppo_penalty_kernel"}
SWEEPS = ("rg_ppo_policy_forward_kernel", "rg_ppo_policy_backward_kernel", "rg_ppo_value_backward_kernel")


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_ppo.hip")


def test_every_ppo_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_ppo_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


def _sweep_lds(settings):
    """Bytes of dynamic LDS of a sweep's tile per network: (obs_dim + sum(out) + 2 max(out)) * RG_PPO_TILE floats."""
    lay = policy_abi.param_layout(**settings)
    out = {}
    for net in ("policy", "value"):
        widths = [o for _, o, _, _ in lay[net]]
        out[net] = 4 * ppo_abi.TILE * (lay[net][0][0] + sum(widths) + 2 * max(widths))
    return out


def test_lds_is_within_the_budget(remarks):
    # static LDS: one float64 per wave of a workgroup's sum in the reducing kernels; the sweeps' tiles are dynamic
    for name in KERNELS:
        static = 4 * 8 if name in ("rg_ppo_prepare_first_kernel", "rg_ppo_prepare_second_kernel", "rg_ppo_prepare_finish_kernel",
                                   "rg_ppo_loss_finish_kernel", "rg_ppo_penalty_kernel") else 0
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= static, (name, remarks[name])
    default = _sweep_lds({})
    assert default == dict(policy=4 * 16 * (16 + 302 + 400), value=4 * 16 * (16 + 301 + 400)) and max(default.values()) <= 48 * 1024
    limits = _sweep_lds(dict(obs_dim=64, act_dim=4, policy_layers=(256, 256, 256), value_layers=(256, 256, 256)))
    assert max(limits.values()) == 4 * 16 * (64 + 768 + 4 + 512) <= 160 * 1024     # the widest configuration fits a compute unit's LDS


# What the device-only compile reports today (upper bounds; occupancy a lower bound).  A sweep's workgroup is four waves, one
# per SIMD: at three waves per SIMD three workgroups share a compute unit where the LDS of their tiles allows it.
REGISTERS = {"rg_ppo_policy_forward_kernel": dict(vgprs=94, agprs=0, occupancy=5), "rg_ppo_policy_backward_kernel": dict(vgprs=156, agprs=0, occupancy=3),
             "rg_ppo_value_backward_kernel": dict(vgprs=124, agprs=0, occupancy=4), "rg_ppo_adam_kernel": dict(vgprs=33, agprs=0, occupancy=8),
             "rg_ppo_loss_finish_kernel": dict(vgprs=29, agprs=0, occupancy=8), "rg_ppo_grad_finish_kernel": dict(vgprs=8, agprs=0, occupancy=8),
             "rg_ppo_prepare_first_kernel": dict(vgprs=18, agprs=0, occupancy=8), "rg_ppo_prepare_second_kernel": dict(vgprs=28, agprs=0, occupancy=8),
             "rg_ppo_prepare_finish_kernel": dict(vgprs=32, agprs=0, occupancy=8), "rg_ppo_transpose_kernel": dict(vgprs=9, agprs=0, occupancy=8),
             "rg_ppo_robot_kl_kernel": dict(vgprs=14, agprs=0, occupancy=8), "rg_ppo_penalty_kernel": dict(vgprs=12, agprs=0, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    own = open(os.path.join(SRC, "rg_ppo.hip")).read()
    shared = [open(os.path.join(SRC, name)).read() for name in ("rg_host.h", "rg_agent_dev.inc", "rg_ppo_dev.inc", "rg_stream_dev.inc")]   # the agents' common code
    src = "\n".join([own] + shared)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    assert "hipMalloc" not in src and "hipMemcpy" not in src and "Synchronize" not in src and "hipFree" not in src
    own_code = re.sub(r"//.*", "", own)
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index("__global__")
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index('#include "rg_agent_dev.inc"')
    assert own_code.index('#include "rg_agent_dev.inc"') < own_code.index('#include "rg_ppo_dev.inc"')
    assert re.findall(r'#include "([^"]+)"', own_code) == ["../../include/rg_ppo.h", "rg_host.h", "rg_agent_dev.inc", "rg_ppo_dev.inc"]
    assert all("__global__" not in text for text in shared)
    assert [re.findall(r'#include "([^"]+)"', text) for text in shared] == [[], ["rg_stream_dev.inc"], [], []]     # the one stream, under the agents' noise
    # the head's and Adam's arithmetic is the shared files' alone: no update writes an exp or a pow of its own
    for name in ("rg_ppo.hip", "rg_bptt.hip", "rg_ddpg.hip"):
        text = re.sub(r"//.*", "", open(os.path.join(SRC, name)).read())
        assert "pow(" not in text, name
        assert name == "rg_ddpg.hip" or "exp(" not in text, name
    assert "pow(" in re.sub(r"//.*", "", shared[1]) and "exp(" in re.sub(r"//.*", "", shared[2])
    import bench
    assert not any("rg_agent_" in rel or "rg_stream_" in rel or "rg_host" in rel for rel in bench.compiled_sources())     # the MPC hash behind profiles/ does not follow them
    for other in ("rg_mpc.hip", "rg_policy.hip"):
        assert "rg_ppo" not in open(os.path.join(SRC, other)).read()                # the source hashes behind profiles/ do not move
    assert "__builtin_fmaf" in code and "mfma" not in code.lower()
    kernel_checks.assert_built_into_both("rg_ppo.hip", header="rg_ppo.h")


# ---- DevicePPO's argument checks ----------------------------------------------------------------------------------------

def _host_update(T=3, B=4):
    pol = BatchedGaussianPolicy(B, device="cpu", **CFG)
    return pol, DevicePPO(pol, T, epochs_policy=2, epochs_value=2, kl_init_penalty=0.5)


def test_device_update_rejects_a_rollout_it_must_not_follow():
    pol, dev = _host_update()
    good = lambda: RolloutBuffer(3, 4, 6, 3)
    with pytest.raises(ppo_abi.RgPpoError) as e:       # every check passes; the host-only handle then has no device
        dev.update(good())
    assert e.value.status == -3
    calls = []
    real = dev._handle._lib
    dev._handle.update = lambda *a: calls.append(a)     # no library call may happen below
    with pytest.raises(ValueError, match="rollout.T is 4"):
        dev.update(RolloutBuffer(4, 4, 6, 3))
    with pytest.raises(ValueError, match="rollout.batch is 5"):
        dev.update(RolloutBuffer(3, 5, 6, 3))
    ro = good()
    ro.adv = ro.adv.double()
    with pytest.raises(ValueError, match="rollout.adv must be a contiguous float32"):
        dev.update(ro)
    ro = good()
    ro.mask = ro.mask.long()
    with pytest.raises(ValueError, match="rollout.mask must be a contiguous int32"):
        dev.update(ro)
    ro = good()
    ro.obs = torch.zeros(3, 4, 6).permute(0, 2, 1)      # the right shape, not contiguous
    assert tuple(ro.obs.shape) == (3, 6, 4)
    with pytest.raises(ValueError, match="rollout.obs must be a contiguous float32"):
        dev.update(ro)
    ro = good()
    ro.action = torch.zeros(3, 4, 2)
    with pytest.raises(ValueError, match="rollout.action"):
        dev.update(ro)
    ro = good()
    ro.logstd = None
    with pytest.raises(ValueError, match="rollout.logstd"):
        dev.update(ro)
    assert calls == [] and real is ppo_abi.load_library()
    with pytest.raises(ValueError, match="out must be"):
        dev.policy_grad(good(), out=torch.zeros(3))
    with pytest.raises(ValueError, match="which"):
        dev.adam("both", None)
    with pytest.raises(ValueError, match="out must be"):
        dev.kl(good(), out=torch.zeros(4))


def test_device_update_state_is_the_documented_layout_and_loads_in_place():
    pol, dev = _host_update()
    pc, vc = pol.layout["policy_count"], pol.layout["value_count"]
    assert dev.opt_state.dtype == torch.float64 and dev.opt_state.numel() * 8 == dev._handle.opt_state_bytes
    assert dev.steps.tolist() == [0, 0] and float(dev.penalty) == 0.5 and dev.moments.numel() >= 2 * (pc + vc) and float(dev.moments.abs().max()) == 0.0
    raw = dev.opt_state.numpy().view(np.uint8)
    assert np.frombuffer(raw[16:24].tobytes(), dtype=np.float64)[0] == 0.5 and not raw[:16].any() and not raw[24:].any()
    dev.steps[0], dev.steps[1] = 7, 9
    dev.moments[:3] = torch.tensor([1.0, 2.0, 3.0])
    assert np.frombuffer(raw[:16].tobytes(), dtype=np.int64).tolist() == [7, 9]
    assert np.frombuffer(raw[32:44].tobytes(), dtype=np.float32).tolist() == [1.0, 2.0, 3.0]
    state = dev.state_dict()
    ptr = dev.opt_state.data_ptr()
    dev.opt_state.zero_()
    dev.load_state_dict(state)
    assert dev.opt_state.data_ptr() == ptr and dev.steps.tolist() == [7, 9] and float(dev.penalty) == 0.5 and dev.moments[:3].tolist() == [1.0, 2.0, 3.0]
    with pytest.raises(ValueError):
        dev.load_state_dict(dict(state, opt_state=torch.zeros(3, dtype=torch.float64)))
    with pytest.raises(ValueError):
        dev.load_state_dict(dict(state, opt_state=state["opt_state"].float()))
    with pytest.raises(ValueError, match="another configuration"):
        dev.load_state_dict(dict(state, fields=dict(state["fields"], kl_target=0.5)))
    with pytest.raises(ValueError, match="another configuration"):
        dev.load_state_dict(dict(state, batch=5))
    with pytest.raises(ValueError, match="T = 9"):
        dev.load_state_dict(dict(state, T=9))
    # T from the first rollout: the same keywords as PPO
    lazy = DevicePPO(pol, epochs_policy=2, kl_init_penalty=0.5)
    assert lazy.T is None and lazy.opt_state.numel() == dev.opt_state.numel()
    with pytest.raises(ValueError, match="no rollout"):
        lazy.adam("policy", None)
    with pytest.raises(ppo_abi.RgPpoError):
        lazy.update(RolloutBuffer(5, 4, 6, 3))
    assert lazy.T == 5 and lazy.workspace.numel() * 8 == lazy._handle.workspace_bytes
    with pytest.raises(ValueError, match="rollout.T is 3"):
        lazy.update(RolloutBuffer(3, 4, 6, 3))
    assert dev.stats_dict()["penalty"] == 0.0 and set(dev.stats_dict()) == set(ppo_abi.STAT_NAMES)
