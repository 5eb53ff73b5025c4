"""The DDPG agent on the device (include/rg_ddpg.h) without a GPU: librg_mpc.so exports every rg_ddpg_* entry, the ctypes binding
matches the header, create validates the configuration field by field (naming the field) before it looks for a device, a
host-only handle checks every pointer and then returns NO_DEVICE; the numpy model (tests/ddpg_model.py) against torch autograd
in float64, its Adam against torch.optim.Adam, the window rule's known answers on a hand-built ring, the Ornstein-Uhlenbeck
step against a literal loop, the sample stream's range; the cases of the GPU tests are built and what their builder promises is
asserted; the kernels of rg_ddpg.hip cross-compile for gfx950 without scratch or spills, within a compute unit's LDS; and
BatchedDDPGAgent rejects a tensor it must not follow before the library sees a pointer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from robot_gym_amd.agents.ddpg import BatchedDDPGAgent, collect
from robot_gym_amd.core import ddpg_abi
from tests import ddpg_cases as DC
from tests import ddpg_model as DM
from tests import kernel_checks
from tests import policy_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rg_ddpg.h")
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
NAN, INF = float("nan"), float("inf")
LOPSIDED = DC.CONFIGS["lopsided"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI and configuration ------------------------------------------------------------------------------------------

def test_library_exports_every_declared_entry():
    lib = ddpg_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_ddpg_[a-z0-9_]+)\s*\(", _header())))
    assert len(declared) == 22
    for name in declared:
        assert hasattr(lib, name), f"librg_mpc.so lacks {name}"
    assert sorted(ddpg_abi.EXPORTS) == declared
    for name in declared:   # bound: load_library gave each a signature
        assert getattr(lib, name).argtypes is not None, name


def test_struct_layouts_and_constants_match_the_header():
    lib = ddpg_abi.load_library()
    structs = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", _header()))
    sizes = {"int32_t": 4, "double": 8, "uint64_t": 8}
    want = []
    for t, names in re.findall(r"\b(int32_t|double|uint64_t)\s+([^;]+);", structs["rg_ddpg_config"]):
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?", n)
            want.append((m.group(1), sizes[t] * int(m.group(2) or 1)))
    assert [n for n, _ in want] == [n for n, _ in ddpg_abi.CConfig._fields_]
    for (n, size), (_, tg) in zip(want, ddpg_abi.CConfig._fields_):
        assert size == C.sizeof(tg), n
    assert sum(s for _, s in want) == C.sizeof(ddpg_abi.CConfig) == lib.rg_ddpg_config_size() == 160   # no padding
    assert lib.rg_ddpg_layout_size() == C.sizeof(ddpg_abi.CLayout) == 4 * (4 + 8 * 4)
    ptrs = re.findall(r"\*(\w+);", structs["rg_ddpg_ring"])
    assert ptrs == [n for n, _ in ddpg_abi.CRing._fields_] == ["obs", "action", "reward", "done", "state"]
    assert lib.rg_ddpg_ring_size() == C.sizeof(ddpg_abi.CRing) == 8 * len(ptrs)
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_DDPG_\w+) (\d+)", _header())}
    assert lib.rg_ddpg_abi_version() == defs["RG_DDPG_ABI_VERSION"] == ddpg_abi.ABI_VERSION == 1
    assert lib.rg_ddpg_tile() == defs["RG_DDPG_TILE"] == ddpg_abi.TILE == DC.TILE
    assert (defs["RG_DDPG_MAX_GROUPS"], defs["RG_DDPG_STATS"], defs["RG_DDPG_OPT_HEADER_BYTES"], defs["RG_DDPG_RING_STATE"]) == \
        (ddpg_abi.MAX_GROUPS, ddpg_abi.STATS, ddpg_abi.OPT_HEADER_BYTES, ddpg_abi.RING_STATE)
    assert (defs["RG_DDPG_MAX_OBS"], defs["RG_DDPG_MAX_ACT"], defs["RG_DDPG_MAX_WINDOW"], defs["RG_DDPG_MAX_INPUT"], defs["RG_DDPG_MAX_LAYERS"],
            defs["RG_DDPG_MAX_WIDTH"]) == (ddpg_abi.MAX_OBS, ddpg_abi.MAX_ACT, ddpg_abi.MAX_WINDOW, ddpg_abi.MAX_INPUT, ddpg_abi.MAX_LAYERS, ddpg_abi.MAX_WIDTH)
    assert len(ddpg_abi.STAT_NAMES) == ddpg_abi.STATS
    assert (defs["RG_DDPG_MODE_SAMPLE"], defs["RG_DDPG_MODE_MEAN"], defs["RG_DDPG_ACTOR"], defs["RG_DDPG_CRITIC"]) == \
        (ddpg_abi.MODE_SAMPLE, ddpg_abi.MODE_MEAN, ddpg_abi.ACTOR, ddpg_abi.CRITIC)


def test_defaults_are_the_references():
    D = ddpg_abi.DEFAULTS    # simple_ddpg_agent.py: the two Sequential models, the OU process, DDPGAgent(...), Adam(lr=.001, clipnorm=1.)
    assert (D["window"], D["actor_layers"], D["critic_layers"]) == (5, (128, 128, 64), (256, 256, 128))
    assert (D["ou_theta"], D["ou_mu"], D["ou_sigma"], D["ou_dt"]) == (0.5, 0.4, 0.3, 1e-2)
    assert (D["gamma"], D["tau"], D["actor_lr"], D["critic_lr"], D["clipnorm"], D["minibatch"]) == (0.99, 1e-3, 1e-3, 1e-3, 1.0, 32)
    assert (D["beta1"], D["beta2"], D["adam_eps"]) == (0.9, 0.999, 1e-8)
    with pytest.raises(TypeError):
        ddpg_abi.make_cconfig(kl_target=0.9)
    with pytest.raises(ValueError):
        ddpg_abi.make_cconfig(actor_layers=(1, 2, 3, 4))


@pytest.mark.parametrize("field,value,text", [
    ("obs_dim", 0, "config.obs_dim"), ("obs_dim", 65, "config.obs_dim"), ("act_dim", 5, "config.act_dim"), ("window", 0, "config.window"),
    ("window", 9, "config.window"), ("n_actor_layers", 4, "config.n_actor_layers"), ("n_critic_layers", -1, "config.n_critic_layers"),
    ("capacity", 1, "config.capacity"), ("capacity", (1 << 20) + 1, "config.capacity"), ("minibatch", 0, "config.minibatch"),
    ("minibatch", (1 << 16) + 1, "config.minibatch"), ("gamma", 1.5, "config.gamma"), ("gamma", NAN, "config.gamma"), ("tau", 0.0, "config.tau"),
    ("tau", 1.01, "config.tau"), ("actor_lr", -1e-3, "config.actor_lr"), ("critic_lr", INF, "config.critic_lr"), ("beta1", 1.0, "config.beta1"),
    ("beta2", -0.1, "config.beta2"), ("adam_eps", 0.0, "config.adam_eps"), ("clipnorm", -1.0, "config.clipnorm"), ("clipnorm", NAN, "config.clipnorm"),
    ("ou_theta", -0.5, "config.ou_theta"), ("ou_mu", INF, "config.ou_mu"), ("ou_sigma", -0.3, "config.ou_sigma"), ("ou_dt", 0.0, "config.ou_dt"),
    ("abi_version", 2, "config.abi_version"),
])
def test_create_rejects_a_bad_config_naming_the_field(field, value, text):
    cc = ddpg_abi.make_cconfig()
    setattr(cc, field, value)
    for device in (0, ddpg_abi.DEVICE_NONE):
        rc, msg = ddpg_abi.create_status(cc, device=device)
        assert rc == -1 and text in msg, (rc, msg)


def test_create_checks_the_layers_the_input_the_batch_and_null_arguments():
    cc = ddpg_abi.make_cconfig()
    cc.actor_layers[1] = 257
    rc, msg = ddpg_abi.create_status(cc)
    assert rc == -1 and "config.actor_layers[1]" in msg
    cc = ddpg_abi.make_cconfig(critic_layers=(8,))
    cc.critic_layers[2] = 3
    rc, msg = ddpg_abi.create_status(cc)
    assert rc == -1 and "config.critic_layers[2]" in msg
    rc, msg = ddpg_abi.create_status(ddpg_abi.make_cconfig(obs_dim=17, window=8))     # 136 inputs
    assert rc == -1 and "config.window" in msg and "128" in msg
    for batch in (0, (1 << 24) + 1):
        rc, msg = ddpg_abi.create_status(batch=batch)
        assert rc == -1 and "batch:" in msg
    lib = ddpg_abi.load_library()
    cc, h = ddpg_abi.make_cconfig(), C.c_void_p()
    assert lib.rg_ddpg_create(None, 4, -1, C.byref(h)) == -1 and lib.rg_ddpg_create(C.byref(cc), 4, -1, None) == -1
    for settings in (dict(), dict(DC.CONFIGS["limits"], tau=1.0, clipnorm=0.0, gamma=0.0, ou_sigma=0.0, capacity=2, minibatch=1 << 16), DC.CONFIGS["flat"]):
        rc, msg = ddpg_abi.create_status(ddpg_abi.make_cconfig(**settings))           # valid, host-only: a handle is made
        assert rc == 0, msg
    assert lib.rg_ddpg_workspace_bytes(None) == -1 and lib.rg_ddpg_opt_state_bytes(None) == -1 and lib.rg_ddpg_groups(None) == -1


def test_layout_against_a_hand_count():
    lay = ddpg_abi.param_layout()
    # actor 80 -> 128 -> 128 -> 64 -> 2; critic 2 + 80 -> 256 -> 256 -> 128 -> 1
    assert lay["actor"] == [(80, 128, 0, 10240), (128, 128, 10368, 26752), (128, 64, 26880, 35072), (64, 2, 35136, 35264)]
    assert lay["actor_count"] == 35266
    assert lay["critic"] == [(82, 256, 0, 20992), (256, 256, 21248, 86784), (256, 128, 87040, 119808), (128, 1, 119936, 120064)]
    assert lay["critic_count"] == 120065
    for name, cfg in DC.CONFIGS.items():
        got, want = ddpg_abi.param_layout(**cfg), DM.layout(**cfg)
        assert got == want, name
    flat = ddpg_abi.param_layout(**DC.CONFIGS["flat"])
    assert flat["actor"] == [(16, 2, 0, 32)] and flat["critic"] == [(18, 1, 0, 18)]


def test_sizes_of_a_handle_follow_the_header():
    for settings, B in ((dict(), 64), (dict(LOPSIDED, minibatch=5), 3), (dict(DC.CONFIGS["limits"], minibatch=DC.BIG), 67)):
        h = ddpg_abi.DdpgHandle(B, ddpg_abi.DEVICE_NONE, **settings)
        lay = h.layout
        want = ddpg_abi.OPT_HEADER_BYTES + 4 * 2 * (lay["actor_count"] + lay["critic_count"])
        assert h.opt_state_bytes == (want + 7) // 8 * 8
        M = h.fields["minibatch"]
        assert h.groups == min(-(-M // ddpg_abi.TILE), ddpg_abi.MAX_GROUPS)
        slabs = 4 * h.groups * max(lay["actor_count"], lay["critic_count"])
        assert h.workspace_bytes % 8 == 0 and slabs <= h.workspace_bytes <= slabs + 8 * M + 16 * (lay["actor_count"] + lay["critic_count"]) + (1 << 16)
        widths = [o for _, o, _, _ in lay["actor"]] + [o for _, o, _, _ in lay["critic"]]
        assert h.lds_bytes == 4 * ddpg_abi.TILE * (lay["critic"][0][0] + lay["actor"][0][0] + sum(widths) + 2 * max(widths)) <= 160 * 1024
        h.close()
    h = ddpg_abi.DdpgHandle(1, ddpg_abi.DEVICE_NONE, **DC.CONFIGS["limits"])
    assert h.lds_bytes == (132 + 768 + 1 + 128 + 768 + 4 + 512) * 64 == 148032       # the widest configuration
    h.close()


def test_host_only_handle_checks_every_pointer_then_reports_no_device():
    h = ddpg_abi.DdpgHandle(4, ddpg_abi.DEVICE_NONE, capacity=4)
    lib = ddpg_abi.load_library()
    dummy = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
    p = dummy.ctypes.data
    last = lambda: lib.rg_ddpg_last_error(h._h).decode()
    slots = ("obs", "action", "reward", "done", "state")
    full = lambda **kw: ddpg_abi.make_cring(**{**{s: p for s in slots}, **kw})
    S, Mn = ddpg_abi.MODE_SAMPLE, ddpg_abi.MODE_MEAN
    # call: (function, the ring's slots it reads, [(argument name or None for a scalar, good value)])
    calls = {
        "act": (lib.rg_ddpg_act, ("obs", "done", "state"),
                [("obs", p), ("actor_params", p), ("ou_state", p), ("act_state", p), (None, S), ("action", p), (None, None)]),
        "store": (lib.rg_ddpg_store, slots, [("obs", p), ("action", p), ("reward", p), ("done", p), (None, None)]),
        "sample": (lib.rg_ddpg_sample, ("state",), [("idx_out", p)]),
        "critic_grad": (lib.rg_ddpg_critic_grad, slots, [("idx", p), ("critic_params", p), ("target_actor_params", p), ("target_critic_params", p),
                                                          ("workspace", p), ("grad_out", p), ("loss_out", p)]),
        "actor_grad": (lib.rg_ddpg_actor_grad, ("obs", "done", "state"), [("idx", p), ("actor_params", p), ("critic_params", p), ("workspace", p),
                                                                        ("grad_out", p), ("loss_out", p)]),
        "advance": (lib.rg_ddpg_advance, ("state",), []),
        "update": (lib.rg_ddpg_update, slots, [("actor_params", p), ("critic_params", p), ("target_actor_params", p), ("target_critic_params", p),
                                               ("opt_state", p), ("workspace", p), (None, 2), ("stats", p)]),
    }
    for call, (fn, needs, args) in calls.items():
        good = [v for _, v in args]
        assert fn(h._h, C.byref(full()), *good, None) == -3 and "host-only" in last(), (call, last())
        assert fn(h._h, C.byref(full(**{s: None for s in slots if s not in needs})), *good, None) == -3, call   # only what it reads
        assert fn(h._h, None, *good, None) == -1 and f"{call}: null ring" in last()
        for s in needs:
            assert fn(h._h, C.byref(full(**{s: None})), *good, None) == -1 and f"{call}: null ring.{s}" in last(), (call, s, last())
        for k, (name, _) in enumerate(args):
            if name is None:
                continue
            a = list(good)
            a[k] = None
            assert fn(h._h, C.byref(full()), *a, None) == -1 and f"{call}: null {name}" in last(), (call, name, last())
        assert fn(None, C.byref(full()), *good, None) == -1 and "null handle" in lib.rg_ddpg_last_error(None).decode()
    # act in MEAN mode needs neither the OU state nor the act state; a bad mode is named
    assert lib.rg_ddpg_act(h._h, C.byref(full()), p, p, None, None, Mn, p, None, None) == -3
    assert lib.rg_ddpg_act(h._h, C.byref(full()), p, p, p, p, 2, p, None, None) == -1 and "mode" in last()
    assert lib.rg_ddpg_update(h._h, C.byref(full()), p, p, p, p, p, p, -1, p, None) == -1 and "n_updates" in last()
    for which in (ddpg_abi.ACTOR, ddpg_abi.CRITIC):
        assert lib.rg_ddpg_adam(h._h, which, p, p, p, p, None, None, None) == -3
        assert lib.rg_ddpg_soft_update(h._h, which, p, p, None, None) == -3
    assert lib.rg_ddpg_adam(h._h, 2, p, p, p, p, None, None, None) == -1 and "which" in last()
    assert lib.rg_ddpg_soft_update(h._h, -1, p, p, None, None) == -1 and "which" in last()
    for k, name in enumerate(("params", "grad", "opt_state", "workspace")):
        a = [p, p, p, p]
        a[k] = None
        assert lib.rg_ddpg_adam(h._h, 0, *a, None, None, None) == -1 and f"adam: null {name}" in last()
    for k, name in enumerate(("target", "online")):
        a = [p, p]
        a[k] = None
        assert lib.rg_ddpg_soft_update(h._h, 0, *a, None, None) == -1 and f"soft_update: null {name}" in last()
    with pytest.raises(ddpg_abi.RgDdpgError) as e:
        h.sample(full(), p)
    assert e.value.status == -3
    h.close()


# ---- the window rule, OU and the sample stream ----------------------------------------------------------------------------

def _hand_ring():
    """Capacity 4, one robot, obs_dim 1, six ticks stored with observations 10, 11, .. 15: the ring has wrapped and holds ticks
    12 .. 15 at ages 3 .. 0 (slots 2, 3, 0, 1).  The tick with observation 13 (age 2) ended an episode."""
    ring = DM.Ring(4, 1, 1, 1)
    for t in range(6):
        ring.store(np.array([[10.0 + t]], dtype=np.float32), np.array([[0.1 * t]], dtype=np.float32), np.array([float(t)], dtype=np.float32),
                   np.array([1 if t == 3 else 0], dtype=np.int32))
    return ring


def test_window_rule_known_answers_on_a_wrapped_ring_with_a_done_in_the_middle():
    ring = _hand_ring()
    assert (ring.head, ring.count) == (2, 4) and ring.obs[:, 0, 0].tolist() == [14.0, 15.0, 12.0, 13.0]
    assert [ring.slot(a) for a in range(4)] == [1, 0, 3, 2] and ring.done[:, 0].tolist() == [0, 0, 0, 1]
    # window 1: the observation itself
    assert [ring.state(a, 0, 1).tolist() for a in range(4)] == [[15.0], [14.0], [13.0], [12.0]]
    # window 3, oldest first.  Age 0: 15, 14, then 13 is masked (done at age 2 lies in ages 1 .. 2)
    assert ring.state(0, 0, 3).tolist() == [0.0, 14.0, 15.0]
    assert ring.state(1, 0, 3).tolist() == [0.0, 0.0, 14.0]        # done at age 2 masks 13 and everything older
    assert ring.state(2, 0, 3).tolist() == [0.0, 12.0, 13.0]       # 13 ends its own episode: it and 12 are kept; age 4 does not exist (overwritten)
    assert ring.state(3, 0, 3).tolist() == [0.0, 0.0, 12.0]
    # acting on a current observation of 16: ages 0 and 1 behind it
    cur = np.array([[16.0]], dtype=np.float32)
    assert ring.state(-1, 0, 3, cur).tolist() == [14.0, 15.0, 16.0] and ring.state(-1, 0, 1, cur).tolist() == [16.0]
    ring.done[ring.slot(0), 0] = 7                                    # the last tick ended an episode: a fresh window
    assert ring.state(-1, 0, 3, cur).tolist() == [0.0, 0.0, 16.0]
    # a transition at age 2 (the done one): s0 ends at 13, s1 ends at age 1 and must not look back across the done
    assert ring.state(2 - 1, 0, 3).tolist() == [0.0, 0.0, 14.0]
    empty = DM.Ring(4, 1, 1, 1)
    assert empty.state(-1, 0, 3, cur).tolist() == [0.0, 0.0, 16.0] and empty.state(0, 0, 3).tolist() == [0.0, 0.0, 0.0]


def test_ou_step_against_a_literal_loop():
    rng = np.random.default_rng(3)
    x = np.zeros(3, dtype=np.float32)
    want = [0.0, 0.0, 0.0]
    for step in range(20):
        eps = rng.normal(size=3).astype(np.float32)
        x = DM.ou_step(x, eps, 0.5, 0.4, 0.3, 1e-2)
        for k in range(3):
            xk = float(np.float32(want[k]))
            want[k] = float(np.float32(xk + 0.5 * (0.4 - xk) * 1e-2 + 0.3 * math.sqrt(1e-2) * float(eps[k])))
        assert x.dtype == np.float32 and x.tolist() == want
    assert DM.ou_step(np.float32(0.4), np.float32(0.0)).tolist() == pytest.approx(0.4)    # the mean is the fixed point
    # the stream behind eps is rg_policy.h's
    assert PM.eps(5, 1, 2, 0) != PM.eps(5, 1, 3, 0) and PM.eps(5, 1, 2, 0) == PM.eps(5, 1, 2, 0)


def test_sample_indices_stay_in_range_and_a_short_ring_gives_none():
    for count, B, M in ((2, 1, 50), (3, 67, 500), (7, 3, 500), (1 << 20, 1 << 24, 200)):
        idx = DM.sample(9, 4, M, count, B)
        assert idx.shape == (M, 2) and idx.dtype == np.int32
        assert idx[:, 0].min() >= 1 and idx[:, 0].max() <= count - 1 and idx[:, 1].min() >= 0 and idx[:, 1].max() < B
    idx = DM.sample(9, 4, 500, 7, 3)
    assert set(idx[:, 0].tolist()) == set(range(1, 7)) and set(idx[:, 1].tolist()) == {0, 1, 2}        # every age, every robot
    assert not np.array_equal(idx, DM.sample(9, 5, 500, 7, 3)) and not np.array_equal(idx, DM.sample(10, 4, 500, 7, 3))
    assert np.array_equal(idx[:100], DM.sample(9, 4, 100, 7, 3))                                       # stateless in m
    assert DM.sample(9, 0, 5, 1, 3) is None and DM.sample(9, 0, 5, 0, 3) is None


# ---- the model against autograd ---------------------------------------------------------------------------------------

def _torch_net(params, layers, x, head):
    p = params
    for k, (i, o, w, b) in enumerate(layers):
        x = x @ p[w:w + i * o].view(i, o) + p[b:b + o]
        if k < len(layers) - 1:
            x = torch.relu(x)
    return torch.tanh(x) if head == "tanh" else x


def _autograd_case():
    c = DC.case("lopsided", 3, 4, 6, 5)
    ring, idx, lay, W = c["ring"], c["idx"], c["lay"], c["cfg"]["window"]
    P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in c["params"].items()}
    ages, robots = idx[:, 0], idx[:, 1]
    slots = np.array([ring.slot(int(a)) for a in ages])
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    s0, s1 = t(ring.states(ages, robots, W)), t(ring.states(ages - 1, robots, W))
    return c, P, s0, s1, t(ring.action[slots, robots]), t(ring.reward[slots, robots]), t(1.0 - (ring.done[slots, robots] != 0))


def test_critic_gradient_of_the_model_equals_autograd():
    c, P, s0, s1, action, reward, nd = _autograd_case()
    lay = c["lay"]
    with torch.no_grad():
        a1 = _torch_net(P["target_actor"], lay["actor"], s1, "tanh")
        y = reward + DC.GAMMA * nd * _torch_net(P["target_critic"], lay["critic"], torch.cat([a1, s1], dim=1), "linear")[:, 0]
    q = _torch_net(P["critic"], lay["critic"], torch.cat([action, s0], dim=1), "linear")[:, 0]
    loss = (0.5 * (y - q) ** 2).sum() / len(q)
    loss.backward()
    want, got = P["critic"].grad.numpy(), c["critic"]["m64"]
    assert (nd.numpy() == 0).any() and (nd.numpy() == 1).any()           # a done transition: its target is exactly the reward
    assert np.array_equal(got["y"][nd.numpy() == 0], reward.numpy()[nd.numpy() == 0])
    assert math.isclose(got["loss"], float(loss.detach()), rel_tol=1e-12)
    assert np.abs(want).max() > 0 and np.allclose(got["grad"], want, rtol=1e-10, atol=1e-13 * np.abs(want).max()), float(np.abs(got["grad"] - want).max())
    assert P["target_critic"].grad is None and P["target_actor"].grad is None


def test_actor_gradient_of_the_model_through_the_critic_equals_autograd():
    for cs in (("lopsided", 67, 7, 6, DC.BIG), ("default", 3, 7, 5, 17)):
        c = DC.case(*cs)
        ring, idx, lay, W = c["ring"], c["idx"], c["lay"], c["cfg"]["window"]
        P = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in c["params"].items()}
        s0 = torch.tensor(ring.states(idx[:, 0], idx[:, 1], W).astype(np.float64))
        mu = _torch_net(P["actor"], lay["actor"], s0, "tanh")
        loss = -_torch_net(P["critic"], lay["critic"], torch.cat([mu, s0], dim=1), "linear")[:, 0].sum() / len(idx)
        loss.backward()
        want, got = P["actor"].grad.numpy(), c["actor"]["m64"]
        assert math.isclose(got["loss"], float(loss.detach()), rel_tol=1e-12) and got["mean_q"] == -got["loss"]
        assert np.abs(want).max() > 0 and np.allclose(got["grad"], want, rtol=1e-10, atol=1e-13 * np.abs(want).max()), float(np.abs(got["grad"] - want).max())


def test_adam_with_the_clip_of_the_model_equals_torch():
    rng = np.random.default_rng(5)
    p0 = rng.normal(size=40)
    grads = rng.normal(size=(5, 40)) * np.logspace(-3, 0.5, 40)
    grads[3] *= 1e-3                                           # a norm below the threshold: left alone
    t = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([t], lr=1e-3)
    p, m, v, step = p0.copy(), np.zeros(40), np.zeros(40), 0
    clipped = []
    for g in grads:
        g32 = g.astype(np.float32)
        t.grad = torch.as_tensor(g32.astype(np.float64))
        norm = float(torch.nn.utils.clip_grad_norm_([t], 1.0))
        gc, n = DM.clip(g32, 1.0)
        clipped.append(n >= 1.0)
        assert math.isclose(n, norm, rel_tol=1e-12)
        # torch multiplies by 1 / (norm + 1e-6) and keeps float64: with norm >= 1 that is at most 1e-6 off clipnorm / norm; the
        # model's rounding to float32 adds 2^-24
        assert np.allclose(gc, t.grad.numpy(), rtol=1e-6 + 2.0 ** -23, atol=0)
        if not clipped[-1]:
            assert gc.tobytes() == g32.tobytes()
        t.grad = torch.as_tensor(gc.astype(np.float64))
        opt.step()
        p, m, v, step = DM.adam_step(p, gc.astype(np.float64), m, v, step, 1e-3)
        assert np.allclose(p, t.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert step == 5 and any(clipped) and not all(clipped)
    g = np.array([3.0, 4.0], dtype=np.float32)
    assert DM.clip(g, 0.0)[0].tobytes() == g.tobytes() and DM.clip(g, 0.0)[1] == 5.0 and DM.clip(g, 5.0)[0].tolist() == [3.0, 4.0]   # off; norm = clipnorm scales by 1
    assert DM.clip(g, 2.5)[0].tolist() == [1.5, 2.0]
    assert DM.soft_update([1.0, 2.0], [3.0, 6.0], 0.25).tolist() == [1.5, 3.0] and DM.soft_update([1.0], [3.0], 1.0).tolist() == [3.0]


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cs", DC.CASES, ids=lambda cs: "-".join(str(v) for v in cs))
def test_every_gpu_case_builds_with_the_model_alone_and_redraws_at_most_one_observation_in_four(cs):
    c = DC.case(*cs)
    ring, idx, M = c["ring"], c["idx"], c["M"]
    print(f"{cs}: redrawn {c['redrawn']:.4f}; critic bounds {c['critic']['tol']}; actor bounds {c['actor']['tol']}")
    assert c["redrawn"] <= 0.25
    assert ring.count == min(c["ticks"], c["C"]) >= 2 and ring.head == c["ticks"] % c["C"]
    assert idx.shape == (M, 2) and idx[:, 0].min() >= 1 and idx[:, 0].max() <= ring.count - 1 and idx[:, 1].min() >= 0 and idx[:, 1].max() < c["B"]
    if M > 1:
        assert tuple(idx[0]) == tuple(idx[1])                                             # a repeated index
    if M >= 100:
        slots = np.array([ring.slot(int(a)) for a in idx[:, 0]])
        assert (ring.done[slots, idx[:, 1]] != 0).any()                                   # done transitions
        assert set(idx[:, 0].tolist()) == set(range(1, ring.count))                       # every age: with a wrapped ring, across the wrap
    for which in ("critic", "actor"):
        r = c[which]
        assert all(math.isfinite(v) and v >= 0 for v in r["tol"].values()) and max(r["tol"].values()) <= 1e-3, (which, r["tol"])
        assert np.all(np.isfinite(r["m64"]["grad"])) and math.isfinite(r["m64"]["loss"])


def test_the_cases_cover_the_shapes_the_kernels_branch_on():
    Bs, Cs, Ms = ({cs[k] for cs in DC.CASES} for k in (1, 2, 4))
    assert Bs == {1, 3, 67} and Cs == {2, 4, 7} and Ms == {1, 5, 17, 100, DC.BIG}
    assert DC.BIG == 16 * 256 + 16 + 3 and -(-DC.BIG // ddpg_abi.TILE) == ddpg_abi.MAX_GROUPS + 2
    assert {cs[0] for cs in DC.CASES} == set(DC.CONFIGS)
    assert any(cs[3] > cs[2] for cs in DC.CASES) and any(cs[3] < cs[2] for cs in DC.CASES)     # wrapped and not wrapped
    assert DC.CONFIGS["lopsided"] == dict(obs_dim=6, act_dim=3, window=3, actor_layers=(5,), critic_layers=(7, 3, 2))
    assert DC.CONFIGS["limits"] == dict(obs_dim=16, act_dim=4, window=8, actor_layers=(256,) * 3, critic_layers=(256,) * 3)
    assert DC.CONFIGS["flat"]["window"] == 1 and DC.CONFIGS["flat"]["actor_layers"] == () == DC.CONFIGS["flat"]["critic_layers"]
    assert {k: DC.CONFIGS["default"][k] for k in DC.CONFIGS["default"]} == {k: ddpg_abi.DEFAULTS[k] for k in DC.CONFIGS["default"]}


# ---- resources of rg_ddpg.hip ------------------------------------------------------------------------------------------

KERNELS = {"rg_ddpg_transpose_kernel", "rg_ddpg_act_kernel", "rg_ddpg_store_kernel", "rg_ddpg_store_advance_kernel", "rg_ddpg_sample_kernel",
           "rg_ddpg_advance_kernel", "rg_ddpg_critic_sweep_kernel", "rg_ddpg_actor_sweep_kernel", "rg_ddpg_grad_finish_kernel",
           "rg_ddpg_loss_finish_kernel", "rg_ddpg_norm_kernel", "rg_ddpg_adam_kernel", "rg_ddpg_adam_count_kernel", "rg_ddpg_soft_update_kernel",
           "rg_ddpg_stats_kernel"}
SWEEPS = ("rg_ddpg_critic_sweep_kernel", "rg_ddpg_actor_sweep_kernel")


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_ddpg.hip")


def test_every_ddpg_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_ddpg_kernel_uses_scratch_spills_or_a_dynamic_stack(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


def test_lds_is_within_a_compute_units_160_kib(remarks):
    widest = (132 + 768 + 1 + 128 + 768 + 4 + 512) * 64          # dynamic, at the limits (rg_ddpg.hip asserts the same figure)
    assert widest == 148032
    for name in SWEEPS:
        static = int(remarks[name]["LDS Size [bytes/block]"])
        assert static <= 1024 and static + widest <= 160 * 1024, (name, remarks[name])
    assert int(remarks["rg_ddpg_act_kernel"]["LDS Size [bytes/block]"]) <= 64 * 1024
    for name in KERNELS - set(SWEEPS) - {"rg_ddpg_act_kernel"}:
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= 32, (name, remarks[name])
    for name in SWEEPS:                                          # one workgroup per compute unit is four waves, one per SIMD
        assert int(remarks[name]["Occupancy [waves/SIMD]"]) >= 1 and int(remarks[name]["AGPRs"]) == 0


def test_source_is_its_own_translation_unit_in_both_library_targets():
    own = open(os.path.join(SRC, "rg_ddpg.hip")).read()
    shared = [open(os.path.join(SRC, name)).read() for name in ("rg_host.h", "rg_agent_dev.inc", "rg_stream_dev.inc")]   # the agents' common code
    src = "\n".join([own] + shared)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    assert "hipMalloc" not in src and "hipMemcpy" not in src and "Synchronize" not in src and "hipFree" not in src
    own_code = re.sub(r"//.*", "", own)
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index("__global__")
    assert own_code.index("#pragma clang fp contract(off)") < own_code.index('#include "rg_agent_dev.inc"')
    assert re.findall(r'#include "([^"]+)"', own_code) == ["../../include/rg_ddpg.h", "rg_host.h", "rg_agent_dev.inc"]
    assert all("__global__" not in text for text in shared)
    assert [re.findall(r'#include "([^"]+)"', text) for text in shared] == [[], ["rg_stream_dev.inc"], []]     # the one stream, under the agents' noise
    import bench
    assert not any("rg_agent_" in rel or "rg_stream_" in rel or "rg_host" in rel for rel in bench.compiled_sources())     # the MPC hash behind profiles/ does not follow them
    assert "#include" not in re.sub(r"#include <stdint.h>", "", open(HEADER).read())
    for other in ("rg_mpc.hip", "rg_policy.hip", "rg_ppo.hip"):
        assert "rg_ddpg" not in open(os.path.join(SRC, other)).read()                # the source hashes behind profiles/ do not move
    assert "__builtin_fmaf" in code and "mfma" not in code.lower()
    assert "static_assert(kMaxLds == 148032 && kMaxLds <= 160 * 1024" in code
    kernel_checks.assert_built_into_both("rg_ddpg.hip", header="rg_ddpg.h")


# ---- BatchedDDPGAgent's argument checks -----------------------------------------------------------------------------------

def _host_agent(B=4):
    return BatchedDDPGAgent(B, 4, device="cpu", minibatch=5, **LOPSIDED)


def test_agent_initialises_like_keras_and_hard_copies_the_targets():
    a = _host_agent()
    for which in ("actor", "critic"):
        for (W, b), (i, o, _, _) in zip(a.layers(which), a.layout[which]):
            limit = math.sqrt(6.0 / (i + o))
            assert tuple(W.shape) == (i, o) and float(W.abs().max()) <= limit and float(W.abs().max()) > 0 and float(b.abs().max()) == 0.0
    assert torch.equal(a.actor_params, a.target_actor_params) and torch.equal(a.critic_params, a.target_critic_params)
    assert a.actor_params.data_ptr() != a.target_actor_params.data_ptr()
    assert a.act_state[0].tolist() == [0, 1, 2, 3] and a.ring_state.tolist() == [0, 0, 0, 0] and a.steps.tolist() == [0, 0]
    assert a.opt_state.numel() * 8 == a._handle.opt_state_bytes and a.workspace.numel() * 8 == a._handle.workspace_bytes
    other = BatchedDDPGAgent(4, 4, device="cpu", minibatch=5, seed=1, **LOPSIDED)
    assert not torch.equal(a.actor_params, other.actor_params)
    assert a.stats_dict() == dict.fromkeys(ddpg_abi.STAT_NAMES, 0.0)


def test_agent_rejects_a_tensor_it_must_not_follow():
    a = _host_agent()
    f = dict(dtype=torch.float32)
    obs, action, reward, done = torch.zeros(6, 4, **f), torch.zeros(4, 3, **f), torch.zeros(4, **f), torch.zeros(4, dtype=torch.int32)
    for call in (lambda: a.act(obs), lambda: a.act(obs, noise=False), lambda: a.store(obs, action, reward, done), lambda: a.update(2), a.sample,
                 a.critic_grad, a.actor_grad, lambda: a.adam("actor"), lambda: a.soft_update("critic"), a.advance):
        with pytest.raises(ddpg_abi.RgDdpgError) as e:     # every check passes; the host-only handle then has no device
            call()
        assert e.value.status == -3
    calls = []
    for name in ("act", "store", "update", "sample", "critic_grad", "actor_grad", "adam", "soft_update"):
        setattr(a._handle, name, lambda *args, _n=name: calls.append(_n))     # no library call may happen below
    with pytest.raises(ValueError, match="act: obs must be a contiguous float32"):
        a.act(torch.zeros(4, 6, **f).t())
    with pytest.raises(ValueError, match="act: obs"):
        a.act(obs.double())
    with pytest.raises(ValueError, match=r"out\['action'\]"):
        a.act(obs, out=dict(action=torch.zeros(4, 2, **f)))
    with pytest.raises(TypeError, match="unknown output"):
        a.act(obs, out=dict(value=reward))
    with pytest.raises(ValueError, match="store: done must be a contiguous int32"):
        a.store(obs, action, reward, done.long())
    with pytest.raises(ValueError, match="store: reward"):
        a.store(obs, action, torch.zeros(5, **f), done)
    with pytest.raises(ValueError, match="store: action"):
        a.store(obs, None, reward, done)
    with pytest.raises(ValueError, match="idx must be a contiguous int32"):
        a.critic_grad(idx=torch.zeros(5, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be"):
        a.actor_grad(out=torch.zeros(3))
    with pytest.raises(ValueError, match="which"):
        a.adam("both")
    with pytest.raises(ValueError, match="which"):
        a.soft_update(2)
    keep = a.ring_done
    a.ring_done = keep.long()
    with pytest.raises(ValueError, match="update: ring_done must be a contiguous int32"):
        a.update()
    a.ring_done = keep
    assert calls == [] and a.ticks_stored == 0


def test_agent_state_loads_in_place_and_clone_copies_it():
    a = _host_agent()
    a.ring_state[:3] = torch.tensor([2, 4, 9])
    a.steps[0], a.steps[1] = 7, 9
    a.moments[:3] = torch.tensor([1.0, 2.0, 3.0])
    a.ou_state.fill_(0.25)
    a.ticks_stored = 6
    raw = a.opt_state.numpy().view(np.uint8)
    assert np.frombuffer(raw[:16].tobytes(), dtype=np.int64).tolist() == [7, 9]
    assert np.frombuffer(raw[16:28].tobytes(), dtype=np.float32).tolist() == [1.0, 2.0, 3.0]
    state = a.state_dict()
    ptrs = {name: getattr(a, name).data_ptr() for name in a._STATE}
    a.opt_state.zero_(), a.ring_state.zero_(), a.actor_params.zero_()
    a.ticks_stored = 0
    a.load_state_dict(state)
    assert {name: getattr(a, name).data_ptr() for name in a._STATE} == ptrs
    assert a.steps.tolist() == [7, 9] and a.ring_state.tolist() == [2, 4, 9, 0] and a.ticks_stored == 6 and float(a.actor_params.abs().max()) > 0
    twin = a.clone()
    assert all(torch.equal(getattr(a, name), getattr(twin, name)) and getattr(a, name).data_ptr() != getattr(twin, name).data_ptr() for name in a._STATE)
    assert twin.ticks_stored == 6 and twin.fields == a.fields
    with pytest.raises(ValueError, match="another configuration"):
        a.load_state_dict(dict(state, fields=dict(state["fields"], tau=0.5)))
    with pytest.raises(ValueError, match="another configuration"):
        a.load_state_dict(dict(state, batch=5))
    with pytest.raises(ValueError, match="opt_state"):
        a.load_state_dict(dict(state, opt_state=state["opt_state"].float()))
    a.close(), twin.close()


def test_collect_needs_auto_reset_and_the_agents_batch():
    a = _host_agent()

    class Env:
        auto_reset, batch = False, 4

    with pytest.raises(ValueError, match="auto_reset"):
        collect(Env(), a, 3)
    Env.auto_reset, Env.batch = True, 5
    with pytest.raises(ValueError, match="batch"):
        collect(Env(), a, 3)
