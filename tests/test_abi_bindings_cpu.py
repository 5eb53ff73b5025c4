"""What the ctypes shims of robot_gym_amd/core (mpc, srb, goto, episode, posctl, policy, ppo, ddpg, rnn) declare, build and
raise, without a GPU, against tests/golden/abi_bindings.json: per module the restype and argtypes of every export, the layout
of every Structure, the upper-case constants, the bytes of make_cconfig, the type and text of the Python-side exceptions,
create_status and, where the unit has one, a host-only handle.

The golden file was recorded from a checkout of the commit BEFORE the shims moved onto core/c_abi.py -- never from the code
under test -- with the library of this tree (the move touched no compiled source):
    RG_MPC_LIB=<this tree>/robot_gym_amd/csrc/librg_mpc.so python tests/test_abi_bindings_cpu.py <out.json> <that checkout>
Only names both sides have are used.  A text that changes on purpose is changed in the golden file by hand.

Left out: whatever depends on the machine -- LIB_PATH, a valid create of rg_srb or rg_posctl (it goes on to look for a device;
rg_mpc has no create_status), and the handles' "no GPU" texts where there is a GPU.

The one GPU test creates every handle on each spelling of device 0 and launches nothing."""
import ctypes as C
import importlib
import json
import os
import sys

import pytest

ROOT = os.path.abspath(sys.argv[2]) if __name__ == "__main__" else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.core.posctl_config import PosCtlConfig  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_bindings.json")
UNITS = ("mpc", "srb", "goto", "episode", "posctl", "policy", "ppo", "ddpg", "rnn")
HOST_ONLY = ("goto", "episode", "policy", "ppo", "ddpg", "rnn")       # the units whose create takes DEVICE_NONE
ERRORS = dict(mpc="RgMpcError", srb="RgSrbError", goto="RgGotoError", episode="RgEpisodeError", posctl="RgPosCtlError", policy="RgPolicyError",
              ppo="RgPpoError", ddpg="RgDdpgError", rnn="RgRnnError")
HANDLES = dict(mpc="MpcHandle", srb="SrbHandle", goto="GotoHandle", episode="EpisodeHandle", posctl="PosCtlHandle", policy="PolicyHandle",
               ppo="PpoHandle", ddpg="DdpgHandle", rnn="RnnHandle")
MODS = {u: importlib.import_module(f"robot_gym_amd.core.{u}_abi") for u in UNITS}


def _plain(x):
    """x as json gives it back: tuples as lists, every key a string."""
    return json.loads(json.dumps(x))


def _type_name(t):
    """A ctypes type by name; a pointer or an array by its target's module and class name."""
    if t is None:
        return "None"
    target = getattr(t, "_type_", None)
    if isinstance(target, type):
        of = f"{target.__module__}.{target.__name__}" if not hasattr(target, "_length_") else _type_name(target)
        return f"{of}[{t._length_}]" if hasattr(t, "_length_") else f"POINTER({of})"
    return t.__name__


def _described(e):
    return [type(e).__name__, str(e), getattr(e, "status", None)]


def _raised(call):
    """[type name, text, status or None] of the exception `call` raises."""
    try:
        got = call()
    except Exception as e:   # noqa: BLE001 -- the type is what is recorded
        return _described(e)
    return ["nothing raised", repr(got), None]


def _declarations(unit, m):
    lib = m.load_library()
    names = m.EXPORTS + getattr(m, "TERRAIN_EXPORTS", ()) + getattr(m, "CONTACT_EXPORTS", ())
    return {n: {"restype": _type_name(getattr(lib, n).restype), "argtypes": [_type_name(a) for a in getattr(lib, n).argtypes or []]} for n in names}


def _structures(unit, m):
    out = {}
    for name, s in vars(m).items():
        if isinstance(s, type) and issubclass(s, C.Structure) and s.__module__ == m.__name__:
            out[name] = {"sizeof": C.sizeof(s), "fields": [[f, getattr(s, f).offset, getattr(s, f).size] for f, _ in s._fields_]}
    return out


def _constants(unit, m):
    """Every public upper-case int, float, str, tuple or dict of plain values (a table of ctypes types is no constant)."""
    out = {}
    for k, v in vars(m).items():
        if k.isupper() and not k.startswith("_") and k != "LIB_PATH" and isinstance(v, (int, float, str, tuple, dict)):
            try:
                out[k] = _plain(v)
            except TypeError:
                pass
    return out


def _mpc(robot, **changes):
    return MPCConfig.for_robot(robot, **{"lane_grid": 0, **changes})      # the recorded bytes are those of the library's own lane grid


def _configs(unit, m):
    """{case: () -> CConfig}: the defaults, both robots where the unit reads one, and off-default integer and array fields."""
    if unit == "mpc":
        return {"ghost": lambda: m.make_cconfig(_mpc("ghost")), "k3lso": lambda: m.make_cconfig(_mpc("k3lso")),
                "integer horizon, window": lambda: m.make_cconfig(_mpc("ghost", horizon=7, window=11)),
                "array weights, init_state": lambda: m.make_cconfig(_mpc("k3lso", weights=tuple(range(1, 14)), init_state=(1, 0, 0, 1)))}
    if unit == "srb":
        return {"ghost": lambda: m.make_cconfig(_mpc("ghost")), "k3lso": lambda: m.make_cconfig(_mpc("k3lso")),
                "integer substeps": lambda: m.make_cconfig(_mpc("ghost"), substeps=7, dt_sim=0.002),
                "array init_q": lambda: m.make_cconfig(_mpc("k3lso"), init_q=[0.1 * k for k in range(12)], fall_tilt=0.5)}
    if unit == "goto":
        return {"defaults": lambda: m.make_cconfig(), "ghost": lambda: m.make_cconfig(_mpc("ghost")), "k3lso": lambda: m.make_cconfig(_mpc("k3lso")),
                "integer n_max, num_cam_pts": lambda: m.make_cconfig(_mpc("ghost"), n_max=33, num_cam_pts=5, max_time=12.5),
                "array action_low, cmd_offset": lambda: m.make_cconfig(_mpc("k3lso"), action_low=(0.1, -0.2), cmd_offset=[1, 2, 3])}
    if unit == "episode":
        return {"defaults": lambda: m.make_cconfig(), "integer seed, max_waypoints": lambda: m.make_cconfig(seed=(1 << 40) + 5, max_waypoints=9, kp=2.5),
                "array obstacles": lambda: m.make_cconfig([(1, 2), (3.5, -4)], grid=0.25), "obstacles None": lambda: m.make_cconfig(None)}
    if unit == "posctl":
        return {"defaults": lambda: m.make_cconfig(PosCtlConfig()), "ghost": lambda: m.make_cconfig(PosCtlConfig.for_robot("ghost")),
                "integer-valued leg": lambda: m.make_cconfig(PosCtlConfig.for_robot("ghost", leg=1, step_offset=0.25)),
                "array leg_offset": lambda: m.make_cconfig(PosCtlConfig.for_robot("ghost", leg_offset=[0.1, 0.2, 0.3, 0.4]))}
    if unit == "policy":
        return {"defaults": lambda: m.make_cconfig(), "integer obs_dim, seed": lambda: m.make_cconfig(obs_dim=5, act_dim=3, seed=(1 << 33) + 1, discount=0.9),
                "array policy_layers": lambda: m.make_cconfig(policy_layers=(7,), value_layers=[3, 4, 5])}
    if unit == "ppo":
        return {"defaults": lambda: m.make_cconfig(), "integer epochs": lambda: m.make_cconfig(epochs_policy=3, epochs_value=0, policy_lr=1),
                "conv_logpdf reference": lambda: m.make_cconfig(conv_logpdf="reference", kl_target=0.5)}
    if unit == "ddpg":
        return {"defaults": lambda: m.make_cconfig(), "integer capacity, window": lambda: m.make_cconfig(capacity=64, window=2, minibatch=8, seed=9, tau=1),
                "array actor_layers": lambda: m.make_cconfig(actor_layers=(5, 6), critic_layers=[])}
    return {"defaults": lambda: m.make_cconfig(), "integer gru_units": lambda: m.make_cconfig(gru_units=17.0, obs_dim=3, seed=4, obs_clip=2),
            "array policy_layers": lambda: m.make_cconfig(policy_layers=(), value_layers=[9])}


def _config_bytes(unit, m):
    return {name: bytes(make()).hex() for name, make in _configs(unit, m).items()}


def _handle(unit, m, batch, device):
    """The unit's handle at `batch` (ppo: T and B) on `device`, default settings."""
    H = getattr(m, HANDLES[unit])
    if unit == "mpc":
        return H(_mpc("ghost"), batch, device)
    if unit == "srb":
        return H(_mpc("ghost"), batch, device)
    if unit == "posctl":
        return H(PosCtlConfig.for_robot("ghost"), batch, device)
    if unit == "goto":
        return H(batch, _mpc("ghost"), device)
    if unit == "episode":
        return H(batch, _mpc("ghost"), device)
    if unit == "ppo":
        return H(batch, batch, device)
    return H(batch, device)


def _exceptions(unit, m):
    E = getattr(m, ERRORS[unit])
    out = {"load_library of a missing file": _raised(lambda: m.load_library("/nonexistent/librg_mpc.so")),
           "error -1": _described(E(-1, "x")), "error -9": _described(E(-9, "x"))}
    unknown = dict(srb=lambda: m.make_cconfig(_mpc("ghost"), bogus=1, also=2), goto=lambda: m.make_cconfig(_mpc("ghost"), bogus=1, also=2),
                   episode=lambda: m.make_cconfig((), bogus=1, also=2))
    if unit in ("policy", "ppo", "ddpg", "rnn"):
        unknown[unit] = lambda: m.make_cconfig(bogus=1, also=2)
    if unit in unknown:
        out["unknown setting"] = _raised(unknown[unit])
    if unit == "srb":
        out["unknown setting next to init_q"] = _raised(lambda: m.sim_fields(_mpc("ghost"), init_q=None, bogus=1))
    layers = dict(policy=("policy_layers", "value_layers"), ddpg=("actor_layers", "critic_layers"), rnn=("policy_layers", "value_layers"))
    for name in layers.get(unit, ()):
        out[f"too many {name}"] = _raised(lambda name=name: m.make_cconfig(**{name: (8,) * 4}))
    if unit == "ppo":
        out["bad conv_logpdf"] = _raised(lambda: m.make_cconfig(conv_logpdf="neither"))
    wrong = dict(mpc=lambda: m.make_cconfig(_mpc("ghost", weights=(1.0,) * 12)), srb=lambda: m.make_cconfig(_mpc("ghost"), init_q=(0.0,) * 11),
                 goto=lambda: m.make_cconfig(action_low=(1, 2, 3)), posctl=lambda: m.make_cconfig(PosCtlConfig.for_robot("ghost", leg_offset=(0.0,) * 3)))
    if unit in wrong:
        out["array of the wrong length"] = _raised(wrong[unit])
    if unit == "srb":
        out["MPCConfig array of the wrong length"] = _raised(lambda: m.make_cconfig(_mpc("ghost", hip=(0.0,) * 13)))
    if unit == "episode":
        out["too many obstacles"] = _raised(lambda: m.make_cconfig([(k, k) for k in range(17)]))
    import torch
    if unit != "mpc" and not torch.cuda.is_available():     # MpcHandle takes an index and leaves the look for a device to the library
        out["no GPU"] = _raised(lambda: _handle(unit, m, 4, None))
    return out


def _create_status(unit, m):
    mpc = _mpc("ghost")
    if unit == "mpc":
        return {}
    if unit in ("srb", "posctl"):     # a valid create goes on to look for a device
        cfg = mpc if unit == "srb" else PosCtlConfig.for_robot("ghost")
        return {"batch zero": _plain(m.create_status(cfg, 0)), "built config, batch zero": _plain(m.create_status(m.make_cconfig(cfg), 0))}
    if unit == "goto":
        return {"defaults": _plain(m.create_status(None, 4, m.DEVICE_NONE)), "MPCConfig and a setting": _plain(m.create_status(mpc, 4, m.DEVICE_NONE, n_max=16)),
                "n_max 1": _plain(m.create_status(mpc, 4, m.DEVICE_NONE, n_max=1)), "built config, batch zero": _plain(m.create_status(m.make_cconfig(mpc), 0, m.DEVICE_NONE))}
    if unit == "episode":
        return {"defaults": _plain(m.create_status()), "grid -1": _plain(m.create_status(m.make_cconfig(grid=-1.0), batch=4, mpc_cfg=mpc))}
    if unit == "ppo":
        return {"defaults": _plain(m.create_status()), "T zero": _plain(m.create_status(T=0)), "beta1 1": _plain(m.create_status(ppo_cconfig=m.make_cconfig(beta1=1.0)))}
    bad = dict(policy=dict(obs_dim=65), ddpg=dict(window=9), rnn=dict(gru_units=129))[unit]
    return {"defaults": _plain(m.create_status()), "batch zero": _plain(m.create_status(batch=0)), " ".join(f"{k} {v}" for k, v in bad.items()): _plain(m.create_status(m.make_cconfig(**bad)))}


def _host_only(unit, m):
    """The host-only handle at batch 4: its attributes, one entry with every pointer NULL through the handle, close twice."""
    if unit not in HOST_ONLY:
        return {}
    h = _handle(unit, m, 4, m.DEVICE_NONE)
    names = ("batch", "T", "B", "n_max", "device", "fields", "layout", "workspace_bytes", "opt_state_bytes", "groups", "lds_bytes", "scalars_offset")
    out = {"attributes": {n: _plain(getattr(h, n)) for n in names if hasattr(h, n)}}
    null_call = dict(goto=lambda: h.pre_step(None, None, m.CPathPtrs(), None, None), episode=lambda: h.accumulate(None, None, None),
                     policy=lambda: h.act(None, None, None, None, None, 0, None), ppo=lambda: h.prepare(m.make_crollout(), None),
                     ddpg=lambda: h.sample(m.make_cring(), None), rnn=lambda: h.unroll(None, None, None, None, None, 4, None))
    out["entry with every pointer NULL"] = _raised(null_call[unit])
    out["stream of a host-only handle"] = _plain(h._s())
    h.close()
    h.close()
    out["handle after close twice"] = bool(h._h)
    return out


SECTIONS = dict(declarations=_declarations, structures=_structures, constants=_constants, config_bytes=_config_bytes, exceptions=_exceptions,
                create_status=_create_status, host_only=_host_only)


def record():
    assert all(os.path.dirname(m.__file__) == os.path.join(ROOT, "robot_gym_amd", "core") for m in MODS.values())
    return {unit: {name: part(unit, MODS[unit]) for name, part in SECTIONS.items()} for unit in UNITS}


def _recorded():
    with open(GOLDEN) as f:
        return json.load(f)


EXPECTED = {} if __name__ == "__main__" else _recorded()


def test_the_recording_covers_every_shim_and_section():
    assert sorted(EXPECTED) == sorted(UNITS)
    for unit in UNITS:
        assert sorted(EXPECTED[unit]) == sorted(SECTIONS), unit
        e = EXPECTED[unit]
        assert len(e["declarations"]) >= len(MODS[unit].EXPORTS) and "CConfig" in e["structures"] and "ABI_VERSION" in e["constants"], unit
        assert len(set(e["config_bytes"].values())) >= 3, unit      # the defaults and two settings that tell themselves apart
        assert bool(e["host_only"]) == (unit in HOST_ONLY) and {"error -1", "error -9", "load_library of a missing file"} <= set(e["exceptions"]), unit
        assert ("no GPU" in e["exceptions"]) == (unit != "mpc"), unit


@pytest.mark.parametrize("section", sorted(SECTIONS))
@pytest.mark.parametrize("unit", UNITS)
def test_binding_is_the_recorded_one(unit, section):
    got, want = SECTIONS[section](unit, MODS[unit]), dict(EXPECTED[unit][section])
    if "no GPU" not in got:          # a machine with a GPU: the handle is created instead
        want.pop("no GPU", None)
    if section == "constants":       # a constant the recording does not have is none of its business; one it has must be there
        assert set(want) <= set(got), sorted(set(want) - set(got))
    else:
        assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], f"{unit} {section}: {key}"


def _device_spellings(unit):
    import torch
    return (0,) if unit == "mpc" else (None, "cuda", "cuda:0", torch.device("cuda", 0), 0)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", UNITS)
def test_every_spelling_of_device_0_gives_a_handle_on_it(unit):
    """Batch 1 (ppo: T 1, B 1), the smallest every create accepts; with the current device 0, None and "cuda" are device 0
    too.  MpcHandle takes an index only and keeps it.  Nothing is launched."""
    import torch
    assert torch.cuda.current_device() == 0
    for device in _device_spellings(unit):
        h = _handle(unit, MODS[unit], 1, device)
        try:
            assert h._h, device
            if unit == "mpc":
                assert h.device == 0 and isinstance(h.device, int)
            else:
                assert h.device == torch.device("cuda", 0), device
        finally:
            h.close()
        assert not h._h


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, indent=1, sort_keys=True)
        f.write("\n")
