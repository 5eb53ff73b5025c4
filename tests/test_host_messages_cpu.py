"""The text of every error the host side of librg_mpc.so forms from shared helpers (robot_gym_amd/csrc/rg_host.h), byte for
byte, without a GPU: the status and the full rg_*_last_error text of each case below against tests/golden/host_messages.json.

The golden file was recorded from a build of the commit BEFORE the simulator, the task, the episode reset and the position-mode
controllers moved onto rg_host.h -- never from the code under test:
    RG_MPC_LIB=<that build>/librg_mpc.so python tests/test_host_messages_cpu.py <out.json>
A message that changes on purpose is changed in the golden file by hand, with the change to the library that rewords it.

Left out: whatever depends on the machine -- a valid create of rg_srb or rg_posctl (it goes on to look for a device) and any
hipGetErrorString text.  The creates of rg_goto, rg_episode and the agents run with their DEVICE_NONE."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from robot_gym_amd.core import ddpg_abi, episode_abi, goto_abi, policy_abi, posctl_abi, ppo_abi, rnn_abi, srb_abi  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.core.posctl_config import PosCtlConfig  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "host_messages.json")
NAN, INF = float("nan"), float("inf")
BIG = (1 << 24) + 1      # one above every RG_*_MAX_BATCH
NONE = -1                # every RG_*_DEVICE_NONE


def _changed(make, changes):
    """make() with each (field, index or None, value) of `changes` written into the structure."""
    c = make()
    for field, index, value in changes:
        if index is None:
            setattr(c, field, value)
        elif isinstance(index, tuple):
            getattr(c, field)[index[0]][index[1]] = value
        else:
            getattr(c, field)[index] = value
    return c


def _config_cases(make, scalars_positive, scalar_finite, array, ints, own, two_faults, reserved=("reserved0",)):
    """{name: (changes, batch)}: the cases every validator shares, by its own fields, then its own checks."""
    out = {"abi_version": ([("abi_version", None, 99)], 4), "batch zero": ([], 0), "batch above the maximum": ([], BIG)}
    for r in reserved:
        out[r] = ([(r, None, 7)], 4)
    for v in (NAN, INF, 0.0, -1.5):
        out[f"positive scalar {scalars_positive} = {v}"] = ([(scalars_positive, None, v)], 4)
    for v in (NAN, INF, -INF):
        out[f"finite scalar {scalar_finite} = {v}"] = ([(scalar_finite, None, v)], 4)
    for field, index, v in array:
        out[f"array {field}[{index}] = {v}"] = ([(field, index, v)], 4)
    for field, below, above in ints:
        out[f"integer {field} = {below}"] = ([(field, None, below)], 4)
        out[f"integer {field} = {above}"] = ([(field, None, above)], 4)
    for name, changes in own.items():
        out[name] = (changes, 4)
    for name, changes in two_faults.items():
        out["two faults: " + name] = (changes, 4)
    return {k: (lambda ch=ch, b=b: (_changed(make, ch), b)) for k, (ch, b) in out.items()}


def _srb_cases():
    mpc = MPCConfig.for_robot("ghost")
    skew = [("inertia", 1, 0.01)]
    return _config_cases(
        lambda: srb_abi.make_cconfig(mpc), "mass", "ik_damping",
        [("hip", 5, NAN), ("jxyz", 35, INF), ("inertia", 8, NAN), ("init_q", 11, -INF)],
        [("ik_iters", 0, 65), ("substeps", 0, 1025)],
        {"inertia beyond 1e300": [("inertia", 0, 1e301)], "inertia not symmetric": skew,
         "inertia not positive definite": [("inertia", 0, -1.0)], "motor_dir not +-1": [("motor_dir", 3, 0.5)],
         "jaxis zero": [("jaxis", 3, 0.0), ("jaxis", 4, 0.0), ("jaxis", 5, 0.0)], "ik_damping negative": [("ik_damping", None, -1.0)],
         "fall_height_scale one": [("fall_height_scale", None, 1.0)], "fall_height_scale negative": [("fall_height_scale", None, -0.5)],
         "fall_height_scale nan": [("fall_height_scale", None, NAN)], "fall_tilt zero": [("fall_tilt", None, 0.0)],
         "fall_tilt above pi": [("fall_tilt", None, 4.0)], "gravity negative": [("gravity", None, -9.81)], "dt_sim zero": [("dt_sim", None, 0.0)]},
        {"mass and fall_tilt": [("mass", None, NAN), ("fall_tilt", None, NAN)], "abi_version and reserved0": [("abi_version", None, 0), ("reserved0", None, 1)],
         "jrpy[2] and jrpy[1]": [("jrpy", 2, NAN), ("jrpy", 1, INF)], "substeps and motor_dir": [("substeps", None, 0), ("motor_dir", 0, 2.0)]})


def _posctl_cases():
    return _config_cases(
        lambda: posctl_abi.make_cconfig(PosCtlConfig.for_robot("ghost")), "hip", "step_offset",
        [("hip_v", 7, NAN), ("leg_offset", 3, INF), ("motor_kd", 11, -INF)], [],
        {"step_offset zero": [("step_offset", None, 0.0)], "step_offset one": [("step_offset", None, 1.0)],
         "step_offset above one": [("step_offset", None, 1.5)], "step_offset negative": [("step_offset", None, -0.25)],
         "leg negative": [("leg", None, -0.2)], "foot zero": [("foot", None, 0.0)]},
        {"hip and motor_kd": [("hip", None, NAN), ("motor_kd", 11, NAN)], "reserved0 and foot": [("reserved0", None, -1), ("foot", None, INF)]})


def _goto_cases(make=goto_abi.make_cconfig):
    return _config_cases(
        make, "window_height", "window_distance",
        [("action_high", 1, NAN), ("cmd_offset", 2, INF), ("action_low", 1, -INF)],
        [("substeps", 0, 1025), ("num_cam_pts", 0, 17), ("num_checkpoints", 0, 65537), ("n_max", 1, 65537), ("max_visible", 1, 129)],
        {"action_low above action_high": [("action_low", 1, 0.5)], "time_penalty nan": [("time_penalty", None, NAN)],
         "checkpoint_reward_total inf": [("checkpoint_reward_total", None, INF)], "dt_sim negative": [("dt_sim", None, -0.001)],
         "continuity_break zero": [("continuity_break", None, 0.0)]},
        {"window_height and max_visible": [("window_height", None, NAN), ("max_visible", None, 0)],
         "reserved0 and reserved1": [("reserved0", None, 3), ("reserved1", None, 4)],
         "action_low above action_high and n_max": [("action_low", 0, 9.0), ("n_max", None, 0)]},
        reserved=("reserved0", "reserved1"))


def _episode_cases():
    return _config_cases(
        lambda: episode_abi.make_cconfig([(1.0, 1.0), (-1.0, 0.5)]), "kp", "eta",
        [("obstacles", (3, 1), NAN), ("obstacles", (15, 0), INF), ("obstacles", (0, 1), -INF)],
        [("oscillation_length", 0, 9), ("max_waypoints", 1, 65), ("num_obstacles", -1, 17)],
        {"eta negative": [("eta", None, -1.0)], "spacing zero": [("spacing", None, 0.0)], "grid nan": [("grid", None, NAN)]},
        {"kp and obstacles": [("kp", None, NAN), ("obstacles", (0, 0), NAN)], "eta negative and max_waypoints": [("eta", None, -2.0), ("max_waypoints", None, 0)],
         "reserved1 and spacing": [("reserved1", None, 1), ("spacing", None, -1.0)]},
        reserved=("reserved0", "reserved1"))


def _create_cases():
    """{id: () -> (status, text)} of the creates of the four environment APIs."""
    out = {}
    mpc = MPCConfig.for_robot("ghost")
    for api, cases, create in (("srb", _srb_cases(), lambda c, b: srb_abi.create_status(c, b)),
                               ("posctl", _posctl_cases(), lambda c, b: posctl_abi.create_status(c, b)),
                               ("goto", _goto_cases(), lambda c, b: goto_abi.create_status(c, b, NONE)),
                               ("episode", _episode_cases(), lambda c, b: episode_abi.create_status(c, batch=b, mpc_cfg=mpc))):
        for name, make in cases.items():
            out[f"{api} create: {name}"] = lambda make=make, create=create: create(*make())
    # the terrain's check forms its version text with the same helper, under its own prefix
    out["srb terrain_check: abi_version"] = lambda: srb_abi.terrain_check(_changed(srb_abi.make_cterrain, [("abi_version", None, 7)]))
    out["srb terrain_check: two faults: abi_version and kind"] = lambda: srb_abi.terrain_check(
        _changed(srb_abi.make_cterrain, [("abi_version", None, 0), ("kind", None, 5)]))
    # the episode's create checks the simulator's and the task's configuration after its own, under a prefix
    bad_s = lambda: _changed(lambda: srb_abi.make_cconfig(mpc), [("mass", None, 0.0)])
    bad_g = lambda: _changed(lambda: goto_abi.make_cconfig(mpc), [("n_max", None, 1)])
    bad_e = lambda: _changed(episode_abi.make_cconfig, [("grid", None, -1.0)])
    out["episode create: simulator config"] = lambda: episode_abi.create_status(scfg=bad_s(), batch=4, mpc_cfg=mpc)
    out["episode create: simulator config array"] = lambda: episode_abi.create_status(
        scfg=_changed(lambda: srb_abi.make_cconfig(mpc), [("toe_com", 4, NAN)]), batch=4, mpc_cfg=mpc)
    out["episode create: task config"] = lambda: episode_abi.create_status(gcfg=bad_g(), batch=4, mpc_cfg=mpc)
    out["episode create: task config abi_version"] = lambda: episode_abi.create_status(
        gcfg=_changed(lambda: goto_abi.make_cconfig(mpc), [("abi_version", None, 2)]), batch=4, mpc_cfg=mpc)
    out["episode create: two faults: simulator and task config"] = lambda: episode_abi.create_status(scfg=bad_s(), gcfg=bad_g(), batch=4, mpc_cfg=mpc)
    out["episode create: two faults: own and simulator config"] = lambda: episode_abi.create_status(ecfg=bad_e(), scfg=bad_s(), batch=4, mpc_cfg=mpc)
    out["episode create: two faults: batch and own config"] = lambda: episode_abi.create_status(ecfg=bad_e(), batch=0, mpc_cfg=mpc)
    return out


def _null_each(out, prefix, fn, handle, last, good, names):
    """One case per named argument of `good` set to NULL, the NULL handle, and the fully valid call."""
    for k, name in enumerate(names):
        if name is None:
            continue
        a = list(good)
        a[k] = None
        out[f"{prefix}: null {name}"] = lambda a=a: (fn(handle, *a, None), last(handle))
    out[f"{prefix}: null handle"] = lambda: (fn(None, *good, None), last(None))
    out[f"{prefix}: valid"] = lambda: (fn(handle, *good, None), last(handle))


def _holed(out, prefix, struct, fields, call):
    """One case per member of the pointer structure set to NULL; call(byref of the structure) -> (status, text)."""
    p = _DUMMY.ctypes.data
    for k, name in enumerate(fields):
        members = [p] * len(fields)
        members[k] = None
        s = struct(*members)
        out[f"{prefix}.{name} null"] = lambda s=s: call(C.byref(s))


_DUMMY = np.zeros(16)     # stands for device memory: a host-only handle never follows these pointers
_KEEP = []                # the handles and host arrays the cases point into


def _goto_handle_cases():
    B, n_max = 4, 16
    lib = goto_abi.load_library()
    h = goto_abi.GotoHandle(B, None, goto_abi.DEVICE_NONE, n_max=n_max)
    _KEEP.append(h)
    last = lambda hh: lib.rg_goto_last_error(hh).decode()
    p = _DUMMY.ctypes.data
    ptrs = goto_abi.CPathPtrs(*([p] * 5))
    t = np.linspace(0.0, 1.0, n_max)
    rows = dict(npts=np.full(B, n_max, np.int32), length=np.ones(B), target=np.ones((2, B)), x=np.tile(t, (B, 1)), y=np.zeros((B, n_max)),
                s=np.tile(t, (B, 1)), first_same_x=np.tile(np.arange(n_max, dtype=np.int32), (B, 1)))
    rows = {k: np.ascontiguousarray(v) for k, v in rows.items()}
    _KEEP.append(rows)
    host = [rows[k].ctypes.data for k in ("npts", "length", "target", "x", "y", "s", "first_same_x")]
    out = {}
    set_path = lambda hh, *a: lib.rg_goto_set_path(hh, None, B, *a)
    _null_each(out, "goto set_path", set_path, h._h, last, host + [C.byref(ptrs), p],
               ("npts", "length", "target", "x", "y", "s", "first_same_x", "paths", "task_state"))
    _null_each(out, "goto pre_step", lib.rg_goto_pre_step, h._h, last, [p, p, C.byref(ptrs), p, p], ("task_state", "sim_state", "paths", "action", "cmd_out"))
    _null_each(out, "goto post_step", lib.rg_goto_post_step, h._h, last, [p, p, C.byref(ptrs), p, p, p],
               ("task_state", "sim_state", "paths", "obs", "reward", "done"))
    _null_each(out, "goto observe", lib.rg_goto_observe, h._h, last, [p, p, C.byref(ptrs), p], ("task_state", "sim_state", "paths", "obs"))
    _holed(out, "goto set_path: paths", goto_abi.CPathPtrs, goto_abi.PATH_FIELDS,
           lambda s: (lib.rg_goto_set_path(h._h, None, B, *host, s, p, None), last(h._h)))
    _holed(out, "goto pre_step: paths", goto_abi.CPathPtrs, goto_abi.PATH_FIELDS, lambda s: (lib.rg_goto_pre_step(h._h, p, p, s, p, p, None), last(h._h)))
    _holed(out, "goto post_step: paths", goto_abi.CPathPtrs, goto_abi.PATH_FIELDS, lambda s: (lib.rg_goto_post_step(h._h, p, p, s, p, p, p, None), last(h._h)))
    _holed(out, "goto observe: paths", goto_abi.CPathPtrs, goto_abi.PATH_FIELDS, lambda s: (lib.rg_goto_observe(h._h, p, p, s, p, None), last(h._h)))
    out["goto post_step: two faults: null sim_state and null obs"] = lambda: (lib.rg_goto_post_step(h._h, p, None, C.byref(ptrs), None, p, p, None), last(h._h))
    out["goto set_path: n is not the batch"] = lambda: (lib.rg_goto_set_path(h._h, None, B - 1, *host, C.byref(ptrs), p, None), last(h._h))
    return out


def _episode_handle_cases():
    lib = episode_abi.load_library()
    h = episode_abi.EpisodeHandle(4, MPCConfig.for_robot("ghost"), episode_abi.DEVICE_NONE, obstacles=[(1, 1)], seed=3)
    _KEEP.append(h)
    last = lambda hh: lib.rg_episode_last_error(hh).decode()
    p, q = _DUMMY.ctypes.data, _DUMMY.ctypes.data + 8
    so, pp = srb_abi.CObsPtrs(*([p] * 9)), goto_abi.CPathPtrs(*([p] * 5))
    good = [p, p, p, p, p, C.byref(so), C.byref(pp), p, p, q]
    out = {}
    _null_each(out, "episode reset", lib.rg_episode_reset, h._h, last, good,
               ("mask", None, "episode_state", "task_state", "sim_state", "sim_obs", "paths", "obs", "final_obs", "reset_mask_out"))
    _null_each(out, "episode accumulate", lib.rg_episode_accumulate, h._h, last, [p, p, p], ("episode_state", "reward", "done"))
    reset_with = lambda k: lambda s: (lib.rg_episode_reset(h._h, *(good[:k] + [s] + good[k + 1:]), None), last(h._h))
    _holed(out, "episode reset: sim_obs", srb_abi.CObsPtrs, srb_abi.OBS_FIELDS, reset_with(5))
    _holed(out, "episode reset: paths", goto_abi.CPathPtrs, goto_abi.PATH_FIELDS, reset_with(6))
    out["episode reset: no targets"] = lambda: (lib.rg_episode_reset(h._h, *(good[:1] + [None] + good[2:]), None), last(h._h))
    out["episode reset: reset_mask_out aliases mask"] = lambda: (lib.rg_episode_reset(h._h, *(good[:9] + [p]), None), last(h._h))
    out["episode reset: two faults: null mask and null obs"] = lambda: (lib.rg_episode_reset(h._h, *([None] + good[1:7] + [None] + good[8:]), None), last(h._h))
    return out


def _agent_cases():
    out = {}
    p = _DUMMY.ctypes.data
    # rg_policy
    pol = lambda *ch: _changed(policy_abi.make_cconfig, ch)
    for name, ch in {"real reward_clip": [("reward_clip", None, -1.0)], "real discount": [("discount", None, 1.5)], "real obs_clip": [("obs_clip", None, NAN)],
                     "real gae_lambda": [("gae_lambda", None, INF)], "integer obs_dim": [("obs_dim", None, 65)], "integer act_dim": [("act_dim", None, 0)],
                     "width": [("policy_layers", 1, 257)], "width past the layers in use": [("n_value_layers", None, 1)], "reserved0": [("reserved0", None, 1)],
                     "abi_version": [("abi_version", None, 0)], "two faults: obs_dim and discount": [("obs_dim", None, 0), ("discount", None, NAN)]}.items():
        out[f"policy create: {name}"] = lambda ch=ch: policy_abi.create_status(pol(*ch))
    out["policy create: batch zero"] = lambda: policy_abi.create_status(batch=0)
    out["policy create: batch above the maximum"] = lambda: policy_abi.create_status(batch=BIG)
    lib_p = policy_abi.load_library()
    hp = policy_abi.PolicyHandle(4, policy_abi.DEVICE_NONE, seed=3)
    _KEEP.append(hp)
    out["policy act: valid"] = lambda: (lib_p.rg_policy_act(hp._h, p, p, p, p, p, 0, p, p, p, p, None), lib_p.rg_policy_last_error(hp._h).decode())
    out["policy act: null obs"] = lambda: (lib_p.rg_policy_act(hp._h, None, p, p, p, p, 0, p, p, p, p, None), lib_p.rg_policy_last_error(hp._h).decode())
    # rg_ppo
    ppo = lambda *ch: _changed(ppo_abi.make_cconfig, ch)
    for name, ch in {"real policy_lr": [("policy_lr", None, -1e-4)], "real beta1": [("beta1", None, 1.0)], "real adam_eps": [("adam_eps", None, 0.0)],
                     "real kl_cutoff_coef": [("kl_cutoff_coef", None, NAN)], "integer epochs_policy": [("epochs_policy", None, -1)],
                     "integer conv_logpdf": [("conv_logpdf", None, 7)], "abi_version": [("abi_version", None, 9)],
                     "two faults: epochs_value and value_lr": [("epochs_value", None, -3), ("value_lr", None, INF)]}.items():
        out[f"ppo create: {name}"] = lambda ch=ch: ppo_abi.create_status(ppo_cconfig=ppo(*ch))
    out["ppo create: width"] = lambda: ppo_abi.create_status(policy_cconfig=pol(("value_layers", 0, 0)))
    out["ppo create: policy real obs_clip"] = lambda: ppo_abi.create_status(policy_cconfig=pol(("obs_clip", None, -5.0)))
    out["ppo create: two faults: policy and ppo config"] = lambda: ppo_abi.create_status(policy_cconfig=pol(("act_dim", None, 5)), ppo_cconfig=ppo(("beta2", None, -0.1)))
    lib_u = ppo_abi.load_library()
    hu = ppo_abi.PpoHandle(3, 4, ppo_abi.DEVICE_NONE)
    _KEEP.append(hu)
    roll = ppo_abi.make_crollout(**{s: p for s in ("obs", "action", "mean", "logstd", "adv", "ret", "mask")})
    out["ppo prepare: valid"] = lambda: (lib_u.rg_ppo_prepare(hu._h, C.byref(roll), p, None), lib_u.rg_ppo_last_error(hu._h).decode())
    out["ppo prepare: null workspace"] = lambda: (lib_u.rg_ppo_prepare(hu._h, C.byref(roll), None, None), lib_u.rg_ppo_last_error(hu._h).decode())
    # rg_ddpg
    dd = lambda *ch: _changed(ddpg_abi.make_cconfig, ch)
    for name, ch in {"real gamma": [("gamma", None, 1.01)], "real tau": [("tau", None, 0.0)], "real actor_lr": [("actor_lr", None, -1.0)],
                     "real beta2": [("beta2", None, 1.0)], "real adam_eps": [("adam_eps", None, NAN)], "real ou_mu": [("ou_mu", None, INF)],
                     "real ou_dt": [("ou_dt", None, -0.01)], "integer capacity": [("capacity", None, 1)], "integer window": [("window", None, 9)],
                     "width": [("critic_layers", 2, 300)], "window times obs_dim": [("obs_dim", None, 64), ("window", None, 8)],
                     "abi_version": [("abi_version", None, 0)], "two faults: minibatch and ou_sigma": [("minibatch", None, 0), ("ou_sigma", None, -0.3)],
                     "two faults: gamma and ou_theta": [("gamma", None, NAN), ("ou_theta", None, NAN)]}.items():
        out[f"ddpg create: {name}"] = lambda ch=ch: ddpg_abi.create_status(dd(*ch))
    out["ddpg create: batch zero"] = lambda: ddpg_abi.create_status(batch=0)
    out["ddpg create: two faults: config and batch"] = lambda: ddpg_abi.create_status(dd(("tau", None, 2.0)), batch=0)
    lib_d = ddpg_abi.load_library()
    hd = ddpg_abi.DdpgHandle(4, ddpg_abi.DEVICE_NONE, capacity=4)
    _KEEP.append(hd)
    ring = ddpg_abi.make_cring(**{s: p for s in ("obs", "action", "reward", "done", "state")})
    out["ddpg sample: valid"] = lambda: (lib_d.rg_ddpg_sample(hd._h, C.byref(ring), p, None), lib_d.rg_ddpg_last_error(hd._h).decode())
    out["ddpg sample: null idx_out"] = lambda: (lib_d.rg_ddpg_sample(hd._h, C.byref(ring), None, None), lib_d.rg_ddpg_last_error(hd._h).decode())
    # rg_rnn
    rn = lambda *ch: _changed(rnn_abi.make_cconfig, ch)
    for name, ch in {"real obs_clip": [("obs_clip", None, -0.5)], "real obs_clip nan": [("obs_clip", None, NAN)], "integer gru_units": [("gru_units", None, 129)],
                     "integer n_policy_layers": [("n_policy_layers", None, 3)], "width": [("policy_layers", 0, 0)], "reserved0": [("reserved0", None, 2)],
                     "abi_version": [("abi_version", None, 5)], "two faults: act_dim and obs_clip": [("act_dim", None, 9), ("obs_clip", None, INF)]}.items():
        out[f"rnn create: {name}"] = lambda ch=ch: rnn_abi.create_status(rn(*ch))
    out["rnn create: batch above the maximum"] = lambda: rnn_abi.create_status(batch=BIG)
    out["rnn create: two faults: batch and config"] = lambda: rnn_abi.create_status(rn(("obs_dim", None, 0)), batch=0)
    lib_r = rnn_abi.load_library()
    hr = rnn_abi.RnnHandle(4, rnn_abi.DEVICE_NONE, seed=3)
    _KEEP.append(hr)
    out["rnn act: valid"] = lambda: (lib_r.rg_rnn_act(hr._h, p, p, p, p, p, p, p, p, 0, p, p, p, p, None), lib_r.rg_rnn_last_error(hr._h).decode())
    out["rnn act: null hidden_in"] = lambda: (lib_r.rg_rnn_act(hr._h, p, p, p, p, p, p, None, p, 0, p, p, p, p, None), lib_r.rg_rnn_last_error(hr._h).decode())
    out["rnn unroll: valid"] = lambda: (lib_r.rg_rnn_unroll(hr._h, p, p, p, p, p, 5, p, p, p, None), lib_r.rg_rnn_last_error(hr._h).decode())
    return out


def all_cases():
    out = {}
    for part in (_create_cases(), _goto_handle_cases(), _episode_handle_cases(), _agent_cases()):
        assert not set(out) & set(part)
        out.update(part)
    return out


def run_cases():
    """{id: [status, text]} from the library that is loaded (RG_MPC_LIB, or the tree's build)."""
    return {name: list(call()) for name, call in all_cases().items()}


def _recorded():
    with open(GOLDEN) as f:
        return json.load(f)


EXPECTED = {} if __name__ == "__main__" else _recorded()


@pytest.fixture(scope="module")
def got():
    return run_cases()


def test_the_case_list_is_the_recorded_one(got):
    assert sorted(got) == sorted(EXPECTED) and len(EXPECTED) == 273


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_status_and_text(got, name):
    assert got[name] == EXPECTED[name]


def test_the_cases_cover_what_the_validators_share():
    texts = [t for _, t in EXPECTED.values()]
    for piece in ("this library is version", "reserved0: must be 0", "reserved1: must be 0", "batch: 0 outside [1, 16777216]", "]: nan is not finite",
                  "must be finite and > 0", ": inf must be finite", "outside [", "srb config.", "goto config.", "host-only handle (RG_GOTO_DEVICE_NONE)",
                  "host-only handle (RG_EPISODE_DEVICE_NONE)", "host-only handle (RG_POLICY_DEVICE_NONE)", "host-only handle (RG_PPO_DEVICE_NONE)",
                  "host-only handle (RG_DDPG_DEVICE_NONE)", "host-only handle (RG_RNN_DEVICE_NONE)", "must not alias mask", "null paths pointer",
                  "null sim_obs pointer", "null host array", "null reward or done", "null handle"):
        assert any(piece in t for t in texts), piece
    assert not any("HIP device" in t or "hipSetDevice" in t for t in texts)   # nothing that depends on the machine


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(run_cases(), f, indent=1, sort_keys=True)
        f.write("\n")
