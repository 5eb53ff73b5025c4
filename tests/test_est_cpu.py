"""The state estimator error model of include/rg_est.h without a GPU: the binding against the header and the library, what
rg_est_create and the entries refuse (by name), the host-only handle, the wrapper's refusals, known answers worked by hand, the
properties of the model of tests/est_model.py, the CPU closed loop that levels the estimated body, and the resources of
robot_gym_amd/csrc/rg_est.hip from one device-only compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import est_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import est_fixtures as EF
from tests import est_model as EM
from tests import kernel_checks
from tests import sensor_model as SM
from tests import srb_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
U = np.uint64
NAN, INF = float("nan"), float("inf")


# ---- the binding -------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rg_est.h")).read(), flags=re.S)


def test_library_exports_every_declared_entry():
    lib = est_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_est_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(est_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rg_est_abi_version() == est_abi.ABI_VERSION == 1
    assert lib.rg_est_state_rows() == est_abi.ROWS == EM.ROWS == 8


def test_config_layout_size_and_constants_match_the_header():
    hdr = _header()
    structs = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", hdr))
    defs = {k: v for k, v in re.findall(r"#define (RG_EST_\w+) (\(?-?[\d< ]+\)?)", hdr)}
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    got = [(n, ctype[t] * int(dim) if dim else ctype[t]) for t, n, dim in re.findall(r"\b(int32_t|uint64_t|double)\s+(\w+)(?:\[(\w+)\])?\s*;", structs["rg_est_config"])]
    want = list(est_abi.CConfig._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):      # array types are made anew by every `*`: compare element type and length
        assert (a._type_, a._length_) == (b._type_, b._length_) if hasattr(a, "_length_") else a is b, n
    assert est_abi.load_library().rg_est_config_size() == C.sizeof(est_abi.CConfig) == 2 * 4 + 8 + 6 * 3 * 8 + 5 * 8 + 2 * 4 == 208
    off = 0
    for n, t in est_abi.CConfig._fields_:     # naturally aligned with no padding anywhere
        assert getattr(est_abi.CConfig, n).offset == off, n
        off += C.sizeof(t)
    assert int(defs["RG_EST_ROWS"]) == est_abi.ROWS
    rows = [int(defs[f"RG_EST_ROW_{n}"]) for n in ("KEY", "DRAWS", "TICKS", "RUN")]
    assert rows == [0, 1, 2, 3] == [EM.ROW_KEY, EM.ROW_DRAWS, EM.ROW_TICKS, EM.ROW_RUN] == [est_abi.ROW_KEY, est_abi.ROW_DRAWS, est_abi.ROW_TICKS, est_abi.ROW_RUN]
    purposes = [int(defs[f"RG_EST_PURPOSE_{n}"]) for n in ("BIAS", "NOISE", "MISS", "GHOST")]
    assert purposes == list(range(32, 36)) == [EM.BIAS, EM.NOISE, EM.MISS, EM.GHOST]
    assert purposes == [est_abi.PURPOSE_BIAS, est_abi.PURPOSE_NOISE, est_abi.PURPOSE_MISS, est_abi.PURPOSE_GHOST]
    # disjoint from every purpose of the units that share the chain
    from robot_gym_amd.core import dr_abi, sensor_abi
    others = {getattr(m, n) for m in (dr_abi, sensor_abi) for n in dir(m) if n.startswith("PURPOSE_")}
    assert len(others) == 12 and not set(purposes) & others
    for rel in ("rg_dr.h", "rg_sensor.h", "rg_episode.h"):
        text = open(os.path.join(ROOT, "include", rel)).read()
        assert not set(purposes) & {int(v) for v in re.findall(r"#define RG_\w*PURPOSE_\w+ (\d+)", text)}, rel
    # the observation rows are those of the simulator's STATE_FIELDS order
    from robot_gym_amd.controllers.mpc.batched import STATE_FIELDS
    first, at = {}, 0
    for name, comps, _ in STATE_FIELDS:
        first[name] = at
        at += comps
    assert at == 77 and [name for name, _, _ in STATE_FIELDS] == [name for name, _, _ in EM.OBS_FIELDS] == list(srb_abi.OBS_FIELDS[:-1])
    obs_rows = [int(defs[f"RG_EST_OBS_ROW_{n}"]) for n in ("RPY", "RPY_RATE", "V_WORLD", "Q", "CONTACT")]
    assert obs_rows == [first[n] for n in ("rpy", "rpy_rate", "v_world", "q", "contact")] == [0, 3, 6, 13, 73]
    assert obs_rows == [EM.OBS_ROW_RPY, EM.OBS_ROW_RPY_RATE, EM.OBS_ROW_V_WORLD, EM.OBS_ROW_Q, EM.OBS_ROW_CONTACT]
    assert obs_rows == [est_abi.OBS_ROW_RPY, est_abi.OBS_ROW_RPY_RATE, est_abi.OBS_ROW_V_WORLD, est_abi.OBS_ROW_Q, est_abi.OBS_ROW_CONTACT]
    assert int(defs["RG_EST_MAX_RISE"]) == est_abi.MAX_RISE == 15 and defs["RG_EST_RUN_MAX"] == "(1 << 20)" and est_abi.RUN_MAX == EM.RUN_MAX == 1 << 20
    assert defs["RG_EST_DEVICE_NONE"] == "(-1)" and est_abi.DEVICE_NONE == -1
    status = dict(re.findall(r"RG_EST_(OK|ERR_\w+) = (-?\d+)", hdr))
    assert {k.replace("ERR_", ""): int(v) for k, v in status.items()} == {v: k for k, v in est_abi.STATUS.items()}


ODD = np.array([0x80000000, 0x7FC12345, 0x00000001, 0xFF800000, 0x3F800000, 0x807FFFFF], dtype=np.uint32)   # -0.0, a NaN payload, denormals, -inf, 1


def _odd_obs(B=3):
    """An observation whose float rows cycle through ODD, so that every row holds bit patterns arithmetic would not keep."""
    o, n = EM.new_obs(B), 0
    for name, comps, dt in EM.OBS_FIELDS:
        if dt == np.float32:
            o[name][:] = ODD[(n + np.arange(comps * B)) % len(ODD)].view(np.float32).reshape(comps, B)
            n += 1
    o["contact"][:] = np.array([[0, 1, -7], [5, 0, 1], [1, 1, 0], [0, 0, 2]], dtype=np.int32)[:, :B]
    o["t_robot"][:] = [0.0, 1.5, -0.0][:B]
    return o


def test_the_defaults_are_the_identity():
    c = est_abi.make_cconfig()
    assert (c.seed, c.contact_rise_ticks, c.reserved0, c.reserved1) == (0, 0, 0, 0)
    for name in est_abi.TRIPLES:
        assert list(getattr(c, name)) == [0.0] * 3, name
    for name in est_abi.SCALARS:
        assert getattr(c, name) == 0.0, name
    assert est_abi.DEFAULTS == EM.DEFAULTS and est_abi.TRIPLES == EM.TRIPLES and est_abi.SCALARS == EM.SCALARS
    assert est_abi.create_status(c, 4) == (0, "")
    assert est_abi.make_cconfig(seed=-1).seed == 2 ** 64 - 1
    from robot_gym_amd.sim import StateEstimator
    assert StateEstimator().settings == dict(seed=0)
    # in the model, the default configuration copies bits in every row and still counts ticks and contact runs
    cfg, st, true = EM.settings(), EM.new_state(3), _odd_obs()
    EM.reset([1, 1, 1], st)
    est = EM.estimate(cfg, None, st, true)
    for name, v in true.items():
        assert est[name] is not v and est[name].dtype == v.dtype and est[name].tobytes() == v.tobytes(), name
    assert (st[:3] == [[0, 1, 2], [1, 1, 1], [1, 1, 1]]).all() and (st[3:7] == np.where(true["contact"] != 0, 2.0 ** 20, 0.0)).all() and (st[7] == 0).all()


BAD = [(dict(contact_rise_ticks=-1), 4, "config.contact_rise_ticks"), (dict(contact_rise_ticks=16), 4, "config.contact_rise_ticks"),
       (dict(imu_bias_half_width=(0.0, -0.1, 0.0)), 4, "config.imu_bias_half_width[1]"), (dict(imu_bias_half_width=(NAN, 0.0, 0.0)), 4, "config.imu_bias_half_width[0]"),
       (dict(imu_noise_sigma=(0.0, 0.0, INF)), 4, "config.imu_noise_sigma[2]"), (dict(gyro_bias_half_width=(-1.0, 0.0, 0.0)), 4, "config.gyro_bias_half_width[0]"),
       (dict(gyro_noise_sigma=(0.0, NAN, 0.0)), 4, "config.gyro_noise_sigma[1]"), (dict(velocity_bias_half_width=(0.0, 0.0, -1e-9)), 4, "config.velocity_bias_half_width[2]"),
       (dict(velocity_noise_sigma=(INF, 0.0, 0.0)), 4, "config.velocity_noise_sigma[0]"), (dict(encoder_bias_half_width=-0.1), 4, "config.encoder_bias_half_width"),
       (dict(encoder_bias_half_width=NAN), 4, "config.encoder_bias_half_width"), (dict(encoder_noise_sigma=-1.0), 4, "config.encoder_noise_sigma"),
       (dict(encoder_noise_sigma=INF), 4, "config.encoder_noise_sigma"), (dict(encoder_quantum=-1e-3), 4, "config.encoder_quantum"),
       (dict(encoder_quantum=INF), 4, "config.encoder_quantum"), (dict(contact_miss_probability=1.5), 4, "config.contact_miss_probability"),
       (dict(contact_miss_probability=-0.1), 4, "config.contact_miss_probability"), (dict(contact_miss_probability=NAN), 4, "config.contact_miss_probability"),
       (dict(contact_ghost_probability=1.0001), 4, "config.contact_ghost_probability"), (dict(contact_ghost_probability=-1.0), 4, "config.contact_ghost_probability"),
       ({}, 0, "batch"), ({}, (1 << 24) + 1, "batch")]


@pytest.mark.parametrize("change,batch,field", BAD)
def test_create_refuses_naming_the_field(change, batch, field):
    rc, msg = est_abi.create_status(est_abi.make_cconfig(**change), batch)
    assert rc == -1 and msg.startswith(field + ":"), (rc, msg)


def test_create_accepts_the_edges_and_refuses_version_reserved_words_a_bad_chain_and_null():
    lib = est_abi.load_library()
    for ok in (dict(contact_rise_ticks=15, contact_miss_probability=1.0, contact_ghost_probability=1.0, seed=2 ** 64 - 1, encoder_quantum=1.0,
                    imu_bias_half_width=(3.0, 3.0, 3.0)), EF.FULL, EF.TILT):
        assert est_abi.create_status(est_abi.make_cconfig(**ok), 1 << 24) == (0, ""), ok
    assert est_abi.create_status(mpc_cfg=MPCConfig.for_robot("k3lso")) == (0, "")
    c = est_abi.make_cconfig()
    c.abi_version = 2
    assert est_abi.create_status(c) == (-1, "config.abi_version: 2, this library is version 1")
    for name in ("reserved0", "reserved1"):
        c = est_abi.make_cconfig()
        setattr(c, name, 1)
        assert est_abi.create_status(c) == (-1, f"config.{name}: must be 0")
    # the simulator's configuration is checked by the simulator's own rules, before a device is looked for
    sc = srb_abi.make_cconfig(MPCConfig.for_robot("ghost"))
    sc.jaxis[3], sc.jaxis[4], sc.jaxis[5] = 0.0, 0.0, 0.0
    assert est_abi.create_status(scfg=sc) == (-1, "srb config.jaxis[3]: zero joint axis")
    sc = srb_abi.make_cconfig(MPCConfig.for_robot("ghost"))
    sc.motor_dir[2] = 0.5
    assert est_abi.create_status(scfg=sc)[1].startswith("srb config.motor_dir[2]:")
    sc = srb_abi.make_cconfig(MPCConfig.for_robot("ghost"))
    sc.abi_version = 9
    assert est_abi.create_status(scfg=sc)[1].startswith("srb config.abi_version:")
    h, ok_s = C.c_void_p(), srb_abi.make_cconfig(MPCConfig.for_robot("ghost"))
    assert lib.rg_est_create(None, C.byref(ok_s), 4, est_abi.DEVICE_NONE, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.rg_est_last_error(None)
    assert lib.rg_est_create(C.byref(est_abi.make_cconfig()), None, 4, est_abi.DEVICE_NONE, C.byref(h)) == -1 and not h.value
    assert lib.rg_est_create(C.byref(est_abi.make_cconfig()), C.byref(ok_s), 4, est_abi.DEVICE_NONE, None) == -1


def _raises(status, *words):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(est_abi.RgEstError)
            self.e = self.cm.__enter__()
            return self.e

        def __exit__(self, *a):
            out = self.cm.__exit__(*a)
            assert self.e.value.status == status, str(self.e.value)
            for w in words:
                assert w in str(self.e.value), (w, str(self.e.value))
            return out
    return Ctx()


def _ptrs(base):
    p = srb_abi.CObsPtrs()
    for k, name in enumerate(srb_abi.OBS_FIELDS):
        setattr(p, name, base + 0x1000 * k)      # stand-ins for addresses: a host-only handle never looks through them
    return p


def test_host_only_handle_checks_every_argument_by_name_then_reports_no_device():
    h = est_abi.EstHandle(4, MPCConfig.for_robot("ghost"), est_abi.DEVICE_NONE, **EF.FULL)
    assert h.device is None and h.batch == 4 and h.fields["contact_rise_ticks"] == 2
    with _raises(-1, "reset", "null mask"):
        h.reset(None, 0x1000)
    with _raises(-1, "reset", "null est_state"):
        h.reset(0x1000, None)
    with _raises(-3, "RG_EST_DEVICE_NONE"):
        h.reset(0x1000, 0x2000)
    t, e = _ptrs(0x100000), _ptrs(0x200000)
    with _raises(-1, "estimate", "null est_state"):
        h.estimate(None, t, e)
    with _raises(-1, "estimate", "null true_obs pointer"):
        h.estimate(0x1000, None, e)
    with _raises(-1, "estimate", "null est_obs pointer"):
        h.estimate(0x1000, t, None)
    for name in srb_abi.OBS_FIELDS:      # every pointer of both structs is required
        for which, word in ((0, "true_obs"), (1, "est_obs")):
            pair = [_ptrs(0x100000), _ptrs(0x200000)]
            setattr(pair[which], name, None)
            with _raises(-1, "estimate", f"null {word} pointer"):
                h.estimate(0x1000, *pair)
    for a, b in (("rpy", "rpy"), ("q", "foot_pos"), ("t_robot", "contact")):      # no pointer of the estimate is one of the truth
        e2 = _ptrs(0x200000)
        setattr(e2, a, getattr(t, b))
        with _raises(-1, "estimate", "est_obs must not alias true_obs"):
            h.estimate(0x1000, t, e2)
    with _raises(-3, "RG_EST_DEVICE_NONE"):
        h.estimate(0x1000, t, e)
    h.close()
    h.close()
    assert not h._h
    lib = est_abi.load_library()
    assert lib.rg_est_reset(None, 0x1000, 0x1000, None) == -1 and b"null handle" in lib.rg_est_last_error(None)
    assert lib.rg_est_estimate(None, 0x1000, C.byref(t), C.byref(e), None) == -1 and b"null handle" in lib.rg_est_last_error(None)


def test_wrapper_refuses_by_name_without_a_device():
    from robot_gym_amd.sim import StateEstimator
    with pytest.raises(TypeError, match="sigma"):
        StateEstimator(imu=dict(sigma=(0, 0, 0)))
    with pytest.raises(TypeError, match="quantum"):
        StateEstimator(gyro=dict(quantum=0.1))
    with pytest.raises(TypeError, match="rise"):
        StateEstimator(contact=dict(rise=2))
    with pytest.raises(TypeError, match="bogus"):
        StateEstimator(bogus=1)
    with pytest.raises(ValueError, match="imu"):
        StateEstimator(imu=dict(bias_half_width=0.03))
    with pytest.raises(ValueError, match="velocity"):
        StateEstimator(velocity=dict(noise_sigma=(0.1, 0.2)))
    with pytest.raises(ValueError, match="encoders"):
        StateEstimator(encoders=dict(quantum=(0.1, 0.1, 0.1)))
    with pytest.raises(ValueError, match="rise_ticks"):
        StateEstimator(contact=dict(rise_ticks=1.5))
    with pytest.raises(ValueError, match="gyro"):
        StateEstimator(gyro=3)
    with pytest.raises(ValueError, match="imu_noise_sigma"):
        est_abi.make_cconfig(imu_noise_sigma=(0.0, 0.0))
    with pytest.raises(TypeError, match="bogus"):
        est_abi.make_cconfig(bogus=1)
    est = StateEstimator(imu=dict(bias_half_width=(0.03, 0.03, 0), noise_sigma=(1e-3, 2e-3, 3e-3)), gyro=dict(noise_sigma=(0.1, 0.1, 0.1)),
                         velocity=dict(bias_half_width=(0.05, 0.05, 0.0)), encoders=dict(bias_half_width=0.01, noise_sigma=0.002, quantum=0.001),
                         contact=dict(miss_probability=0.02, ghost_probability=0.01, rise_ticks=2), seed=7)
    assert est.settings == dict(seed=7, imu_bias_half_width=(0.03, 0.03, 0.0), imu_noise_sigma=(1e-3, 2e-3, 3e-3), gyro_noise_sigma=(0.1, 0.1, 0.1),
                                velocity_bias_half_width=(0.05, 0.05, 0.0), encoder_bias_half_width=0.01, encoder_noise_sigma=0.002, encoder_quantum=0.001,
                                contact_miss_probability=0.02, contact_ghost_probability=0.01, contact_rise_ticks=2)
    assert est_abi.create_status(est_abi.make_cconfig(**est.settings)) == (0, "")
    for call in (lambda: est.on_reset(), lambda: est.estimate(), lambda: est.copy_columns([0], [1])):
        with pytest.raises(RuntimeError, match="bind"):
            call()
    est.close()
    # the wiring exists and defaults to None everywhere
    import inspect
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import srb
    assert inspect.signature(BatchedGoEnv.__init__).parameters["state_estimator"].default is None
    assert inspect.signature(srb.rollout).parameters["estimator"].default is None and inspect.signature(srb.clone).parameters["estimator"].default is None


# ---- known answers worked by hand ------------------------------------------------------------------------------------------

def _standing(B):
    o = EM.new_obs(B)
    o["quat"][3] = 1.0
    return o


def test_known_answer_a_contact_trace_through_a_debounce_of_two_with_a_lift_off_in_the_middle():
    cfg, st = EM.settings(contact_rise_ticks=2), EM.new_state(1)
    st[EM.ROW_RUN:EM.ROW_RUN + 4] = 0.0      # a foot that has been in the air (a reset would set 2^20: see the next test)
    st[EM.ROW_DRAWS] = 1.0
    true = [0, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1]
    runs = [0, 1, 2, 3, 4, 0, 1, 2, 0, 1, 2, 3]      # consecutive ticks of true contact
    want = [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1]      # reported once the run exceeds 2: two ticks late, and a two-tick touch is never seen
    for k, (c, r, w) in enumerate(zip(true, runs, want)):
        o = _standing(1)
        o["contact"][1, 0] = c
        est = EM.estimate(cfg, None, st, o)
        assert (st[EM.ROW_RUN + 1, 0], est["contact"][1, 0]) == (r, w), k
        assert (est["contact"][[0, 2, 3], 0] == 0).all() and st[EM.ROW_TICKS, 0] == k + 1
    # after a reset the four feet have been down: the debounce does not blind the robot, and the run saturates
    EM.reset([1], st)
    assert (st[EM.ROW_RUN:EM.ROW_RUN + 4, 0] == 2 ** 20).all() and st[EM.ROW_DRAWS, 0] == 2 and st[EM.ROW_TICKS, 0] == 0
    o = _standing(1)
    o["contact"][:] = 1
    assert (EM.estimate(cfg, None, st, o)["contact"] == 1).all() and (st[EM.ROW_RUN:EM.ROW_RUN + 4, 0] == 2 ** 20).all()
    # rows a caller wrote are clamped: a NaN or a negative run is 0, a huge one 2^20
    st[EM.ROW_RUN:EM.ROW_RUN + 4, 0] = [np.nan, -5.0, 1e30, 1.0]
    assert EM.estimate(cfg, None, st, o)["contact"][:, 0].tolist() == [0, 0, 1, 0] and st[EM.ROW_RUN:EM.ROW_RUN + 4, 0].tolist() == [1, 1, 2 ** 20, 2]


def test_known_answer_a_quantised_encoder_at_a_tie():
    chain = M.Chain(MPCConfig.for_robot("ghost"))
    cfg, st = EM.settings(encoder_quantum=0.25), EM.new_state(1)
    EM.reset([1], st)
    o = _standing(1)
    o["q"][:, 0] = [0.125, 0.375, -0.125, 0.625, 0.3, -0.875, 1.0, 0.124, 0.126, -0.376, 2.0 ** 20 + 0.125, 0.0]
    est = EM.estimate(cfg, chain, st, o)
    # x / 0.25 = 0.5, 1.5, -0.5, 2.5 are ties and go to the even multiple: 0, 2, -0, 2
    assert est["q"][:, 0].tolist() == [0.0, 0.5, -0.0, 0.5, 0.25, -1.0, 1.0, 0.0, 0.25, -0.5, 2.0 ** 20, 0.0]
    assert np.signbit(est["q"][2, 0]) and not np.signbit(est["q"][0, 0])


def test_known_answer_the_hamilton_product_on_a_quarter_turn_of_yaw_with_a_pure_roll_error():
    # q = 90 degrees about z = (0, 0, s, s) with s = sqrt(1/2); error e = (e0, 0, 0) in the BODY frame, dq = (e0 / 2, 0, 0, 1):
    #   x' = qw dx = s h, y' = qz dx = s h, z' = qz = s, w' = qw = s      (h = e0 / 2);  |q'|^2 = 1 + h^2
    # the body x axis points along world y after the yaw, so a body-frame roll error stays a roll: rpy_est = (2 atan h, 0, pi / 2)
    e0, B = 0.04, 1
    cfg, st = EM.settings(seed=3, imu_bias_half_width=(1.0, 0.0, 0.0)), EM.new_state(B, keys=[6])
    EM.reset([1], st)
    drawn = 2.0 * SM.uniform(3, 6, 0, EM.BIAS, 0) - 1.0
    o = _standing(B)
    s = np.float32(np.sqrt(0.5))
    o["quat"][:, 0] = [0.0, 0.0, s, s]
    est = EM.estimate(cfg, None, st, o)
    h, sd = drawn / 2.0, float(s)
    n = np.sqrt(((sd * h) ** 2 + (sd * h) ** 2 + sd * sd) + sd * sd)
    assert est["quat"][:, 0].tolist() == [np.float32(sd * h / n), np.float32(sd * h / n), np.float32(sd / n), np.float32(sd / n)]
    assert abs(est["rpy"][0, 0] - 2.0 * np.arctan(h)) < 1e-7 and abs(est["rpy"][1, 0]) < 1e-7 and abs(est["rpy"][2, 0] - np.pi / 2) < 2e-7
    # with a fixed error by hand instead of a draw: the product itself
    del e0
    qx, qy, qz, qw, dx, dy, dz = 0.1, -0.2, 0.3, 0.9, 0.01, -0.02, 0.03
    x = ((qw * dx + qx) + qy * dz) - qz * dy
    y = ((qw * dy - qx * dz) + qy) + qz * dx
    z = ((qw * dz + qx * dy) - qy * dx) + qz
    w = ((qw - qx * dx) - qy * dy) - qz * dz
    v, u = np.array([qx, qy, qz]), np.array([dx, dy, dz])
    assert np.allclose([x, y, z], qw * u + 1.0 * v + np.cross(v, u), rtol=0, atol=1e-16) and abs(w - (qw - v @ u)) < 1e-16
    # the angle applied is 2 atan(|e| / 2), |e|^3 / 12 short of |e|
    for mag in (0.03, 0.1):
        assert abs((mag - 2.0 * np.arctan(mag / 2.0)) - mag ** 3 / 12.0) < mag ** 5 / 50.0


# ---- properties of the model -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full_run():
    """Both robots' chains, 40 robots, 12 ticks under FULL with a reset of every third robot at tick 5: (robot, true, est, state after) per tick."""
    out = {}
    for robot in ("ghost", "k3lso"):
        chain, rng, B = M.Chain(MPCConfig.for_robot(robot)), np.random.default_rng(4), 40
        cfg, st = EM.settings(**EF.FULL), EM.new_state(B, keys=rng.permutation(1000)[:B] + 2 ** 33)
        EM.reset(np.ones(B), st)
        trace, ticks = EF.contact_trace(rng, 12, B), []
        for k in range(12):
            if k == 5:
                EM.reset(np.arange(B) % 3 == 0, st)
            true = EM.random_obs(rng, B, chain)
            true["contact"][:] = trace[k]
            before = st.copy()
            ticks.append((true, EM.estimate(cfg, chain, st, true), before, st.copy()))
        out[robot] = (chain, cfg, ticks)
    return out


def test_quat_est_is_a_unit_quaternion_and_rpy_est_are_its_zyx_angles(full_run):
    for robot, (chain, cfg, ticks) in full_run.items():
        for true, est, _, _ in ticks:
            q = est["quat"].astype(np.float64)
            assert np.abs(np.sqrt((q * q).sum(0)) - 1.0).max() < 4 * 2.0 ** -24      # each of four components rounded to float32
            R = M.quat_rot(list(q))
            rpy = np.stack([np.arctan2(R[7], R[8]), -np.arcsin(np.clip(R[6], -1, 1)), np.arctan2(R[3], R[0])])
            # the float32 quat is within 2^-24 of the float64 one per component: the angles move by a few 1e-7 at most
            assert np.abs(rpy - est["rpy"]).max() < 1e-6
            assert np.abs(est["rpy"][:2] - true["rpy"][:2]).max() < 0.2 and not (est["quat"] == true["quat"]).all(axis=0).any()
            # the error applied is small and of the drawn size: the rotation between truth and estimate is at most |e| = |bias| + 3.47 |sigma|
            qt = true["quat"].astype(np.float64)
            dot = np.abs((q * qt).sum(0))
            bound = np.linalg.norm(np.asarray(cfg["imu_bias_half_width"]) + 3.4642 * np.asarray(cfg["imu_noise_sigma"]))
            assert (2.0 * np.arccos(np.minimum(dot, 1.0)) < bound + 1e-3).all()


def test_foot_pos_est_and_jac_est_are_the_kinematics_of_q_est_for_both_robots(full_run):
    from robot_gym_amd.controllers.mpc.kinematics import ChainKinematics
    for robot, (chain, cfg, ticks) in full_run.items():
        ck = ChainKinematics(MPCConfig.for_robot(robot))
        true, est, _, _ = ticks[3]
        assert np.abs(est["q"] - true["q"]).max() < 0.01 + 3.4642 * 0.002 + np.pi / 4096 + 1e-6 and not (est["q"] == true["q"]).all()
        step = est["q"].astype(np.float64) / cfg["encoder_quantum"]
        assert np.abs(step - np.rint(step)).max() < 2e-4      # float32 rounding of a multiple of the quantum: half an ulp of 4 rad is 1.6e-4 quanta
        for b in range(0, 40, 7):
            for leg in range(4):
                pf, J = ck.foot_position_and_jacobian(leg, est["q"][3 * leg:3 * leg + 3, b].astype(np.float64))
                assert np.abs(pf - est["foot_pos"][3 * leg:3 * leg + 3, b]).max() < 1e-7, (robot, b, leg)
                assert np.abs(np.asarray(J).reshape(9) - est["jac"][9 * leg:9 * leg + 9, b]).max() < 1e-7, (robot, b, leg)
    # the two chains differ: the same angles give different feet
    a, b = (full_run[r][2][3][1]["foot_pos"] for r in ("ghost", "k3lso"))
    assert np.abs(a - b).max() > 1e-3


def test_a_bias_is_constant_over_an_episode_and_redrawn_at_a_reset():
    B = 9
    cfg = EM.settings(seed=2, gyro_bias_half_width=(0.1, 0.2, 0.3), velocity_bias_half_width=(0.5, 0.0, 0.25), encoder_bias_half_width=0.05,
                      imu_bias_half_width=(0.03, 0.03, 0.01))
    chain, st = M.Chain(MPCConfig.for_robot("ghost")), EM.new_state(B)
    EM.reset(np.ones(B), st)
    true = EM.random_obs(np.random.default_rng(1), B, chain)
    first = EM.estimate(cfg, chain, st, true)
    for _ in range(3):
        again = EM.estimate(cfg, chain, st, true)
        for name in first:
            assert again[name].tobytes() == first[name].tobytes(), name
    off = first["rpy_rate"].astype(np.float64) - true["rpy_rate"]
    assert (np.abs(off) <= np.array([[0.1], [0.2], [0.3]]) + 1e-6).all() and np.abs(off).min() > 0
    assert (first["v_world"][1] == true["v_world"][1]).all()                   # an axis with no amplitude is copied
    want = true["rpy_rate"][1].astype(np.float64) + 0.2 * (2.0 * np.array([SM.uniform(2, b, 0, EM.BIAS, 4) for b in range(B)]) - 1.0)
    assert (first["rpy_rate"][1] == want.astype(np.float32)).all()
    EM.reset(np.arange(B) % 2 == 0, st)
    redrawn = EM.estimate(cfg, chain, st, true)
    for name in ("rpy", "quat", "rpy_rate", "q", "foot_pos"):
        same = (redrawn[name] == first[name]).all(axis=0)
        assert same[1::2].all() and not same[0::2].any(), name
    assert (st[EM.ROW_DRAWS] == np.where(np.arange(B) % 2 == 0, 2, 1)).all() and (st[EM.ROW_TICKS] == np.where(np.arange(B) % 2 == 0, 1, 5)).all()


@pytest.mark.parametrize("p", [0.01, 0.3, 0.9])
def test_miss_and_ghost_frequencies_are_within_five_standard_errors(p):
    B, T = 2000, 25
    cfg, st = EM.settings(seed=9, contact_miss_probability=p, contact_ghost_probability=p), EM.new_state(B)
    EM.reset(np.ones(B), st)
    true = _standing(B)
    true["contact"][:2], true["contact"][2:] = 1, 0      # two feet down the whole time (the run stays at 2^20), two in the air
    miss = ghost = 0
    for _ in range(T):
        est = EM.estimate(cfg, None, st, true)
        miss += int((est["contact"][:2] == 0).sum())
        ghost += int((est["contact"][2:] == 1).sum())
    n = 2 * B * T
    for hits in (miss, ghost):
        assert abs(hits / n - p) < 5.0 * np.sqrt(p * (1.0 - p) / n), (hits / n, p)
    assert miss != ghost      # two purposes, two streams


def test_a_robot_outside_the_mask_is_untouched_and_streams_follow_the_key_not_the_position():
    B = 8
    rng = np.random.default_rng(0)
    st = rng.standard_normal((EM.ROWS, B)) * 50.0
    st[EM.ROW_KEY], st[EM.ROW_DRAWS] = [9, 7, 7, 3, 4, 5, 6, 8], 2.0
    before, mask = st.copy(), np.array([1, 1, 1, 0, 0, 1, 0, 0])
    EM.reset(mask, st)
    assert (st[:, mask == 0] == before[:, mask == 0]).all() and (st[EM.ROW_KEY] == before[EM.ROW_KEY]).all() and (st[7] == before[7]).all()
    assert (st[EM.ROW_DRAWS, mask == 1] == 3).all() and (st[EM.ROW_TICKS, mask == 1] == 0).all() and (st[3:7, mask == 1] == 2 ** 20).all()
    # robots 1 and 2 share a key: the same truth gives the same estimate; a permutation of robots with their keys permutes the output
    chain, cfg = M.Chain(MPCConfig.for_robot("ghost")), EM.settings(**EF.FULL)
    st = EM.new_state(B, keys=[9, 7, 7, 3, 4, 5, 6, 8])
    EM.reset(np.ones(B), st)
    true = EM.random_obs(rng, B, chain)
    for v in true.values():
        v[..., 2] = v[..., 1]
    perm = np.array([3, 0, 6, 1, 7, 2, 5, 4])
    st2, true2 = st[:, perm].copy(), {n: v[..., perm].copy() for n, v in true.items()}
    est, est2 = EM.estimate(cfg, chain, st, true), EM.estimate(cfg, chain, st2, true2)
    for name in est:
        assert (est[name][..., 1] == est[name][..., 2]).all(), name
        assert est2[name].tobytes() == np.ascontiguousarray(est[name][..., perm]).tobytes(), name
    assert not (est["rpy_rate"][:, 0] == est["rpy_rate"][:, 1]).any() and (st2 == st[:, perm]).all()


def test_each_effect_alone_moves_its_own_rows_and_leaves_the_others_bits():
    chain, B = M.Chain(MPCConfig.for_robot("ghost")), 16
    rng = np.random.default_rng(3)
    trace = EF.contact_trace(rng, 6, B)
    for effect, (fields, rows) in EF.EFFECTS.items():
        cfg, st = EM.settings(seed=1, **fields), EM.new_state(B)
        st[EM.ROW_DRAWS] = 1.0      # in the air before: a debounce shows
        moved = set()
        for k in range(6):
            true = EM.random_obs(rng, B, chain)
            true["contact"][:] = trace[k]
            est = EM.estimate(cfg, chain, st, true)
            for name in est:
                if est[name].tobytes() != true[name].tobytes():
                    moved.add(name)
        assert moved == set(rows), (effect, moved)


# ---- the closed loop ---------------------------------------------------------------------------------------------------------

def test_closed_loop_levels_the_estimated_body():
    """The controller levels the ESTIMATED body: with a roll and pitch bias of half-width 0.03 rad alone, zero command, 32 robots
    per model and 4 s, nobody falls and the true roll and pitch over the last second sit at minus the drawn error.  Measured
    slopes of the settled true angle on the drawn error (slope, standard error of the fit):
        ghost   roll -1.04243 (8.0e-05)   pitch -1.01357 (3.4e-05)
        k3lso   roll -1.03831 (5.1e-05)   pitch -1.01360 (3.7e-05)
    1 to 4 % steeper than -1; why has not been looked into.  EF.CPU_SLOPES holds these figures for the GPU test and is recomputed
    here."""
    for robot in ("ghost", "k3lso"):
        got, loop, traj = EF.run_cpu_tilt(robot)
        print(robot, got)
        assert not loop.model.fallen().any() and all(np.isfinite(v).all() for v in traj.values())
        err = EF.drawn_tilt(np.arange(EF.LOOP_ROBOTS))
        assert np.abs(err).max() < EF.TILT_HALF_WIDTH and np.abs(err).max() > 0.8 * EF.TILT_HALF_WIDTH
        # what the controller was given on the last tick is level to a few milliradians; the truth is not
        assert np.abs(loop.est_obs["rpy"][:2]).max() < 0.2 * np.abs(loop.model.obs["rpy"][:2]).max()
        for axis in ("roll", "pitch"):
            slope, se = got[axis]
            assert slope < 0 and abs(slope + 1.0) < 0.1, (robot, axis, slope)
            want_slope, want_se = EF.CPU_SLOPES[robot][axis]
            # the constants are this measurement: within a tenth of the standard error the GPU test allows three of
            assert abs(slope - want_slope) <= 0.1 * want_se and abs(se - want_se) <= 0.01 * want_se, (robot, axis, slope, se)


# ---- resources of rg_est.hip -------------------------------------------------------------------------------------------------

KERNELS = {"rg_est_reset_kernel", "rg_est_estimate_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_est.hip")


def test_exactly_the_two_kernels_are_reported(remarks):
    assert set(remarks) == KERNELS


def test_the_kernels_use_no_scratch_no_spills_and_no_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds).  estimate holds one leg's forward kinematics in flight (three
# joint rotations and the Jacobian in float64); reset holds a column of six rows.
REGISTERS = {"rg_est_reset_kernel": dict(vgprs=18, sgprs=16, agprs=0, occupancy=8), "rg_est_estimate_kernel": dict(vgprs=127, sgprs=78, agprs=0, occupancy=4)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    src = open(os.path.join(SRC, "rg_est.hip")).read()
    code = re.sub(r"//.*", "", src)
    pragma = code.index("#pragma clang fp contract(off)")
    assert pragma < code.index("__global__") and pragma < code.index("__device__") and pragma < code.index('#include "rg_mpc_dev.h"')
    assert "asm" not in code and "atomic" not in code.lower() and "__shared__" not in src and "__shfl" not in src
    assert len(re.findall(r"__global__", code)) == len(KERNELS) and code.count("__launch_bounds__(kBlock)") == 2 and "kBlock = 256" in code
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_est.h", "rg_host.h", "rg_mpc_dev.h", "rg_srb_dev.inc", "rg_stream_dev.inc"]
    stream = open(os.path.join(SRC, "rg_stream_dev.inc")).read()                 # the stream's device functions, included after the pragma
    assert pragma < code.index('#include "rg_stream_dev.inc"') < code.index("__device__")
    assert "__global__" not in stream and '#include "' not in stream and "asm" not in re.sub(r"//.*", "", stream) and "atomic" not in stream.lower()
    assert "__shared__" not in stream and "__shfl" not in stream
    # one barrier in the kernel that gives a robot several lanes, and it comes before the first store and the first return
    body = code[code.index("rg_est_estimate_kernel("):]
    body = body[:body.index("\n}\n")]
    assert body.count("__syncthreads()") == 1 and "return" not in body[:body.index("__syncthreads()")]
    assert not re.search(r"\]\s*=[^=]", body[:body.index("__syncthreads()")])
    for other in sorted(os.listdir(SRC)):                                        # included from nowhere
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_est.hip":
            assert "rg_est" not in open(os.path.join(SRC, other)).read(), other
    import bench
    assert not any("rg_est" in rel for rel in bench.compiled_sources())          # the MPC hash behind profiles/ does not follow it
    kernel_checks.assert_built_into_both("rg_est.hip", header="rg_est.h")


def test_the_documents_no_longer_say_the_controllers_state_estimate_stays_exact():
    for rel in ("include/rg_sensor.h", "robot_gym_amd/sim/sensor_model.py", "README.md", "INTEGRATION.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, rel)).read().split())
        for gone in ("state estimate stays exact", "state estimate (the simulator's obs tensors) stays exact"):
            assert gone not in text, (rel, gone)
    for rel in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "rg_est.h" in open(os.path.join(ROOT, rel)).read(), rel
