"""The sensor and actuator model of include/rg_sensor.h without a GPU: the binding against the header and the library, what
rg_sensor_create and the entries refuse (by name), the host-only handle, the stream of tests/sensor_model.py against
tests/episode_model.py and known answers worked by hand, the properties of the model, and the resources of
robot_gym_amd/csrc/rg_sensor.hip from one device-only compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import sensor_abi
from tests import episode_model as EM
from tests import kernel_checks
from tests import sensor_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
U = np.uint64


# ---- the binding -------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rg_sensor.h")).read(), flags=re.S)


def test_library_exports_every_declared_entry():
    lib = sensor_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_sensor_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(sensor_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rg_sensor_abi_version() == sensor_abi.ABI_VERSION == 1
    assert lib.rg_sensor_state_rows() == sensor_abi.ROWS == SM.ROWS == 8


def test_config_layout_size_and_constants_match_the_header():
    hdr = _header()
    structs = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", hdr))
    defs = {k: v for k, v in re.findall(r"#define (RG_SENSOR_\w+) (\(?-?[\d< ]+\)?)", hdr)}
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double, "rg_sensor_group": sensor_abi.CGroup}

    def fields(body):
        out = []
        for t, n, dim in re.findall(r"\b(int32_t|uint64_t|double|rg_sensor_group)\s+(\w+)(?:\[(\w+)\])?\s*;", body):
            out.append((n, ctype[t] * int(defs[dim]) if dim else ctype[t]))
        return out

    def same(got, want):
        assert [n for n, _ in got] == [n for n, _ in want]
        for (n, a), (_, b) in zip(got, want):      # array types are made anew by every `*`: compare element type and length
            assert (a._type_, a._length_) == (b._type_, b._length_) if hasattr(a, "_length_") else a is b, n

    same(fields(structs["rg_sensor_group"]), list(sensor_abi.CGroup._fields_))
    same(fields(structs["rg_sensor_config"]), list(sensor_abi.CConfig._fields_))
    assert C.sizeof(sensor_abi.CGroup) == 2 * 4 + 5 * 8 == 48
    assert sensor_abi.load_library().rg_sensor_config_size() == C.sizeof(sensor_abi.CConfig) == 2 * 4 + 8 + 2 * 4 + 4 * 48 + 4 * 4 + 2 * 8 * 8 + 2 * 4
    off = 0
    for n, t in sensor_abi.CConfig._fields_:     # naturally aligned with no padding anywhere
        assert getattr(sensor_abi.CConfig, n).offset == off, n
        off += C.sizeof(t)
    off = 0
    for n, t in sensor_abi.CGroup._fields_:
        assert getattr(sensor_abi.CGroup, n).offset == off, n
        off += C.sizeof(t)
    assert int(defs["RG_SENSOR_ROWS"]) == sensor_abi.ROWS
    rows = [int(defs[f"RG_SENSOR_ROW_{n}"]) for n in ("KEY", "DRAWS", "OBS_TICKS", "ACT_TICKS", "OBS_DELAY", "ACT_DELAY")]
    assert rows == list(range(6)) == [SM.ROW_KEY, SM.ROW_DRAWS, SM.ROW_OBS_TICKS, SM.ROW_ACT_TICKS, SM.ROW_OBS_DELAY, SM.ROW_ACT_DELAY]
    assert rows == [sensor_abi.ROW_KEY, sensor_abi.ROW_DRAWS, sensor_abi.ROW_OBS_TICKS, sensor_abi.ROW_ACT_TICKS, sensor_abi.ROW_OBS_DELAY, sensor_abi.ROW_ACT_DELAY]
    purposes = [int(defs[f"RG_SENSOR_PURPOSE_{n}"]) for n in ("OBS_DELAY", "ACT_DELAY", "BIAS", "NOISE", "DROPOUT", "ACT_NOISE")]
    assert purposes == list(range(16, 22)) == [SM.OBS_DELAY, SM.ACT_DELAY, SM.BIAS, SM.NOISE, SM.DROPOUT, SM.ACT_NOISE]
    assert purposes == [sensor_abi.PURPOSE_OBS_DELAY, sensor_abi.PURPOSE_ACT_DELAY, sensor_abi.PURPOSE_BIAS, sensor_abi.PURPOSE_NOISE,
                        sensor_abi.PURPOSE_DROPOUT, sensor_abi.PURPOSE_ACT_NOISE]
    from robot_gym_amd.core import dr_abi
    assert not set(purposes) & {dr_abi.PURPOSE_MASS, dr_abi.PURPOSE_INERTIA, dr_abi.PURPOSE_WORLD, dr_abi.PURPOSE_PUSH_START, dr_abi.PURPOSE_PUSH_COMPONENT,
                                dr_abi.PURPOSE_PUSH_GATE}
    maxima = [int(defs[f"RG_SENSOR_MAX_{n}"]) for n in ("GROUPS", "OBS", "ACT", "DELAY")]
    assert maxima == [4, 256, 8, 15] == [sensor_abi.MAX_GROUPS, sensor_abi.MAX_OBS, sensor_abi.MAX_ACT, sensor_abi.MAX_DELAY]
    assert defs["RG_SENSOR_DEVICE_NONE"] == "(-1)" and sensor_abi.DEVICE_NONE == -1
    status = dict(re.findall(r"RG_SENSOR_(OK|ERR_\w+) = (-?\d+)", hdr))
    assert {k.replace("ERR_", ""): int(v) for k, v in status.items()} == {v: k for k, v in sensor_abi.STATUS.items()}


def test_the_defaults_are_the_identity():
    c = sensor_abi.make_cconfig()
    assert (c.n_groups, c.seed, c.obs_delay_min, c.obs_delay_max, c.act_delay_min, c.act_delay_max, c.reserved0, c.reserved1) == (0,) * 8
    assert list(c.act_noise_sigma) == [0.0] * 8 == list(c.act_fill)
    for g in c.groups:
        assert (g.begin, g.end, g.noise_sigma, g.bias_half_width, g.dropout_probability, g.dropout_value, g.quantum) == (0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert sensor_abi.DEFAULTS == SM.DEFAULTS and sensor_abi.GROUP_DEFAULTS == SM.GROUP_DEFAULTS
    assert sensor_abi.create_status(c, 4) == (0, "")
    assert sensor_abi.make_cconfig(seed=-1).seed == 2 ** 64 - 1
    with pytest.raises(TypeError, match="bogus"):
        sensor_abi.make_cconfig(bogus=1)
    with pytest.raises(TypeError, match="bogus"):
        sensor_abi.make_cconfig(groups=[(0, 1, dict(bogus=1.0))])
    with pytest.raises(ValueError, match="groups"):
        sensor_abi.make_cconfig(obs_dim=8, groups=[(k, k + 1, {}) for k in range(5)])
    with pytest.raises(ValueError, match="act_fill"):
        sensor_abi.make_cconfig(act_dim=8, act_fill=[0.0] * 9)
    from robot_gym_amd.sim import SensorModel
    sm = SensorModel()
    assert {**sensor_abi.DEFAULTS, **sm.settings} == sensor_abi.DEFAULTS and sm.path is None and sm.scan is None and sm.groups is None
    # in the model, the default configuration copies bits: -0.0, a NaN with a payload, a denormal
    odd = np.array([0x80000000, 0x7FC12345, 0x00000001, 0xFF800000], dtype=np.uint32).view(np.float32).reshape(4, 1)
    cfg = SM.settings(obs_dim=4)
    buf = SM.new_buffers(cfg, 1)
    SM.reset(cfg, [1], buf, odd)
    SM.observe(cfg, buf, odd)
    assert (buf["obs_out"].view(np.uint32) == odd.view(np.uint32)).all() and (buf["state"][:, 0] == [0, 1, 2, 0, 0, 0, 0, 0]).all()
    assert (SM.act(cfg, buf, odd[:1].T.copy()).view(np.uint32) == odd[:1].view(np.uint32)).all()


NAN, INF = float("nan"), float("inf")


def _g(begin=0, end=4, **f):
    return (begin, end, f)


BAD = [(dict(obs_dim=0), 4, "config.obs_dim"), (dict(obs_dim=257), 4, "config.obs_dim"), (dict(act_dim=0), 4, "config.act_dim"), (dict(act_dim=9), 4, "config.act_dim"),
       (dict(obs_delay_min=-1), 4, "config.obs_delay_min"), (dict(obs_delay_min=16, obs_delay_max=16), 4, "config.obs_delay_min"),
       (dict(obs_delay_max=16), 4, "config.obs_delay_max"), (dict(obs_delay_min=3, obs_delay_max=2), 4, "config.obs_delay_max"),
       (dict(act_delay_min=-1), 4, "config.act_delay_min"), (dict(act_delay_max=16), 4, "config.act_delay_max"),
       (dict(act_delay_min=5, act_delay_max=4), 4, "config.act_delay_max"),
       (dict(obs_dim=8, groups=[_g(-1, 4)]), 4, "config.groups[0].begin"), (dict(obs_dim=8, groups=[_g(8, 9)]), 4, "config.groups[0].begin"),
       (dict(obs_dim=8, groups=[_g(2, 2)]), 4, "config.groups[0].end"), (dict(obs_dim=8, groups=[_g(2, 9)]), 4, "config.groups[0].end"),
       (dict(obs_dim=8, groups=[_g(0, 4), _g(3, 6)]), 4, "config.groups[1].begin"), (dict(obs_dim=8, groups=[_g(4, 8), _g(0, 8)]), 4, "config.groups[1].begin"),
       (dict(obs_dim=8, groups=[_g(0, 2), _g(4, 6), _g(5, 6)]), 4, "config.groups[2].begin"),
       (dict(obs_dim=8, groups=[_g(noise_sigma=-1.0)]), 4, "config.groups[0].noise_sigma"), (dict(obs_dim=8, groups=[_g(noise_sigma=NAN)]), 4, "config.groups[0].noise_sigma"),
       (dict(obs_dim=8, groups=[_g(), _g(4, 8, bias_half_width=-0.5)]), 4, "config.groups[1].bias_half_width"),
       (dict(obs_dim=8, groups=[_g(bias_half_width=INF)]), 4, "config.groups[0].bias_half_width"),
       (dict(obs_dim=8, groups=[_g(dropout_probability=1.5)]), 4, "config.groups[0].dropout_probability"),
       (dict(obs_dim=8, groups=[_g(dropout_probability=-0.1)]), 4, "config.groups[0].dropout_probability"),
       (dict(obs_dim=8, groups=[_g(dropout_probability=NAN)]), 4, "config.groups[0].dropout_probability"),
       (dict(obs_dim=8, groups=[_g(dropout_value=INF)]), 4, "config.groups[0].dropout_value"), (dict(obs_dim=8, groups=[_g(dropout_value=NAN)]), 4, "config.groups[0].dropout_value"),
       (dict(obs_dim=8, groups=[_g(quantum=-1e-3)]), 4, "config.groups[0].quantum"), (dict(obs_dim=8, groups=[_g(quantum=INF)]), 4, "config.groups[0].quantum"),
       (dict(act_dim=2, act_noise_sigma=[0.0, -1.0]), 4, "config.act_noise_sigma[1]"), (dict(act_dim=2, act_noise_sigma=[NAN]), 4, "config.act_noise_sigma[0]"),
       (dict(act_dim=2, act_noise_sigma=[0.0, 0.0, 0.1]), 4, "config.act_noise_sigma[2]"), (dict(act_dim=2, act_fill=[INF]), 4, "config.act_fill[0]"),
       (dict(act_dim=2, act_fill=[0.0, 0.0, 0.0, 1.0]), 4, "config.act_fill[3]"), ({}, 0, "batch"), ({}, (1 << 24) + 1, "batch")]


@pytest.mark.parametrize("change,batch,field", BAD)
def test_create_refuses_naming_the_field(change, batch, field):
    rc, msg = sensor_abi.create_status(sensor_abi.make_cconfig(**change), batch)
    assert rc == -1 and msg.startswith(field + ":"), (rc, msg)


def test_create_accepts_the_edges_and_refuses_version_reserved_words_unused_groups_and_null():
    lib = sensor_abi.load_library()
    full = dict(noise_sigma=1.0, bias_half_width=2.0, dropout_probability=1.0, dropout_value=-3.0, quantum=0.5)
    for ok in (dict(obs_dim=256, act_dim=8, groups=[_g(0, 1, **full), _g(255, 256), _g(1, 255, dropout_probability=0.0)], obs_delay_min=15,
                    obs_delay_max=15, act_delay_min=0, act_delay_max=15, act_noise_sigma=[1.0] * 8, act_fill=[-1.0] * 8, seed=2 ** 64 - 1),
               dict(obs_dim=1, groups=[_g(0, 1)]), dict(obs_dim=8, groups=[_g(4, 8), _g(0, 4)])):
        assert sensor_abi.create_status(sensor_abi.make_cconfig(**ok), 1 << 24) == (0, ""), ok
    c = sensor_abi.make_cconfig()
    c.abi_version = 2
    assert sensor_abi.create_status(c) == (-1, "config.abi_version: 2, this library is version 1")
    for name in ("reserved0", "reserved1"):
        c = sensor_abi.make_cconfig()
        setattr(c, name, 1)
        assert sensor_abi.create_status(c) == (-1, f"config.{name}: must be 0")
    c = sensor_abi.make_cconfig()
    c.n_groups = 5
    assert sensor_abi.create_status(c)[1].startswith("config.n_groups:")
    for field, value in (("begin", 1), ("end", 1), ("noise_sigma", 0.1), ("bias_half_width", 0.1), ("dropout_probability", 0.1), ("dropout_value", 0.1),
                         ("quantum", 0.1), ("quantum", NAN)):
        c = sensor_abi.make_cconfig(obs_dim=8, groups=[_g()])
        setattr(c.groups[2], field, value)
        rc, msg = sensor_abi.create_status(c)
        assert rc == -1 and msg.startswith(f"config.groups[2].{field}: must be 0 past"), msg
    h = C.c_void_p()
    assert lib.rg_sensor_create(None, 4, sensor_abi.DEVICE_NONE, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.rg_sensor_last_error(None)
    assert lib.rg_sensor_create(C.byref(sensor_abi.make_cconfig()), 4, sensor_abi.DEVICE_NONE, None) == -1


def _raises(status, *words):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(sensor_abi.RgSensorError)
            self.e = self.cm.__enter__()
            return self.e

        def __exit__(self, *a):
            out = self.cm.__exit__(*a)
            assert self.e.value.status == status, str(self.e.value)
            for w in words:
                assert w in str(self.e.value), (w, str(self.e.value))
            return out
    return Ctx()


def test_host_only_handle_checks_every_argument_by_name_then_reports_no_device():
    p = [0x1000 * (k + 1) for k in range(7)]      # stand-ins for addresses: a host-only handle never looks through them
    h = sensor_abi.SensorHandle(4, sensor_abi.DEVICE_NONE, obs_dim=8, act_dim=2, groups=[_g(noise_sigma=0.1)], obs_delay_max=2)
    assert h.device is None and h.batch == 4 and h.fields["obs_delay_max"] == 2
    names = ("mask", "sensor_state", "obs_clean", "obs_ring", "obs_out", "obs_prev", "act_ring")
    for k, name in enumerate(names):
        args = list(p)
        args[k] = None
        if name == "obs_prev":                      # optional
            with _raises(-3, "RG_SENSOR_DEVICE_NONE"):
                h.reset(*args)
        else:
            with _raises(-1, "reset", "null " + name):
                h.reset(*args)
    same = list(p)
    same[5] = same[4]
    with _raises(-1, "reset", "obs_prev must not be obs_out"):
        h.reset(*same)
    with _raises(-3, "RG_SENSOR_DEVICE_NONE"):
        h.reset(*p)
    for k, name in enumerate(("sensor_state", "obs_clean", "obs_ring", "obs_out")):
        args = list(p[:4])
        args[k] = None
        with _raises(-1, "observe", "null " + name):
            h.observe(*args)
    with _raises(-3, "RG_SENSOR_DEVICE_NONE"):
        h.observe(*p[:4])
    for k, name in enumerate(("sensor_state", "act_in", "act_ring", "act_out")):
        args = list(p[:4])
        args[k] = None
        with _raises(-1, "act", "null " + name):
            h.act(*args)
    with _raises(-3, "RG_SENSOR_DEVICE_NONE"):
        h.act(p[0], p[1], p[2], p[1])               # in place is allowed
    h.close()
    h.close()
    assert not h._h
    lib = sensor_abi.load_library()
    for call, n in (("reset", 9), ("observe", 6), ("act", 6)):
        assert getattr(lib, "rg_sensor_" + call)(None, *([0x1000] * (n - 1))) == -1 and b"null handle" in lib.rg_sensor_last_error(None), call


def test_wrapper_refuses_by_name_without_a_device():
    from robot_gym_amd.sim import SensorModel
    with pytest.raises(ValueError, match="obs_delay"):
        SensorModel(obs_delay=1)
    with pytest.raises(ValueError, match="act_delay"):
        SensorModel(act_delay=(0, 1, 2))
    with pytest.raises(TypeError, match="sigma"):
        SensorModel(path=dict(sigma=1.0))
    with pytest.raises(ValueError, match="not both"):
        SensorModel(path={}, groups=[])
    sm = SensorModel(path=dict(noise_sigma=0.1), obs_delay=(1, 3), act_delay=(0, 2), act_noise_sigma=(0.1, 0.2), act_fill=(0.5,), seed=7)
    assert sm.settings == dict(seed=7, obs_delay_min=1, obs_delay_max=3, act_delay_min=0, act_delay_max=2, act_noise_sigma=(0.1, 0.2), act_fill=(0.5,))
    for call in (lambda: sm.on_reset(None, None), lambda: sm.observe(None), lambda: sm.act(None), lambda: sm.delays, lambda: sm.copy_columns([0], [1])):
        with pytest.raises(RuntimeError, match="bind"):
            call()
    with pytest.raises(ValueError, match="path_rows"):
        sm.bind(4, sensor_abi.DEVICE_NONE, 8, 2)
    sm.close()


# ---- the stream ----------------------------------------------------------------------------------------------------------

def test_the_stream_is_the_episode_stream_and_the_vector_form_is_the_scalar_form():
    rng = np.random.default_rng(0)
    words = rng.integers(0, 2 ** 63, (200, 5), dtype=np.int64).tolist() + [[0, 0, 0, 0, 0], [2 ** 64 - 1, 2 ** 53, 7, 21, 2 ** 40], [3, 64, 1, 19, (5 << 12) | (7 << 2) | 3]]
    for seed, key, draw, purpose, index in words:
        assert SM.uniform(seed, key, draw, purpose, index) == EM.uniform(seed, key, draw, purpose, index)
    assert SM.mix64(12345) == EM.mix64(12345) and SM.GOLDEN == EM.GOLDEN
    w = np.array(words, dtype=object)
    for seed in (0, 12345, 2 ** 64 - 1):
        key, draw, purpose, index = (np.array([int(x) & SM.M64 for x in w[:, c]], dtype=U) for c in (1, 2, 3, 4))
        got = SM.vhash(seed, key, draw, purpose, index)
        assert got.tolist() == [SM.hash4(seed, int(a), int(b), int(c), int(d)) for a, b, c, d in zip(key, draw, purpose, index)]
        assert SM.vuniform(seed, key, draw, purpose, index).tolist() == [SM.uniform(seed, int(a), int(b), int(c), int(d)) for a, b, c, d in zip(key, draw, purpose, index)]
    k, row = np.array([0, 1, 77, 2 ** 40], dtype=U), np.array([0, 255, 3, 19], dtype=U)
    assert SM.vnoise(9, U(5), U(2), SM.NOISE, k, row).tolist() == [SM.noise(9, 5, 2, SM.NOISE, int(a), int(b)) for a, b in zip(k, row)]


def test_known_answers_worked_by_hand():
    # the first output of splitmix64 seeded with 0 (Vigna's reference implementation), and the all-zero chain of four rounds
    assert SM.mix64(SM.GOLDEN) == 0xE220A8397B1DCDAF and SM.hash4(0, 0, 0, 0, 0) == 0x2130748AAAC80268
    # the index word: k in the bits from 12 up, the row in bits 2..11, j in bits 0..1
    assert SM.ix(0, 0, 0) == 0 and SM.ix(1, 0, 0) == 4096 and SM.ix(0, 1, 0) == 4 and SM.ix(0, 0, 3) == 3 and SM.ix(5, 255, 3) == 5 * 4096 + 1023
    assert SM.ix(3, 19, 2) == 3 * 4096 + 19 * 4 + 2 == 12366 and SM.ix(2 ** 52, 0) == 0      # 2^64 wraps
    assert len({SM.ix(k, r, j) for k in range(3) for r in range(256) for j in range(4)}) == 3 * 256 * 4      # no two draws share a word
    # a noise draw is the four uniforms of j = 0..3, summed as two pairs
    u = [SM.uniform(4, 6, 1, SM.NOISE, 12366 - 2 + j) for j in range(4)]
    assert SM.noise(4, 6, 1, SM.NOISE, 3, 19) == (((u[0] + u[1]) + (u[2] + u[3])) - 2.0) * 1.7320508075688772
    # the delay draw at min == max: (double) 1 * u < 1 truncates to 0, min(0, 0) = 0
    for lo in (0, 1, 15):
        assert all(SM.delay_draw(s, k, d, SM.OBS_DELAY, lo, lo) == lo for s in (0, 9) for k in range(20) for d in range(3))
    assert SM.delay_draw(0, 0, 0, SM.OBS_DELAY, 2, 5) == 2 + int(4.0 * SM.uniform(0, 0, 0, 16, 0))
    # dropout at probability 1 (u < 1 always) and 0 (the step is skipped); quantisation ties to even
    clean = np.array([[0.5, 1.5, 2.5, -0.5, 0.125, 0.375, -7.3, 2.0 ** 30]], dtype=np.float32).T.copy()     # [8, 1]
    key, d, k = np.array([3], dtype=U), np.array([0], dtype=U), np.array([7], dtype=U)
    drop1 = SM.settings(obs_dim=8, groups=[(0, 8, dict(dropout_probability=1.0, dropout_value=-2.5))])
    assert (SM.measure(drop1, key, d, k, clean) == np.float32(-2.5)).all()
    drop0 = SM.settings(obs_dim=8, groups=[(0, 8, dict(dropout_probability=0.0, dropout_value=-2.5))])
    assert (SM.measure(drop0, key, d, k, clean).view(np.uint32) == clean.view(np.uint32)).all()
    q1 = SM.settings(obs_dim=8, groups=[(0, 8, dict(quantum=1.0))])
    assert SM.measure(q1, key, d, k, clean)[:, 0].tolist() == [0.0, 2.0, 2.0, -0.0, 0.0, 0.0, -7.0, 2.0 ** 30]
    assert np.signbit(SM.measure(q1, key, d, k, clean)[3, 0])                                         # -0.5 rounds to -0.0
    q4 = SM.settings(obs_dim=8, groups=[(0, 8, dict(quantum=0.25))])
    assert SM.measure(q4, key, d, k, clean)[:, 0].tolist() == [0.5, 1.5, 2.5, -0.5, 0.0, 0.5, -7.25, 2.0 ** 30]      # 0.125 / 0.25 = 0.5 -> 0, 1.5 -> 2
    # the bias of a row is the same on every tick and differs between draws; rows outside the group pass through
    b = SM.settings(obs_dim=8, seed=5, groups=[(2, 5, dict(bias_half_width=0.5))])
    m7, m8 = SM.measure(b, key, d, k, clean), SM.measure(b, key, d, k + U(1), clean)
    want = clean.astype(np.float64)[2:5, 0] + 0.5 * (2.0 * np.array([SM.uniform(5, 3, 0, SM.BIAS, r) for r in (2, 3, 4)]) - 1.0)
    assert (m7 == m8).all() and (m7[2:5, 0] == want.astype(np.float32)).all() and (m7[[0, 1, 5, 6, 7]] == clean[[0, 1, 5, 6, 7]]).all()
    assert not (SM.measure(b, key, d + U(1), k, clean)[2:5] == m7[2:5]).any()
    assert SM.words(-1.0) == 2 ** 64 - 1 and SM.words(2.0 ** 40) == 2 ** 40
    assert SM.bounded([np.nan, -3.0, 2.0, 99.0], 15).tolist() == [0, 0, 2, 15]


# ---- properties of the model ---------------------------------------------------------------------------------------------

def test_noise_draws_have_zero_mean_unit_variance_and_bounded_support():
    N = 200_000
    key = (np.arange(N, dtype=U) % U(400))
    k = (np.arange(N, dtype=U) // U(400))
    n = SM.vnoise(17, key, U(3), SM.NOISE, k, U(11))
    # the mean within five standard errors (its variance is 1 / N).  The sample variance within 5 * sqrt(1.4 / N): an
    # Irwin-Hall(4) draw scaled to unit variance has fourth moment 3 - 6 / 20 = 2.7, so the variance of the sample variance is
    # 1.7 / N and this bound is 4.5 of its standard errors, a little tighter than five
    assert abs(n.mean()) < 5.0 / np.sqrt(N), n.mean()
    assert abs(n.var() - 1.0) < 5.0 * np.sqrt(1.4 / N), n.var()
    assert np.abs(n).max() <= 3.4642 and np.abs(n).max() > 2.5
    assert abs((n ** 4).mean() - 2.7) < 0.1
    # white: neighbouring ticks, rows and keys do not correlate (five standard errors of a correlation, 1 / sqrt N)
    for other in (SM.vnoise(17, key, U(3), SM.NOISE, k + U(1), U(11)), SM.vnoise(17, key, U(3), SM.NOISE, k, U(12)), SM.vnoise(17, key + U(1), U(3), SM.NOISE, k, U(11)),
                  SM.vnoise(17, key, U(3), SM.ACT_NOISE, k, U(11))):
        assert abs(np.mean(n * other)) < 5.0 / np.sqrt(N)


@pytest.mark.parametrize("p", [0.01, 0.3, 0.9])
def test_dropout_frequency_is_within_five_standard_errors(p):
    B, T, D = 500, 50, 8
    cfg = SM.settings(obs_dim=D, seed=2, groups=[(0, D, dict(dropout_probability=p, dropout_value=-9.0))])
    buf = SM.new_buffers(cfg, B)
    clean = np.ones((D, B), dtype=np.float32)
    SM.reset(cfg, np.ones(B), buf, clean)
    hits = int((buf["obs_out"] == -9.0).sum())
    for _ in range(T - 1):
        SM.observe(cfg, buf, clean)
        hits += int((buf["obs_out"] == -9.0).sum())
    n = B * T * D
    assert abs(hits / n - p) < 5.0 * np.sqrt(p * (1.0 - p) / n), (hits / n, p)


def test_delay_draws_cover_exactly_min_to_max_and_stay_for_the_episode():
    B = 400
    cfg = SM.settings(obs_dim=2, act_dim=2, seed=8, obs_delay_min=1, obs_delay_max=4, act_delay_min=0, act_delay_max=15)
    buf = SM.new_buffers(cfg, B)
    clean = np.zeros((2, B), dtype=np.float32)
    seen = []
    for episode in range(3):
        SM.reset(cfg, np.ones(B), buf, clean)
        od, ad = buf["state"][SM.ROW_OBS_DELAY].copy(), buf["state"][SM.ROW_ACT_DELAY].copy()
        assert set(od.tolist()) == {1.0, 2.0, 3.0, 4.0} and set(ad.tolist()) == set(float(x) for x in range(16))
        assert [od[b] for b in range(5)] == [SM.delay_draw(8, b, episode, SM.OBS_DELAY, 1, 4) for b in range(5)]
        for _ in range(3):
            SM.observe(cfg, buf, clean)
            SM.act(cfg, buf, np.zeros((B, 2), dtype=np.float32))
        assert (buf["state"][SM.ROW_OBS_DELAY] == od).all() and (buf["state"][SM.ROW_ACT_DELAY] == ad).all()
        assert (buf["state"][SM.ROW_OBS_TICKS] == 4).all() and (buf["state"][SM.ROW_ACT_TICKS] == 3).all() and (buf["state"][SM.ROW_DRAWS] == episode + 1).all()
        seen.append(od)
    assert not (seen[0] == seen[1]).all() and (buf["state"][6:] == 0).all() and (buf["state"][SM.ROW_KEY] == np.arange(B)).all()
    counts = np.bincount(np.concatenate(seen).astype(int), minlength=5)[1:]
    assert (np.abs(counts - 300) < 5 * np.sqrt(1200 * 0.25 * 0.75)).all()      # uniform over the four values


def test_latency_delivers_the_measurement_of_d_ticks_ago_and_a_young_robot_sees_its_first():
    B, D, T = 6, 3, 12
    cfg = SM.settings(obs_dim=D, act_dim=2, seed=1, obs_delay_min=0, obs_delay_max=3, act_delay_min=0, act_delay_max=2, act_fill=[0.25, -0.5])
    buf = SM.new_buffers(cfg, B)
    clean = lambda t: (np.arange(D * B, dtype=np.float32).reshape(D, B) + 100.0 * t)      # noqa: E731
    action = lambda t: (np.arange(B * 2, dtype=np.float32).reshape(B, 2) + 100.0 * t)      # noqa: E731
    SM.reset(cfg, np.ones(B), buf, clean(0))
    od, ad = buf["state"][SM.ROW_OBS_DELAY].astype(int), buf["state"][SM.ROW_ACT_DELAY].astype(int)
    assert len(set(od)) > 1 and len(set(ad)) > 1
    for t in range(1, T):
        out = SM.act(cfg, buf, action(t - 1))
        for b in range(B):
            first = t - 1 - ad[b]
            assert (out[b] == (action(first)[b] if first >= 0 else np.array([0.25, -0.5], dtype=np.float32))).all(), (t, b)
        SM.observe(cfg, buf, clean(t))
        for b in range(B):
            assert (buf["obs_out"][:, b] == clean(max(t - od[b], 0))[:, b]).all(), (t, b)


def test_a_robot_outside_the_mask_is_untouched_and_streams_follow_the_key():
    B = 8
    cfg = SM.settings(obs_dim=4, act_dim=2, seed=3, groups=[(0, 4, dict(noise_sigma=0.1, bias_half_width=0.2))], obs_delay_max=2, act_delay_max=1,
                      act_noise_sigma=[0.1, 0.2])
    rng = np.random.default_rng(0)
    clean = rng.standard_normal((4, B)).astype(np.float32)
    buf = SM.new_buffers(cfg, B, keys=[9, 7, 7, 3, 4, 5, 6, 8])
    for v in buf.values():
        v[:] = rng.standard_normal(v.shape)
    buf["state"][SM.ROW_KEY] = [9, 7, 7, 3, 4, 5, 6, 8]
    buf["state"][SM.ROW_DRAWS] = 2.0
    before = {n: v.copy() for n, v in buf.items()}
    prev = np.full((4, B), 5.0, dtype=np.float32)
    mask = np.array([1, 1, 1, 0, 0, 1, 0, 0])
    SM.reset(cfg, mask, buf, np.repeat(clean[:, :1], B, axis=1), prev)
    off = mask == 0
    for n, v in buf.items():
        assert (v[..., off] == before[n][..., off]).all(), n
    assert (prev[:, off] == 5.0).all() and (prev[:, ~off] == before["obs_out"][:, ~off]).all()
    assert (buf["obs_out"][:, 1] == buf["obs_out"][:, 2]).all() and not (buf["obs_out"][:, 0] == buf["obs_out"][:, 1]).any()      # same key, same stream
    assert (buf["state"][1:6, 1] == buf["state"][1:6, 2]).all() and (buf["state"][SM.ROW_DRAWS, ~off] == 3).all()


# ---- resources of rg_sensor.hip --------------------------------------------------------------------------------------------

KERNELS = {"rg_sensor_reset_kernel", "rg_sensor_observe_kernel", "rg_sensor_act_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_sensor.hip")


def test_exactly_the_three_kernels_are_reported(remarks):
    assert set(remarks) == KERNELS


def test_the_kernels_use_no_scratch_no_spills_and_no_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds).  reset and observe hold the settings of four groups in scalar
# registers and one row's hashes in flight; act holds one hash prefix.
REGISTERS = {"rg_sensor_reset_kernel": dict(vgprs=36, sgprs=95, agprs=0, occupancy=8), "rg_sensor_observe_kernel": dict(vgprs=46, sgprs=95, agprs=0, occupancy=8),
             "rg_sensor_act_kernel": dict(vgprs=30, sgprs=28, agprs=0, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    src = open(os.path.join(SRC, "rg_sensor.hip")).read()
    code = re.sub(r"//.*", "", src)
    pragma = code.index("#pragma clang fp contract(off)")
    assert pragma < code.index("__global__") and pragma < code.index("__device__")
    assert "asm" not in code and "atomic" not in code.lower() and "__shared__" not in src and "__shfl" not in src
    stream = open(os.path.join(SRC, "rg_stream_dev.inc")).read()                 # the stream's device functions, included after the pragma
    assert "__global__" not in stream and '#include "' not in stream and "asm" not in re.sub(r"//.*", "", stream) and "atomic" not in stream.lower()
    for call in ("sin(", "cos(", "pow(", "exp(", "sqrt(", "log(", "fma("):
        assert call not in code and call not in stream, call
    assert len(re.findall(r"__global__", code)) == len(KERNELS) and code.count("__launch_bounds__(kBlock)") == 3 and "kBlock = 256" in code
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_sensor.h", "rg_host.h", "rg_stream_dev.inc"]
    assert pragma < code.index('#include "rg_stream_dev.inc"') < code.index("__device__")
    # one barrier in each kernel that gives a robot several lanes, and it comes before the first store of the kernel
    for kernel in ("rg_sensor_reset_kernel", "rg_sensor_observe_kernel"):
        body = code[code.index(kernel + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("__syncthreads()") == 1 and "return" not in body[:body.index("__syncthreads()")]
        assert not re.search(r"\]\s*=[^=]", body[:body.index("__syncthreads()")]), kernel
    for other in sorted(os.listdir(SRC)):                                        # included from nowhere
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_sensor.hip":
            assert "rg_sensor" not in open(os.path.join(SRC, other)).read(), other
    import bench
    assert not any("rg_sensor" in rel for rel in bench.compiled_sources())       # the MPC hash behind profiles/ does not follow it
    kernel_checks.assert_built_into_both("rg_sensor.hip", header="rg_sensor.h")


def test_the_documents_no_longer_list_sensor_effects_as_missing():
    for rel in ("include/rg_dr.h", "robot_gym_amd/sim/randomizer.py", "README.md", "INTEGRATION.md", "include/rg_scan.h", "robot_gym_amd/sim/height_scan.py"):
        text = " ".join(open(os.path.join(ROOT, rel)).read().split())
        for gone in ("observation or action noise", "no sensor noise"):
            assert gone not in text, (rel, gone)
