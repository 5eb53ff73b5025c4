"""The domain randomisation of include/rg_dr.h without a GPU: the binding against the header and the library, what
rg_dr_create and the entries refuse (by name), the host-only handle, the stream of tests/dr_model.py against
tests/episode_model.py and known answers, the properties of the model, and the resources of robot_gym_amd/csrc/rg_dr.hip from
one device-only compile.  The batch check of rg_dr_capture_body needs a simulator handle, which needs a device: it is in
tests/test_dr_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import dr_abi
from tests import dr_model as DM
from tests import episode_model as EM
from tests import kernel_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")


# ---- the binding -------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rg_dr.h")).read(), flags=re.S)


def test_library_exports_every_declared_entry():
    lib = dr_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_dr_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(dr_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rg_dr_abi_version() == dr_abi.ABI_VERSION == 1
    assert lib.rg_dr_state_rows() == dr_abi.ROWS == DM.ROWS == 8


def test_config_layout_size_and_constants_match_the_header():
    hdr = _header()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", hdr))["rg_dr_config"]
    fields = [(t, n) for t, n in re.findall(r"\b(int32_t|uint64_t|double)\s+(\w+)\s*;", body)]
    ctype = {"int32_t": C.c_int32, "uint64_t": C.c_uint64, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(dr_abi.CConfig._fields_)
    assert dr_abi.load_library().rg_dr_config_size() == C.sizeof(dr_abi.CConfig) == 2 * 4 + 8 + 4 * 8 + 2 * 4 + 5 * 8 + 2 * 4
    off = 0
    for t, n in fields:     # naturally aligned with no padding anywhere
        assert getattr(dr_abi.CConfig, n).offset == off, n
        off += C.sizeof(ctype[t])
    defs = {k: v for k, v in re.findall(r"#define (RG_DR_\w+) (\(?-?[\d< ]+\)?)", hdr)}
    assert int(defs["RG_DR_ROWS"]) == dr_abi.ROWS and int(defs["RG_DR_BODY_ROWS"]) == dr_abi.BODY_ROWS == DM.BODY_ROWS == 19
    rows = [int(defs[f"RG_DR_ROW_{n}"]) for n in ("KEY", "DRAWS", "MASS_SCALE", "INERTIA_SCALE", "WORLD")]
    assert rows == [dr_abi.ROW_KEY, dr_abi.ROW_DRAWS, dr_abi.ROW_MASS_SCALE, dr_abi.ROW_INERTIA_SCALE, dr_abi.ROW_WORLD] == list(range(5))
    assert rows == [DM.ROW_KEY, DM.ROW_DRAWS, DM.ROW_MASS_SCALE, DM.ROW_INERTIA_SCALE, DM.ROW_WORLD]
    purposes = [int(defs[f"RG_DR_PURPOSE_{n}"]) for n in ("MASS", "INERTIA", "WORLD", "PUSH_START", "PUSH_COMPONENT", "PUSH_GATE")]
    assert purposes == list(range(6)) == [DM.MASS, DM.INERTIA, DM.WORLD, DM.PUSH_START, DM.PUSH_COMPONENT, DM.PUSH_GATE]
    assert defs["RG_DR_DEVICE_NONE"] == "(-1)" and dr_abi.DEVICE_NONE == -1
    status = dict(re.findall(r"RG_DR_(OK|ERR_\w+) = (-?\d+)", hdr))
    assert {k.replace("ERR_", ""): int(v) for k, v in status.items()} == {v: k for k, v in dr_abi.STATUS.items()}


def test_the_defaults_are_the_identity():
    c = dr_abi.make_cconfig()
    assert (c.mass_lo, c.mass_hi, c.inertia_lo, c.inertia_hi) == (1.0, 1.0, 1.0, 1.0)
    assert (c.worlds, c.seed, c.push_interval, c.push_ticks, c.push_probability) == (0, 0, 0, 0, 0.0)
    assert (c.push_force_xy, c.push_force_z, c.push_torque_xy, c.push_torque_z) == (0.0, 0.0, 0.0, 0.0) and c.substeps == 10
    assert dr_abi.DEFAULTS == DM.DEFAULTS
    assert dr_abi.create_status(c, 4) == (0, "")
    assert dr_abi.make_cconfig(seed=-1).seed == 2 ** 64 - 1
    with pytest.raises(TypeError, match="bogus"):
        dr_abi.make_cconfig(bogus=1)
    from robot_gym_amd.sim import DomainRandomizer
    assert {**dr_abi.DEFAULTS, **DomainRandomizer().settings} == dr_abi.DEFAULTS      # the wrapper's defaults are the library's


NAN, INF = float("nan"), float("inf")
PUSH = dict(push_interval=8, push_ticks=3)
BAD = [(dict(mass_lo=0.0), 4, "config.mass_lo"), (dict(mass_lo=-1.0), 4, "config.mass_lo"), (dict(mass_hi=INF), 4, "config.mass_hi"),
       (dict(mass_lo=NAN), 4, "config.mass_lo"), (dict(mass_lo=1.5, mass_hi=1.25), 4, "config.mass_hi"),
       (dict(inertia_lo=0.0), 4, "config.inertia_lo"), (dict(inertia_hi=NAN), 4, "config.inertia_hi"),
       (dict(inertia_lo=2.0, inertia_hi=1.0), 4, "config.inertia_hi"), (dict(worlds=2), 4, "config.worlds"), (dict(worlds=-1), 4, "config.worlds"),
       (dict(push_interval=-1), 4, "config.push_interval"), (dict(push_interval=8, push_ticks=9), 4, "config.push_ticks"),
       (dict(push_interval=8, push_ticks=0), 4, "config.push_ticks"), (dict(push_interval=0, push_ticks=1), 4, "config.push_ticks"),
       (dict(push_ticks=-1), 4, "config.push_ticks"), (dict(PUSH, push_probability=1.5), 4, "config.push_probability"),
       (dict(PUSH, push_probability=-0.1), 4, "config.push_probability"), (dict(PUSH, push_probability=NAN), 4, "config.push_probability"),
       (dict(push_force_xy=-1.0), 4, "config.push_force_xy"), (dict(push_force_z=INF), 4, "config.push_force_z"),
       (dict(push_torque_xy=NAN), 4, "config.push_torque_xy"), (dict(push_torque_z=-1e-9), 4, "config.push_torque_z"),
       (dict(substeps=0), 4, "config.substeps"), (dict(substeps=1025), 4, "config.substeps"), ({}, 0, "batch"), ({}, (1 << 24) + 1, "batch")]


@pytest.mark.parametrize("change,batch,field", BAD)
def test_create_refuses_naming_the_field(change, batch, field):
    rc, msg = dr_abi.create_status(dr_abi.make_cconfig(**change), batch)
    assert rc == -1 and msg.startswith(field + ":"), (rc, msg)


def test_create_accepts_the_edges_and_refuses_version_reserved_word_and_null():
    lib = dr_abi.load_library()
    for ok in (dict(mass_lo=0.5, mass_hi=0.5), dict(push_interval=8, push_ticks=8, push_probability=1.0), dict(push_interval=1, push_ticks=1),
               dict(substeps=1024, worlds=1, seed=2 ** 64 - 1), dict(push_interval=2 ** 31 - 1, push_ticks=1)):
        assert dr_abi.create_status(dr_abi.make_cconfig(**ok), 1 << 24) == (0, ""), ok
    c = dr_abi.make_cconfig()
    c.abi_version = 2
    assert dr_abi.create_status(c) == (-1, "config.abi_version: 2, this library is version 1")
    c = dr_abi.make_cconfig()
    c.reserved0 = 1
    assert dr_abi.create_status(c) == (-1, "config.reserved0: must be 0")
    h = C.c_void_p()
    assert lib.rg_dr_create(None, 4, dr_abi.DEVICE_NONE, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.rg_dr_last_error(None)
    assert lib.rg_dr_create(C.byref(dr_abi.make_cconfig()), 4, dr_abi.DEVICE_NONE, None) == -1


def _raises(status, *words):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(dr_abi.RgDrError)
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
    a, b, c, k = 0x1000, 0x2000, 0x3000, 0x4000      # stand-ins for addresses: a host-only handle never looks through them
    h = dr_abi.DrHandle(4, dr_abi.DEVICE_NONE, **PUSH, push_probability=0.5)
    assert h.device is None and h.batch == 4 and h.fields["push_interval"] == 8
    with _raises(-1, "capture_body", "null srb"):
        h.capture_body(None)
    for args, name in (((None, a, b, None), "srb"), ((a, None, b, None), "mask"), ((a, b, None, None), "dr_state")):
        with _raises(-1, "reset", "null " + name):
            h.reset(*args)
    srb = C.create_string_buffer(8192)      # zeroed memory where a simulator handle would be: the rules below are decided before it is read
    with _raises(-1, "reset", "terrain_key must be null", "worlds"):      # a key without worlds
        h.reset(C.addressof(srb), b, c, k)
    for args, name in (((None, None, b), "srb"), ((a, None, None), "dr_state")):
        with _raises(-1, "apply", "null " + name):
            h.apply(*args)
    for args, name in (((None, b, c), "sim_state"), ((a, None, c), "dr_state"), ((a, b, None), "ext")):
        with _raises(-1, "push", "null " + name):
            h.push(*args)
    with _raises(-3, "RG_DR_DEVICE_NONE"):
        h.push(a, b, c)
    for args, name in (((None, a), "srb"), ((a, None), "out")):
        with _raises(-1, "get_body", "null " + name):
            h.get_body(*args)
    h.close()
    h.close()
    assert not h._h
    # worlds without a key, and push with interval 0
    w = dr_abi.DrHandle(4, dr_abi.DEVICE_NONE, worlds=1)
    with _raises(-1, "reset", "null terrain_key", "worlds"):
        w.reset(C.addressof(srb), b, c, None)
    with _raises(-1, "push", "push_interval"):
        w.push(a, b, c)
    w.close()
    lib = dr_abi.load_library()
    for call, args in (("capture_body", (None, a)), ("reset", (None, a, b, c, None, None)), ("apply", (None, a, None, c, None)),
                       ("push", (None, a, b, c, None)), ("get_body", (None, a, b, None))):
        assert getattr(lib, "rg_dr_" + call)(*args) == -1 and b"null handle" in lib.rg_dr_last_error(None), call


# ---- the stream ----------------------------------------------------------------------------------------------------------

def test_the_stream_is_the_episode_stream_on_the_same_four_words():
    rng = np.random.default_rng(0)
    words = rng.integers(0, 2 ** 63, (200, 5), dtype=np.int64)
    for seed, key, draw, purpose, index in words.tolist() + [[0, 0, 0, 0, 0], [2 ** 64 - 1, 2 ** 53, 7, 5, 2 ** 40], [3, 64, 1, 4, 8 * 5 + 3]]:
        assert DM.uniform(seed, key, draw, purpose, index) == EM.uniform(seed, key, draw, purpose, index)
    assert DM.mix64(12345) == EM.mix64(12345) and DM.GOLDEN == EM.GOLDEN


def test_known_answers_of_the_stream():
    # the first output of splitmix64 seeded with 0 (Vigna's reference implementation): one round of the chain on zero words
    assert DM.mix64(DM.GOLDEN) == 0xE220A8397B1DCDAF
    # the all-zero words: four rounds, each h = mix((h ^ 0) + GOLDEN); restated by hand in tests/test_stream_cpu.py
    assert DM.hash4(0, 0, 0, 0, 0) == 0x2130748AAAC80268
    assert DM.uniform(0, 0, 0, 0, 0) == float.fromhex("0x1.0983a45556400p-3") == (0x2130748AAAC80268 >> 11) / 2 ** 53
    # one key (5) of seed 12345: the world of its first draw, a push component, and its first scales
    assert DM.hash4(12345, 5, 0, DM.WORLD, 0) == 0x40153532777E0227 and 0x40153532777E0227 >> 33 == 537565849 < 2 ** 31
    assert DM.uniform(12345, 5, 1, DM.PUSH_COMPONENT, 19) == float.fromhex("0x1.fbcc85a234504p-2")
    cfg = DM.settings(seed=12345, mass_lo=0.8, mass_hi=1.2, inertia_lo=0.5, inertia_hi=2.0)
    assert DM.draw_scales(cfg, 5, 0) == (float.fromhex("0x1.ea0274e79b111p-1"), float.fromhex("0x1.77c5016103ffdp+0"))
    assert DM.word(-1.0) == 2 ** 64 - 1 and DM.word(2.0 ** 40) == 2 ** 40


# ---- properties of the model ---------------------------------------------------------------------------------------------

def _base(B, seed=1):
    rng = np.random.default_rng(seed)
    base = np.empty((DM.BODY_ROWS, B))
    base[0] = rng.uniform(5, 30, B)
    for b in range(B):
        A = rng.uniform(-0.1, 0.1, (3, 3))
        inertia = np.diag(rng.uniform(0.1, 1.0, 3)) + A @ A.T
        base[1:10, b], base[10:19, b] = inertia.ravel(), np.linalg.inv(inertia).ravel()
    return base


def test_scales_lie_in_their_ranges_and_a_point_range_is_exact():
    B = 257
    cfg = DM.settings(seed=9, mass_lo=0.8, mass_hi=1.2, inertia_lo=0.5, inertia_hi=2.0)
    st, base = DM.new_state(B), _base(B)
    body = base.copy()
    for _ in range(4):
        DM.reset(cfg, np.ones(B), st, base, body)
        assert (st[DM.ROW_MASS_SCALE] >= 0.8).all() and (st[DM.ROW_MASS_SCALE] <= 1.2).all()
        assert (st[DM.ROW_INERTIA_SCALE] >= 0.5).all() and (st[DM.ROW_INERTIA_SCALE] <= 2.0).all()
        assert (body[0] == base[0] * st[DM.ROW_MASS_SCALE]).all() and (body[10:] == base[10:] / st[DM.ROW_INERTIA_SCALE]).all()
        assert len(np.unique(st[DM.ROW_MASS_SCALE])) == B                     # every robot its own
    assert (st[DM.ROW_DRAWS] == 4).all() and (st[DM.ROW_WORLD] == 0).all() and (st[5:] == 0).all()
    point = DM.settings(seed=9, mass_lo=0.7, mass_hi=0.7, inertia_lo=1.3, inertia_hi=1.3)
    DM.reset(point, np.ones(B), st, base, body)
    assert (st[DM.ROW_MASS_SCALE] == 0.7).all() and (st[DM.ROW_INERTIA_SCALE] == 1.3).all()
    ident = DM.settings(seed=9)
    DM.reset(ident, np.ones(B), st, base, body)
    assert (body == base).all()                                               # x * 1.0 and x / 1.0 are x


def test_worlds_are_31_bit_keys_written_for_masked_robots_only():
    B = 64
    cfg = DM.settings(seed=2, worlds=1)
    st, base = DM.new_state(B, world=np.arange(B)), _base(B)
    body, keys = base.copy(), np.arange(B, dtype=np.int64)
    mask = (np.arange(B) % 3 == 0).astype(np.int32)
    DM.reset(cfg, mask, st, base, body, keys)
    on = mask != 0
    assert (keys[~on] == np.arange(B)[~on]).all() and (st[DM.ROW_WORLD] == keys).all() and (st[DM.ROW_DRAWS] == on).all()
    assert (keys[on] >= 0).all() and (keys[on] < 2 ** 31).all() and len(np.unique(keys[on])) == on.sum()


def test_every_window_has_exactly_push_ticks_consecutive_active_ticks_or_none():
    cfg1 = DM.settings(seed=4, push_interval=8, push_ticks=3, push_probability=1.0, push_force_xy=1.0, push_force_z=2.0, push_torque_xy=3.0,
                       push_torque_z=4.0, substeps=10)
    cfg0 = dict(cfg1, push_probability=0.0)
    amp = np.array(DM.amplitudes(cfg1))
    starts = set()
    for key in range(257):
        for win in range(6):
            start, gate = DM.push_window(cfg1, key, 3, win)
            assert gate and 0 <= start and start + cfg1["push_ticks"] <= cfg1["push_interval"]
            starts.add(start)
            cols = [DM.push_one(cfg1, key, 3, float((win * 8 + r) * 10 + (r % 10))) for r in range(8)]      # steps that are no multiple of substeps
            active = [bool(np.any(c != 0)) for c in cols]
            assert active == [start <= r < start + 3 for r in range(8)], (key, win)
            on = [c for c, a in zip(cols, active) if a]
            assert all((c == on[0]).all() for c in on) and (np.abs(on[0]) <= amp).all() and np.all(on[0] != 0)      # constant over the push
            assert not any(np.any(DM.push_one(cfg0, key, 3, float((win * 8 + r) * 10))) for r in range(8))
    assert starts == set(range(6))                                            # every start from 0 to interval - ticks occurs
    half = dict(cfg1, push_probability=0.5)
    gates = [DM.push_window(half, key, 0, win)[1] for key in range(257) for win in range(4)]
    assert 0.4 < np.mean(gates) < 0.6


def test_push_steps_are_clamped():
    cfg = DM.settings(seed=4, push_interval=8, push_ticks=8, push_probability=1.0, push_force_xy=1.0, substeps=10)
    assert DM.tick_of(np.nan, 10) == DM.tick_of(-5.0, 10) == DM.tick_of(9.0, 10) == 0 and DM.tick_of(25.0, 10) == 2
    assert DM.tick_of(1e300, 10) == DM.tick_of(np.inf, 10) == 2 ** 52 // 10
    zero = DM.push_one(cfg, 1, 0, 0.0)
    assert (DM.push_one(cfg, 1, 0, np.nan) == zero).all() and (DM.push_one(cfg, 1, 0, -3.0) == zero).all() and zero[0] != 0


def test_draws_of_a_robot_do_not_depend_on_the_masks_of_the_others():
    B = 16
    cfg = DM.settings(seed=6, worlds=1, mass_lo=0.8, mass_hi=1.2, inertia_lo=0.9, inertia_hi=1.1, push_interval=8, push_ticks=3, push_probability=0.5,
                      push_force_xy=10.0)
    base = _base(B)
    rng = np.random.default_rng(3)
    histories = []
    for trial in range(3):
        st, body, keys = DM.new_state(B, world=np.arange(B)), base.copy(), np.arange(B, dtype=np.int64)
        seen = []
        for step in range(12):
            mask = rng.integers(0, 2, B).astype(np.int32)
            mask[7] = int(step % 3 == 0)                                      # robot 7: the same history in every trial
            DM.reset(cfg, mask, st, base, body, keys)
            sim = np.zeros((43, B))
            sim[DM.STEPS_ROW] = 10.0 * step
            seen.append((st[:, 7].copy(), body[:, 7].copy(), int(keys[7]), DM.push(cfg, sim, st)[:, 7].copy()))
        histories.append(seen)
    for other in histories[1:]:
        for x, y in zip(histories[0], other):
            assert (x[0] == y[0]).all() and (x[1] == y[1]).all() and x[2] == y[2] and (x[3] == y[3]).all()
    # and a robot's stream is its key's, wherever it sits
    st = DM.new_state(4, keys=[9, 7, 7, 3])
    DM.reset(cfg, np.ones(4), st, _base(4)[:, [0, 1, 1, 3]], np.zeros((19, 4)), np.zeros(4, dtype=np.int64))
    assert (st[1:, 1] == st[1:, 2]).all() and not (st[2:5, 0] == st[2:5, 1]).any()


def test_apply_skips_scales_that_are_not_finite_and_positive():
    B = 6
    base = _base(B)
    st = DM.new_state(B)
    st[DM.ROW_MASS_SCALE] = [1.1, np.nan, 0.9, -1.0, np.inf, 1.0]
    st[DM.ROW_INERTIA_SCALE] = [0.9, 1.0, 0.0, 1.0, 1.0, 2.0]
    body = np.full((19, B), 7.0)
    DM.apply(None, st, base, body)
    assert (body[:, [1, 2, 3, 4]] == 7.0).all()
    assert (body[:, 0] == DM.scaled_body(base, 0, 1.1, 0.9)).all() and (body[10:, 5] == base[10:, 5] / 2.0).all()
    body[:] = 7.0
    DM.apply(np.array([0, 0, 0, 0, 0, 1]), st, base, body)
    assert (body[:, :5] == 7.0).all() and (body[0, 5] == base[0, 5]).all()


def test_wrapper_refuses_by_name_without_a_device():
    from robot_gym_amd.sim import DomainRandomizer
    with pytest.raises(ValueError, match="mass_scale"):
        DomainRandomizer(mass_scale=1.0)
    with pytest.raises(ValueError, match="inertia_scale"):
        DomainRandomizer(inertia_scale=(1.0, 2.0, 3.0))
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), new_world_each_episode=True, seed=5, push_interval=8, push_ticks=3)
    assert dr.settings["worlds"] == 1 and dr.settings["mass_lo"] == 0.8 and dr.pushing and set(dr.settings) | {"substeps"} == set(dr_abi.DEFAULTS)
    for call in (lambda: dr.on_reset(None), dr.pushes, dr.apply, dr.body, lambda: dr.scales, lambda: dr.copy_columns([0], [1]), lambda: dr.set_body(mass=[1.0])):
        with pytest.raises(RuntimeError, match="bind"):
            call()
    dr.close()


# ---- resources of rg_dr.hip ------------------------------------------------------------------------------------------------

KERNELS = {"rg_dr_reset_kernel", "rg_dr_apply_kernel", "rg_dr_push_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_dr.hip")


def test_exactly_the_three_kernels_are_reported(remarks):
    assert set(remarks) == KERNELS


def test_the_kernels_use_no_scratch_and_no_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds): reset and apply hold a robot's 19 base values and their
# addresses in flight; push holds one hash prefix and six outputs.
REGISTERS = {"rg_dr_reset_kernel": dict(vgprs=50, agprs=0, occupancy=8), "rg_dr_apply_kernel": dict(vgprs=55, agprs=0, occupancy=8),
             "rg_dr_push_kernel": dict(vgprs=16, agprs=0, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_source_is_its_own_translation_unit_in_both_library_targets():
    src = open(os.path.join(SRC, "rg_dr.hip")).read()
    code = re.sub(r"//.*", "", src)
    pragma = code.index("#pragma clang fp contract(off)")
    assert pragma < code.index('#include "rg_mpc_dev.h"') < code.index('#include "rg_srb_dev.inc"') < code.index('#include "rg_srb_handle.h"')
    assert pragma < code.index("__global__") and pragma < code.index("__device__")
    assert "asm" not in code and "atomic" not in src.lower() and "__shared__" not in src and "__shfl" not in src
    stream = open(os.path.join(SRC, "rg_stream_dev.inc")).read()                 # the stream's device functions, included after the pragma
    assert "__global__" not in stream and '#include "' not in stream and "asm" not in re.sub(r"//.*", "", stream) and "atomic" not in stream.lower()
    for call in ("sin(", "cos(", "pow(", "exp(", "sqrt(", "fma("):
        assert call not in code and call not in stream, call
    assert len(re.findall(r"__global__", code)) == len(KERNELS) and code.count("__launch_bounds__(kBlock)") == 3 and "kBlock = 256" in code
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_dr.h", "rg_host.h", "rg_mpc_dev.h", "rg_srb_dev.inc", "rg_srb_handle.h",
                                                      "rg_stream_dev.inc"]
    assert pragma < code.index('#include "rg_stream_dev.inc"') < code.index("__device__")
    for other in sorted(os.listdir(SRC)):                                        # included from nowhere
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_dr.hip":
            assert "rg_dr" not in open(os.path.join(SRC, other)).read(), other
    # the simulator's ABI did not move
    srb = open(os.path.join(ROOT, "include", "rg_srb.h")).read()
    assert "#define RG_SRB_ABI_VERSION 1" in srb and "rg_dr" not in srb
    import bench
    assert not any("rg_dr" in rel for rel in bench.compiled_sources())           # the MPC hash behind profiles/ does not follow it
    kernel_checks.assert_built_into_both("rg_dr.hip", header="rg_dr.h")
