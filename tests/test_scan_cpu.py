"""The height scan of include/rg_scan.h without a GPU: the binding against the header and the library, what rg_scan_create and
rg_scan_set_terrain refuse, the host-only handle, known answers of the numpy model (tests/scan_model.py) and the resources of
robot_gym_amd/csrc/rg_scan.hip from one device-only compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import scan_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import kernel_checks
from tests import scan_model as SM
from tests import terrain_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")


# ---- the binding -------------------------------------------------------------------------------------------------------

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rg_scan.h")).read(), flags=re.S)


def test_library_exports_every_declared_entry():
    lib = scan_abi.load_library()
    declared = sorted(set(re.findall(r"\b(rg_scan_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(scan_abi.EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.rg_scan_abi_version() == scan_abi.ABI_VERSION == 1


def test_config_layout_and_size_match_the_header():
    hdr = _header()
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", hdr))["rg_scan_config"]
    fields = [(t, n) for t, n in re.findall(r"\b(int32_t|double)\s+(\w+)\s*;", body)]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(scan_abi.CConfig._fields_)
    assert scan_abi.load_library().rg_scan_config_size() == C.sizeof(scan_abi.CConfig) == 4 * 4 + 7 * 8 + 2 * 4
    off = 0
    for t, n in fields:     # naturally aligned with no padding anywhere
        assert getattr(scan_abi.CConfig, n).offset == off, n
        off += C.sizeof(ctype[t])
    defs = {k: v for k, v in re.findall(r"#define (RG_SCAN_\w+) (\(?-?[\d< ]+\)?)", hdr)}
    assert int(defs["RG_SCAN_MAX_POINTS"]) == scan_abi.MAX_POINTS == 256
    assert defs["RG_SCAN_DEVICE_NONE"] == "(-1)" and scan_abi.DEVICE_NONE == -1
    status = dict(re.findall(r"RG_SCAN_(OK|ERR_\w+) = (-?\d+)", hdr))
    assert {k.replace("ERR_", ""): int(v) for k, v in status.items()} == {v: k for k, v in scan_abi.STATUS.items()}


def test_defaults_are_the_documented_ones():
    cfg = MPCConfig.for_robot("ghost")
    c = scan_abi.make_cconfig(cfg)
    assert (c.nx, c.ny, c.x_first, c.dx, c.y_first, c.dy, c.clip, c.scale) == (8, 6, -0.2, 0.1, -0.25, 0.1, 1.0, 1.0)
    assert c.z_offset == cfg.body_height and c.nx * c.ny + 16 == 64       # the scan fills a 64-wide observation next to the path
    assert scan_abi.make_cconfig(cfg, z_offset=0.5).z_offset == 0.5
    assert scan_abi.create_status(c, 4) == (0, "")
    with pytest.raises(TypeError, match="bogus"):
        scan_abi.make_cconfig(cfg, bogus=1)


BAD = [(dict(nx=0), 4, "config.nx"), (dict(ny=0), 4, "config.ny"), (dict(nx=-3), 4, "config.nx"), (dict(nx=257, ny=1), 4, "config.nx * ny"),
       (dict(nx=1, ny=257), 4, "config.nx * ny"), (dict(nx=129, ny=2), 4, "config.nx * ny"), (dict(nx=65536, ny=65536), 4, "config.nx * ny"),
       (dict(dx=float("inf")), 4, "config.dx"), (dict(dx=float("nan")), 4, "config.dx"), (dict(dy=float("nan")), 4, "config.dy"),
       (dict(x_first=float("-inf")), 4, "config.x_first"), (dict(y_first=float("nan")), 4, "config.y_first"),
       (dict(z_offset=float("nan")), 4, "config.z_offset"), (dict(clip=-1e-9), 4, "config.clip"), (dict(clip=float("inf")), 4, "config.clip"),
       (dict(scale=float("nan")), 4, "config.scale"), ({}, 0, "batch"), ({}, (1 << 24) + 1, "batch")]


@pytest.mark.parametrize("change,batch,field", BAD)
def test_create_refuses_naming_the_field(change, batch, field):
    rc, msg = scan_abi.create_status(scan_abi.make_cconfig(**change), batch)
    assert rc == -1 and msg.startswith(field + ":"), (rc, msg)


def test_create_refuses_version_reserved_words_and_null():
    lib = scan_abi.load_library()
    c = scan_abi.make_cconfig()
    c.abi_version = 2
    assert scan_abi.create_status(c) == (-1, "config.abi_version: 2, this library is version 1")
    for name in ("reserved0", "reserved1", "reserved2"):
        c = scan_abi.make_cconfig()
        setattr(c, name, 1)
        assert scan_abi.create_status(c) == (-1, f"config.{name}: must be 0")
    h = C.c_void_p()
    assert lib.rg_scan_create(None, 4, scan_abi.DEVICE_NONE, C.byref(h)) == -1 and not h.value
    assert b"null" in lib.rg_scan_last_error(None)
    assert scan_abi.create_status(scan_abi.make_cconfig(nx=16, ny=16), 1 << 24) == (0, "")     # the largest of both


def test_host_only_handle_checks_arguments_then_reports_no_device():
    h = scan_abi.ScanHandle(4, None, scan_abi.DEVICE_NONE)
    assert h.device is None and h.batch == 4 and h.fields["z_offset"] == MPCConfig.for_robot("ghost").body_height
    a, b = 0x1000, 0x2000      # stand-ins for device addresses: a host-only handle never looks through them
    for args, name in (((None, None, a, None), "sim_state"), ((a, None, None, None), "out"), ((a, None, b, b), "prev")):
        with pytest.raises(scan_abi.RgScanError) as e:
            h.observe(*args)
        assert e.value.status == -1 and "observe" in str(e.value) and name in str(e.value), str(e.value)
    for args in ((a, None, b, None), (a, a, b, a)):
        with pytest.raises(scan_abi.RgScanError) as e:
            h.observe(*args)
        assert e.value.status == -3 and "RG_SCAN_DEVICE_NONE" in str(e.value)
    lib = scan_abi.load_library()
    assert lib.rg_scan_observe(None, a, None, b, None, None) == -1 and b"null handle" in lib.rg_scan_last_error(None)
    h.close()
    h.close()
    assert not h._h


def test_set_terrain_passes_on_the_text_of_the_terrain_check():
    h = scan_abi.ScanHandle(4, None, scan_abi.DEVICE_NONE)
    good = dict(kind=srb_abi.TERRAIN_GRID, cell=0.05, heights=0x2000, rows=2, cols=3)
    for change in (dict(cell=0.0), dict(rows=1), dict(heights=None), dict(key=0x1000), dict(kind=3)):
        t = srb_abi.make_cterrain(**{**good, **change})
        rc, text = srb_abi.terrain_check(t)
        assert rc == -1 and text
        with pytest.raises(scan_abi.RgScanError) as e:
            h.set_terrain(t)
        assert e.value.status == -1 and str(e.value).endswith("set_terrain: " + text), str(e.value)
    for t in (None, srb_abi.make_cterrain(), srb_abi.make_cterrain(**good), srb_abi.make_cterrain(kind=1, cell=0.05, amplitude=0.06, seed=3)):
        with pytest.raises(scan_abi.RgScanError) as e:      # valid: the host-only handle has no device to scan on
            h.set_terrain(t)
        assert e.value.status == -3
    lib = scan_abi.load_library()
    assert lib.rg_scan_set_terrain(None, None) == -1 and b"null handle" in lib.rg_scan_last_error(None)
    h.close()


# ---- known answers of the model --------------------------------------------------------------------------------------------

def _state(B, p=(0.0, 0.0, 0.3), quat=(0.0, 0.0, 0.0, 1.0)):
    st = np.zeros((43, B))
    for i in range(3):
        st[SM.ROW_P + i] = p[i]
    for i in range(4):
        st[SM.ROW_QUAT + i] = quat[i]
    return st


def test_on_the_plane_every_point_is_the_clipped_and_scaled_body_height():
    st = _state(5)
    st[2] = [0.3, 0.25, 2.0, -3.0, 0.31]
    st[0], st[1] = np.linspace(-50, 50, 5), np.linspace(7, -7, 5)
    got = SM.scan(st, None, z_offset=0.3, clip=1.0, scale=2.5)
    assert got.shape == (48, 5) and got.dtype == np.float32
    want = (np.clip(st[2] - 0.3, -1.0, 1.0) * 2.5).astype(np.float32)
    assert (got == want[None, :]).all()
    assert (SM.scan(st, None, z_offset=0.3, clip=0.0)[0] == (st[2] - 0.3).astype(np.float32)).all()      # 0: no clipping
    assert (SM.scan(st, TM.Random(0.0, 0.05, seed=1, keys=np.arange(5)), z_offset=0.3, scale=2.5) == got).all()   # zero amplitude is the plane


def test_point_order_is_a_times_ny_plus_c():
    s = dict(nx=3, ny=5, x_first=-0.25, dx=0.125, y_first=0.5, dy=-0.25)
    fx, fy = SM.points({**SM.DEFAULTS, **s})
    for a in range(3):
        for c in range(5):
            assert (fx[a * 5 + c], fy[a * 5 + c]) == (-0.25 + a * 0.125, 0.5 - c * 0.25)
    from robot_gym_amd.sim.height_scan import HeightScan
    assert (HeightScan(**s).points == np.stack([fx, fy], axis=1)).all() and HeightScan().points.shape == (48, 2)
    # on a ground that rises along x only, the scan is constant over c and falls with a
    ramp = TM.Grid(0.5 * np.arange(64)[:, None] * 0.125 * np.ones((1, 4)), 0.125, (-4.0, -4.0))
    got = SM.scan(_state(1, p=(0.0, 0.0, 5.0)), ramp, z_offset=0.0, clip=0.0, **s).reshape(3, 5)
    assert (got == got[:, :1]).all() and (np.diff(got[:, 0]) == np.float32(-0.5 * 0.125)).all()


def test_a_ramp_at_yaw_zero_a_quarter_and_a_half_turn_is_the_closed_form():
    cell, rows = 0.125, 64                              # a power of two: every point sits on a lattice line exactly
    H = (0.5 * np.arange(rows) * cell)[:, None] * np.ones((1, rows))       # heights 0.5 * i * cell: h(x, y) = 0.5 * (x - x0), exactly
    ramp = TM.Grid(H, cell, (-4.0, -4.0))
    s = dict(nx=4, ny=3, x_first=-0.25, dx=0.125, y_first=-0.125, dy=0.125, z_offset=0.25, clip=0.0, scale=1.0)
    fx, fy = SM.points({**SM.DEFAULTS, **s})
    px, py, pz = 0.5, -0.375, 3.0
    # quaternions whose products are exact: the identity; (1/2, 1/2, 1/2, 1/2), a third of a turn about (1, 1, 1), which takes the
    # x axis to the y axis: c0 = 1 - 2 (1/4 + 1/4) = 0, s0 = 2 (1/4 + 1/4) = 1, a quarter turn of the heading; (0, 0, 1, 0), a half turn
    st = np.concatenate([_state(1, (px, py, pz)), _state(1, (px, py, pz), (0.5, 0.5, 0.5, 0.5)), _state(1, (px, py, pz), (0.0, 0.0, 1.0, 0.0))], axis=1)
    c, sn = SM.heading(st)
    assert (c[0], sn[0]) == (1.0, 0.0) and (c[1], sn[1]) == (0.0, 1.0) and (c[2], sn[2]) == (-1.0, 0.0)
    X, Y = SM.world_points(st, s)
    assert (X[:, 0] == px + fx).all() and (Y[:, 0] == py + fy).all()
    assert (X[:, 1] == px - fy).all() and (Y[:, 1] == py + fx).all()
    assert (X[:, 2] == px - fx).all() and (Y[:, 2] == py - fy).all()
    got = SM.scan(st, ramp, **s)
    base = pz - 0.25
    assert (got[:, 0] == (base - 0.5 * ((px + fx) + 4.0)).astype(np.float32)).all()
    assert (got[:, 1] == (base - 0.5 * ((px - fy) + 4.0)).astype(np.float32)).all()
    assert (got[:, 2] == (base - 0.5 * ((px - fx) + 4.0)).astype(np.float32)).all()
    assert len(np.unique(got[:, 0])) == 4 and len(np.unique(got[:, 1])) == 3          # the ramp is felt along the heading


def test_nan_height_and_degenerate_headings():
    # robots: NaN pz; a zero quaternion (c0 = 1, s0 = 0: heading (1, 0) through the division); a NaN quaternion (n NaN);
    # a NaN x; and (-1/2, 1/2, 1/2, 1/2), whose x axis points straight down: c0 = s0 = 0 exactly, n == 0
    st = np.concatenate([_state(1, (0.1, 0.2, np.nan)), _state(1, quat=(0.0, 0.0, 0.0, 0.0)), _state(1, quat=(np.nan,) * 4),
                         _state(1, (np.nan, 0.0, 0.3)), _state(1, (0.7, -0.4, 0.3), quat=(-0.5, 0.5, 0.5, 0.5))], axis=1)
    with np.errstate(all="ignore"):
        n = np.sqrt((1 - 2 * (st[4] ** 2 + st[5] ** 2)) ** 2 + (2 * (st[3] * st[4] + st[5] * st[6])) ** 2)
    assert n[1] == 1.0 and np.isnan(n[2]) and n[4] == 0.0
    c, sn = SM.heading(st)
    assert (c[1], sn[1]) == (1.0, 0.0) and (c[2], sn[2]) == (1.0, 0.0) and (c[4], sn[4]) == (1.0, 0.0)
    fx, fy = SM.points(SM.DEFAULTS)
    X, Y = SM.world_points(st, {})
    assert (X[:, 4] == 0.7 + fx).all() and (Y[:, 4] == -0.4 + fy).all()          # n == 0: scanned along the world's axes
    ground = TM.Random(0.06, 0.05, seed=2, keys=np.arange(5))
    got = SM.scan(st, ground, z_offset=0.3, clip=0.75, scale=2.0)
    assert (got[:, 0] == np.float32(-1.5)).all()                      # NaN pz: -clip * scale
    assert np.isfinite(got).all()                                     # a NaN x has a finite ground (the lattice's lower bound)
    assert np.isnan(SM.scan(st, ground, z_offset=0.3, clip=0.0)[:, 0]).all()      # unclipped, the NaN stays


def test_mask_and_prev_semantics_of_the_model():
    rng = np.random.default_rng(0)
    st = _state(6)
    st[0], st[1] = rng.uniform(-2, 2, (2, 6))
    ground = TM.Random(0.06, 0.05, seed=4, keys=np.arange(6))
    new = SM.scan(st, ground, z_offset=0.3)
    out, prev = np.full((48, 6), 7.0, np.float32), np.full((48, 6), -9.0, np.float32)
    mask = np.array([0, 1, 0, 5, -1, 0])
    SM.observe(st, out, ground, mask=mask, prev=prev, z_offset=0.3)
    on = mask != 0
    assert (out[:, on] == new[:, on]).all() and (prev[:, on] == 7.0).all()
    assert (out[:, ~on] == 7.0).all() and (prev[:, ~on] == -9.0).all()
    assert (SM.observe(st, np.zeros((48, 6), np.float32), ground, z_offset=0.3) == new).all()


# ---- resources of rg_scan.hip ----------------------------------------------------------------------------------------------

KERNELS = {"rg_scan_observe_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_scan.hip")


def test_exactly_the_scan_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_the_scan_kernel_uses_no_scratch_and_no_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds): a lane's pose, heading and two hash prefixes, no more.
REGISTERS = {"rg_scan_observe_kernel": dict(vgprs=40, agprs=0, occupancy=8)}


def test_scan_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_scan_source_is_its_own_translation_unit_in_both_library_targets():
    src = open(os.path.join(SRC, "rg_scan.hip")).read()
    code = re.sub(r"//.*", "", src)
    pragma = code.index("#pragma clang fp contract(off)")
    assert pragma < code.index('#include "rg_mpc_dev.h"') < code.index('#include "rg_srb_dev.inc"') < code.index('#include "rg_srb_ground.inc"')
    assert pragma < code.index("__global__") and "__device__" not in code     # every device function is an included file's, after the pragma
    assert "asm" not in code and "atomic" not in src.lower() and "__shared__" not in src
    assert len(re.findall(r"__global__", code)) == len(KERNELS)
    assert re.findall(r'#include "([^"]+)"', code) == ["../../include/rg_scan.h", "rg_host.h", "rg_mpc_dev.h", "rg_srb_dev.inc", "rg_srb_handle.h",
                                                      "rg_srb_ground.inc"]
    for other in sorted(os.listdir(SRC)):                                        # included from nowhere, and no rg_srb_* file holds the kernel
        if other.endswith((".hip", ".inc", ".h")) and other != "rg_scan.hip":
            assert "rg_scan" not in open(os.path.join(SRC, other)).read(), other
    import bench
    assert not any("rg_scan" in rel for rel in bench.compiled_sources())         # the MPC hash behind profiles/ does not follow it
    kernel_checks.assert_built_into_both("rg_scan.hip", header="rg_scan.h")
    for lib, t in kernel_checks.library_targets().items():                       # directly after the unit before it, the newest header last
        assert t["sources"][t["sources"].index("rg_scan.hip") - 1] == "rg_bptt.hip" and t["prerequisites"][-1] == "../../include/rg_scan.h", (lib, t)
