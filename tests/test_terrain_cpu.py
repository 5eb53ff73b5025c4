"""The terrain of include/rg_srb.h without a GPU: the hash words and known answers of the ground function
(tests/terrain_model.py), rg_srb_terrain_check rule by rule, the CPU reference closed loop on the ground (zero amplitude is
the plane bit for bit; on the reference's random terrain nobody falls and the bands of tests/terrain_fixtures.py are twice
what this run produces), and the resources of robot_gym_amd/csrc/rg_srb_terrain.hip from one device-only compile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from robot_gym_amd.core import srb_abi
from tests import kernel_checks
from tests import srb_fixtures as F
from tests import terrain_fixtures as TF
from tests import terrain_model as TM
from tests.episode_model import GOLDEN, M64, mix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")


# ---- hash words ------------------------------------------------------------------------------------------------------

WORDS = [((0, 0, 0, 0), 0x238275bc38fcbe91), ((0, 1, 0, 0), 0xb18a02f46d8d86c3), ((7, 3, -1, -1), 0x26feb16dbf775448),
         ((2 ** 63 + 5, -4, 123456789, -987654321), 0x35a8006dd1c13e37), ((0xDEADBEEF, 31, -(2 ** 39), 2 ** 39 - 1), 0xc43205ccd626c027),
         ((1, 2, 3, -4), 0x2bc3448c21076916)]


def test_hash_words_are_the_mix_chain_of_the_episode_model():
    for (seed, key, I, J), want in WORDS:
        h = seed & M64
        h = mix64(((h ^ (key & M64)) + GOLDEN) & M64)
        h = mix64(((h ^ (I & M64)) + GOLDEN) & M64)
        h = mix64(((h ^ (J & M64)) + GOLDEN) & M64)
        assert TM.hash_words(seed, key, I, J) == h == want, (seed, key, I, J)
        assert TM.unit(seed, key, I, J) == (want >> 11) * 2.0 ** -53
        assert float(TM.unit_vec(seed, [key], [I], [J])[0]) == TM.unit(seed, key, I, J)     # the vectorised form wraps as Python masks
    assert 0.0 <= min(TM.unit(*w) for w, _ in WORDS) and max(TM.unit(*w) for w, _ in WORDS) < 1.0


# ---- ground known answers --------------------------------------------------------------------------------------------

def _random_points(rng, n, span=3.0):
    return rng.uniform(-span, span, n), rng.uniform(-span, span, n)


def test_random_heights_are_constant_over_two_by_two_vertex_groups_and_inside_the_amplitude():
    g = TM.Random(0.06, 0.05, seed=3, keys=np.array([0, 5, -7]))
    i, j = np.meshgrid(np.arange(-9, 9), np.arange(-9, 9), indexing="ij")
    for robot in range(3):
        key = np.full(i.shape, g.keys[robot])
        hv = g.vertex(key, i, j)
        assert (hv == g.vertex(key, (i >> 1) << 1, (j >> 1) << 1)).all()       # the group's first vertex, negative indices included
        assert hv[1, 1] == hv[2, 2] and hv[1, 1] == hv[1, 2] and hv[0, 0] != hv[1, 1]   # -8, -7 share a group; -9 does not
        assert (hv >= 0).all() and (hv < 0.06).all() and len(np.unique(hv)) == 100   # -9 | 8 full groups | 8: ten groups a side
    assert not (g.vertex(np.full(i.shape, 0), i, j) == g.vertex(np.full(i.shape, 5), i, j)).all()   # keys are worlds
    x, y = _random_points(np.random.default_rng(0), 4000)
    h = g.height(x, y, np.random.default_rng(1).integers(0, 3, 4000))
    assert (h >= 0).all() and (h < 0.06).all()


def test_zero_amplitude_is_exactly_zero_everywhere():
    g = TM.Random(0.0, 0.05, seed=9, keys=np.arange(4))
    x, y = _random_points(np.random.default_rng(2), 2000, 50.0)
    h = g.height(x, y, np.arange(2000) % 4)
    assert (h == 0.0).all() and not np.signbit(h).any()
    z = TM.Grid(np.zeros((5, 4)), 0.1, (-0.2, 0.3)).height(x, y)
    assert (z == 0.0).all() and not np.signbit(z).any()


def test_the_value_at_a_vertex_is_the_vertex_height():
    cell = 0.0625                      # a power of two: (i * cell) / cell is i exactly, so the point IS the vertex
    g = TM.Random(0.06, cell, seed=1, keys=np.array([11]))
    i, j = np.meshgrid(np.arange(-6, 7), np.arange(-6, 7), indexing="ij")
    i, j = i.ravel(), j.ravel()
    assert (g.height(i * cell, j * cell, np.zeros(len(i), int)) == g.vertex(np.full(len(i), 11), i, j)).all()
    H = np.random.default_rng(3).uniform(-0.1, 0.1, (9, 7))
    gr = TM.Grid(H, 0.25, (0.0, 0.0))
    ii, jj = np.meshgrid(np.arange(9), np.arange(7), indexing="ij")
    assert (gr.height(ii.ravel() * 0.25, jj.ravel() * 0.25) == H.ravel()).all()


def test_both_triangle_formulas_agree_on_the_diagonal_and_across_cell_edges():
    rng = np.random.default_rng(4)
    n = 5000
    h00, h10, h01, h11, far0, far1 = rng.uniform(0, 0.06, (6, n))
    t = rng.uniform(0, 1, n)
    one, zero = np.ones(n), np.zeros(n)
    # on the diagonal u == v
    lower = h00 + t * (h10 - h00) + t * (h11 - h10)
    upper = h00 + t * (h11 - h01) + t * (h01 - h00)
    assert np.abs(lower - upper).max() <= 1e-15
    # the edge u = 1 of a cell (its lower triangle) is the edge u = 0 of the next cell in x (its upper triangle; v = 0: lower)
    here = TM._interpolate(one, t, h00, h10, h01, h11)
    there = TM._interpolate(zero, t, h10, far0, h11, far1)
    assert np.abs(here - there).max() <= 1e-15
    # the edge v = 1 (upper triangle) is the edge v = 0 of the next cell in y (lower triangle)
    here = TM._interpolate(t, one, h00, h10, h01, h11)
    there = TM._interpolate(t, zero, h01, h11, far0, far1)
    assert np.abs(here - there).max() <= 1e-15
    # through the ground function: stepping from eps before a lattice line to eps after it moves the height by no more than
    # the steepest facet allows: per eps, eps / cell * amplitude for each of the two edge differences of a triangle
    g = TM.Random(0.06, 0.05, seed=5, keys=np.array([2]))
    s = rng.uniform(-2, 2, 3000)
    rob, eps, line = np.zeros(3000, int), 1e-13, rng.integers(-40, 40, 3000) * 0.05
    bound = 2 * eps / 0.05 * 0.06 + 1e-15
    for a, b in ((g.height(line - eps, s, rob), g.height(line + eps, s, rob)), (g.height(s, line - eps, rob), g.height(s, line + eps, rob))):
        assert np.abs(a - b).max() <= 2 * bound
    # and the diagonal through the ground function (u == v exactly on a power-of-two cell)
    g2 = TM.Random(0.06, 0.125, seed=6, keys=np.array([0]))
    d = rng.integers(-64, 64, 2000) * 0.125 + rng.integers(0, 8, 2000) / 64.0
    i, uu = TM._lattice(d / 0.125)
    key = np.zeros(2000, np.int64)
    v00, v10, v01, v11 = g2.vertex(key, i, i), g2.vertex(key, i + 1, i), g2.vertex(key, i, i + 1), g2.vertex(key, i + 1, i + 1)
    assert np.abs(g2.height(d, d, key) - (v00 + uu * (v11 - v01) + uu * (v01 - v00))).max() <= 1e-15


def test_a_grid_sampled_from_a_plane_is_reproduced_inside_and_held_outside():
    a, b, c = 0.07, -0.04, 0.3
    cell, x0, y0, rows, cols = 0.25, -1.0, 0.5, 9, 7
    ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    g = TM.Grid(a * (x0 + ii * cell) + b * (y0 + jj * cell) + c, cell, (x0, y0))
    rng = np.random.default_rng(5)
    x, y = rng.uniform(x0, x0 + (rows - 1) * cell, 3000), rng.uniform(y0, y0 + (cols - 1) * cell, 3000)
    assert np.abs(g.height(x, y) - (a * x + b * y + c)).max() <= 1e-15
    # outside: the edge clamp holds the border value
    xo, yo = rng.uniform(-30, 30, 3000), rng.uniform(-30, 30, 3000)
    xc, yc = np.clip(xo, x0, x0 + (rows - 1) * cell), np.clip(yo, y0, y0 + (cols - 1) * cell)
    assert np.abs(g.height(xo, yo) - (a * xc + b * yc + c)).max() <= 1e-15
    assert g.height(np.array([-1e9]), np.array([1e9]))[0] == g.heights[0, cols - 1]


def test_any_coordinate_has_a_finite_ground():
    bad = np.array([1e300, -1e300, np.inf, -np.inf, np.nan, 0.3])
    x, y = np.meshgrid(bad, bad, indexing="ij")
    x, y = x.ravel(), y.ravel()
    r = TM.Random(0.06, 0.05, seed=1, keys=np.arange(3))
    h = r.height(x, y, np.arange(len(x)) % 3)
    assert np.isfinite(h).all() and (h >= 0).all() and (h < 0.06).all()
    H = np.random.default_rng(6).uniform(-1, 1, (9, 7))
    gh = TM.Grid(H, 0.05, (0.1, 0.2)).height(x, y)
    assert np.isfinite(gh).all() and (gh >= H.min()).all() and (gh <= H.max()).all()
    # a NaN is the lower bound of the clamp: the first row / column of the grid
    assert TM.Grid(H, 0.05).height(np.array([np.nan]), np.array([np.nan]))[0] == H[0, 0]
    assert TM.Grid(H, 0.05).height(np.array([np.inf]), np.array([-np.inf]))[0] == H[8, 0]


# ---- rg_srb_terrain_check ----------------------------------------------------------------------------------------------

def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_terrain_struct_matches_the_header_and_the_library():
    lib = srb_abi.load_library()
    assert lib.rg_srb_terrain_size() == C.sizeof(srb_abi.CTerrain)
    hdr = _header("rg_srb_terrain.h")
    body = dict((n, b) for b, n in re.findall(r"typedef struct \{([^{}]*)\} (\w+);", hdr))["rg_srb_terrain"]
    names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"\*?(\w+)(?:\[\d+\])?(?=\s*(?:,|$))", decl.strip())]
    assert names == [n for n, _ in srb_abi.CTerrain._fields_]
    declared = sorted(set(re.findall(r"\b(rg_srb_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(srb_abi.TERRAIN_EXPORTS)
    for name in declared:
        assert hasattr(lib, name), name
    assert '#include "rg_srb_terrain.h"' in open(os.path.join(ROOT, "include", "rg_srb.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (RG_SRB_\w+) (\d+)", hdr)}
    assert (defs["RG_SRB_TERRAIN_FLAT"], defs["RG_SRB_TERRAIN_RANDOM"], defs["RG_SRB_TERRAIN_GRID"]) == (0, 1, 2)
    assert defs["RG_SRB_TERRAIN_MAX_DIM"] == srb_abi.TERRAIN_MAX_DIM == TM.MAX_DIM


KEY, HEIGHTS = 0x1000, 0x2000      # stand-ins for device addresses: the check looks at NULL or not, never through them
GOOD = {"flat": dict(kind=0), "random": dict(kind=1, cell=0.05, amplitude=0.06, seed=2 ** 64 - 1, key=KEY),
        "random_shared": dict(kind=1, cell=0.05, amplitude=0.0), "grid": dict(kind=2, cell=0.05, heights=HEIGHTS, rows=2, cols=4096, x0=-3.0, y0=1e6)}


@pytest.mark.parametrize("name", sorted(GOOD))
def test_terrain_check_accepts(name):
    rc, msg = srb_abi.terrain_check(srb_abi.make_cterrain(**GOOD[name]))
    assert rc == 0 and msg == "", (rc, msg)


BAD = [("random", dict(cell=0.0), "cell"), ("random", dict(cell=-0.05), "cell"), ("random", dict(cell=np.nan), "cell"), ("grid", dict(cell=np.inf), "cell"),
       ("grid", dict(cell=0.0), "cell"), ("flat", dict(cell=0.05), "cell"),
       ("random", dict(amplitude=-1e-9), "amplitude"), ("random", dict(amplitude=np.inf), "amplitude"), ("random", dict(amplitude=np.nan), "amplitude"),
       ("grid", dict(amplitude=0.06), "amplitude"), ("flat", dict(amplitude=0.06), "amplitude"),
       ("flat", dict(kind=3), "kind"), ("flat", dict(kind=-1), "kind"),
       ("grid", dict(seed=1), "seed"), ("flat", dict(seed=1), "seed"),
       ("grid", dict(key=KEY), "key"), ("flat", dict(key=KEY), "key"),
       ("grid", dict(heights=None), "heights"), ("random", dict(heights=HEIGHTS), "heights"), ("flat", dict(heights=HEIGHTS), "heights"),
       ("grid", dict(rows=1), "rows"), ("grid", dict(rows=4097), "rows"), ("random", dict(rows=2), "rows"),
       ("grid", dict(cols=1), "cols"), ("grid", dict(cols=4097), "cols"), ("grid", dict(cols=-5), "cols"), ("random", dict(cols=2), "cols"),
       ("grid", dict(x0=np.nan), "x0"), ("grid", dict(y0=-np.inf), "y0"), ("random", dict(x0=1.0), "x0"), ("random", dict(y0=1.0), "y0")]


@pytest.mark.parametrize("base,change,field", BAD)
def test_terrain_check_refuses_naming_the_field(base, change, field):
    rc, msg = srb_abi.terrain_check(srb_abi.make_cterrain(**{**GOOD[base], **change}))
    assert rc == -1 and f"terrain.{field}" in msg, (rc, msg)


def test_terrain_check_refuses_version_reserved_and_null_and_fits_a_short_buffer():
    lib = srb_abi.load_library()
    t = srb_abi.make_cterrain(**GOOD["random"])
    t.abi_version = 2
    assert srb_abi.terrain_check(t) == (-1, "terrain.abi_version: 2, this library is version 1")
    for k in range(4):
        t = srb_abi.make_cterrain(**GOOD["grid"])
        t.reserved[k] = 1
        rc, msg = srb_abi.terrain_check(t)
        assert rc == -1 and f"terrain.reserved[{k}]" in msg
    buf = C.create_string_buffer(64)
    assert lib.rg_srb_terrain_check(None, buf, 64) == -1 and b"null" in buf.value
    t = srb_abi.make_cterrain(**{**GOOD["grid"], "rows": 1})
    small = C.create_string_buffer(b"\x7f" * 16, 16)
    assert lib.rg_srb_terrain_check(C.byref(t), small, 8) == -1
    assert small.raw[:8] == b"terrain\0" and small.raw[8:] == b"\x7f" * 8      # truncated and terminated inside n, nothing past it
    assert lib.rg_srb_terrain_check(C.byref(t), None, 0) == -1                    # msg may be NULL


# ---- the CPU closed loop -----------------------------------------------------------------------------------------------

def test_zero_amplitude_is_the_plane_bit_for_bit_in_closed_loop():
    for robot in F.ROBOTS:
        cmd, hs = F.cases(robot)
        flat = F.CpuLoop(robot, cmd, hs)
        zero = TF.TerrainCpuLoop(robot, cmd, hs, TM.Random(0.0, TF.CELL, TF.SEED, np.arange(len(hs))))
        assert flat.model.state.tobytes() == zero.model.state.tobytes()
        for k in range(F.TICKS):
            flat.tick()
            zero.tick()
            assert flat.model.state.tobytes() == zero.model.state.tobytes(), (robot, k)
        for name in flat.model.obs:
            assert flat.model.obs[name].tobytes() == zero.model.obs[name].tobytes(), (robot, name)


@pytest.fixture(scope="module")
def rough():
    out = {}
    for robot in F.ROBOTS:
        cmd, hs = F.cases(robot)
        feet_on_ground = []

        def look(k, loop):
            if k % 50 == 49:
                m, st = loop.model, loop.model.state
                for l in range(4):
                    on = st[F.M.ROW_STANCE + l] == 1.0
                    h = m.ground_height(st[F.M.ROW_FOOT + 3 * l], st[F.M.ROW_FOOT + 3 * l + 1])
                    feet_on_ground.append(bool((st[F.M.ROW_FOOT + 3 * l + 2][on] == h[on]).all()))
        traj, loop, walked = TF.run_cpu(robot, TM.Random(TF.AMPLITUDE, TF.CELL, TF.SEED, np.arange(len(hs))), every_tick=look)
        out[robot] = (cmd, traj, loop, walked, feet_on_ground)
    return out


def test_on_the_reference_terrain_nobody_falls_and_every_robot_walks_inside_the_bands(rough):
    for robot, (cmd, traj, loop, walked, feet_on_ground) in rough.items():
        assert not loop.model.fallen().any(), robot
        assert (loop.model.state[F.M.ROW_STEPS] == 10 * F.TICKS).all()
        assert all(np.isfinite(v).all() for v in traj.values())
        assert all(feet_on_ground) and len(feet_on_ground) == 8 * 4          # a stance foot stands on the ground, exactly
        assert (walked >= TF.WALKED * TF.commanded_distance(cmd)).all(), robot
        worst = F.worst_in_window(F.window(traj, F.TICKS - F.WINDOW), cmd, loop.cfg.body_height)
        print(robot, {k: float(v.max()) for k, v in worst.items()})
        assert not F.outside_bands(worst, TF.BANDS), (robot, F.outside_bands(worst, TF.BANDS))
        # the ground is felt: the feet do not all stand at one height
        fz = loop.model.state[F.M.ROW_FOOT + 2::3][:4]
        assert np.ptp(fz, axis=0).max() > 0.01


def test_the_terrain_bands_are_twice_what_this_run_produces(rough):
    total = {k: 0.0 for k in TF.BANDS}
    for robot, (cmd, traj, loop, walked, _) in rough.items():
        worst = F.worst_in_window(F.window(traj, F.TICKS - F.WINDOW), cmd, loop.cfg.body_height)
        for k in total:
            total[k] = max(total[k], float(worst[k].max()))
    print("measured worst", total)
    for k, band in TF.BANDS.items():
        assert abs(band - 2 * total[k]) <= 0.01 * band, (k, band, total[k])


# ---- resources of rg_srb_terrain.hip -----------------------------------------------------------------------------------

KERNELS = {"rg_srb_terrain_step_kernel", "rg_srb_terrain_settle_kernel", "rg_srb_terrain_height_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_srb_terrain.hip")


def test_every_terrain_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_terrain_kernel_uses_scratch_or_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today (upper bounds).  The step kernel is where the flat one is (256 + 40: the ground
# lookup sits outside the sub-step loop and costs no register there); the settle kernel carries the reset's IK passes.
REGISTERS = {"rg_srb_terrain_step_kernel": dict(vgprs=256, agprs=40), "rg_srb_terrain_settle_kernel": dict(vgprs=256, agprs=40),
             "rg_srb_terrain_height_kernel": dict(vgprs=26, agprs=0)}


def test_terrain_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_terrain_source_keeps_contraction_off_and_both_library_targets_compile_it():
    src = open(os.path.join(SRC, "rg_srb_terrain.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_mpc_dev.h"') < src.index("__global__")
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_srb_tick.inc"') < src.index("__global__")
    for text in (src, open(os.path.join(SRC, "rg_srb_tick.inc")).read()):
        assert "asm" not in re.sub(r"//.*", "", text) and "atomic" not in text and "__shared__" not in text
    kernel_checks.assert_built_into_both("rg_srb_terrain.hip")
