"""The host side of the go-to-target task (robot_gym_amd/gym/goto_path.py) against what the reference's own functions
returned (tests/golden/goto_reference.npz, recorded by tests/golden/make_goto_golden.py), and the path tables."""
import math
import os

import numpy as np
import pytest

from robot_gym_amd.gym import goto_path

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goto_reference.npz"))


def _cases(name):
    off = GOLDEN[name + "_off"]
    return [GOLDEN[name][off[k]:off[k + 1]] for k in range(len(off) - 1)]


def test_planner_reproduces_the_reference_exactly():
    targets, obstacles, paths = GOLDEN["planner_targets"], _cases("planner_obstacles"), _cases("planner_paths")
    assert len(targets) == len(paths) >= 200 and sum(len(o) > 0 for o in obstacles) >= 4
    for t, o, want in zip(targets, obstacles, paths):
        got = goto_path.plan_path(t, o)
        assert got.shape == want.shape and np.array_equal(got, want), (t, o)
        assert np.array_equal(got[0], [0.0, 0.0]) and np.array_equal(got[-1], t)


def test_chain_sort_reproduces_the_reference_exactly():
    clouds, chains = _cases("sort_clouds"), _cases("sort_chains")
    assert len(clouds) >= 200
    broken = 0
    for cloud, want in zip(clouds, chains):
        got, order = goto_path.chain_sort(cloud)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert np.array_equal(cloud[order], got)
        broken += len(want) < len(cloud)
    assert broken >= 20   # the continuity break is exercised


def test_random_targets_follow_the_env_distribution():
    rng = np.random.default_rng(0)
    t = np.array([goto_path.random_target(rng) for _ in range(2000)])
    assert np.all(np.abs(t) <= 2.5) and np.all((np.abs(t) >= 1.0) | (t == 0.0)) and np.array_equal(t, np.round(t, 2))   # an exact 0.0 stays
    assert (np.abs(t) == 1.0).mean() > 0.2   # values drawn inside (-1, 1) are pushed onto +-1
    again = np.random.default_rng(0)
    assert np.array_equal(t[:50], np.array([goto_path.random_target(again) for _ in range(50)]))   # seeded


def test_build_path_spacing_tables_and_start():
    pts = goto_path.plan_path((2.0, 1.5))
    p = goto_path.build_path(pts)
    way_len = sum(math.hypot(*(pts[i + 1] - pts[i])) for i in range(len(pts) - 1))
    assert p.n == int(way_len / 1e-2) == len(p.x) == len(p.y) == len(p.s) == len(p.first_same_x)
    assert p.start_xy == (0.0, 0.0) and p.target == (2.0, 1.5)
    assert (p.x[-1], p.y[-1]) == (2.0, 1.5)
    seg = np.hypot(np.diff(p.x), np.diff(p.y))
    assert np.allclose(seg, way_len / (p.n - 1), atol=1e-3)            # corners cut a chord a little short
    assert p.s[0] == 0.0 and np.allclose(p.s[1:], np.cumsum(seg), rtol=0, atol=1e-12) and np.all(np.diff(p.s) > 0)
    assert p.length == p.s[-1] <= way_len + 1e-12
    assert np.array_equal(p.checkpoints, np.array([i * (p.length / 100) for i in range(1, 101)]))
    # first_same_x is np.where(x == x[i])[0][0]
    assert all(p.first_same_x[i] == np.where(p.x == p.x[i])[0][0] for i in range(p.n))


@pytest.mark.parametrize("target,angle", [((2.0, 0.0), 0.0), ((0.0, 2.0), math.pi / 2), ((-2.0, 0.0), math.pi), ((0.0, -2.0), 1.5 * math.pi),
                                          ((2.0, 2.0), math.pi / 4), ((-1.5, 1.5), 0.75 * math.pi), ((1.5, -1.5), 1.75 * math.pi)])
def test_start_angle_is_in_0_2pi_from_the_first_segment(target, angle):
    p = goto_path.build_path(goto_path.plan_path(target))
    assert 0.0 <= p.start_angle < 2 * math.pi and abs(p.start_angle - angle) < 1e-12


def test_first_same_x_is_not_the_nearest_index_on_a_vertical_segment():
    """A path straight up the y axis has one x: every point maps back to index 0."""
    p = goto_path.build_path(goto_path.plan_path((0.0, 2.0)))
    assert np.all(p.x == 0.0) and np.all(p.first_same_x == 0) and p.n == 200


def test_interpolate_points_semantics():
    line = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]])
    out = goto_path.interpolate_points(line, 5)
    assert np.allclose(out, [[0, 0], [0.5, 0], [1, 0], [1, 0.5], [1, 1]], atol=1e-15)
    assert np.array_equal(goto_path.interpolate_points(line[:1], 8), line[:1])
    assert np.array_equal(goto_path.interpolate_points(line, 1), line[:1])
    assert goto_path.interpolate_points(np.zeros((3, 2)), 4) is None
    with pytest.raises(ValueError):
        goto_path.interpolate_points(line, 0)


def test_length_between_idx_closes_the_loop_with_the_reference_sign_rules():
    p = goto_path.build_path(goto_path.plan_path((2.0, 0.0)))     # straight, 200 points, length ~2
    assert goto_path.length_between_idx(p, 7, 7) == 0.0
    assert goto_path.length_between_idx(p, 10, 30) == p.s[30] - p.s[10] > 0
    assert goto_path.length_between_idx(p, 30, 10) == -(p.s[30] - p.s[10])
    # far apart on an open straight path the "loop" closes through the chord, which is as long as the direct way: len_1 <
    # len_2 fails on the tie or by rounding, and the reference then returns -len_2 for idx1 < idx2
    len_1 = p.s[199] - p.s[0]
    len_2 = p.s[0] + math.hypot(p.x[199] - p.x[0], p.y[199] - p.y[0]) + (p.s[199] - p.s[199])
    want = len_1 if len_1 < len_2 else -len_2
    assert goto_path.length_between_idx(p, 0, 199) == want


def test_pack_paths_layout_and_limit():
    a, b = goto_path.build_path(goto_path.plan_path((1.0, 1.0))), goto_path.build_path(goto_path.plan_path((2.0, 0.0)))
    rows = goto_path.pack_paths([a, b], 256)
    assert rows["x"].shape == (2, 256) and rows["first_same_x"].dtype == np.int32 and list(rows["npts"]) == [a.n, b.n]
    assert np.array_equal(rows["s"][1, :b.n], b.s) and np.all(rows["x"][0, a.n:] == 0) and np.array_equal(rows["target"], [[1.0, 2.0], [1.0, 0.0]])
    with pytest.raises(ValueError):
        goto_path.pack_paths([b], 128)
