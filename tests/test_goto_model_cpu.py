"""Known answers of the go-to-target model (tests/goto_model.py): what rg_goto_post_step and rg_goto_pre_step must compute,
worked out by hand on paths simple enough to do so -- and the share of the GPU test's robot-ticks that its margin rule
leaves out, measured with the model alone."""
import math

import numpy as np
import pytest

from robot_gym_amd.core import goto_abi
from robot_gym_amd.gym import goto_path
from tests import goto_fixtures, goto_model
from tests.goto_model import REASON

C = goto_model.config()
QUAT0 = (0.0, 0.0, 0.0, 1.0)


def quat(yaw):
    return (0.0, 0.0, math.sin(0.5 * yaw), math.cos(0.5 * yaw))


@pytest.fixture(scope="module")
def straight():
    """(0,0) -> (2,0): 200 points 2/199 apart on the x axis, every x distinct."""
    p = goto_path.build_path(goto_path.plan_path((2.0, 0.0)))
    assert p.n == 200 and np.all(p.y == 0.0) and np.array_equal(p.first_same_x, np.arange(200))
    return p


def start(path, xy, yaw=0.0, c=C):
    st = goto_model.new_state()
    r = goto_model.post_step(c, st, path, xy, quat(yaw), observe_only=True)
    return st, r


def test_defaults_are_the_reference_constants():
    f = goto_abi.task_fields()
    assert (f["window_height"], f["window_top_width"], f["window_bottom_width"], f["window_distance"]) == (0.160, 0.270, 0.120, 0.112)
    assert (f["num_cam_pts"], f["max_track_err"], f["progress_window"], f["progress_limit"], f["target_radius"]) == (8, 0.1, 0.4, 0.5, 0.15)
    assert (f["time_penalty"], f["checkpoint_reward_total"], f["num_checkpoints"], f["max_time"], f["continuity_break"]) == (0.15, 1000.0, 100, 90.0, 0.030)
    assert (f["action_low"], f["action_high"], f["n_max"], f["max_visible"]) == ((0.0, -0.4), (0.35, 0.4), 1024, 128)
    assert C["max_steps"] == 90.0 / (0.001 * 10) and C["cp_reward"] == 10.0


def test_robot_stepped_along_a_straight_path(straight):
    """Robot 2 cm left of the line, above path points 0, 10, 20, ...: track_err 0.02, position_on_track grows by
    s[i+10] - s[i], a checkpoint every length / 100, reward k * 10 * (1 - 0.02 / 0.1)^2 - 0.15."""
    p = straight
    st, _ = start(p, (p.x[0], 0.02))
    per = p.length / 100
    passed = 0
    for step, i in enumerate(range(10, 150, 10), 1):
        r = goto_model.post_step(C, st, p, (p.x[i], 0.02), QUAT0, 0.0, 10.0 * step)
        assert r["track_err"] == 0.02 and r["first_same"] == (i - 10, i)
        assert abs(r["position_on_track"] - p.s[i]) < 1e-12
        k = int(math.floor(p.s[i] / per + 1e-9)) - passed
        passed += k
        assert r["checkpoints"] == k and k in (4, 5, 6) and st[goto_abi.ROW_NEXT_CP] == passed
        assert abs(r["reward64"] - (k * 10 * (1 - 0.02 / 0.1) ** 2 - 0.15)) < 1e-12
        assert r["done"] == 0 and r["reason"] == REASON["none"] and st[goto_abi.ROW_ENV_STEPS] == step
        assert np.array_equal(st[goto_abi.ROW_PREV:goto_abi.ROW_PREV + 2], (p.x[i - 10], 0.02))


def test_observation_of_a_straight_path_is_eight_points_through_the_window(straight):
    """On the axis, heading along it: the window spans x in [0.112, 0.272]; the visible points are chained from the
    nearest and resampled to 8 at equal spacing, all with y = 0."""
    p = straight
    st, r = start(p, (0.5, 0.0))
    vis = p.x[(p.x - 0.5 >= 0.112) & (p.x - 0.5 <= 0.272)] - 0.5
    obs = r["obs"].reshape(8, 2)
    assert r["visible"] == r["chain"] == len(vis) and r["latched"] == 1
    assert np.allclose(obs[:, 1], 0.0, atol=1e-7) and np.allclose(obs[:, 0], np.linspace(vis[0], vis[-1], 8), atol=1e-6)
    # turned by +90 degrees about a point right of the line, the path runs through the window from left to right:
    # the chain starts at the point nearest the robot frame's origin
    st, r = start(p, (0.5, -0.2), math.pi / 2)
    obs = r["obs"].reshape(8, 2)
    assert np.allclose(obs[:, 0], 0.2, atol=1e-6) and r["latched"] == 1
    assert abs(obs[0, 1]) == np.abs(obs[:, 1]).min() or abs(obs[0, 1]) < 0.011


def test_eleven_centimetres_off_the_line_is_the_track_limit(straight):
    p = straight
    st, _ = start(p, (p.x[20], 0.0))
    r = goto_model.post_step(C, st, p, (p.x[22], 0.11), QUAT0)
    assert r["reward64"] == -100.0 and r["done"] == 1 and r["reason"] == REASON["track"] and abs(r["track_err"] - 0.11) < 1e-15


def test_a_teleport_of_sixty_centimetres_is_the_progress_limit(straight):
    p = straight
    st, _ = start(p, (p.x[20], 0.0))
    r = goto_model.post_step(C, st, p, (p.x[20] + 0.6, 0.0), QUAT0)
    # the jump is above the 0.4 window, so progress stays 0 and |0.6 - 0| > 0.5
    assert r["checkpoints"] == 0 and st[goto_abi.ROW_PROGRESS] == 0.0 and abs(r["position_on_track"] - 0.6) < 0.011
    assert r["reward64"] == -100.0 and r["done"] == 1 and r["reason"] == REASON["progress"]


def test_done_robots_are_frozen(straight):
    p = straight
    st, _ = start(p, (p.x[20], 0.0))
    goto_model.post_step(C, st, p, (p.x[22], 0.11), QUAT0)
    before = st.copy()
    r = goto_model.post_step(C, st, p, (p.x[40], 0.0), QUAT0)
    assert r["frozen"] and r["reward"] == 0.0 and r["done"] == 1 and np.array_equal(st, before)
    assert np.array_equal(r["obs"], before[goto_abi.ROW_OBS:goto_abi.ROW_OBS + 16].astype(np.float32))
    assert np.array_equal(goto_model.pre_step(C, st, p, (p.x[40], 0.0), (0.3, 0.2)), np.zeros(3, dtype=np.float32))


def test_a_vertical_segment_maps_every_nearest_point_to_index_zero():
    """first_same_x on a path up the y axis: the reference's np.where(x == near_x)[0][0] is 0 for every point, so walking
    along the path moves position_on_track by length_between_idx(0, 0) = 0 -- with nearest indices it would be s[60] - s[40]."""
    p = goto_path.build_path(goto_path.plan_path((0.0, 2.0)))
    st, _ = start(p, (0.0, p.y[40]), math.pi / 2)
    r = goto_model.post_step(C, st, p, (0.0, p.y[60]), quat(math.pi / 2))
    assert (r["nearest_prev"], r["nearest"]) == (40, 60) and r["first_same"] == (0, 0)
    assert r["position_on_track"] == 0.0 and r["checkpoints"] == 0 and r["reward64"] == -0.15
    assert p.s[60] - p.s[40] > 0.19   # what nearest indices would have given


def test_an_empty_window_latches_the_previous_observation(straight):
    p = straight
    st, r0 = start(p, (0.5, 0.0))
    assert r0["latched"] == 1
    r = goto_model.post_step(C, st, p, (0.5, 0.0), quat(math.pi))     # facing back along the path: still sees it
    assert r["latched"] == 1 and not np.array_equal(r["obs"], r0["obs"])
    seen = r["obs"].copy()
    r = goto_model.post_step(C, st, p, (1.95, 0.05), quat(0.0))       # the window lies past the end of the path
    assert r["visible"] == 0 and r["chain"] == 0 and r["latched"] == 0 and np.array_equal(r["obs"], seen)
    # a single visible point is no line either
    st, r0 = start(p, (0.5, 0.0))
    r = goto_model.post_step(C, st, p, (1.883, 0.0), QUAT0)      # the window starts between the last two path points
    assert r["visible"] == 1 and r["chain"] == 1 and r["latched"] == 0 and np.array_equal(r["obs"], r0["obs"])


def test_path_done_comes_at_ninety_nine_checkpoints(straight):
    """update_progress sets done when next_checkpoint_idx reaches num_checkpoints - 1 (path.py:311): 99 of the 100.  With
    the target far from the path's end (so that "on target" does not end the episode first) the cause is "path done"."""
    p = straight._replace(target=(9.0, 9.0))
    st, _ = start(p, (p.x[0], 0.0))
    total, step = 0, 0
    stops = list(range(10, 200, 10)) + [199]
    for i in stops:
        step += 1
        r = goto_model.post_step(C, st, p, (p.x[i], 0.0), QUAT0, 0.0, 10.0 * step)
        total += r["checkpoints"]
        if r["done"]:
            break
        assert st[goto_abi.ROW_PATH_DONE] == 0.0 and total < 99
    assert r["reason"] == REASON["path_done"] and total == 99 == st[goto_abi.ROW_NEXT_CP] and st[goto_abi.ROW_PATH_DONE] == 1.0
    assert i == 199 and p.s[199] >= 0.99 * p.length > p.s[190]      # the 99th checkpoint lies at 0.99 of the length
    # the tick that ends the path still pays its checkpoints
    assert abs(r["reward64"] - (r["checkpoints"] * 10.0 - 0.15)) < 1e-12


def test_termination_order_and_the_remaining_causes(straight):
    p = straight
    st, _ = start(p, (p.x[20], 0.0))
    r = goto_model.post_step(C, st, p, (p.x[22], 0.11), QUAT0, sim_status=1.0)
    assert r["reason"] == REASON["fallen"] and r["reward64"] == -100.0       # fallen wins over track; the reward is still the follower's
    st, _ = start(p, (1.8, 0.0))
    r = goto_model.post_step(C, st, p, (1.86, 0.0), QUAT0)
    assert r["reason"] == REASON["on_target"] and r["done"] == 1             # 0.14 m from (2, 0)
    st, _ = start(p, (1.0, 0.0))
    assert goto_model.post_step(C, st, p, (1.0, 0.0), QUAT0, 0.0, 9000.0)["done"] == 0     # the counter must EXCEED max_time / (dt * substeps)
    assert goto_model.post_step(C, st, p, (1.0, 0.0), QUAT0, 0.0, 9010.0)["reason"] == REASON["time"]


def test_pre_step_clips_stands_on_target_and_adds_the_offsets_in_float32(straight):
    p = straight
    st = goto_model.new_state()
    c = goto_model.config(cmd_offset=(0.01, -0.02, 0.03))
    f32 = np.float32
    assert np.array_equal(goto_model.pre_step(c, st, p, (0.5, 0.0), (0.2, 0.1)), [f32(0.2) + f32(0.01), f32(-0.02), f32(0.1) + f32(0.03)])
    assert np.array_equal(goto_model.pre_step(c, st, p, (0.5, 0.0), (0.9, -0.9)), [f32(0.35) + f32(0.01), f32(-0.02), f32(-0.4) + f32(0.03)])
    assert np.array_equal(goto_model.pre_step(c, st, p, (0.5, 0.0), (-1.0, float("nan"))), [f32(0.01), f32(-0.02), f32(0.03)])
    assert np.array_equal(goto_model.pre_step(c, st, p, (1.9, 0.0), (0.2, 0.1)), [f32(0.01), f32(-0.02), f32(0.03)])   # on target: standing
    assert np.array_equal(goto_model.pre_step(c, st, None, (0.5, 0.0), (0.2, 0.1)), [f32(0.01), f32(-0.02), f32(0.03)])  # no path


def test_more_visible_points_than_max_visible_sets_the_overflow_flag():
    """A path folded on itself inside the window: the first max_visible points in path order are kept."""
    x = np.concatenate([np.linspace(0.12, 0.26, 15)] * 12)
    y = np.concatenate([np.full(15, 0.004 * (k - 6)) for k in range(12)])
    p = goto_path.build_path(np.stack((x, y), axis=-1), target=(5.0, 5.0))
    st, r = start(p, (0.0, 0.0))
    assert r["visible"] > 128 and r["chain"] <= 128 and st[goto_abi.ROW_OVERFLOW] == 1.0 and np.all(np.isfinite(r["obs"]))
    c = goto_model.config(max_visible=16)
    st, r = start(p, (0.0, 0.0), c=c)
    assert r["visible"] > 128 and r["chain"] <= 16 and st[goto_abi.ROW_OVERFLOW] == 1.0


def test_a_second_configuration_moves_every_decision(straight):
    c = goto_model.config(**goto_fixtures.CONFIG_B)
    p = goto_path.build_path(goto_path.plan_path((2.0, 0.0)), 37)
    st, r = start(p, (0.5, 0.0), c=c)
    assert len(r["obs"]) == 10 and r["visible"] == np.sum((p.x - 0.5 >= 0.07) & (p.x - 0.5 <= 0.28)) and st[goto_abi.ROW_OVERFLOW] == (r["visible"] > 24)
    r = goto_model.post_step(c, st, p, (p.x[60], 0.09), QUAT0)
    assert r["reason"] == REASON["track"]            # 0.09 > 0.085, inside the default 0.1
    assert c["max_steps"] == 6.0 / (0.002 * 5)


def test_the_gpu_test_seeds_leave_out_less_than_one_percent():
    """The margin rule of tests/test_goto_gpu.py (goto_fixtures.excluded, threshold 1e-9) on a 256-robot slice of each of
    its two cases, with the model alone.  Observed on 512 robots: 0.013 % of robot-ticks (and of observations) under the
    defaults, 0.005 % of robot-ticks and 0.30 % of observations under the second configuration."""
    from tests.test_goto_gpu import CASES, TICKS
    for name, (task, path_seed, pose_seed) in CASES.items():
        c = goto_model.config(**task)
        paths = goto_fixtures.planned_paths(256, path_seed, c["num_checkpoints"])
        poses = goto_fixtures.pose_sequences(paths, TICKS, pose_seed, c["substeps"])
        m = goto_fixtures.run_model(c, paths, poses, workers=1)
        out_tick, out_obs = goto_fixtures.excluded(m)
        print(f"{name}: {out_tick.mean():.4%} of robot-ticks left out, {out_obs.mean():.4%} of their observations")
        assert out_tick.mean() <= out_obs.mean() <= 0.01, (name, out_tick.mean(), out_obs.mean())
        live = m["frozen"] == 0
        assert live.mean() > 0.25 and set(np.unique(m["reason"][-1])) >= {3.0, 4.0, 5.0}   # the sequences exercise the causes


def test_the_models_chain_reproduces_the_recorded_sort_points():
    """The kernels are held to goto_model.chain_points; this holds chain_points to what the reference's sort_points returned
    on the recorded clouds (tests/golden/goto_reference.npz), exactly."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goto_reference.npz"))
    co, ho = g["sort_clouds_off"], g["sort_chains_off"]
    assert len(co) - 1 >= 200
    for k in range(len(co) - 1):
        cloud, want = g["sort_clouds"][co[k]:co[k + 1]], g["sort_chains"][ho[k]:ho[k + 1]]
        chain, cs, acc, *_ = goto_model.chain_points(cloud[:, 0].copy(), cloud[:, 1].copy(), 30e-3)
        assert np.array_equal(np.array(chain).reshape(-1, 2), want), k
        assert len(cs) == len(chain) and abs(acc - np.hypot(*np.diff(want, axis=0).T).sum()) < 1e-12


def test_copies_of_a_point_tie_exactly_and_only_the_old_margin_counts_it(straight):
    """Every 2nd point of the straight path given twice: the chain's arg-min ties exactly between the copies, so margin_frame
    is 0, margin_frame_ties_ok is not; the copies enter the chain in index order (goto_path.chain_sort, strict <, reports
    the indices), as links of length zero; and the nearest-point arg-min takes the lower index of two copies."""
    from tests import goto_edges
    p = goto_edges.with_copies(straight, every=2)
    assert p.n == 300 and p.x[0] == p.x[1] and p.s[1] == 0.0 and p.first_same_x[1] == 0
    plain_st, plain = start(straight, (0.5, 0.0))
    st, r = start(p, (0.5, 0.0))
    assert plain["margin_frame"] > 1e-6 and plain["margin_frame_ties_ok"] == plain["margin_frame"] and plain["zero_links"] == 0
    assert r["margin_frame"] == 0.0 and r["margin_frame_ties_ok"] > 1e-6 and r["zero_links"] >= 5
    assert r["visible"] == plain["visible"] + r["zero_links"] == r["chain"] and r["latched"] == 1
    assert np.array_equal(r["obs"], plain["obs"])                 # copies add no length: the resampled line is the same
    vis = np.nonzero((p.x - 0.5 >= 0.112) & (p.x - 0.5 <= 0.272))[0]
    pts, order = goto_path.chain_sort(np.stack((p.x[vis] - 0.5, p.y[vis]), axis=-1))
    assert np.array_equal(order, np.arange(len(vis)))            # index order, the copies included
    chain, cs, acc, gap, _, gap_ties_ok = goto_model.chain_points(p.x[vis] - 0.5, p.y[vis].copy(), 30e-3)
    assert np.array_equal(np.array(chain), pts) and gap == 0.0 and gap_ties_ok > 1e-6
    assert goto_model._argmin2(np.array([3.0, 1.0, 1.0, 2.0])) == (1, 0.0)
    r = goto_model.post_step(C, st, p, (p.x[100], 0.0), QUAT0)    # on a doubled point: copies 99 and 100
    assert p.x[99] == p.x[100] and (r["nearest"], r["margin"]) == (99, 0.0) and r["first_same"][1] == 99
    # a stretch of triple points
    p3 = goto_edges.with_copies(straight, triple=(60, 90))
    st, r = start(p3, (0.5, 0.0))
    assert r["margin_frame"] == 0.0 and r["margin_frame_ties_ok"] > 1e-6 and r["zero_links"] >= 10 and np.array_equal(r["obs"], plain["obs"])
