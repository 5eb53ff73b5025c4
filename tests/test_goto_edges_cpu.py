"""The inputs of tests/test_goto_edges_gpu.py (tests/goto_edges.py) on the float64 model alone: that each run meets what it is
there to compare and how much of it the margin rule leaves out, so that the seeds are known to be good before a GPU is used.
Measured: dense paths (all 256 robots) 0 of 15360 robot-ticks left out, 84.0 % of the 14106 live ones with a chain above 64
points, 2233 with fewer than 64 visible, 711 with more than 128 and the overflow flag set; repeated points 0 % under the
tie rule (67 % under margin_frame); every shape-limit case and every odd batch 0 %."""
import numpy as np
import pytest

from robot_gym_amd.core import goto_abi
from tests import goto_edges as E
from tests import goto_fixtures as F


def test_dense_paths_use_the_second_register_slot():
    """A 64-robot slice of the dense case: most live chains are longer than 64 points, some robots see fewer than 64, some
    (on the 1.3 mm paths) more than 128 with the overflow flag set."""
    c, paths, poses = E.dense_case(64)
    assert c["n_max"] == 2048 and c["max_visible"] == 128 and max(p.n for p in paths) <= 2048
    assert all(abs(np.diff(p.s).mean() - E.DENSE["fine_spacing" if b % 4 == 3 else "spacing"]) < 1e-5 for b, p in enumerate(paths))
    m = F.run_model(c, paths, poses, workers=1)
    out_tick, out_obs = F.excluded(m)
    live = (m["frozen"] == 0) & ~out_tick
    share = (m["chain"][live] > 64).mean()
    print(f"dense: left out {out_tick.mean():.4%} of robot-ticks, {out_obs.mean():.4%} of observations; chain > 64 on {share:.1%} of {live.sum()}")
    assert out_tick.mean() <= out_obs.mean() <= 0.01
    assert share >= 0.30 and (m["visible"][live] < 64).sum() > 0
    over = live & (m["visible"] > 128)
    print(f"dense: {over.sum()} live compared robot-ticks see more than 128 points, the most {m['visible'][live].max():.0f}")
    assert over.sum() >= 25 and (m["overflow"][over] == 1).all()


def test_repeated_points_are_compared_under_the_tie_rule():
    c, paths, poses = E.ties_case()
    assert {int((np.diff(p.s) == 0).sum() > 0) for p in paths} == {1} and max(p.n for p in paths) <= c["n_max"]
    m = F.run_model(c, paths, poses, workers=1)
    live = m["frozen"] == 0
    old, _ = F.excluded(m)
    new, new_obs = F.excluded(m, ties_ok=True)
    print(f"ties: margin_frame leaves out {old.mean():.2%}, margin_frame_ties_ok {new.mean():.4%} / {new_obs.mean():.4%}; zero-length links on {(live & (m['zero_links'] > 0)).sum()} live robot-ticks")
    assert old.mean() > 0.5 and new.mean() <= new_obs.mean() <= 0.01
    assert (live & ~new & (m["zero_links"] > 0)).sum() >= 100


def test_the_mirrored_path_ties_between_different_points():
    c, paths, poses = E.mirror_case()
    m = F.run_model(c, paths, poses, workers=1)
    assert (m["margin_frame"] == 0).all() and (m["margin_frame_ties_ok"] == 0).all()      # no copies: a tie of two points
    assert (m["frozen"] == 0).all() and (2 * m["chain"] == m["visible"]).all() and (m["chain"] >= 10).all()
    assert (m["obs"][0, 1] < 0).all() and (m["obs0"][1] < 0).all() and (m["latched"] == 1).all()


@pytest.mark.parametrize("name", list(E.SHAPES))
def test_shape_limit_runs(name):
    c, paths, poses = E.shape_case(name)
    m = F.run_model(c, paths, poses, workers=1)
    out_tick, out_obs = F.excluded(m)
    live = (m["frozen"] == 0) & ~out_tick
    assert out_tick.mean() <= out_obs.mean() <= 0.01 and live.sum() > 0.2 * live.size
    assert np.isfinite(m["obs"]).all() and (m["latched"][live] == 1).sum() > 100
    packed = E.poisoned_pack(paths, c["n_max"])
    assert all(np.isfinite(packed["x"][k, :p.n]).all() and np.isnan(packed["x"][k, p.n:]).all() for k, p in enumerate(paths))
    if name == "n_max_100":
        npts = np.array([p.n for p in paths])
        assert set(npts.tolist()) == set(E.SHAPE_NPTS) and (m["frozen"][0, npts == 2] == 0).all()
    if name == "two_visible":
        assert m["overflow"][-1].sum() > 32 and m["chain"].max() == 2
    if name == "one_checkpoint":
        assert (m["next_cp"] <= 1).all()


@pytest.mark.parametrize("B", E.ODD_BATCHES)
def test_odd_batch_runs_leave_nothing_out(B):
    """goto_edges.odd_model: what the margin rule leaves out of the 8 ticks around the partial set_path, and that the run has
    live robots to compare before and after it."""
    m = E.odd_model(B)
    print(f"odd batch {B}: left out {m['out_tick'].sum()} of {m['out_tick'].size} robot-ticks, {m['out_obs'].sum()} of their observations")
    assert m["out_tick"].mean() <= m["out_obs"].mean() <= 0.01
    if B < 100:
        assert not m["out_obs"].any()                  # one doubtful robot-tick would be above 1 % of a batch this small
    assert sorted(m["idx"].tolist()) == sorted({0, B // 2, B - 1}) and (B < 3 or m["idx"].tolist() != sorted(m["idx"].tolist()))
    live = m["state"][:, goto_abi.ROW_DONE] == 0
    assert live[5].mean() > 0.5 and live[6][m["idx"]].all() and (m["state"][7, goto_abi.ROW_VISIBLE] > 0).mean() > 0.5
