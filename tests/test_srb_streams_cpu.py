"""The seeded inputs of tests/test_srb_edges_gpu.py on the float64 model alone (tests/srb_edges.py): that every run meets
what it is there to compare, and that no fall decision of a run lies so near its threshold that kernel and model could
legitimately part -- checked here, so that the seeds are known to be good before a GPU is used."""
import numpy as np
import pytest

from tests import srb_model as M
from tests import srb_edges as E


@pytest.mark.parametrize("name", list(E.OFF_DEFAULT))
def test_off_default_runs_fall_by_height_and_by_tilt(name):
    rec = E.run_off_default(name)
    by_height, by_tilt, near = E.fall_causes(rec)
    st = rec.states[-1]
    running = int((st[M.ROW_STATUS] == 0).sum())
    print(name, "by height", int(by_height.sum()), "by tilt", int(by_tilt.sum()), "running", running, "near a threshold", near)
    assert by_height.sum() >= 8 and by_tilt.sum() >= 8 and running >= rec.B // 2
    assert (by_height & rec.s["sink"]).sum() >= 8 and (by_tilt & rec.s["tip"]).sum() >= 8
    assert near == 0
    assert np.isfinite(st).all()
    # the robots fall at ticks of their own, so a frozen and a running robot share waves for most of the run
    fell_at = np.array([s[M.ROW_STATUS] != 0 for s in rec.states]).argmax(0)[by_tilt]
    assert len(np.unique(fell_at)) >= 8
    # steps counts substeps, t_robot is steps * dt_sim
    kw = rec.sim_kw
    assert (st[M.ROW_STEPS, st[M.ROW_STATUS] == 0] == kw["substeps"] * rec.ticks).all()
    assert np.array_equal(rec.obs[-1]["t_robot"], st[M.ROW_STEPS] * kw["dt_sim"])


@pytest.mark.parametrize("B", E.ODD_BATCHES)
def test_odd_batch_runs_end_with_the_last_robot_frozen(B):
    rec = E.run_odd_batch(B)
    status = np.array([s[M.ROW_STATUS] for s in rec.states])          # [T + 1, B]
    assert status[-1, B - 1] == 1 and status[-6, B - 1] == 1          # frozen for the last five ticks at least
    assert status[E.ODD_RESET_AT + 1, B - 1] == 0                      # the reset stood it up
    assert (status[-1, :B - 1] == 0).all()
    assert E.fall_causes(rec)[2] == 0
    idx = E.odd_reset_list(B)
    assert {0, B - 1} <= set(idx.tolist()) and len(set(idx.tolist())) == len(idx) == min(B, 3)
    if B > 2:
        assert 0 < idx[2] < B - 1 and list(idx) != sorted(idx)
    steps = rec.states[-1][M.ROW_STEPS]
    others = np.setdiff1d(np.arange(B), idx)
    assert (steps[others] == 10 * E.ODD_TICKS).all() and (steps[idx[1:]] == 10 * (E.ODD_TICKS - E.ODD_RESET_AT)).all()


def test_poisoned_run_flags_the_victims_and_nobody_else():
    clean, bad = E.run_poison(False), E.run_poison(True)
    victims = list(E.POISON_VICTIMS)
    others = np.setdiff1d(np.arange(E.POISON_BATCH), victims)
    at = E.POISON_AT
    for k in range(E.POISON_TICKS + 1):
        assert np.array_equal(clean.states[k][:, others], bad.states[k][:, others]), k
        assert np.isfinite(bad.states[k]).all()
    assert (clean.states[-1][M.ROW_STATUS] == 0).all()
    assert (bad.states[-1][M.ROW_STATUS, victims] == 1).all() and (bad.states[-1][M.ROW_STATUS, others] == 0).all()
    rows = np.arange(M.STATE_ROWS) != M.ROW_STATUS
    # state index k + 1 is the state after tick k: after the poisoned tick the victims hold their state of tick at - 1
    assert np.array_equal(bad.states[-1][rows][:, victims], bad.states[at][rows][:, victims])
    for name, v in bad.obs[-1].items():
        assert np.array_equal(v[..., victims], bad.obs[at][name][..., victims]), name
    assert np.isnan(bad.inputs[at][0][E.POISON_IGNORED]).sum() == 1      # the NaN of the swing leg was there, and changed nothing
