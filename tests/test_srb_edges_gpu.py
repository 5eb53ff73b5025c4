"""The single-rigid-body simulator's kernels where tests/test_srb_gpu.py does not go: batches that leave a partial wave and a
partial workgroup, settings other than the defaults, non-finite inputs, a side stream, and a step before any reset.

Every run is a model run recorded before the GPU is opened (tests/srb_edges.py; tests/test_srb_streams_cpu.py checks the
same runs on the model alone) and replayed through a raw-buffer harness whose state and observation tensors lie between
sentinels.  The comparison and its tolerances are those of test_kernel_vs_model.

Every test prints its largest deviations (pytest -s).  No robot-tick is left out: the model alone finds no fall decision
within 1e-9 of its threshold.
"""
import numpy as np
import pytest
import torch

from tests import srb_model as M
from tests import srb_edges as E
from tests import srb_streams as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recordings():
    """Every model run of this module, made BEFORE a test opens the GPU: `dev` depends on this fixture."""
    out = {("odd", B): E.run_odd_batch(B) for B in E.ODD_BATCHES}
    out.update({("off", name): E.run_off_default(name) for name in E.OFF_DEFAULT})
    out["clean"], out["poisoned"] = E.run_poison(False), E.run_poison(True)
    return out


@pytest.fixture(scope="module")
def dev(recordings):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.mark.parametrize("B", E.ODD_BATCHES)
def test_odd_batches(B, recordings, dev):
    """Kernel against model with the assertions of test_kernel_vs_model, on batches that end inside a wave (1, 3, 15, 17, 63
    robots), inside a workgroup (65, 257, 1000) or one robot past one (65, 257), with a reset of robots B-1, 0 and one in
    between at tick 10 and the last robot frozen at the end -- where the lanes past the batch read.  Sentinels before and
    after every buffer are checked after every tick."""
    rec = recordings["odd", B]
    cmp = S.Comparison()
    raw = S.replay(rec, dev, cmp)
    st, _ = raw.numpy()
    print(f"B={B}: largest deviations", cmp.worst)
    assert st[M.ROW_STATUS, B - 1] == 1 and (st[M.ROW_STATUS, :B - 1] == 0).all()
    assert np.isfinite(st).all()
    assert cmp.clean(), (cmp.bad, cmp.worst)
    raw.close()


@pytest.mark.parametrize("name", list(E.OFF_DEFAULT))
def test_off_default_settings(name, recordings, dev):
    """512 robots, 60 ticks under (substeps, dt_sim, fall_height_scale, fall_tilt) = (1, 0.001, 0.5, 1.0), (7, 0.002, 0.8, 0.3)
    -- k3lso, with its init_q and ik_iters -- and (33, 0.0005, 0.9, 0.15).  In each, 32 robots pass the height threshold
    and 32 the tilt threshold at ticks of their own; none of those decisions is within 1e-9 of its threshold in the model, so
    nothing is left out.  steps and t_robot are bit-exact (Comparison's integer rows and t_robot)."""
    rec = recordings["off", name]
    by_height, by_tilt, near = E.fall_causes(rec)
    assert by_height.sum() >= 8 and by_tilt.sum() >= 8 and near == 0
    assert (rec.states[-1][M.ROW_STATUS] == 0).sum() >= rec.B // 2
    cmp = S.Comparison()
    raw = S.replay(rec, dev, cmp)
    st, obs = raw.numpy()
    print(f"{name}: largest deviations", cmp.worst, "fell by height", int(by_height.sum()), "by tilt", int(by_tilt.sum()))
    assert np.array_equal(st[M.ROW_STEPS], rec.states[-1][M.ROW_STEPS]) and np.array_equal(obs["t_robot"], rec.obs[-1]["t_robot"])
    assert np.array_equal(st[M.ROW_STATUS], rec.states[-1][M.ROW_STATUS])
    assert np.isfinite(st).all()
    assert cmp.clean(), (cmp.bad, cmp.worst)
    raw.close()


def _trace(rec, dev, cmp=None):
    """-> per tick (after the start, then after every tick): (state, obs dict) host copies, and the RawSim."""
    out = []
    raw = S.replay(rec, dev, cmp, after=lambda k, raw: out.append(raw.numpy()))
    return out, raw


def test_non_finite_inputs_stay_in_their_robot(recordings, dev):
    """130 robots; at tick 12 robots 0, 1, 63 and 64 are handed a NaN / an Inf in the grf of a stance leg, a NaN in the
    foot_target of a swing leg and a NaN in ext: they are flagged, and state and observation keep the values of tick 11 bit
    for bit.  Robot 129's NaN in the grf of a swing leg is never read.  Every other robot -- the neighbours 2, 62 and 65 in
    the victims' waves among them -- is bit-identical to the run without those values at every tick, and the model gives
    the same flags.  These are values in the data; nothing is done to the device.
    What this does not tell apart: each poisoned value reaches all four leg lanes of its robot anyway (through the summed
    wrench, or the NaN torque of the swing foot), so the test sees the flag leak to a neighbour, robots 62 and 65 for a
    shuffle over the wrong distance, but would not notice the shuffles of `bad` being dropped altogether."""
    clean_rec, bad_rec = recordings["clean"], recordings["poisoned"]
    cmp_clean, cmp_bad = S.Comparison(), S.Comparison()
    clean, raw0 = _trace(clean_rec, dev, cmp_clean)
    bad, raw1 = _trace(bad_rec, dev, cmp_bad)
    assert cmp_clean.clean() and cmp_bad.clean(), (cmp_clean.bad, cmp_bad.bad)       # the model's flags among the integer rows
    B, at = E.POISON_BATCH, E.POISON_AT
    victims = list(E.POISON_VICTIMS)
    others = np.setdiff1d(np.arange(B), victims)
    assert E.POISON_IGNORED in others and {2, 62, 65} <= set(others.tolist())
    for k, ((st0, obs0), (st1, obs1)) in enumerate(zip(clean, bad)):
        assert np.array_equal(st0[:, others], st1[:, others]), k
        for name in obs0:
            assert np.array_equal(obs0[name][..., others], obs1[name][..., others]), (k, name)
        assert np.isfinite(st1).all() and all(np.isfinite(v).all() for v in obs1.values()), k
    rows = np.arange(M.STATE_ROWS) != M.ROW_STATUS
    kept_st, kept_obs = bad[at]                       # entry k + 1 is the state after tick k: this is after tick 11
    assert (kept_st[M.ROW_STATUS, victims] == 0).all()
    for k in range(at + 1, len(bad)):
        st, obs = bad[k]
        assert (st[M.ROW_STATUS, victims] == 1).all() and (st[M.ROW_STATUS, others] == 0).all(), k
        assert np.array_equal(st[rows][:, victims], kept_st[rows][:, victims]), k
        for name in obs:
            assert np.array_equal(obs[name][..., victims], kept_obs[name][..., victims]), (k, name)
    assert (clean[-1][0][M.ROW_STATUS] == 0).all()
    raw0.close()
    raw1.close()


def test_side_stream(recordings, dev):
    """The first 20 ticks of the 257-robot run enqueued on a side stream (the handle takes torch's current stream): bit
    for bit the result of the default stream."""
    rec = recordings["odd", 257]
    ticks = 20

    def run():
        raw = S.RawSim(rec.cfg, rec.B, dev, **rec.sim_kw)
        raw.set_body(rec.body_idx, rec.s["mass"][rec.body_idx], rec.s["inertia"][:, rec.body_idx])
        raw.reset(xy=rec.start[0], yaw=rec.start[1], height=rec.start[2])
        held = []
        for k in range(ticks):
            if k in rec.resets:
                idx, xy, yaw, h = rec.resets[k]
                raw.reset(idx=idx, xy=xy, yaw=yaw, height=h)
            raw.step(*rec.inputs[k])
            held.append(raw._held)           # the inputs stay allocated until the stream has run
        return raw, held

    ref, _ = run()
    want = ref.numpy()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got_raw, held = run()
    side.synchronize()
    got = got_raw.numpy()
    assert np.array_equal(want[0], got[0]) and all(np.array_equal(want[1][k], got[1][k]) for k in want[1])
    assert (got[0][M.ROW_STEPS] > 0).all() and got_raw.guards_intact()
    cmp = S.Comparison()
    cmp.check(got[0], got[1], rec.states[ticks], rec.obs[ticks])
    assert cmp.clean(), cmp.bad
    ref.close()
    got_raw.close()


def test_step_before_any_reset_touches_nothing(recordings, dev):
    """A handle whose robots were never reset (status 1) is stepped: state, observation and sentinels stay as they were."""
    rec = recordings["odd", 65]
    raw = S.RawSim(rec.cfg, rec.B, dev)
    raw.state[:M.ROW_STATUS] = 0.25                 # recognisable values a store would change
    for v in raw.obs.values():
        v.fill_(3)
    st0, obs0 = raw.numpy()
    for k in range(3):
        raw.step(*rec.inputs[k])
    st1, obs1 = raw.numpy()
    assert np.array_equal(st0, st1) and all(np.array_equal(obs0[k], obs1[k]) for k in obs0)
    assert (st1[M.ROW_STATUS] == 1).all() and raw.guards_intact()
    raw.close()
