"""The float64 model of the position-mode controllers (tests/posctl_model.py) against the recordings of the reference
classes, and the recordings against the question they exist to answer: do they tell the configuration's fields apart?

No GPU: the model is plain numpy.  The GPU kernels are held to the same recordings and to this model in
tests/test_posctl_gpu.py and tests/test_posctl_configs_gpu.py."""
import os

import numpy as np
import pytest

from tests import posctl_fixtures as F
from tests import posctl_model as M


@pytest.fixture(scope="module")
def configs():
    return F.load_configs()


@pytest.fixture(scope="module")
def default():
    return F.load_default()


def _replay(rec):
    worst, m = F.model_gait_diff(rec)
    pose, pm = F.model_pose_diff(rec)
    print(f"{rec['name']}: phi {worst['phi']} last_time {worst['last_time']} mismatches, alpha {worst['alpha']:.3g} "
          f"frames {worst['frames']:.3g} (relative), angles {worst['angles']:.3g} pose angles {pose:.3g} rad")
    assert worst["phi"] == 0 and worst["last_time"] == 0, worst
    assert worst["alpha"] <= F.REL_TOL and worst["frames"] <= F.REL_TOL and worst["angles"] <= F.ANG_TOL, worst
    assert pose <= F.ANG_TOL
    assert F.model_motor_ok(rec)
    return m, pm


def test_model_replays_the_default_recordings(default):
    _replay(default)


@pytest.mark.parametrize("i", range(6))
def test_model_replays_the_configured_recordings(configs, i):
    assert len(configs) == 6
    _replay(configs[i])


def test_recorded_configurations_are_what_the_issue_asks_for(configs):
    """Four different hip vertices, foot frames and offsets with no mirror symmetry, three different link lengths, twelve
    different gains, stance shares on both sides of 0.5 (one dyadic), a walk set of offsets, and one configuration where
    the sign of a start frame's y does not follow its leg's side."""
    crossed = 0
    for rec in configs:
        c = rec["cfg"]
        assert len({c.hip, c.leg, c.foot}) == 3
        assert len(set(c.motor_kp)) == 12 and len(set(c.motor_kd)) == 12
        for field in ("hip_v", "pose_frames", "start_frames"):
            v = np.abs(np.asarray(getattr(c, field)).reshape(4, 3))
            for a in range(4):
                for b in range(a + 1, 4):
                    assert not np.array_equal(v[a], v[b]), (rec["name"], field, a, b)     # no leg mirrors another
        y = np.asarray(c.start_frames).reshape(4, 3)[:, 1]
        crossed += int(not np.array_equal(y > 0, [False, True, False, True]))
    so = [rec["cfg"].step_offset for rec in configs]
    assert min(so) < 0.5 < max(so) and 0.625 in so
    offsets = [rec["cfg"].leg_offset for rec in configs]
    assert any(len(set(o)) == 4 for o in offsets) and (0.0, 0.5, 0.5, 0.0) in offsets
    assert crossed >= 1


def test_new_recordings_tell_every_field_apart(configs):
    unseen = F.unseen_exchanges(configs)
    assert unseen == [], f"the recorded configurations are too symmetric to notice: {unseen}"


def test_default_recordings_cannot_tell_these_apart(default):
    """The same exchanges against the three recordings on the reference's own constants: what they cannot see, as a list.
    It is the reason posctl_configs.npz exists, and it is asserted so that a change of the model or of the comparison that
    made it blind would show here: the old recordings must go on noticing what they notice."""
    legs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
    expected = {"leg_offset[leg 0<->1]", "leg_offset[leg 2<->3]", "step_offset<->1-step_offset"}        # 0, 0, 0.8, 0.8 and 0.5
    expected |= {f"motor_kp[{j}<->{j + 1}]" for j in range(11)}                                          # 220 x 12
    expected |= {f"motor_{g}[{3 * a + j}<->{3 * b + j}]" for g in ("kp", "kd") for a, b in legs for j in range(3)}
    expected |= {f"motor_kd[{j}<->{j + 1}]" for j in (1, 4, 7, 10)}                                      # (1, 2, 2) x 4
    unseen = F.unseen_exchanges([default])
    print(f"the default recordings do not notice {len(unseen)} of {len(F.exchanges(default['cfg']))} exchanges")
    assert set(unseen) == expected, sorted(set(unseen) ^ expected)


def test_branch_census(configs):
    """Every branch of the three operations is taken at least once by the recordings of posctl_configs.npz, the two exact
    equalities and the negative phase included."""
    census = M.new_census()
    for rec in configs:
        _, m = F.model_gait_diff(rec)
        _, pm = F.model_pose_diff(rec)
        for k in census:
            census[k] += m.census[k] + pm.census[k]
    print(census)
    missing = [k for k, v in census.items() if v == 0]
    assert not missing, missing


def test_boundary_streams_hit_their_equalities(configs):
    for rec in configs:
        sub = dict(rec)
        b = rec["boundary_streams"]
        for k in F.GAIT_KEYS[:-1]:
            sub[k] = rec[k][b]
        _, m = F.model_gait_diff(sub)
        assert m.census["p_eq_step_offset"] >= 1 and m.census["p_eq_1"] >= 1 and m.census["p_negative"] >= 16, (rec["name"], m.census)


@pytest.mark.parametrize("seed", F.SEEDS + (F.SCALAR_CLOCK_SEED,))
def test_random_inputs_stay_well_conditioned(configs, seed):
    """The inputs of the GPU-against-model tests, on the model alone: the share of angle triples that the comparison
    would leave out (an IK domain within 1e-6 of +-1, sqrt_value within its margin of 0) stays under the cap, so this is
    known before a GPU is involved."""
    cfg, params, clock, resets, shift_at = F.gait_case(configs, seed, scalar_clock=seed == F.SCALAR_CLOCK_SEED)
    out, m = F.model_run(cfg, params, clock, resets, shift_at=shift_at)
    left_out = sum(int((~ok).sum()) for _, _, ok in out)
    total = sum(ok.size for _, _, ok in out)
    print(f"seed {seed}: {left_out} of {total} angle triples left out; clamped {m.census['domain_above_1'] + m.census['domain_below_m1']}")
    assert left_out <= F.MASK_CAP * total
    assert m.census["p_negative"] > 0 and m.census["swing"] > 0 and m.census["stance"] > 0


@pytest.mark.parametrize("batch", [4096, 32768])
def test_random_poses_stay_well_conditioned(configs, batch):
    for seed in F.POSE_SEEDS:
        cfg = F.random_config(configs[seed % len(configs)], seed)
        pm = M.PoseModel(cfg)
        pm.angles(F.random_poses(batch, seed))
        ok = M.comparable(*pm.ik_margin(), cfg, F.ANG_TOL)
        print(f"seed {seed} batch {batch}: {int((~ok).sum())} of {ok.size} angle triples left out; census {pm.census['domain_above_1']} "
              f"{pm.census['domain_below_m1']} {pm.census['sqrt_value_negative']}")
        assert (~ok).sum() <= F.MASK_CAP * ok.size


def test_generator_keeps_reference_text_out():
    """posctl_configs.npz holds arrays of numbers, names and flags only."""
    g = np.load(os.path.join(F.GOLDEN, "posctl_configs.npz"))
    for k in g.files:
        assert g[k].dtype.kind in "fbiU", (k, g[k].dtype)
    assert os.path.getsize(os.path.join(F.GOLDEN, "posctl_configs.npz")) < os.path.getsize(os.path.join(F.GOLDEN, "bezier_gait.npz"))
