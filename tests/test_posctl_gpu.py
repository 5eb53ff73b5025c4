"""The position-mode controllers on the GPU against golden vectors recorded from the reference classes themselves
(tests/golden/make_posctl_golden.py): the Bezier trot, the pose IK and the POSITION motor model.

Tolerances (defined once, in tests/posctl_fixtures.py): phi and last_time bit-identical every tick (one subtraction and
one IEEE division, the branches taken on them); alpha and frames within 1e-9 * max(1, |value|) (irregular ticks put the
swing phase far above 1, where the degree-11 curve puts frames far from the body); angles within 2e-6 rad; torques
within one float32 ulp.  The same operations on configurations other than the default: tests/test_posctl_configs_gpu.py."""
import os
import types

import numpy as np
import pytest
import torch

from tests.posctl_fixtures import ANG_TOL, REL_TOL, Replay, clean as _clean

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gait():
    g = np.load(os.path.join(GOLDEN, "bezier_gait.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _bezier(batch, dev):
    from robot_gym_amd.controllers.bezier.batched import BatchedBezierController
    return BatchedBezierController(batch, device=dev)


def test_golden_streams_one_robot_each(gait, dev):
    S = gait["phi"].shape[0]
    ctrl = _bezier(S, dev)
    bad = Replay(gait, np.arange(S), dev).run(ctrl)
    assert _clean(bad), bad


@pytest.mark.parametrize("batch", [4096, 32768])
def test_golden_streams_at_scale(gait, dev, batch):
    S = gait["phi"].shape[0]
    perm = np.random.default_rng(batch).permutation(batch)
    ctrl = _bezier(batch, dev)
    bad = Replay(gait, perm % S, dev).run(ctrl)
    assert _clean(bad), bad


@pytest.mark.parametrize("batch", [1, 63, 65])
def test_tail_workgroups(gait, dev, batch):
    S = gait["phi"].shape[0]
    ctrl = _bezier(batch, dev)
    bad = Replay(gait, (np.arange(batch) * 7 + 3) % S, dev).run(ctrl)
    assert _clean(bad), bad


def test_get_action_without_update(gait, dev):
    ctrl = _bezier(65, dev)
    first = ctrl.get_action().cpu().numpy()
    assert np.abs(first - gait["angles_first"][None, :]).max() <= ANG_TOL
    rp = Replay(gait, np.arange(65) % gait["phi"].shape[0], dev)
    for k in range(20):
        a = rp.tick(ctrl, k).clone()
    again = ctrl.get_action()
    assert torch.equal(again, a)
    # params NULL on the frames held: the same IK as the update's, bit for bit, and the state untouched
    state = ctrl.state.clone()
    out = torch.full_like(a, float("nan"))
    ctrl._handle.bezier_step(123.0, None, None, ctrl.state.data_ptr(), out.data_ptr())
    assert torch.equal(out, a) and torch.equal(ctrl.state, state)
    # after a reset, get_action is the IK of the constructor frames again
    ctrl.reset([4, 64], t0=1.0)
    b = ctrl.get_action().cpu().numpy()
    assert np.abs(b[[4, 64]] - gait["angles_first"][None, :]).max() <= ANG_TOL
    assert np.array_equal(b[:4], a[:4].cpu().numpy())


def _pose_ctrl(batch, dev):
    from robot_gym_amd.controllers.pose.batched import BatchedPoseController
    return BatchedPoseController(batch, device=dev)


def test_pose_golden(dev):
    p = np.load(os.path.join(GOLDEN, "pose_ik.npz"))
    n = len(p["pose"])
    ctrl = _pose_ctrl(n, dev)
    ctrl.update_controller_params(torch.as_tensor(p["pose"]))
    a = ctrl.get_action().cpu().numpy().astype(np.float64)
    assert np.abs(a - p["angles"]).max() <= ANG_TOL
    # embedded at scattered robots of a batch of 4096, the others on other poses
    B = 4096
    rng = np.random.default_rng(5)
    where = rng.choice(B, n, replace=False)
    poses = rng.uniform(-0.3, 0.3, (B, 6)).astype(np.float32)
    poses[where] = p["pose"]
    big = _pose_ctrl(B, dev)
    big.update_controller_params(torch.as_tensor(poses))
    a = big.get_action().cpu().numpy().astype(np.float64)
    assert np.abs(a[where] - p["angles"]).max() <= ANG_TOL
    # the zero pose (the drop-in's start: deviation 3) is the fixture's first pose
    fresh = _pose_ctrl(3, dev).get_action().cpu().numpy()
    assert np.abs(fresh - p["angles"][0]).max() <= ANG_TOL


@pytest.mark.parametrize("substeps", [1, 10])
def test_position_torque(dev, substeps):
    m = np.load(os.path.join(GOLDEN, "motor_position.npz"))
    n = len(m["angles"])
    ctrl = _pose_ctrl(n, dev)
    q = torch.as_tensor(m["q"][:, :substeps].astype(np.float32).transpose(1, 2, 0).copy())     # [S, 12, n]
    qd = torch.as_tensor(m["qd"][:, :substeps].astype(np.float32).transpose(1, 2, 0).copy())
    tau = ctrl.position_to_torque(torch.as_tensor(m["angles"]), q, qd, substeps=substeps).cpu().numpy()   # [S, n, 12]
    want = m["tau"][:, :substeps].transpose(1, 0, 2).astype(np.float32)
    assert tau.shape == want.shape
    assert np.all(np.abs(tau - want) <= np.spacing(np.abs(want))), np.abs(tau - want).max()


def test_save_load_copy(gait, dev):
    S, T = gait["phi"].shape
    half = T // 2
    sidx = np.arange(S)
    rp = Replay(gait, sidx, dev)
    ctrl = _bezier(S, dev)
    for k in range(half):
        rp.tick(ctrl, k)
    saved = ctrl.save_state()
    assert saved.rows.shape == (S, 15) and saved.rows.dtype == np.float64 and list(saved.robots) == list(range(S))
    first = []
    for k in range(half, T):
        first.append((rp.tick(ctrl, k).clone(), ctrl.state.clone()))
    ctrl.load_state(saved)
    for k in range(half, T):
        a = rp.tick(ctrl, k)
        assert torch.equal(a, first[k - half][0]) and torch.equal(ctrl.state, first[k - half][1]), k
    # a clone follows its source bit for bit under the same inputs
    rp2 = Replay(gait, np.concatenate([sidx, sidx]), dev)
    two = _bezier(2 * S, dev)
    for k in range(half):
        rp2.tick(two, k)
    two.reset(np.arange(S, 2 * S), t0=-5.0)
    two.copy_state(np.arange(S), np.arange(S, 2 * S))
    for k in range(half, T):
        a = rp2.tick(two, k)
        assert torch.equal(a[:S], a[S:]) and torch.equal(two.state[:, :S], two.state[:, S:]), k
    # clock_shift: the saved state resumed on a clock shifted by dt runs as a controller that ran on the shifted clock
    # from the start (same clock origin, so phi and last_time bit-identical from the resume on).  Streams with irregular
    # ticks only: on a regular 0.01 s clock a phase can land within an ulp of a branch point (0.5, 0.99), where the
    # rounding of the shifted clock alone would pick the other branch.
    irregular = np.array([s for s in range(S) if np.ptp(np.diff(gait["clock"][s])) > 1e-9])
    assert len(irregular) >= 6
    rp = Replay(gait, irregular, dev)
    n = len(irregular)
    base = _bezier(n, dev)
    for k in range(half):
        rp.tick(base, k)
    saved = base.save_state()
    dt = 17.5
    shifted = _bezier(n, dev)
    for k in range(half):
        rp.tick(shifted, k, clock_shift=dt)
    resumed = _bezier(n, dev)
    resumed.load_state(saved, clock_shift=dt)
    for k in range(half, T):
        a1, a2 = rp.tick(shifted, k, clock_shift=dt), rp.tick(resumed, k, clock_shift=dt)
        assert torch.equal(shifted.state[:2], resumed.state[:2]), k
        d = (shifted.state[2:] - resumed.state[2:]).abs() <= REL_TOL * shifted.state[2:].abs().clamp(min=1)
        assert bool(d.all()), k
        assert float((a1 - a2).abs().max()) <= ANG_TOL, k


def test_nan_param_stays_in_its_robot(gait, dev):
    S, T = gait["phi"].shape
    rp = Replay(gait, np.arange(S), dev)
    clean, dirty = _bezier(S, dev), _bezier(S, dev)
    victim, k_bad = 5, 40
    for k in range(T):
        a = rp.tick(clean, k)
        robots = np.nonzero(rp.reset[:, k])[0]
        if robots.size:
            dirty.reset(robots, t0=rp.t0[robots, k])
        p = rp.params[:, k].clone()
        if k == k_bad:
            p[victim, 3] = float("nan")
        dirty.update_controller_params(p, rp.clock[:, k])
        b = dirty.get_action()
        others = np.r_[0:victim, victim + 1:S]
        assert torch.equal(a[others], b[others]) and torch.equal(clean.state[:, others], dirty.state[:, others]), k
        if k >= k_bad and not rp.reset[victim, k_bad:k + 1].any():
            assert not bool(torch.isfinite(b[victim]).any()), k


def test_non_default_stream(gait, dev):
    S = gait["phi"].shape[0]
    rp = Replay(gait, np.arange(S), dev)
    ref = _bezier(S, dev)
    outs = [rp.tick(ref, k).clone() for k in range(48)]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        ctrl = _bezier(S, dev)
        got = [rp.tick(ctrl, k).clone() for k in range(48)]
        pose = _pose_ctrl(S, dev)
        pose.update_controller_params(torch.full((S, 6), 0.01))
        pa = pose.get_action().clone()
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, got))
    pose0 = _pose_ctrl(S, dev)
    pose0.update_controller_params(torch.full((S, 6), 0.01))
    assert torch.equal(pose0.get_action(), pa)


# ---- drop-in plugins on a stub robot with a fake clock ----

def _stub_robot():
    p = np.load(os.path.join(GOLDEN, "pose_ik.npz"))
    hip, leg, foot = p["ghost_hip_leg_foot"]
    fr, hv = p["ghost_pose_frames"], p["ghost_hip_v"]
    ctrl = types.SimpleNamespace(hip=hip, leg=leg, foot=foot, x_dist=2 * fr[0, 0], y_dist=2 * fr[1, 1], height=-fr[0, 2],
                                 hip_front_right_v=hv[0], hip_front_left_v=hv[1], hip_rear_right_v=hv[2], hip_rear_left_v=hv[3])
    motor = types.SimpleNamespace(MOTOR_POSITION_GAINS=list(p["ghost_motor_kp"]), MOTOR_VELOCITY_GAINS=p["ghost_motor_kd"])
    return types.SimpleNamespace(GetCtrlConstants=lambda: ctrl, GetMotorConstants=lambda: motor)


class FakeBullet:
    def __init__(self):
        self.added = []

    def addUserDebugParameter(self, name, lo, hi, init):
        self.added.append((name, lo, hi, init))
        return len(self.added) - 1

    def readUserDebugParameter(self, i):
        return 10.0 + i


def test_bezier_drop_in(gait, dev):
    from robot_gym_amd.controllers.bezier.bezier_controller import BezierController
    clock = types.SimpleNamespace(now=0.0)
    S, T = gait["phi"].shape
    assert BezierController.MOTOR_CONTROL_MODE == 1
    for s in (0, 5, 7, 13, 14, 20):
        c = BezierController(_stub_robot(), lambda: clock.now, device=dev)
        assert np.abs(c.get_action() - gait["angles_first"]).max() <= ANG_TOL
        for k in range(T):
            if gait["reset"][s, k]:
                clock.now = float(gait["t0"][s, k])
                c.reset()
            clock.now = float(gait["clock"][s, k])
            c.update_controller_params(tuple(float(x) for x in gait["params"][s, k]))
            a = c.get_action()
            st = c._batched.state[:, 0].cpu().numpy()
            assert st[0] == gait["phi"][s, k] and st[1] == gait["last_time"][s, k], (s, k)
            assert np.abs(a - gait["angles"][s, k]).max() <= ANG_TOL, (s, k)
    ui = FakeBullet()
    handles = BezierController.setup_ui_params(ui)
    assert [n for n, *_ in ui.added] == ["step_length", "step_rotation", "step_angle", "step_period"]
    assert [(lo, hi) for _, lo, hi, _ in ui.added] == [(-1.5, 1.5), (-1.5, 1.5), (-180., 180.), (-1., 1.)]
    assert BezierController.read_ui_params(ui, handles) == (10.0, 11.0, 12.0, 13.0)


def test_pose_drop_in(dev):
    from robot_gym_amd.controllers.pose.pose_controller import PoseController
    p = np.load(os.path.join(GOLDEN, "pose_ik.npz"))
    c = PoseController(_stub_robot(), lambda: 0.0, device=dev)
    assert PoseController.MOTOR_CONTROL_MODE == 1
    assert np.abs(c.get_action() - p["angles"][0]).max() <= ANG_TOL      # the zero pose before any update
    for k in range(0, len(p["pose"]), 7):
        c.update_controller_params((p["pose"][k, :3].astype(np.float64), p["pose"][k, 3:].astype(np.float64)))
        assert np.abs(c.get_action() - p["angles"][k]).max() <= ANG_TOL, k
    ui = FakeBullet()
    handles = PoseController.setup_ui_params(ui)
    assert [n for n, *_ in ui.added] == ["base_x", "base_y", "base_z", "roll", "pitch", "yaw"]
    pos, orient = PoseController.read_ui_params(ui, handles)
    assert list(pos) == [10.0, 11.0, 12.0] and list(orient) == [13.0, 14.0, 15.0]
