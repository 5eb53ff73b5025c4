"""The terrain height scan on the GPU (include/rg_scan.h, robot_gym_amd/csrc/rg_scan.hip) against tests/scan_model.py BIT FOR
BIT: every terrain kind, grid shape and awkward pose at B = 67 (one full 64-robot wave plus a tail of 3) and B = 1; that a
robot's scan does not depend on where in the batch it sits; the mask / prev rule; row views of a taller buffer; and the scan
inside BatchedGoEnv (observation, terminal observation under auto-reset, clone) and under the PPO collector.

Bit-exactness rests on float64 sqrt and division being correctly rounded on the device, as the simulator's ground test
already assumes of the division."""
import numpy as np
import pytest
import torch

from robot_gym_amd.core import srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import scan_model as SM
from tests import terrain_model as TM

pytestmark = pytest.mark.gpu

GRIDS = (dict(nx=8, ny=6), dict(nx=3, ny=5, x_first=0.15, dx=-0.2, y_first=-0.3, dy=0.15), dict(nx=1, ny=1, x_first=0.35, y_first=0.0))
AMPLITUDE, CELL, SEED = 0.06, 0.05, 12345
GRID_CELL, GRID_ORIGIN = 0.25, (-0.4, 0.3)                       # 5 x 7 vertices: x in [-0.4, 0.6], y in [0.3, 1.8]
SENTINEL_OUT, SENTINEL_PREV = 7.25, -9.5


def _poses(B, seed):
    """A simulator state [43, B] of which the scan reads rows 0..6: yaw over the full circle, roll and pitch up to 0.3 rad,
    positions on both sides of zero (most within 1.5 m, so that a 5 x 7 grid is walked off on every side; every eighth robot
    up to 1e3 m out), heights around the body height.  With B >= 8: robot 5 has a NaN pz, robot 6 a zero quaternion."""
    rng = np.random.default_rng(seed)
    st = np.zeros((srb_abi.STATE_ROWS, B))
    span = np.where(np.arange(B) % 8 == 7, 1e3, 1.5)
    st[0], st[1] = rng.uniform(-1, 1, B) * span, rng.uniform(-1, 1, B) * span
    st[2] = rng.uniform(0.2, 0.45, B)
    yaw = np.linspace(-np.pi, np.pi, B) if B > 1 else np.array([2.5])
    roll, pitch = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B)
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    q = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])
    st[3:7] = q / np.sqrt((q * q).sum(0))
    if B >= 8:
        st[2, 5] = np.nan
        st[3:7, 6] = 0.0
    return st


def _keys(B, repeated):
    k = (np.arange(B, dtype=np.int64) * 7919 - 1000) % 4001 - 2000      # not the indices; negative ones among them
    return k % 3 - 1 if repeated else k


def _grid_heights():
    return np.random.default_rng(77).uniform(-0.05, 0.1, (5, 7))


class _Sim:
    """What HeightScan.bind reads of a simulator: the scan needs no BatchedSRBSim, only a state tensor."""

    def __init__(self, B, dev, cfg):
        self.batch, self.device, self.cfg, self.terrain = B, dev, cfg, None


def _world(kind, B, dev):
    """(model ground, terrain for HeightScan.set_terrain) of a terrain kind."""
    if kind == "plane":
        return TM.Flat(), None
    if kind == "grid":
        H = _grid_heights()
        from robot_gym_amd.sim.terrain import GridTerrain
        t = GridTerrain(H, GRID_CELL, GRID_ORIGIN)
        t.bind(B, dev)
        return TM.Grid(H, GRID_CELL, GRID_ORIGIN), t
    if kind == "random_null_key":
        return TM.Random(AMPLITUDE, CELL, SEED, None), srb_abi.make_cterrain(srb_abi.TERRAIN_RANDOM, cell=CELL, amplitude=AMPLITUDE, seed=SEED)
    from robot_gym_amd.sim.terrain import RandomTerrain
    keys = _keys(B, kind == "random_repeated")
    t = RandomTerrain(AMPLITUDE, CELL, SEED, keys=keys)
    t.bind(B, dev)
    return TM.Random(AMPLITUDE, CELL, SEED, keys), t


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cfg():
    return MPCConfig.for_robot("ghost")


def _scanner(B, dev, cfg, terrain=None, **settings):
    from robot_gym_amd.sim.height_scan import HeightScan
    scan = HeightScan(**settings).bind(_Sim(B, dev, cfg))
    scan.set_terrain(terrain)
    return scan


# ---- 1. the model, bit for bit -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", (67, 1))
@pytest.mark.parametrize("kind", ("random", "random_repeated", "random_null_key", "grid", "plane"))
def test_scan_is_the_model_bit_for_bit(dev, cfg, kind, B):
    st = _poses(B, 11)
    state = torch.as_tensor(st, device=dev)
    ground, terrain = _world(kind, B, dev)
    for n, grid in enumerate(GRIDS):
        settings = dict(grid, clip=(1.0, 0.0, 0.02)[n], scale=(1.0, 2.5, -4.0)[n])      # clipped, unclipped, clipped hard with a negative scale
        scan = _scanner(B, dev, cfg, terrain, **settings)
        got = scan.observe(state)
        want = SM.scan(st, ground, z_offset=cfg.body_height, **settings)
        assert tuple(got.shape) == want.shape == (grid["nx"] * grid["ny"], B) and got.dtype == torch.float32
        w = torch.as_tensor(want, device=dev)
        same = (w.view(torch.int32) == got.view(torch.int32)) | (torch.isnan(w) & torch.isnan(got))      # bits: -0.0 is not 0.0; any NaN is a NaN
        miss = ~same.cpu().numpy()
        assert not miss.any(), (kind, grid, np.argwhere(miss)[:8], got.cpu().numpy()[miss][:8], want[miss][:8])
        if kind in ("random", "grid") and n == 0:
            assert len(np.unique(want[np.isfinite(want)])) >= 8                # the ground is felt: the scan is not one height
        if B >= 8 and n != 1:
            assert (want[:, 5] == np.float32(-settings["clip"] * settings["scale"])).all()      # the NaN pz, clipped
        scan.close()


def test_a_lane_that_walks_several_points_gives_the_same_scan(dev, cfg):
    """At the batches above every lane has one point.  16 x 16 points (the most a scan may have) at B = 1100 are 18 waves a
    slice, so the launch splits the 256 points into 85 slices of 3 and one of 1 (rg_scan.hip, points_per_lane): a lane steps
    from point to point, across the end of a grid row, and the last slice is cut short."""
    B = 1100
    st = _poses(B, 14)
    ground, terrain = _world("random", B, dev)
    settings = dict(nx=16, ny=16, x_first=-0.4, dx=0.05, y_first=-0.35, dy=0.05)
    scan = _scanner(B, dev, cfg, terrain, **settings)
    got = scan.observe(torch.as_tensor(st, device=dev))
    want = torch.as_tensor(SM.scan(st, ground, z_offset=cfg.body_height, **settings), device=dev)
    assert tuple(got.shape) == (256, B)
    assert bool(((want.view(torch.int32) == got.view(torch.int32)) | (torch.isnan(want) & torch.isnan(got))).all())
    scan.close()


# ---- 2. a robot's scan does not depend on its place in the batch ---------------------------------------------------------------

def test_scan_does_not_depend_on_the_position_in_the_batch(dev, cfg):
    from robot_gym_amd.sim.terrain import RandomTerrain
    pose = _poses(1, 3)[:, 0]
    rows = []
    for B, at in ((1, 0), (67, 66), (200, 130)):
        st = _poses(B, 20 + B)
        st[:, at] = pose
        keys = _keys(B, False)
        keys[at] = 5
        t = RandomTerrain(AMPLITUDE, CELL, SEED, keys=keys)
        t.bind(B, dev)
        scan = _scanner(B, dev, cfg, t)
        rows.append(scan.observe(torch.as_tensor(st, device=dev))[:, at].clone())
        scan.close()
    assert torch.equal(rows[0], rows[1]) and torch.equal(rows[0], rows[2])
    assert len(torch.unique(rows[0])) > 8


# ---- 3. mask and prev ----------------------------------------------------------------------------------------------------------

def test_mask_and_prev(dev, cfg):
    B = 67
    st = _poses(B, 12)
    st[2, 5] = 0.3                                            # no NaN here: the sentinels are compared with ==
    state = torch.as_tensor(st, device=dev)
    ground, terrain = _world("random", B, dev)
    scan = _scanner(B, dev, cfg, terrain)
    new = torch.as_tensor(SM.scan(st, ground, z_offset=cfg.body_height), device=dev)
    mask = torch.as_tensor((np.arange(B) % 2).astype(np.int32) * np.where(np.arange(B) % 4 == 1, -3, 1).astype(np.int32), device=dev)   # odd robots, any non-zero value
    on = mask != 0
    out = torch.full((48, B), SENTINEL_OUT, dtype=torch.float32, device=dev)
    prev = torch.full((48, B), SENTINEL_PREV, dtype=torch.float32, device=dev)
    scan.observe(state, out=out, mask=mask, prev=prev)
    assert torch.equal(out[:, on], new[:, on]) and bool((prev[:, on] == SENTINEL_OUT).all())
    assert bool((out[:, ~on] == SENTINEL_OUT).all()) and bool((prev[:, ~on] == SENTINEL_PREV).all())
    # without prev only out is written; without a mask every robot is
    out.fill_(SENTINEL_OUT)
    scan.observe(state, out=out, mask=mask)
    assert torch.equal(out[:, on], new[:, on]) and bool((out[:, ~on] == SENTINEL_OUT).all())
    prev.fill_(SENTINEL_PREV)
    scan.observe(state, out=out, prev=prev)
    assert torch.equal(out, new)
    assert torch.equal(prev[:, on], new[:, on]) and bool((prev[:, ~on] == SENTINEL_OUT).all())
    none = torch.zeros(B, dtype=torch.int32, device=dev)
    out.fill_(SENTINEL_OUT)
    scan.observe(state, out=out, mask=none, prev=prev)
    assert bool((out == SENTINEL_OUT).all())
    scan.close()


# ---- 4. rows of a taller buffer --------------------------------------------------------------------------------------------------

def test_out_and_prev_may_be_rows_of_a_taller_buffer(dev, cfg):
    B = 67
    st = _poses(B, 13)
    st[2, 5] = 0.3
    state = torch.as_tensor(st, device=dev)
    ground, terrain = _world("grid", B, dev)
    scan = _scanner(B, dev, cfg, terrain)
    new = torch.as_tensor(SM.scan(st, ground, z_offset=cfg.body_height), device=dev)
    buf = torch.full((64, B), SENTINEL_OUT, dtype=torch.float32, device=dev)
    last = torch.full((70, B), SENTINEL_PREV, dtype=torch.float32, device=dev)
    scan.observe(state, out=buf[16:], prev=last[16:64])
    assert torch.equal(buf[16:], new) and bool((buf[:16] == SENTINEL_OUT).all())
    assert bool((last[16:64] == SENTINEL_OUT).all()) and bool((last[:16] == SENTINEL_PREV).all()) and bool((last[64:] == SENTINEL_PREV).all())
    for bad in (buf[:48].t(), buf[10:], torch.zeros(48, B, dtype=torch.float64, device=dev), buf[16:, :60], torch.zeros(48, B + 1, dtype=torch.float32, device=dev)[:, :B], buf[16:].cpu()):     # shape, dtype, row stride, device
        with pytest.raises(ValueError, match="observe: out"):
            scan.observe(state, out=bad)
    scan.close()


# ---- 5. the go-to task with the scan ---------------------------------------------------------------------------------------------

def _env(dev, B, scan, **kw):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim.terrain import RandomTerrain
    return BatchedGoEnv(B, device=dev, terrain=RandomTerrain(), contact="measured", max_time=0.75, seed=3, height_scan=scan, **kw)   # the time limit fires on tick 8


def _model_scan(env):
    t = env.sim.terrain
    ground = TM.Random(t.amplitude, t.cell, t.seed, t.keys.cpu().numpy())
    return torch.as_tensor(SM.scan(env.sim.state.cpu().numpy(), ground, z_offset=env.cfg.body_height), device=env.device).t()


def test_go_env_appends_the_scan_and_moves_the_terminal_one_into_final_obs(dev):
    """The twin has no scan and no auto-reset: it is stepped and then reset by hand with the calls step() makes under auto_reset,
    so its simulator state between the two is the terminal state, whose model scan is what final_obs must hold."""
    from robot_gym_amd.sim.height_scan import HeightScan
    B, STEPS = 8, 20
    env, twin = _env(dev, B, HeightScan(), auto_reset=True), _env(dev, B, None)
    assert tuple(env.obs.shape) == (B, 64) and tuple(env.final_obs.shape) == (B, 64) and tuple(twin.obs.shape) == (B, 16)
    low, high = env.observation_space_bounds
    assert low.shape == high.shape == (64,) and (low[16:] == -1.0).all() and (high[16:] == 1.0).all()
    assert (low[:16] == twin.observation_space_bounds[0]).all() and (high[:16] == twin.observation_space_bounds[1]).all()
    obs = env.reset()
    twin.reset()
    assert torch.equal(obs[:, :16], twin.obs) and torch.equal(obs[:, 16:], _model_scan(env))
    assert len(torch.unique(obs[:, 16:])) > 48                # the ground is felt, and differently by each robot
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    resets = 0
    for k in range(STEPS):
        final_before = env.final_obs.clone()
        obs, reward, done = env.step(action)
        twin.step(action)
        terminal = _model_scan(twin)                          # of the state the robots that just finished ended in
        terminal_path = twin.obs.clone()
        twin._episode.accumulate(twin.episode_state.data_ptr(), twin.reward.data_ptr(), twin.done.data_ptr())
        twin.reset_on_device(twin.done)
        twin.ctl.reset_masked(twin.reset_mask)
        assert torch.equal(env.sim.state, twin.sim.state), k
        assert torch.equal(obs[:, :16], twin.obs) and torch.equal(reward, twin.reward) and torch.equal(done, twin.done), k
        assert torch.equal(env.reset_mask, twin.reset_mask), k
        assert torch.equal(obs[:, 16:], _model_scan(env)), k  # of the reset state, for the robots that were reset
        r = env.reset_mask != 0
        resets += int(r.sum())
        assert torch.equal(env.final_obs[r, 16:], terminal[r]) and torch.equal(env.final_obs[r, :16], terminal_path[r]), k
        assert torch.equal(env.final_obs[~r], final_before[~r]), k
        if bool(r.any()):
            assert not torch.equal(env.final_obs[r, 16:], obs[r, 16:]), k
    assert resets >= B and bool(torch.isfinite(env.obs).all())
    env.close()
    twin.close()


def test_a_cloned_robot_scans_its_sources_ground(dev):
    """B = 24, the smallest batch with dst = src + 16: the controller's continuation is bit-identical only for the same index
    modulo 16 (robot_gym_amd.sim.clone)."""
    from robot_gym_amd.sim.height_scan import HeightScan
    B = 24
    env = _env(dev, B, HeightScan(), auto_reset=True)
    env.reset()
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    for _ in range(3):
        env.step(action)
    src = np.arange(4)
    dst = src + 16
    assert not torch.equal(env.obs[src, 16:], env.obs[dst, 16:])
    env.clone(src, dst)
    assert torch.equal(env.obs[src], env.obs[dst])
    for k in range(10):                                       # across the reset on tick 8
        obs, _, _ = env.step(action)
        assert torch.equal(obs[src], obs[dst]) and torch.equal(env.final_obs[src], env.final_obs[dst]), k
        assert torch.equal(obs[:, 16:], _model_scan(env)), k  # the model reads the keys the clone copied
    env.close()


# ---- 6. the collector ------------------------------------------------------------------------------------------------------------

def test_collect_takes_the_wider_observation_as_it_is(dev):
    from robot_gym_amd.agents.ppo.policy import BatchedGaussianPolicy
    from robot_gym_amd.agents.ppo.rollout import RolloutBuffer, collect
    from robot_gym_amd.sim.height_scan import HeightScan
    B, T = 8, 4
    env, twin = _env(dev, B, HeightScan(), auto_reset=True), _env(dev, B, HeightScan(), auto_reset=True)
    policy = BatchedGaussianPolicy(B, obs_dim=env.obs.shape[1], device=dev)
    assert policy.obs_dim == 64
    ro = RolloutBuffer(T, B, obs_dim=64, device=dev)
    env.reset()
    twin.reset()
    collect(env, policy, ro)
    for name in ("obs", "action", "mean", "value", "logprob", "reward", "ret", "adv", "last_value"):
        assert bool(torch.isfinite(getattr(ro, name)).all()), name
    for t in range(T):                                         # the twin replays the actions: its scan at tick t is the rollout's
        assert torch.equal(ro.obs[t, 16:], twin._obs_cm[16:]) and torch.equal(ro.obs[t, :16], twin._obs_cm[:16]), t
        assert torch.equal(ro.obs[t, 16:], _model_scan(twin).t()), t
        twin.step(ro.action[t])
    assert torch.equal(env.obs, twin.obs)
    env.close()
    twin.close()
