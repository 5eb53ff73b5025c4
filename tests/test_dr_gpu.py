"""The domain randomisation on the GPU (include/rg_dr.h, robot_gym_amd/csrc/rg_dr.hip) against tests/dr_model.py BIT FOR
BIT at batches 1 (a single lane), 65 (across a wave) and 257 (across a workgroup): the draw of a reset under masks, the push of
a tick, the identity of the defaults inside BatchedGoEnv, a randomised env replayed into the model tick by tick, the drawn body
in the dynamics, set_body after bind, clone, independence of the position in the batch, and the PPO collector.

Bit-exactness rests on float64 multiplication, addition and division being correctly rounded on the device and on nothing
else: the kernels call no other function."""
import warnings

import numpy as np
import pytest
import torch

from robot_gym_amd.core import dr_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from tests import dr_model as DM
from tests import scan_model as SM
from tests import srb_model as M
from tests import srb_streams as S
from tests import terrain_model as TM

pytestmark = pytest.mark.gpu

BATCHES = (1, 65, 257)
PUSH = dict(push_interval=8, push_ticks=3, push_probability=0.5, push_force_xy=30.0, push_force_z=10.0, push_torque_xy=5.0, push_torque_z=2.0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _bits(t, want):
    """A float64 / int64 device tensor equals the numpy array bit for bit (-0.0 is not 0.0)."""
    got = t.detach().cpu().contiguous().numpy()
    want = np.ascontiguousarray(want, dtype=got.dtype)
    return got.shape == want.shape and np.array_equal(got.view(np.int64), want.view(np.int64))


def _keys(B):
    return (np.arange(B, dtype=np.int64) * 7919 - 1000) % 4001 - 2000      # not the indices; negative ones among them


def _true_bodies(cfg, B, seed):
    """A per-robot base body: mass [B] and inertia [9, B], symmetric positive definite."""
    rng = np.random.default_rng(seed)
    mass = cfg.mass * rng.uniform(0.85, 1.15, B)
    inertia = np.tile(np.asarray(cfg.inertia, dtype=np.float64).reshape(9, 1), (1, B))
    for a in range(3):
        inertia[4 * a] *= rng.uniform(0.8, 1.25, B)
    off = rng.uniform(-0.004, 0.004, B)
    inertia[1] = inertia[3] = off
    return mass, inertia


def _sim(B, dev, robot="ghost", terrain=None, body_seed=None):
    from robot_gym_amd.sim import BatchedSRBSim
    cfg = MPCConfig.for_robot(robot)
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=terrain)
    if body_seed is not None:
        sim.set_body(*_true_bodies(cfg, B, body_seed))
    return cfg, sim


def _model_cfg(dr):
    return DM.settings(**dr._handle.fields)


def _mask(on, dev):
    return torch.as_tensor(np.asarray(on).astype(np.int32), device=dev)


# ---- 1. a reset against the model --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("robot,body_seed", [("ghost", None), ("k3lso", 5)])
@pytest.mark.parametrize("B", BATCHES)
def test_reset_is_the_model_bit_for_bit(dev, B, robot, body_seed):
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain
    keys0 = _keys(B)
    terrain = RandomTerrain(keys=keys0)
    cfg, sim = _sim(B, dev, robot, terrain, body_seed)
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.5, 2.0), new_world_each_episode=True, seed=77).bind(sim)
    base = dr.body().cpu().numpy()
    if body_seed is None:
        assert (base[0] == cfg.mass).all() and (base[1:10] == np.asarray(cfg.inertia).reshape(9, 1)).all()
    else:
        mass, inertia = _true_bodies(cfg, B, body_seed)
        assert (base[0] == mass).all() and (base[1:10] == inertia).all() and len(np.unique(base[0])) == B
    for b in range(min(B, 3)):
        assert np.allclose(base[10:, b].reshape(3, 3) @ base[1:10, b].reshape(3, 3), np.eye(3), atol=1e-12)
    mcfg = _model_cfg(dr)
    assert mcfg["worlds"] == 1 and mcfg["seed"] == 77 and mcfg["substeps"] == sim.substeps
    st, body, keys = DM.new_state(B, world=keys0), base.copy(), keys0.copy()
    assert _bits(dr.state, st) and _bits(terrain.keys, keys) and tuple(dr.scales.shape) == (2, B)
    third = np.arange(B) % 3 == 0
    for on in (third, ~third, np.ones(B, dtype=bool), third):
        before = (dr.state.clone(), dr.body(), terrain.keys.clone())
        mask = _mask(on * np.where(np.arange(B) % 2, -5, 1), dev)                 # any non-zero value
        dr.on_reset(mask)
        DM.reset(mcfg, on, st, base, body, keys)
        got_body = dr.body()
        assert _bits(dr.state, st) and _bits(got_body, body) and _bits(terrain.keys, keys)
        off = torch.as_tensor(~on, device=dev)
        for was, now in zip(before, (dr.state, got_body, terrain.keys)):          # a robot outside the mask is written nowhere
            assert torch.equal(was[..., off], now[..., off])
        si = st[DM.ROW_INERTIA_SCALE]
        assert _bits(got_body[10:], base[10:] / si) and _bits(got_body[1:10], base[1:10] * si) and _bits(got_body[0], base[0] * st[DM.ROW_MASS_SCALE])
        assert _bits(dr.scales, st[2:4])
    assert (st[DM.ROW_DRAWS] == 2 + third).all() and (keys >= 0).all() and (keys < 2 ** 31).all()
    assert (st[DM.ROW_MASS_SCALE] >= 0.8).all() and (st[DM.ROW_MASS_SCALE] <= 1.2).all() and (st[DM.ROW_INERTIA_SCALE] >= 0.5).all()
    assert B == 1 or len(np.unique(st[DM.ROW_MASS_SCALE])) == B
    assert dr.pushes() is None
    dr.close()
    sim.close()


def test_reset_takes_the_key_only_with_worlds_and_capture_body_the_same_batch(dev):
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain
    B = 65
    _, sim = _sim(B, dev, terrain=RandomTerrain())
    _, other = _sim(B + 1, dev)
    dr = DomainRandomizer().bind(sim)
    mask = _mask(np.ones(B), dev)
    with pytest.raises(dr_abi.RgDrError, match="terrain_key must be null"):
        dr._handle.reset(sim._handle, mask.data_ptr(), dr.state.data_ptr(), sim.terrain.keys.data_ptr())
    with pytest.raises(dr_abi.RgDrError, match=f"capture_body: srb has batch {B + 1}, this handle {B}") as e:
        dr._handle.capture_body(other._handle)
    assert e.value.status == -1
    for call in (lambda: dr._handle.reset(other._handle, mask.data_ptr(), dr.state.data_ptr(), None), lambda: dr._handle.apply(other._handle, None, dr.state.data_ptr()),
                 lambda: dr._handle.get_body(other._handle, dr.state.data_ptr())):
        with pytest.raises(dr_abi.RgDrError, match="srb has batch"):
            call()
    with pytest.raises(ValueError, match="on_reset: mask"):
        dr.on_reset(mask.to(torch.int64))
    with pytest.raises(ValueError, match="apply: mask"):
        dr.apply(mask[:-1])
    with pytest.raises(RuntimeError, match="already bound"):
        dr.bind(sim)
    with pytest.raises(ValueError, match="new_world_each_episode"):
        DomainRandomizer(new_world_each_episode=True).bind(other)                # the plane has no worlds
    w = DomainRandomizer(new_world_each_episode=True).bind(sim)
    with pytest.raises(dr_abi.RgDrError, match="null terrain_key"):
        w._handle.reset(sim._handle, mask.data_ptr(), w.state.data_ptr(), None)
    for x in (dr, w, sim, other):
        x.close()


# ---- 2. the push of a tick against the model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("B", BATCHES)
def test_push_is_the_model_bit_for_bit(dev, B):
    from robot_gym_amd.sim import DomainRandomizer
    _, sim = _sim(B, dev)
    dr = DomainRandomizer(seed=31, **PUSH).bind(sim)
    mcfg = _model_cfg(dr)
    st = DM.new_state(B)
    base = dr.body().cpu().numpy()
    on = np.arange(B) % 2 == 0
    dr.on_reset(_mask(on, dev))                                                  # robots with different draw counts
    DM.reset(mcfg, on, st, base, base.copy())
    assert _bits(dr.state, st)
    offset = (np.arange(B) % 10) + 80.0 * (np.arange(B) % 7) + np.where(np.arange(B) % 16 == 9, 2.0 ** 40, 0.0)     # robots at different ticks, far ones among them
    sim_state = np.zeros((srb_abi.STATE_ROWS, B))
    active = 0
    specials = [np.nan, -25.0] if B == 1 else []
    for t in range(40 + len(specials)):
        sim_state[DM.STEPS_ROW] = 10.0 * t + offset                               # non-multiples of substeps among them
        if t >= 40:
            sim_state[DM.STEPS_ROW, 0] = specials[t - 40]
        elif B > 1:
            sim_state[DM.STEPS_ROW, B // 2] = np.nan                              # both take the clamped value, tick 0
            sim_state[DM.STEPS_ROW, B - 1] = -10.0 * t - 1.0
        sim.state.copy_(torch.as_tensor(sim_state, device=dev))
        ext = dr.pushes()
        want = DM.push(mcfg, sim_state, st)
        assert ext is dr.ext and _bits(ext, want), t
        if B > 1:
            assert (want[:, B // 2] == DM.push_one(mcfg, DM.word(st[0, B // 2]), DM.word(st[1, B // 2]), 0.0)).all()
            assert (want[:, B - 1] == DM.push_one(mcfg, DM.word(st[0, B - 1]), DM.word(st[1, B - 1]), 0.0)).all()
        active += int((want != 0).any(0).sum())
    total = (40 + len(specials)) * B
    assert 0 < active < total and (B == 1 or 0.05 * total < active < 0.35 * total)       # 3 of 8 ticks of half the windows
    amp = np.array(DM.amplitudes(mcfg))[:, None]
    assert (np.abs(want) <= amp).all()
    assert _bits(dr.state, st)                                                    # the push writes no state
    dr.close()
    sim.close()


# ---- 3. the defaults change nothing --------------------------------------------------------------------------------------------

def _env(dev, B, randomizer=None, **kw):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    from robot_gym_amd.sim import RandomTerrain
    kw.setdefault("max_time", 0.45)                                               # 45 sub-steps: the time limit ends every episode on tick 5
    return BatchedGoEnv(B, device=dev, terrain=RandomTerrain(), auto_reset=True, seed=3, randomizer=randomizer, **kw)


def _actions(B, T, dev, seed=0, same=False):
    rng = np.random.default_rng(seed)
    a = rng.uniform([0.1, -0.3], [0.4, 0.3], (T, 1 if same else B, 2)).astype(np.float32)
    return torch.as_tensor(np.broadcast_to(a, (T, B, 2)).copy(), device=dev)


def test_the_default_randomizer_is_the_identity_inside_the_env(dev):
    from robot_gym_amd.sim import DomainRandomizer
    B, T = 65, 60
    plain, env = _env(dev, B), _env(dev, B, DomainRandomizer())
    assert plain.randomizer is None and env.randomizer.ext is None
    assert torch.equal(plain.reset(), env.reset()) and torch.equal(plain.sim.state, env.sim.state)
    actions = _actions(B, T, dev)
    for t in range(T):
        a, b = plain.step(actions[t]), env.step(actions[t])
        for x, y in zip(a, b):
            assert torch.equal(x, y), t
        assert torch.equal(plain.sim.state, env.sim.state) and torch.equal(plain.episode_state, env.episode_state), t
        assert torch.equal(plain.reset_mask, env.reset_mask) and torch.equal(plain.final_obs, env.final_obs), t
    assert int(env.episode_count.sum()) >= 5 * B                                  # resets happened
    assert torch.equal(env.randomizer.state[dr_abi.ROW_DRAWS].to(torch.int64), 1 + env.episode_count)
    assert bool((env.randomizer.scales == 1.0).all()) and torch.equal(env.sim.terrain.keys, plain.sim.terrain.keys)
    plain.close()
    env.close()


# ---- 4. a randomised env, replayed into the model --------------------------------------------------------------------------------

def test_env_with_a_randomizer_is_the_model_on_every_tick(dev):
    from robot_gym_amd.sim import DomainRandomizer
    from robot_gym_amd.sim.height_scan import HeightScan
    B, T = 65, 80
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2), new_world_each_episode=True, seed=11, **PUSH)
    env = _env(dev, B, dr, height_scan=HeightScan())
    terrain = env.sim.terrain
    mcfg = _model_cfg(dr)
    base = dr.body().cpu().numpy()
    keys = np.arange(B, dtype=np.int64)
    st, body = DM.new_state(B, world=keys), base.copy()
    assert _bits(dr.state, st) and _bits(terrain.keys, keys)
    env.reset()
    DM.reset(mcfg, np.ones(B), st, base, body, keys)                              # the host reset draws for every robot
    assert _bits(dr.state, st) and _bits(dr.body(), body) and _bits(terrain.keys, keys) and (keys != np.arange(B)).all()

    def model_scan():
        ground = TM.Random(terrain.amplitude, terrain.cell, terrain.seed, keys)
        return SM.scan(env.sim.state.cpu().numpy(), ground, z_offset=env.cfg.body_height)

    assert np.array_equal(env._obs_cm[16:].cpu().numpy(), model_scan())           # the host reset stood the robots in the new world
    actions = _actions(B, T, dev, seed=1)
    resets = pushed = 0
    for t in range(T):
        want_ext = DM.push(mcfg, env.sim.state.cpu().numpy(), st)                 # from the step counts before the tick
        obs, _, _ = env.step(actions[t])
        assert _bits(dr.ext, want_ext), t                                         # what the simulator was handed
        pushed += int((want_ext != 0).any(0).sum())
        mask = env.reset_mask.cpu().numpy()
        old = keys.copy()
        DM.reset(mcfg, mask, st, base, body, keys)
        assert _bits(dr.state, st) and _bits(dr.body(), body) and _bits(terrain.keys, keys), t
        assert torch.equal(dr.state[dr_abi.ROW_DRAWS].to(torch.int64), 1 + env.episode_count), t
        if mask.any():
            on = mask != 0
            resets += int(on.sum())
            assert (keys[on] != old[on]).all()
            assert np.array_equal(obs[:, 16:].t().cpu().numpy(), model_scan()), t     # the first observation is taken in the new world
            steps = env.sim.state[srb_abi.ROW_STEPS].cpu().numpy()
            assert (steps[on] == 0).all()
    assert resets >= 10 * B and 0 < pushed < T * B
    assert bool(torch.isfinite(env.obs).all())
    env.close()


# ---- 5. the drawn body reaches the dynamics --------------------------------------------------------------------------------------

def test_the_drawn_body_is_the_body_the_simulator_integrates(dev):
    from robot_gym_amd.sim import DomainRandomizer
    B, seed = 65, 201
    cfg, sim = _sim(B, dev)
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.7, 1.4), seed=5).bind(sim)
    base = dr.body().cpu().numpy()
    dr.on_reset(_mask(np.ones(B), dev))
    sm, si = dr.scales.cpu().numpy()
    assert len(np.unique(sm)) == B and len(np.unique(si)) == B
    s = S.streams(cfg, B, 1, seed)
    s["mass"] = base[0] * sm                                                      # stream_grf holds the TRUE weight
    s["fall"][:] = False
    xy, yaw, hs = S.start_poses(cfg, B, np.random.default_rng(seed + 1000))
    model, plain = M.SRBModel(B, cfg), M.SRBModel(B, cfg)
    model.set_body(mass=base[0] * sm, inertia=base[1:10] * si)
    for m in (model, plain):
        m.reset(xy=xy, yaw=yaw, height=hs)
    sim.reset(xy=xy, yaw=yaw, height=hs)
    grf = S.stream_grf(model, cfg, s, 0)
    ext = s["ext"][0] * 5.0
    outputs = dict(grf=torch.as_tensor(grf, device=dev), foot_target=torch.as_tensor(s["foot_target"][0], device=dev),
                   desired_state=torch.as_tensor(s["desired"][0], device=dev))
    sim.step(outputs, torch.as_tensor(ext, device=dev))
    for m in (model, plain):
        m.step(grf, s["foot_target"][0], s["desired"][0], ext)
    cmp = S.Comparison()                                                          # the tolerances of test_srb_gpu.py::test_kernel_vs_model
    got = sim.state.cpu().numpy()
    cmp.check(got, {k: v.cpu().numpy() for k, v in sim.obs.items()}, model.state, model.obs)
    assert cmp.clean(), (cmp.bad, cmp.worst)
    # and it is not the base body's motion: the velocities differ from the unscaled model's far above that tolerance
    rows = list(range(M.ROW_V, M.ROW_V + 3)) + list(range(M.ROW_W, M.ROW_W + 3))
    assert (np.abs(got[rows] - plain.state[rows]).max(0) > 1e-6).all()
    dr.close()
    sim.close()


# ---- 6. set_body after bind ----------------------------------------------------------------------------------------------------

def test_set_body_through_the_randomizer_keeps_the_scales_and_a_bare_one_loses_them(dev):
    from robot_gym_amd.sim import DomainRandomizer
    B = 65
    cfg, sim = _sim(B, dev)
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.7, 1.4), seed=9).bind(sim)
    base = dr.body().cpu().numpy()
    dr.on_reset(_mask(np.ones(B), dev))
    sm, si = dr.scales.cpu().numpy()
    mass, inertia = _true_bodies(cfg, B, 3)
    idx = np.arange(0, B, 2)
    dr.set_body(mass=mass[idx], idx=idx)                                          # new base of the even robots, the scales kept
    base1 = base.copy()
    base1[0, idx] = mass[idx]
    st = np.zeros((8, B))
    st[2], st[3] = sm, si
    want = np.empty_like(base)
    DM.apply(None, st, base1, want)
    assert _bits(dr.body(), want) and _bits(dr.body()[0], base1[0] * sm)
    dr.set_body(inertia=inertia)
    base2 = dr.body().cpu().numpy()                                               # I^-1 is the simulator's own inversion: read, not modelled
    assert _bits(dr.body()[1:10], inertia * si) and _bits(dr.body()[0], base1[0] * sm)
    # a bare sim.set_body uploads the simulator's whole mirror: every scale is gone ...
    sim.set_body(mass=mass)
    bare = dr.body().cpu().numpy()
    assert (bare[0] == mass).all() and (bare[1:10] == inertia).all() and not (bare[0] == mass * sm).any()
    # ... apply() alone scales the base captured BEFORE it ...
    dr.apply()
    assert _bits(dr.body()[0], base1[0] * sm) and not _bits(dr.body()[0], mass * sm)
    # ... and after a capture, the new one
    dr._handle.capture_body(sim._handle)
    dr.apply()
    assert _bits(dr.body()[0], mass * sm) and _bits(dr.body()[1:10], inertia * si) and _bits(dr.body()[10:], bare[10:] / si)
    assert np.allclose(base2[10:] * si, bare[10:], rtol=1e-12)
    # a scale that is not finite and positive leaves that robot's body as it was
    dr.state[dr_abi.ROW_MASS_SCALE, 0] = float("nan")
    dr.state[dr_abi.ROW_INERTIA_SCALE, 1 % B] = 0.0
    dr.state[dr_abi.ROW_MASS_SCALE, 2] = 2.0
    before = dr.body()
    dr.apply()
    after = dr.body()
    assert torch.equal(after[:, :2], before[:, :2]) and _bits(after[0, 2:3], mass[2:3] * 2.0) and torch.equal(after[:, 3:], before[:, 3:])
    dr.close()
    sim.close()


# ---- 7. clone ------------------------------------------------------------------------------------------------------------------

def test_a_clone_has_its_sources_body_world_pushes_and_draws(dev):
    """B = 24, the smallest batch with dst = src + 16: the controller's continuation is bit-identical only for the same index
    modulo 16 (robot_gym_amd.sim.clone)."""
    from robot_gym_amd.sim import DomainRandomizer
    B = 24
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2), new_world_each_episode=True, seed=13, **PUSH)
    env = _env(dev, B, dr)
    base = dr.body().cpu().numpy()
    env.reset()
    actions = _actions(B, 33, dev, seed=2, same=True)
    for t in range(3):
        env.step(actions[t])
    src = np.arange(4)
    dst = src + 16
    keys = env.sim.terrain.keys
    assert not bool((dr.scales[:, src] == dr.scales[:, dst]).any()) and not bool((keys[src] == keys[dst]).any())
    env.clone(src, dst)
    assert torch.equal(dr.state[:, src], dr.state[:, dst]) and torch.equal(keys[src], keys[dst])
    body = dr.body()
    assert torch.equal(body[:, src], body[:, dst])
    want = np.empty((19, B))
    DM.apply(None, dr.state.cpu().numpy(), base, want)
    assert _bits(body, want)                                                      # the clone's body is the base times the copied scales
    draws0 = dr.state[dr_abi.ROW_DRAWS, dst].clone()
    pushed = 0
    for t in range(30):                                                           # across the resets on ticks 5, 10, ...
        obs, reward, done = env.step(actions[3 + t])
        assert torch.equal(obs[src], obs[dst]) and torch.equal(reward[src], reward[dst]) and torch.equal(done[src], done[dst]), t
        assert torch.equal(env.sim.state[:, src], env.sim.state[:, dst]) and torch.equal(dr.ext[:, src], dr.ext[:, dst]), t
        assert torch.equal(dr.state[:, src], dr.state[:, dst]) and torch.equal(keys[src], keys[dst]), t
        body = dr.body()
        assert torch.equal(body[:, src], body[:, dst]), t
        pushed += int((dr.ext[:, dst] != 0).any(0).sum())
    assert bool((dr.state[dr_abi.ROW_DRAWS, dst] >= draws0 + 4).all()) and pushed > 0
    env.close()


# ---- 8. a robot's draws do not depend on its place in the batch ----------------------------------------------------------------

def test_the_same_keys_in_a_permuted_batch_give_the_permuted_outputs(dev):
    from robot_gym_amd.sim import DomainRandomizer, RandomTerrain
    B = 65
    perm = np.random.default_rng(4).permutation(B)
    steps = 10.0 * np.arange(B) + 3.0
    out = []
    for order in (np.arange(B), perm):
        _, sim = _sim(B, dev, terrain=RandomTerrain())
        dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.5, 2.0), new_world_each_episode=True, seed=21, **PUSH).bind(sim)
        dr.state[dr_abi.ROW_KEY] = torch.as_tensor(order.astype(np.float64), device=dev)
        for _ in range(2):
            dr.on_reset(_mask(np.ones(B), dev))
        sim.state[srb_abi.ROW_STEPS] = torch.as_tensor(steps[order], device=dev)
        out.append((dr.state.clone(), dr.body(), sim.terrain.keys.clone(), dr.pushes().clone()))
        dr.close()
        sim.close()
    p = torch.as_tensor(perm, device=dev)
    for a, b in zip(*out):
        assert torch.equal(a[..., p], b)
    assert len(torch.unique(out[0][2])) == B and bool((out[0][3] != 0).any())


# ---- 9. the collector ----------------------------------------------------------------------------------------------------------

def test_collect_runs_on_a_randomised_env_with_no_host_read(dev):
    from robot_gym_amd.agents.ppo.policy import BatchedGaussianPolicy
    from robot_gym_amd.agents.ppo.rollout import RolloutBuffer, collect
    from robot_gym_amd.sim import DomainRandomizer
    B, T = 65, 16
    dr = DomainRandomizer(mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2), new_world_each_episode=True, seed=17, **PUSH)
    env = _env(dev, B, dr)
    env.reset()
    pol = BatchedGaussianPolicy(B, seed=7, device=dev)
    ro = RolloutBuffer(T, B, device=dev)
    torch.cuda.synchronize(dev)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            collect(env, pol, ro)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert not [str(w.message) for w in caught if "synchroniz" in str(w.message).lower()]       # the loop issued no host read
    for name in ("obs", "action", "mean", "value", "logprob", "reward", "ret", "adv", "last_value"):
        assert bool(torch.isfinite(getattr(ro, name)).all()), name
    assert bool(torch.isfinite(env.sim.state).all()) and bool(torch.isfinite(dr.body()).all()) and bool(torch.isfinite(dr.ext).all())
    assert int(env.episode_count.sum()) >= 3 * B                                  # resets on ticks 5, 10, 15: the draws ran inside the loop
    assert torch.equal(dr.state[dr_abi.ROW_DRAWS].to(torch.int64), 1 + env.episode_count)
    assert len(torch.unique(dr.scales[0])) == B
    env.close()
    pol.close()
