"""The episode reset on the device (include/rg_episode.h) off its defaults and at its edges, on the GPU, over the cases of
tests/episode_edges.py (its docstring says what a case keeps): every planner field of rg_episode_config, the grid's edge, a
descent with no finite neighbour, the way-point limit met and passed, the oscillation ring at lengths 1, 2, 3 and 8, sixteen
obstacles, path lengths around the 64-lane chunks, every failure status beside successes in one call with the failed robots'
data left alone, the target stream at keys that are drawn again and at keys and an episode number beyond 32 bits, the host
reset against the device reset under off-default episode_settings, mask values other than 1, and rg_episode_accumulate on
its own at ragged batches with robots that stay frozen.  Counts are printed before they are asserted.

What is bit-exact and what is not is as in tests/test_episode_gpu.py: a flagged target (a stop test within FLAG_REL of its
threshold) may take the plan of either outcome."""
import collections

import numpy as np
import pytest
import torch

from robot_gym_amd.core import episode_abi, goto_abi, srb_abi
from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.gym import goto_path
from tests import episode_edges as EE
from tests import episode_model as EM
from tests import srb_streams
from tests.test_episode_gpu import OBS_ABS

pytestmark = pytest.mark.gpu

SENTINEL, INT_SENTINEL = -7.25, -7
GUARD = 64
EPISODE0, REASON0, STATUS0 = 5.0, 3.0, 9.0     # what the episode rows and the task's done_reason hold before the call


@pytest.fixture(scope="module")
def planned():
    """Every case planned by the model in worker processes BEFORE this module opens the GPU (`dev` depends on this fixture)."""
    return dict(cases=EE.cases(), host_device=EE.host_device_targets())


@pytest.fixture(scope="module")
def dev(planned):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _env(dev, batch, **kw):
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    return BatchedGoEnv(batch, device=dev, **kw)


def _ones(env):
    return torch.ones(env.batch, dtype=torch.int32, device=env.device)


def _snapshot(env):
    out = dict(sim=env.sim.state.cpu().numpy(), task=env.task_state.cpu().numpy(), obs=env._obs_cm.cpu().numpy(), hdr=env.path_hdr.cpu().numpy(),
               x=env.path_x.cpu().numpy(), y=env.path_y.cpu().numpy(), s=env.path_s.cpu().numpy(), fsx=env.path_first_same_x.cpu().numpy(),
               ep=env.episode_state.cpu().numpy(), rm=env.reset_mask.cpu().numpy(), final=env._final_obs_cm.cpu().numpy())
    out["sim_obs"] = {k: v.cpu().numpy() for k, v in env.sim.obs.items()}
    return out


_RUNS = {}


def _run(dev, c):
    """One reset_on_device of a configuration over all of its targets (B = their number), from a state in which a write
    shows: the whole path slab and every column of the robots the model fails hold a sentinel, the episode rows hold values
    that a latch moves.  (before, after), made once per configuration and shared by the tests below."""
    if c["name"] in _RUNS:
        return _RUNS[c["name"]]
    B = len(c["plans"])
    assert B % 2 == 1 and B <= 400
    env = _env(dev, B, obstacles=c["obstacles"] or None, seed=EE.SEED, episode_settings=c["settings"], **c["task"])
    assert env.n_max == c["n_max"]
    rng = np.random.default_rng(40)
    failed = torch.as_tensor(np.flatnonzero([p["status"] != EM.PLAN_OK for p in c["plans"]]), device=dev)
    for t in (env.path_x, env.path_y, env.path_s, env.path_hdr):
        t.fill_(SENTINEL)
    env.path_first_same_x.fill_(INT_SENTINEL)
    env._final_obs_cm.fill_(SENTINEL)
    env._obs_cm.copy_(torch.as_tensor(rng.uniform(-0.2, 0.3, tuple(env._obs_cm.shape)).astype(np.float32)))
    env.task_state[goto_abi.ROW_REASON] = REASON0
    for t in [env.sim.state, env.task_state] + list(env.sim.obs.values()):
        t[..., failed] = SENTINEL
    ep = np.zeros((EM.ROWS, B))
    ep[EM.ROW_EPISODE], ep[EM.ROW_PLAN_STATUS], ep[EM.ROW_ENDED], ep[EM.ROW_KEY] = EPISODE0, STATUS0, 1.0, np.arange(B)
    ep[EM.ROW_RETURN], ep[EM.ROW_LENGTH] = rng.normal(0.0, 5.0, B), rng.integers(1, 200, B)
    ep[[EM.ROW_LAST_RETURN, EM.ROW_LAST_LENGTH, EM.ROW_LAST_REASON, EM.ROW_NPTS, EM.ROW_NWAY, 11]] = SENTINEL
    env.episode_state.copy_(torch.as_tensor(ep))
    before = _snapshot(env)
    env.reset_on_device(_ones(env), torch.as_tensor(c["targets"], device=dev))
    after = _snapshot(env)
    env.close()
    _RUNS[c["name"]] = (before, after)
    return before, after


def _outcome(c, after, b):
    """(index of the model's variant robot b took or None, its variants)."""
    variants = c["plans"][b]["variants"]
    status = after["ep"][EM.ROW_PLAN_STATUS, b]
    row = (after["hdr"][0, b], after["hdr"][1, b], after["hdr"][2:, b], after["x"][b], after["y"][b], after["s"][b], after["fsx"][b])
    for k, (vs, path, nway) in enumerate(variants):
        if vs != status:
            continue
        if vs != EM.PLAN_OK or (EM.path_equal(path, *row) and after["ep"][EM.ROW_NWAY, b] == nway and after["ep"][EM.ROW_NPTS, b] == path.n):
            return k, variants
    return None, variants


# ---- 1. plans, statuses and what a failure leaves alone, per configuration ---------------------------------------------

@pytest.mark.parametrize("name", list(EE.CONFIGS))
def test_path_slab_header_npts_and_nway_are_the_models(name, planned, dev):
    c = planned["cases"][name]
    before, after = _run(dev, c)
    exact = flagged = other = 0
    wrong = []
    took = collections.Counter()
    for b, p in enumerate(c["plans"]):
        k, variants = _outcome(c, after, b)
        if k is None or (k > 0 and not p["flagged"]):
            wrong.append((b, p["target"], p["flagged"], p["status"], float(after["ep"][EM.ROW_PLAN_STATUS, b]), float(after["hdr"][0, b]),
                          p["path"].n if p["path"] else None))
            continue
        exact += not p["flagged"]
        flagged += p["flagged"]
        other += k > 0
        if p["flagged"]:
            took["numpy's" if k == 0 else "the other"] += 1
    print(f"{name}: B = {len(c['plans'])}, {exact} unflagged and bit-exact, {flagged} flagged and equal to one outcome of the stop test "
          f"({dict(took)}), {other} of them took the other outcome than numpy's, {len(wrong)} wrong")
    assert not wrong, wrong[:8]


@pytest.mark.parametrize("name", list(EE.CONFIGS))
def test_failure_status_per_robot_and_the_latch_of_the_others(name, planned, dev):
    c = planned["cases"][name]
    before, after = _run(dev, c)
    ep0, ep, rm = before["ep"], after["ep"], after["rm"]
    counts = collections.Counter()
    for b, p in enumerate(c["plans"]):
        status = int(ep[EM.ROW_PLAN_STATUS, b])
        counts[episode_abi.PLAN_STATUS[status] if 0 <= status < len(episode_abi.PLAN_STATUS) else status] += 1
        allowed = {v[0] for v in p["variants"]} if p["flagged"] else {p["status"]}
        assert status in allowed, (b, p["target"], status, allowed)
        if status != EM.PLAN_OK:
            assert rm[b] == 0 and ep[EM.ROW_EPISODE, b] == EPISODE0, b
            want = ep0[:, b].copy()
            want[EM.ROW_PLAN_STATUS] = status
            assert np.array_equal(ep[:, b], want), (b, ep[:, b], want)
        else:
            assert rm[b] == 1, b
            want = EM.latch(ep0[:, b], REASON0, after["hdr"][0, b], ep[EM.ROW_NWAY, b])
            assert np.array_equal(ep[:, b], want), (b, ep[:, b], want)
    print(f"{name}: device statuses {dict(counts)}")
    model = collections.Counter(episode_abi.PLAN_STATUS[p["status"]] for p in c["plans"])
    if not any(p["flagged"] for p in c["plans"]):
        assert counts == model
    assert np.array_equal(after["final"], before["obs"])          # every masked robot, whatever its plan


@pytest.mark.parametrize("name", list(EE.CONFIGS))
def test_a_failed_robot_keeps_its_data_and_neighbours_stay_in_their_rows(name, planned, dev):
    c = planned["cases"][name]
    before, after = _run(dev, c)
    failed = np.flatnonzero(after["rm"] == 0)
    done = np.flatnonzero(after["rm"] == 1)
    assert len(failed) + len(done) == len(c["plans"])
    assert len(failed) == sum(int(after["ep"][EM.ROW_PLAN_STATUS, b]) != EM.PLAN_OK for b in range(len(c["plans"])))
    for key in ("sim", "task", "obs", "hdr"):
        assert np.array_equal(after[key][:, failed], before[key][:, failed]), key
    for key in ("x", "y", "s", "fsx"):
        assert np.array_equal(after[key][failed], before[key][failed]), key
    for key, v in after["sim_obs"].items():
        assert np.array_equal(v[..., failed], before["sim_obs"][key][..., failed]), key
    rows = [r for r in range(EM.ROWS) if r != EM.ROW_PLAN_STATUS]
    assert np.array_equal(after["ep"][rows][:, failed], before["ep"][rows][:, failed])
    modelled = [b for b in failed if c["plans"][b]["status"] != EM.PLAN_OK]
    if modelled:                                                   # those held the sentinel everywhere
        assert (after["sim"][:, modelled] == SENTINEL).all() and (after["task"][:, modelled] == SENTINEL).all()
        assert (after["x"][modelled] == SENTINEL).all() and (after["fsx"][modelled] == INT_SENTINEL).all()
    # a robot that was reset wrote its own npts points and nothing past them
    for b in done:
        n = int(after["hdr"][0, b])
        assert 2 <= n <= c["n_max"]
        for key in ("x", "y", "s"):
            assert (after[key][b, n:] == SENTINEL).all() and not (after[key][b, :n] == SENTINEL).any(), (key, b, n)
        assert (after["fsx"][b, n:] == INT_SENTINEL).all() and (after["fsx"][b, :n] >= 0).all(), (b, n)
        assert after["task"][goto_abi.ROW_DONE, b] == 0 and after["sim"][srb_abi.ROW_STEPS, b] == 0
    print(f"{name}: {len(failed)} robots not reset and untouched, {len(done)} reset, longest path {int(after['hdr'][0, done].max()) if len(done) else 0} "
          f"of n_max = {c['n_max']}")


# ---- 2. the target stream ---------------------------------------------------------------------------------------------

def test_stream_redraws_wide_keys_a_wide_episode_and_nonfinite_targets(dev):
    B = len(EE.STREAM)
    env = _env(dev, B, seed=EE.SEED)
    keys, episodes = [k for k, _, _ in EE.STREAM], [e for _, e, _ in EE.STREAM]
    env.episode_state[EM.ROW_KEY] = torch.tensor(keys, dtype=torch.float64, device=dev)
    env.episode_state[EM.ROW_EPISODE] = torch.tensor(episodes, dtype=torch.float64, device=dev)
    assert env.episode_state[EM.ROW_KEY].cpu().numpy().astype(np.int64).tolist() == keys
    given = torch.tensor([g for _, _, g in EE.STREAM], dtype=torch.float64, device=dev)
    env.path_hdr.fill_(SENTINEL)
    env.reset_on_device(_ones(env), given)
    hdr, ep, rm = env.path_hdr.cpu().numpy(), env.episode_state.cpu().numpy(), env.reset_mask.cpu().numpy()
    want = EE.stream_expectation()
    for b, (target, status) in enumerate(want):
        print(f"key {keys[b]} episode {episodes[b]} given {EE.STREAM[b][2]}: model {target} status {status}, device {tuple(hdr[2:, b])} "
              f"status {int(ep[EM.ROW_PLAN_STATUS, b])}")
    for b, (target, status) in enumerate(want):
        assert ep[EM.ROW_PLAN_STATUS, b] == status, b
        if status == EM.PLAN_OK:
            assert tuple(hdr[2:, b]) == target and rm[b] == 1 and ep[EM.ROW_EPISODE, b] == episodes[b] + 1, b
        else:
            assert status == EM.PLAN_TARGET and rm[b] == 0 and ep[EM.ROW_EPISODE, b] == episodes[b] and (hdr[:, b] == SENTINEL).all(), b
    assert np.array_equal(ep[EM.ROW_KEY], np.array(keys, dtype=np.float64))      # nothing writes the key
    for b, key in enumerate(keys):
        if key in EE.REDRAWN and episodes[b] == 0:
            assert tuple(hdr[2:, b]) == EE.REDRAWN[key]
    # no target tensor at all: every robot draws, at the episode its row now holds
    now = ep[EM.ROW_EPISODE].astype(np.int64).tolist()
    env.reset_on_device(_ones(env))
    hdr2, ep2 = env.path_hdr.cpu().numpy(), env.episode_state.cpu().numpy()
    for b in range(B):
        assert tuple(hdr2[2:, b]) == EM.draw_target(EE.SEED, keys[b], now[b]) and ep2[EM.ROW_PLAN_STATUS, b] == 0 and ep2[EM.ROW_EPISODE, b] == now[b] + 1, b
    env.close()


# ---- 3. the host reset plans as the device reset does -----------------------------------------------------------------

def _everything(env):
    out = _snapshot(env)
    out["ctl"] = env.ctl.save_state().rows.copy()
    return out


@pytest.mark.parametrize("name", list(EE.HOST_DEVICE))
def test_host_reset_equals_device_reset_off_the_defaults(name, planned, dev):
    robot, settings, obstacles, sim_settings, task = EE.HOST_DEVICE[name]
    targets = planned["host_device"][name]
    B = len(targets)
    cfg = None if robot is None else MPCConfig.for_robot(robot)
    make = lambda: _env(dev, B, cfg=cfg, obstacles=obstacles, episode_settings=settings, sim_settings=sim_settings, **task)
    host, device = make(), make()
    host.reset(targets=targets)
    device.reset_on_device(_ones(device), torch.as_tensor(targets, device=dev))
    device.ctl.reset_masked(device.reset_mask)
    want, got = _everything(host), _everything(device)
    assert (got["rm"] == 1).all() and (got["ep"][EM.ROW_PLAN_STATUS] == 0).all()
    assert np.array_equal(got["hdr"], want["hdr"])
    default_n = [EM.plan_build(t, obstacles).n for t in targets[:8]]
    assert [int(v) for v in got["hdr"][0, :8]] != default_n           # not the plan of the defaults
    for b in range(B):
        n = int(want["hdr"][0, b])
        assert n == host.paths[b].n
        for key in ("x", "y", "s", "fsx"):
            assert np.array_equal(got[key][b, :n], want[key][b, :n]), (key, b)
    assert np.array_equal(got["ctl"], want["ctl"])
    cmp = srb_streams.Comparison()
    cmp.check(got["sim"], got["sim_obs"], want["sim"], want["sim_obs"])
    err = np.abs(got["obs"].astype(np.float64) - want["obs"]).max()
    terr = np.abs(got["task"] - want["task"]).max()
    print(f"{name}: simulator {cmp.worst} {cmp.bad}, observation max error {err:.3g} m, task state max error {terr:.3g}, "
          f"path points {int(got['hdr'][0].min())}..{int(got['hdr'][0].max())}")
    assert cmp.clean(), (cmp.bad, cmp.worst)
    assert err <= OBS_ABS and terr <= OBS_ABS
    assert got["obs"].shape[0] == 2 * task.get("num_cam_pts", 8) and np.abs(got["obs"]).max() > 0
    for e in (host, device):
        e.close()


def test_host_reset_passes_its_settings_on_and_refuses_what_the_device_refuses(dev, monkeypatch):
    settings = dict(kp=7.0, eta=50.0, area_width=3.0, grid=0.4, robot_radius=0.3, spacing=0.015, oscillation_length=4, max_waypoints=7)
    env = _env(dev, 3, obstacles=EE.OBSTACLES, episode_settings=settings, n_max=200)
    seen = []
    plan, build = goto_path.plan_path, goto_path.build_path
    monkeypatch.setattr(goto_path, "plan_path", lambda *a, **kw: (seen.append(("plan", a, kw)), plan(*a, **kw))[1])
    monkeypatch.setattr(goto_path, "build_path", lambda *a, **kw: (seen.append(("build", a, kw)), build(*a, **kw))[1])
    env.reset(targets=[(1.0, 1.0), (-1.0, 2.0), (1.0, 1.0)])
    plans, builds = [s for s in seen if s[0] == "plan"], [s for s in seen if s[0] == "build"]
    assert len(plans) == len(builds) == 2                                  # one per distinct target
    for _, a, kw in plans:
        assert kw == {k: v for k, v in settings.items() if k != "spacing"} and a[1] == EE.OBSTACLES
    for _, a, kw in builds:
        assert kw["spacing"] == 0.015 and kw["n_max"] == 200
    before = _snapshot(env)
    for target, text in (((2.5, 2.5), "max_waypoints"), ((0.0, 0.02), "at least 2"), ((2.5, -2.0), "n_max is 200")):
        with pytest.raises(ValueError, match=text):
            env.reset([1], [target])
    after = _snapshot(env)
    for key in ("sim", "task", "obs", "hdr", "x", "y", "s", "fsx", "ep"):
        assert np.array_equal(after[key], before[key]), key
    assert EM.plan_status((2.5, 2.5), EE.OBSTACLES, 200, **settings) == EM.PLAN_WAYPOINTS
    assert EM.plan_status((2.5, -2.0), EE.OBSTACLES, 200, **settings) == EM.PLAN_LONG
    env.close()


# ---- 4. mask values ---------------------------------------------------------------------------------------------------

def test_any_nonzero_mask_value_selects_and_stale_flags_are_cleared(dev):
    values = [-3, 0, 2 ** 31 - 1, 0, 1, 0, -2 ** 31]
    B = len(values)
    env = _env(dev, B)
    env.path_hdr.fill_(SENTINEL)
    env.reset_mask.fill_(1)                                                # stale flags: a robot whose mask is 0 clears its own
    targets = np.array([(1.0 + 0.1 * b, -1.5) for b in range(B)])
    env.reset_on_device(torch.tensor(values, dtype=torch.int32, device=dev), torch.as_tensor(targets, device=dev))
    hdr, ep, rm = env.path_hdr.cpu().numpy(), env.episode_state.cpu().numpy(), env.reset_mask.cpu().numpy()
    sel = np.array(values) != 0
    assert np.array_equal(rm, sel.astype(np.int32)) and np.array_equal(ep[EM.ROW_EPISODE], sel.astype(np.float64))
    assert np.array_equal(hdr[2:, sel].T, targets[sel]) and (hdr[:, ~sel] == SENTINEL).all()
    for b in np.flatnonzero(sel):
        p = EM.plan_build(targets[b])
        assert EM.path_equal(p, hdr[0, b], hdr[1, b], hdr[2:, b], env.path_x[b].cpu().numpy(), env.path_y[b].cpu().numpy(), env.path_s[b].cpu().numpy(),
                             env.path_first_same_x[b].cpu().numpy())
    env.close()


# ---- 5. rg_episode_accumulate on its own ------------------------------------------------------------------------------

@pytest.mark.parametrize("B", EE.ACC_BATCHES)
def test_accumulate_alone_at_ragged_batches_with_frozen_robots(B, dev):
    c = EE.accumulate_case(B)
    env = _env(dev, B)
    n = EM.ROWS * B
    big = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    state = big[GUARD:GUARD + n].view(EM.ROWS, B)
    state.copy_(torch.as_tensor(c["state0"]))
    reward, done = torch.as_tensor(c["reward"], device=dev), torch.as_tensor(c["done"], device=dev)
    wrong = 0
    for t in range(EE.ACC_TICKS):
        env._episode.accumulate(state.data_ptr(), reward[t].data_ptr(), done[t].data_ptr())
        got = state.cpu().numpy()
        wrong += got.tobytes() != c["want"][t].tobytes()
    a = big.cpu().numpy()
    print(f"B = {B}: {wrong} of {EE.ACC_TICKS} ticks differ from the model; {int(c['want'][-1, EM.ROW_ENDED].sum())} robots ended")
    assert wrong == 0
    assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all()
    assert (env.episode_state[EM.ROW_KEY].cpu().numpy() == np.arange(B)).all() and (env.episode_state[:EM.ROW_KEY] == 0).all()   # the environment's own rows: not touched
    env.close()
