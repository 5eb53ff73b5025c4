"""The go-to-target task's kernels where tests/test_goto_gpu.py does not go (inputs: tests/goto_edges.py; the model alone over
the same inputs: tests/test_goto_edges_cpu.py): dense paths that fill both register slots of the chain loop and overflow
max_visible; paths whose points repeat, so that the chain's arg-min ties exactly and the resampling meets links of length
zero; an exact tie between two different points; the limits of the configuration's shapes; batches that are no multiple of
anything, and rg_goto_set_path with an index list.

The comparison is that of test_kernels_against_the_model with its figures (OBS_ABS, REWARD_REL, MARGIN, MAX_LEFT_OUT).
Left-out shares, measured with the model alone: dense paths 0 of 15360 robot-ticks (of the 14106 live ones 84.0 % have a
chain above 64 points, the longest 128; 2233 see fewer than 64 points, 711 more than 128 -- up to 143 -- with the overflow
flag set); shape limits 0 %; repeated points 0 % of 2560 robot-ticks under the rule built on margin_frame_ties_ok (under
margin_frame 1716 of them would be left out: every tick with a copy in view); odd batches 0 of 8, 504, 520 and 2056; the
exact tie between different points compares every robot-tick (goto_edges.mirror_case says why it may).

Every test prints its largest deviations (pytest -s).
"""
import numpy as np
import pytest
import torch

from robot_gym_amd.core import goto_abi
from robot_gym_amd.gym import goto_path
from tests import goto_edges as E
from tests import goto_fixtures as F
from tests import goto_model as M
from tests.test_goto_gpu import MARGIN, MAX_LEFT_OUT, OBS_ABS, REWARD_REL, STATE_FIGURES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models():
    """Every case's inputs and its model run, made BEFORE a test of this module opens the GPU: `dev` depends on this fixture."""
    out = {"dense": E.dense_case(), "ties": E.ties_case(), "mirror": E.mirror_case()}
    out.update({name: E.shape_case(name) for name in E.SHAPES})
    out = {k: (c, paths, poses, F.run_model(c, paths, poses)) for k, (c, paths, poses) in out.items()}
    out.update({("odd", B): E.odd_model(B) for B in E.ODD_BATCHES})
    return out


@pytest.fixture(scope="module")
def dev(models):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def run(raw, poses):
    """observe on poses[0], post_step on the rest -> (reset observation, dict of per-tick [T, B] figures and obs [T, 2 ncp, B])."""
    T, B = len(poses) - 1, raw.batch
    raw.pose(poses[0])
    raw.observe()
    obs0 = raw.obs.cpu().numpy()
    got = {k: np.zeros((T, B)) for k in list(STATE_FIGURES) + ["done", "reward"]}
    got["obs"] = np.zeros((T, 2 * raw.ncp, B), dtype=np.float32)
    for t in range(T):
        raw.pose(poses[t + 1])
        raw.post()
        st = raw.state.cpu().numpy()
        for k, row in STATE_FIGURES.items():
            got[k][t] = st[row]
        got["done"][t], got["reward"][t], got["obs"][t] = raw.done.cpu().numpy(), raw.reward.cpu().numpy(), raw.obs.cpu().numpy()
        assert np.isfinite(st).all() and np.isfinite(got["obs"][t]).all() and np.isfinite(got["reward"][t]).all(), t
    assert raw.guards_intact()
    return obs0, got


def compare(label, obs0, got, model, out_tick, out_obs, first):
    """test_kernels_against_the_model's comparison; out_tick / out_obs: what may be left out, first: the robots whose reset
    observation is compared.  -> the live compared mask."""
    keep, keep_obs = ~out_tick, ~out_obs
    live = (model["frozen"] == 0) & keep
    print(f"{label}: left out {out_tick.mean():.4%} of {out_tick.size} robot-ticks, {out_obs.mean():.4%} of their observations; live and compared {live.sum()}")
    assert out_tick.mean() <= out_obs.mean() <= MAX_LEFT_OUT
    if first.any():
        err0 = np.abs(obs0.T[first] - model["obs0"].T[first]).max()
        print(f"{label}: reset observation max error {err0:.3g} m")
        assert err0 <= OBS_ABS
    for k in ("visible", "chain", "latched", "next_cp", "done", "reason", "overflow"):
        bad = (got[k] != model[k]) & keep
        assert not bad.any(), (label, k, np.argwhere(bad)[:5].tolist())
    want = model["reward"].astype(np.float32).astype(np.float64)
    rel = np.abs(got["reward"] - want) / np.maximum(np.abs(want), 1e-30)
    rel[want == got["reward"]] = 0.0
    err = np.abs(got["obs"].astype(np.float64) - model["obs"]).max(axis=1)
    print(f"{label}: reward max relative error {rel[keep].max():.3g}, observation max error {err[keep_obs].max():.3g} m")
    assert rel[keep].max() <= REWARD_REL
    assert err[keep_obs].max() <= OBS_ABS
    return live


def test_dense_paths_fill_both_register_slots(models, dev):
    """256 robots, 60 ticks on smooth curves resampled at 2 mm, every fourth robot's at 1.3 mm (n_max = 2048, max_visible =
    128): most chains are longer than 64 points, so visible points `lane + 64` -- the second register slot of the chain
    loop, its `free1` flag and its half of the arg-min -- carry most links; some robots see fewer than 64 points (slot 1
    empty) and some more than 128 (the rank cut in the scan's third chunk, both slots full, the overflow flag stored) in the
    same launch."""
    c, paths, poses, model = models["dense"]
    raw = F.RawTask(paths, dev, **E.DENSE["task"])
    obs0, got = run(raw, poses)
    out_tick, out_obs = F.excluded(model, MARGIN)
    live = compare("dense paths", obs0, got, model, out_tick, out_obs, model["margin0"] >= MARGIN)
    share = (model["chain"][live] > 64).mean()
    over = live & (model["visible"] > 128)
    print(f"dense paths: {share:.1%} of live compared robot-ticks have a chain above 64, {(model['visible'][live] < 64).sum()} see fewer than 64 points, "
          f"{over.sum()} more than 128 (the most {model['visible'][live].max():.0f}), longest chain {model['chain'][live].max():.0f}")
    assert share >= 0.30 and (model["visible"][live] < 64).sum() > 0 and live.sum() > 0.2 * live.size
    assert over.sum() >= 100 and (model["overflow"][over] == 1).all() and (got["overflow"][over] == 1).all()
    assert (got["chain"][over] == 128).sum() > 0                  # a chain that uses every kept point
    assert (model["latched"][live] == 0).sum() > 0


def test_repeated_points_tie_exactly(models, dev):
    """64 robots, 40 ticks on paths with every 2nd or every 5th point doubled, or a stretch tripled.  The copies tie exactly in
    the chain's arg-min and make links of length zero (cs[k + 1] == cs[k] in the resampling).  The ticks with such a tie ARE
    compared: the exclusion rule is built on margin_frame_ties_ok.  Everything is finite (run)."""
    c, paths, poses, model = models["ties"]
    raw = F.RawTask(paths, dev)
    obs0, got = run(raw, poses)
    out_tick, out_obs = F.excluded(model, MARGIN, ties_ok=True)
    live = compare("repeated points", obs0, got, model, out_tick, out_obs, model["margin0_ties_ok"] >= MARGIN)
    tie_ticks = live & (model["zero_links"] > 0)
    print(f"repeated points: {tie_ticks.sum()} compared robot-ticks whose chain holds a link of length zero, {(live & (model['margin_frame'] == 0)).sum()} with an exact tie")
    assert tie_ticks.sum() >= 100 and (live & (model["margin_frame"] == 0)).sum() >= 100
    assert (model["latched"][live] == 1).sum() > 1000


def test_exact_tie_between_different_points_goes_to_the_lower_index(models, dev):
    """goto_edges.mirror_case: points k and 79 - k of a path across the view are at bitwise equal distances, yaw is exactly 0.
    The chain must start at the lower index, y = -0.005, and run down that side.  No robot-tick is left out."""
    c, paths, poses, model = models["mirror"]
    assert (model["margin_frame"] == 0).all() and (model["frozen"] == 0).all()        # the tie is met, on the one live tick
    raw = F.RawTask(paths, dev)
    obs0, got = run(raw, poses)
    nothing = np.zeros_like(model["frozen"], dtype=bool)
    compare("exact tie", obs0, got, model, nothing, nothing, np.ones(len(paths), dtype=bool))
    assert (got["obs"][0, 1] < 0).all() and (obs0[1] < 0).all()                       # the first chain point: y = -0.005
    assert (2 * got["chain"] == got["visible"]).all()


@pytest.mark.parametrize("name", list(E.SHAPES))
def test_shape_limits(name, models, dev):
    """64 robots, 20 ticks with one group of settings off its default: 16 camera points (the most), 1 camera point, n_max = 100
    with paths of 2, 63, 64, 65, 99 and 100 points (one short of, at, and one past a 64-point chunk of the scan), max_visible =
    2 (the least), one checkpoint.  The unused tail of every path slab is NaN when set_path copies it: were a point past
    npts read, the finite checks of `run` or the comparison would show it."""
    c, paths, poses, model = models[name]
    task = E.SHAPES[name]
    raw = F.RawTask(paths, dev, packed=E.poisoned_pack(paths, c["n_max"]), **task)
    assert raw.ncp == c["num_cam_pts"] and bool(torch.isnan(raw.px).any())
    obs0, got = run(raw, poses)
    out_tick, out_obs = F.excluded(model, MARGIN)
    live = compare(name, obs0, got, model, out_tick, out_obs, model["margin0"] >= MARGIN)
    assert live.sum() > 0.2 * live.size
    if name == "n_max_100":
        npts = np.array([p.n for p in paths])
        assert set(npts.tolist()) == set(E.SHAPE_NPTS)
        assert (model["frozen"][0, npts == 2] == 0).all()          # a two-point path is a path: its robot runs
    if name == "two_visible":
        assert model["overflow"][-1].sum() > 32 and model["chain"].max() == 2
    if name == "one_checkpoint":
        assert (model["next_cp"] <= 1).all()


@pytest.mark.parametrize("B", E.ODD_BATCHES)
def test_odd_batches_and_partial_set_path(B, models, dev):
    """observe, pre_step and post_step against the model for 5 ticks on 1, 63, 65 and 257 robots, the guard rows intact; then
    set_path for robots B-1, 0 and one in between (in that order): their task state is new_state(), their header and slabs
    are the new paths, everybody else's state column, header column and slabs are bit for bit what they were; one more tick
    matches the model for all robots.  The model's run is goto_edges.odd_model, recorded before the GPU is opened; what the
    margin rule leaves out of it is tests/test_goto_edges_cpu.py's to bound (nothing, for these seeds)."""
    m = models["odd", B]
    c, paths, idx, new, poses = m["c"], m["paths"], m["idx"], m["new"], m["poses"]
    raw = F.RawTask(paths, dev)
    rows = [goto_abi.ROW_VISIBLE, goto_abi.ROW_CHAIN, goto_abi.ROW_LATCHED, goto_abi.ROW_NEXT_CP, goto_abi.ROW_DONE, goto_abi.ROW_REASON]
    worst = dict(obs=0.0, reward=0.0)
    assert m["out_tick"].mean() <= m["out_obs"].mean() <= MAX_LEFT_OUT

    def tick(t):
        observe_only = t in E.ODD_OBSERVE
        keep, keep_obs = ~m["out_tick"][t], ~m["out_obs"][t]
        raw.pose(poses[t])
        if observe_only:
            raw.observe()
        else:
            raw.action.copy_(torch.as_tensor(m["actions"][t]))
            raw.pre()
            sure = ~m["out_tick"][:t].any(axis=0)          # pre_step reads the done flag, which a doubtful tick may have set
            assert np.array_equal(raw.cmd.cpu().numpy()[:, sure], m["cmd"][t][:, sure]), t
            raw.post()
        assert raw.guards_intact()
        st, obs = raw.state.cpu().numpy(), raw.obs.cpu().numpy()
        assert np.isfinite(st).all() and np.isfinite(obs).all()
        bad = (st[rows] != m["state"][t][rows]) & keep
        assert not bad.any(), (t, np.argwhere(bad)[:5].tolist())
        if keep_obs.any():
            worst["obs"] = max(worst["obs"], np.abs(obs.astype(np.float64) - m["obs"][t])[:, keep_obs].max())
        if not observe_only:
            got, want = raw.reward.cpu().numpy().astype(np.float64), m["reward"][t].astype(np.float32).astype(np.float64)
            rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
            rel[got == want] = 0.0
            worst["reward"] = max(worst["reward"], rel[keep].max() if keep.any() else 0.0)
            assert np.array_equal(raw.done.cpu().numpy()[keep], m["done"][t][keep]), t

    for t in range(6):
        tick(t)
    before = {k: getattr(raw, k).clone() for k in ("state", "hdr", "px", "py", "ps", "pf")}
    raw.set_path(idx, new)
    assert raw.guards_intact()
    others = torch.as_tensor(np.setdiff1d(np.arange(B), idx), device=dev, dtype=torch.int64)
    for k in ("state", "hdr"):
        assert torch.equal(getattr(raw, k)[:, others], before[k][:, others]), k
    for k in ("px", "py", "ps", "pf"):
        assert torch.equal(getattr(raw, k)[others], before[k][others]), k
    packed = goto_path.pack_paths(new, raw.handle.n_max)
    i_t = torch.as_tensor(idx, device=dev, dtype=torch.int64)
    assert np.array_equal(raw.state[:, i_t].cpu().numpy(), np.stack([M.new_state()] * len(idx), axis=-1))
    hdr = raw.hdr[:, i_t].cpu().numpy()
    assert np.array_equal(hdr[0], packed["npts"]) and np.array_equal(hdr[1], packed["length"]) and np.array_equal(hdr[2:4], packed["target"])
    for k, name in (("px", "x"), ("py", "y"), ("ps", "s"), ("pf", "first_same_x")):
        assert np.array_equal(getattr(raw, k)[i_t].cpu().numpy(), packed[name]), k
    tick(6)
    tick(7)
    print(f"odd batch {B}: observation max error {worst['obs']:.3g} m, reward max relative error {worst['reward']:.3g}")
    assert worst["obs"] <= OBS_ABS and worst["reward"] <= REWARD_REL
