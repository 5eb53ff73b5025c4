"""Host-side logic that needs no GPU: sharding, the world_size-2 action all-gather over gloo,
synthetic-state generator determinism."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from robot_gym_amd.core.config import MPCConfig
from robot_gym_amd.core.sharding import shard_bounds, all_gather_actions
from robot_gym_amd import synthetic


def test_shard_bounds_partition_the_batch():
    for total, world in ((32768, 8), (4097, 8), (7, 8), (4096, 1), (10, 3)):
        edges = [shard_bounds(total, r, world) for r in range(world)]
        assert edges[0][0] == 0 and edges[-1][1] == total
        assert all(edges[i][1] == edges[i + 1][0] for i in range(world - 1))
        sizes = [hi - lo for lo, hi in edges]
        assert max(sizes) - min(sizes) <= 1
    assert shard_bounds(32768, 3, 8) == (12288, 16384)  # BASELINE config 4: 8 x 4096


def _gather_worker(rank, world, port, tmp):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_bounds(64, rank, world)
    full = torch.arange(64 * 60, dtype=torch.float32).view(64, 60)
    out = all_gather_actions(full[lo:hi].clone())
    ok = torch.equal(out, full)
    # the direct schedule (every rank sends its slab straight to every peer: one hop over the pairwise xGMI links) and uneven
    # shards (61 robots over the ranks: slabs that differ by one row travel padded)
    ok = ok and torch.equal(all_gather_actions(full[lo:hi].clone(), schedule="direct"), full)
    for schedule in ("ring", "direct"):
        l2, h2 = shard_bounds(61, rank, world)
        ok = ok and torch.equal(all_gather_actions(full[l2:h2].clone(), schedule=schedule, total=61), full[:61])
    # max-over-ranks timing reduction used by bench.py
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ok = ok and t.item() == float(world)
    with open(os.path.join(tmp, f"r{rank}"), "w") as f:
        f.write("ok" if ok else "bad")
    dist.destroy_process_group()


def test_all_gather_actions_world_size_2_gloo(tmp_path):
    port = 29500 + (os.getpid() % 2000)
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert [open(tmp_path / f"r{r}").read() for r in range(2)] == ["ok", "ok"]


def _subgroup_worker(rank, world, port, tmp):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from robot_gym_amd.core.sharding import GatherBuffers
    grp = dist.new_group([1, 2])   # group ranks 0, 1 are GLOBAL ranks 1, 2: point-to-point peers must be mapped
    ok = True
    if rank in (1, 2):
        gr = dist.get_rank(grp)
        full = torch.arange(21 * 60, dtype=torch.float32).view(21, 60)
        lo, hi = shard_bounds(21, gr, 2)    # uneven: 11 + 10 robots
        bufs = GatherBuffers(21, 2, 60, torch.float32, "cpu")
        out = torch.empty(21, 60)
        for schedule in ("direct", "ring"):
            for _ in range(2):   # the staging buffers are reused
                got = all_gather_actions(full[lo:hi].clone(), group=grp, out=out, schedule=schedule, total=21, buffers=bufs)
                ok = ok and got is out and torch.equal(got, full)
        ok = ok and torch.equal(all_gather_actions(full[10 * gr:10 * gr + 10].clone(), group=grp, schedule="direct"), full[:20])
    with open(os.path.join(tmp, f"r{rank}"), "w") as f:
        f.write("ok" if ok else "bad")
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_actions_on_a_subgroup_world_size_3_gloo(tmp_path):
    """The direct schedule's point-to-point peers are global ranks: on a process group that is a SUBSET of the ranks the
    group-relative indices must be mapped (they used to be passed as they were: wrong peers, a hang)."""
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_subgroup_worker, args=(3, port, str(tmp_path)), nprocs=3, join=True)
    assert [open(tmp_path / f"r{r}").read() for r in range(3)] == ["ok", "ok", "ok"]


def test_bench_launches_its_own_ranks_dry_run_world_size_2(tmp_path):
    """`python bench.py --gpus 2` without RANK in the environment must start its own ranks (the driver's form for the
    scaling runs): a fresh torch.distributed.run child with two processes.  --dry-launch --full runs the whole protocol on CPU
    over gloo with a stub controller: rendezvous on 127.0.0.1, barriers, MAX-over-ranks timing, both all-gather variants, the
    per-rank kernel-time gather and the JSON contract.  --dump-outputs writes the timed pass's last action slab: the stub
    adds one to every entry per call, so it also counts the warm-up and timed steps that ran."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--full", "--batch", "64", "--steps", "3",
                          "--warmup", "1", "--ring", "4", "--dump-outputs", str(tmp_path / "out")], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines                      # rank 0's JSON line and nothing else on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1 and out["scaling"] == "weak" and out["value"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["action.npy"]
    act = np.load(tmp_path / "out" / "action.npy")
    assert act.dtype == np.float32 and act.shape == (64, 60) and (act == 1 + 3).all()
    c = out["config"]
    assert c["dry_launch"] is True and c["rccl_ranks"] == 2 and c["backend"] == "gloo" and len(c["kernel_ms_per_rank"]) == 2
    assert c["with_allgather_steps_per_s"] > 0 and c["without_allgather_steps_per_s"] == out["value"]
    assert c["sharding"].startswith("2 x 64 robots")
    assert c["with_allgather_direct_steps_per_s"] > 0 and c["allgather_schedule"] is None
    # a rank count the node cannot serve is refused before anything is launched
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "64"], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode != 0 and "GPU(s)" in res.stderr


def test_bench_plain_run_times_only_its_headline_dry_run_world_size_2(tmp_path):
    """Without --full the ranks run the timed pass and nothing after it: with --allgather the exchange is inside `value` (the
    ring rate IS `value`), and the passes with the other schedule and without the exchange are not run -- their rates are
    null.  --dump-outputs still writes the timed pass's last action slab (warm-up + timed steps = 1 + 3 calls of the stub)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--allgather", "--batch", "64", "--steps", "3",
                          "--warmup", "1", "--ring", "4", "--dump-outputs", str(tmp_path / "out")], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    c = out["config"]
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0 and c["allgather"] is True and c["allgather_schedule"] == "ring"
    assert c["with_allgather_steps_per_s"] == out["value"]
    assert c["with_allgather_direct_steps_per_s"] is None and c["without_allgather_steps_per_s"] is None and c["allgather_note"] is None
    assert sorted(os.listdir(tmp_path / "out")) == ["action.npy", "action_allgathered.npy"]
    act, gathered = np.load(tmp_path / "out" / "action.npy"), np.load(tmp_path / "out" / "action_allgathered.npy")
    assert (act == 1 + 3).all() and gathered.shape == (128, 60) and (gathered == 1 + 3).all()


def test_bench_dry_run_world_size_8_uneven_shards():
    """The shape of the driver's scaling run at N = 8 (SCALE record: n_gpus, eight ranks in the process group, both all-gather
    rates -- ring and direct -- next to the rate without, one row of kernel times per rank), on CPU over gloo, and with a batch
    that does not divide by the ranks: 8 x 4096 + 5 robots through core.sharding.shard_bounds (shards of 4096 and 4097)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "8", "--dry-launch", "--full", "--total-batch", str(8 * 64 + 5), "--steps", "2",
                          "--warmup", "1", "--ring", "2"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    c = out["config"]
    assert out["n_gpus"] == 8 and c["rccl_ranks"] == 8 and len(c["kernel_ms_per_rank"]) == 8 and all(len(r) == 6 for r in c["kernel_ms_per_rank"])
    assert out["scaling"] == "weak" and out["value"] == c["without_allgather_steps_per_s"] > 0
    assert c["with_allgather_steps_per_s"] > 0 and c["with_allgather_direct_steps_per_s"] > 0
    assert c["sharding"].startswith("517 robots over 8 ranks")
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - 517) < 1e-6 * 517        # value = all robots of all ranks per step time


def test_bench_dump_outputs_stays_under_its_budget_with_a_fixed_sample(tmp_path, monkeypatch):
    """bench.dump_outputs: float32 / float64 .npy files; over the byte budget every array keeps the same seeded row sample."""
    import bench
    act = torch.arange(1000 * 60, dtype=torch.float32).view(1000, 60)
    legs = np.arange(1000 * 4, dtype=np.int32).reshape(1000, 4)
    bench.dump_outputs(tmp_path / "full", {"action": act, "legs": legs})
    assert np.array_equal(np.load(tmp_path / "full" / "action.npy"), act.numpy())
    assert np.load(tmp_path / "full" / "legs.npy").dtype == np.float64
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, {"action": act, "legs": legs})
    a, l = np.load(tmp_path / "a" / "action.npy"), np.load(tmp_path / "a" / "legs.npy")
    assert a.nbytes + l.nbytes <= 100_000 and 0 < a.shape[0] == l.shape[0] < 1000
    rows = a[:, 0].astype(np.int64) // 60
    assert (np.diff(rows) > 0).all() and np.array_equal(l[:, 0], 4 * rows)   # the same rows of both arrays, in order
    assert np.array_equal(np.load(tmp_path / "b" / "action.npy"), a)


def test_synthetic_states_are_deterministic_and_shaped():
    cfg = MPCConfig.for_robot("ghost")
    a, ca, ta = synthetic.make_states(128, cfg, seed=3)
    b, cb, tb = synthetic.make_states(128, cfg, seed=3)
    for k in a:
        assert np.array_equal(a[k], b[k])
    assert np.array_equal(ca, cb) and np.array_equal(ta, tb)
    assert a["rpy"].shape == (3, 128) and a["jac"].shape == (36, 128) and a["q"].dtype == np.float32
    assert np.abs(a["rpy"][:2]).max() <= 0.2 + 1e-6 and np.abs(ca[0]).max() <= 0.35 + 1e-6
    c = synthetic.gait_consistent_contacts(cfg, ta, np.zeros((4, 128), dtype=bool))
    assert set(np.unique(c.sum(0))) <= {2, 4}  # trot: a diagonal pair or all four
    fixed, cf, _ = synthetic.make_states(16, cfg, seed=0, fixed_cmd=(0.3, 0.0, 0.0))
    assert np.all(cf[0] == np.float32(0.3)) and np.all(cf[1:] == 0)


def test_packed_state_views_share_one_slab():
    """PackedState: the per-robot float64 clock and every field are contiguous views into ONE [82, B] slab (host and
    device side), contact as int32; the clock rows come first so that they are 8-byte aligned for odd B too."""
    import torch
    from robot_gym_amd.controllers.mpc.batched import PackedState, STATE_FIELDS
    B = 5
    ps = PackedState(B, torch.device("cpu"), pin=False)
    assert ps.host_slab.shape == (2 + sum(c for _, c, _ in STATE_FIELDS) + 3, B) == (82, B)
    assert ps.host_clock.shape == (B,) and ps.host_clock.dtype == torch.float64 and ps.host_clock.data_ptr() == ps.host_slab.data_ptr()
    row = 2
    for name, comps, dt in STATE_FIELDS:
        h = ps.host[name]
        assert h.shape == (comps, B) and h.dtype == dt and h.is_contiguous()
        assert h.data_ptr() == ps.host_slab[row].data_ptr()
        row += comps
    ps.host["contact"][:] = torch.arange(4 * B, dtype=torch.int32).reshape(4, B)
    ps.host["rpy"][:] = 1.5
    ps.host_clock[:] = torch.tensor([0.1, 0.2, 1e6 + 0.001, 3.0, 4.0], dtype=torch.float64)
    dev = ps.upload(with_clock=True)
    assert torch.equal(dev["contact"], ps.host["contact"]) and torch.equal(dev["rpy"], ps.host["rpy"])
    assert torch.equal(dev["t_robot"], ps.host_clock) and float(ps.host["rpy"][0, 0]) == 1.5   # the clock did not spill into rpy
    assert dev["jac"].data_ptr() == ps.dev_slab[39].data_ptr()
    assert "t_robot" not in ps.upload() and ps.upload(with_cmd=True)["cmd"].data_ptr() == ps.dev_slab[79].data_ptr()


class _RecordingBatchedController:
    """CPU stand-in for BatchedMPCController inside MPCVecEnv's host-logic test: records what the wrapper hands to the one
    batched call and returns action rows that encode (slot, command)."""

    def __init__(self, batch, cfg, device=None, extra_outputs=False):
        import torch
        self.batch, self.cfg, self.device = batch, cfg, torch.device("cpu")
        self.resets, self.calls, self.closed = [], [], False

    def reset_at(self, t0s, idx=None):
        self.resets.append((list(t0s), list(idx)))

    def get_action(self, t, state):
        import torch
        self.calls.append({k: v.clone() for k, v in state.items()})
        act = torch.zeros(self.batch, 60)
        act[:, 0] = torch.arange(self.batch, dtype=torch.float32)
        act[:, 1:4] = state["cmd"].T
        return act

    def close(self):
        self.closed = True


def test_vec_env_host_logic_keeps_each_envs_own_step(monkeypatch):
    """MPCVecEnv on the CPU with a recording controller: BatchEnv surface (space checks, contains, __getattr__, close), the
    envs' own step() semantics survive (GoEnv clipping, standing action on target, update_equip), ONE batched call per
    tick, per-env clocks and resets (a partial reset that includes env 0 does not touch the others)."""
    import torch
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeGoEnv, SplitGoEnv, FakeRobotGymEnv, Box
    from robot_gym_amd.gym.split_step import one_pass
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")          # VY_OFFSET 0.08, WZ_OFFSET -0.025
    B = 5
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=3)
    OnePassGoEnv = one_pass(FakeGoEnv, FakeRobotGymEnv)   # generic interceptor after the task env in the MRO: no env code restated
    assert [k.__name__ for k in OnePassGoEnv.__mro__[:4]] == ["OnePassFakeGoEnv", "FakeGoEnv", "_InterceptFakeRobotGymEnv", "FakeRobotGymEnv"]
    envs = [FakeGoEnv(cfg, state, 0, BatchSlotController), OnePassGoEnv(cfg, state, 1, BatchSlotController, on_target=True),
            SplitGoEnv(cfg, state, 2, BatchSlotController, follow_camera=True), OnePassGoEnv(cfg, state, 3, BatchSlotController, follow_camera=True),
            SplitGoEnv(cfg, state, 4, BatchSlotController)]
    venv = vec_env.MPCVecEnv(envs, config=cfg)
    assert len(venv) == B and venv[3] is envs[3] and venv.action_space == Box([-1, -1], [1, 1]) and venv.observation_space is envs[0].observation_space
    with pytest.raises(AttributeError):
        venv._missing
    # construction resets every slot at its env's clock 0; nothing is applied before the first step
    actions = np.array([[0.9, 0.1], [0.3, 0.2], [-0.5, -0.9], [0.2, 0.0], [0.1, 0.3]], dtype=np.float32)
    obs, rew, done, info = venv.step(actions)
    ctl = venv.controller
    assert len(ctl.calls) == 1 and venv.batched_calls == 1
    assert ctl.resets == [([0.0] * B, list(range(B)))]
    assert obs.shape == (B, 2) and rew.shape == (B,) and done.shape == (B,) and len(info) == B
    off = np.array([0.0, 0.08, -0.025], dtype=np.float32)
    want = np.array([[0.35, 0.0, 0.1], [0.0, 0.0, 0.0], [0.0, 0.0, -0.4], [0.2, 0.0, 0.0], [0.1, 0.0, 0.3]], dtype=np.float32) + off
    np.testing.assert_array_equal(ctl.calls[0]["cmd"].numpy().T, want)         # clipped / standing commands, float32 offsets
    for b, env in enumerate(envs):
        row = env.simulation.applied[-1]
        assert row[0] == b and np.array_equal(row[1:4], want[b])               # every env applied ITS row
        assert env.simulation.robot.equipment_updates == (1 if b in (2, 3) else 0)
        assert env.pre_controller_runs == (2 if type(env) is FakeGoEnv else 1)   # capture + replay vs one pass (pre_step / post_step, or the interceptor)
    np.testing.assert_array_equal(ctl.calls[0]["t_robot"].numpy(), np.zeros(B))
    np.testing.assert_array_equal(ctl.calls[0]["rpy"].numpy(), state["rpy"])
    for k in range(3):
        venv.step(actions)
    np.testing.assert_array_equal(ctl.calls[-1]["t_robot"].numpy(), np.full(B, 30 * 0.001))
    # partial reset INCLUDING env 0: only those slots get a reset, each at its own (zeroed) clock; the others keep theirs
    venv.reset([0, 3])
    venv.step(actions)
    assert ctl.resets[-1] == ([0.0, 0.0], [0, 3]) and len(ctl.resets) == 2
    np.testing.assert_array_equal(ctl.calls[-1]["t_robot"].numpy(), np.array([0.0, 0.04, 0.04, 0.0, 0.04]))
    # validation and error paths
    with pytest.raises(ValueError, match="Invalid action at index 2"):
        venv.step(np.array([[0, 0], [0, 0], [1.5, 0], [0, 0], [0, 0]], dtype=np.float32))
    with pytest.raises(ValueError):
        venv.step(actions[:3])
    with pytest.raises(RuntimeError, match="outside MPCVecEnv.step"):
        envs[0].simulation.controller.get_action()
    with pytest.raises(ValueError, match="same action space"):
        vec_env.MPCVecEnv([envs[0], FakeRobotGymEnv(cfg, state, 1, BatchSlotController)], config=cfg)
    from robot_gym_amd.controllers.controller import Controller

    class _Other(Controller):
        MOTOR_CONTROL_MODE = 3
        def update_controller_params(self, params): pass
        def get_action(self): return np.zeros(60)
        def setup_ui_params(self, c): pass
        def read_ui_params(self, c, ui): pass
        def reset(self): pass
    with pytest.raises(TypeError, match="BatchSlotController"):
        vec_env.MPCVecEnv([FakeGoEnv(cfg, state, 0, _Other)], config=cfg)
    venv.close()
    assert all(e.closed for e in envs) and ctl.closed


def test_vec_env_worker_processes_match_the_in_process_path(monkeypatch):
    """MPCVecEnv(blocking=False): the envs live in spawned worker processes (slices of the batch), phases 1 and 3 run there
    in parallel, the state travels through ONE shared slab and the parent makes the one batched call -- the reference's
    BatchEnv(envs, blocking=False) over ExternalProcess workers (batch_env.py:80-84, wrappers.py:294-458) with the
    controller call cut out of the middle.  Same observations, same commands, clocks, resets and action rows as the
    in-process path; attribute forwarding goes through the first worker; a worker-side exception is re-raised here."""
    import functools
    import torch
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym import vec_env
    from tests.fake_envs import make_fake_env, Box
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    B = 7
    kinds = ["go", "split", "go", "split", "go", "go", "split"]
    kw = [dict(on_target=(b == 1), follow_camera=(b == 4)) for b in range(B)]
    ctors = [functools.partial(make_fake_env, kinds[b], "ghost", 3, B, b, **kw[b]) for b in range(B)]
    par = vec_env.MPCVecEnv(blocking=False, constructors=ctors, workers=3, config=cfg)
    ser = vec_env.MPCVecEnv([c() for c in ctors], config=cfg)
    try:
        assert len(par) == B and par.action_space == Box([-1, -1], [1, 1]) and par.closed is False   # `closed`: forwarded to env 0 in worker 0
        np.testing.assert_array_equal(par.reset(), ser.reset())
        rng = np.random.default_rng(5)
        for k in range(4):
            actions = rng.uniform(-1, 1, (B, 2)).astype(np.float32)
            if k == 2:
                np.testing.assert_array_equal(par.reset([0, 5]), ser.reset([0, 5]))
            op, rp, dp, ip = par.step(actions)
            os_, rs, ds, is_ = ser.step(actions)
            np.testing.assert_array_equal(op, os_)
            np.testing.assert_array_equal(rp, rs)
            np.testing.assert_array_equal(dp, ds)
            assert ip == is_
            a, b_ = par.controller.calls[-1], ser.controller.calls[-1]
            assert sorted(a) == sorted(b_)
            for name in a:
                assert torch.equal(a[name], b_[name]), name       # the same slab reached the one batched call
        assert par.controller.resets == ser.controller.resets and par.batched_calls == 4
        with pytest.raises(ValueError, match="Invalid action at index 3"):
            par.step(np.array([[0, 0]] * 3 + [[2.0, 0]] + [[0, 0]] * 3, dtype=np.float32))
        with pytest.raises(Exception, match="AttributeError"):
            par.no_such_attribute
    finally:
        par.close()
        ser.close()
    assert par.controller.closed


def test_vec_env_worker_processes_feed_every_shard_its_own_clocks(monkeypatch):
    """blocking=False with devices=[...]: the workers write ONE shared slab, and every shard's handle must get exactly its
    columns of it.  Rows 0-1 are not per-column -- they hold B float64 clocks back to back -- so a column slice of them hands a
    shard other robots' clocks.  After two partial resets every shard and every worker slice holds envs at different clocks;
    each shard's recorded call must equal the single-handle call's columns [lo, hi) bit for bit, t_robot included.  B = 13
    (odd: the clock of robot 6 straddles the two clock rows) and worker slices that cross the shard boundaries."""
    import functools
    import torch
    from robot_gym_amd.gym import vec_env
    from tests.fake_envs import make_fake_env
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    B = 13
    ctors = [functools.partial(make_fake_env, "base", "ghost", 3, B, b) for b in range(B)]
    acts = np.random.default_rng(7).uniform(-1, 1, (8, B, 3)).astype(np.float32)
    resets = {3: [0, 4, 6, 7, 9, 12], 5: [0, 2, 5, 8, 11]}   # env 0, both sides of every shard and worker boundary

    def run(workers, devices):
        venv = vec_env.MPCVecEnv(blocking=False, constructors=ctors, workers=workers, config=cfg, devices=devices)
        controllers = list(venv.controllers)
        try:
            venv.reset()
            for k in range(len(acts)):
                if k in resets:
                    venv.reset(resets[k])
                venv.step(acts[k])
        finally:
            venv.close()
        return controllers
    for workers, devices in ((3, [None, None]), (2, [None, None, None])):
        one, = run(workers, None)
        shards = run(workers, devices)
        assert [c.batch for c in shards] == [hi - lo for lo, hi in (shard_bounds(B, s, len(devices)) for s in range(len(devices)))]
        # the single-handle run itself: every env at its own clock at the last tick (FakeSimulation: 10 steps of 1 ms per tick)
        counters = np.array([20, 70, 20, 70, 40, 20, 40, 40, 20, 40, 70, 20, 40])
        np.testing.assert_array_equal(one.calls[-1]["t_robot"].numpy(), counters * 0.001)
        lo = 0
        for s, ctl in enumerate(shards):
            hi = lo + ctl.batch
            assert len(ctl.calls) == len(one.calls) == len(acts)
            for k, (call, ref) in enumerate(zip(ctl.calls, one.calls)):
                assert sorted(call) == sorted(ref)
                for name, v in ref.items():
                    want = v[lo:hi] if name == "t_robot" else v[:, lo:hi]
                    assert torch.equal(call[name], want), (devices, s, k, name, call[name].numpy(), want.numpy())
            lo = hi


def test_vec_env_cleans_up_when_a_shard_fails_to_build(monkeypatch):
    """The second shard's controller raises in the constructor: the handle already made is closed, the worker processes have
    exited and the shared memory is gone; in-process envs stay open (they are the caller's, as on the body-rows refusal)."""
    import functools
    import torch
    from multiprocessing import shared_memory
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeGoEnv, make_fake_env
    made, workers = [], []

    class FailsSecond(_RecordingBatchedController):
        def __init__(self, *args, **kw):
            if len(made) == 1:
                raise RuntimeError("second handle refused")
            super().__init__(*args, **kw)
            made.append(self)

    class Worker(vec_env._Worker):
        def __init__(self, ctx, constructors, lo, batch, shm_state, shm_act, *rest):
            super().__init__(ctx, constructors, lo, batch, shm_state, shm_act, *rest)
            self.shm_names = (shm_state, shm_act)
            workers.append(self)
    monkeypatch.setattr(vec_env, "BatchedMPCController", FailsSecond)
    monkeypatch.setattr(vec_env, "_Worker", Worker)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    B = 5
    ctors = [functools.partial(make_fake_env, "go", "ghost", 3, B, b) for b in range(B)]
    with pytest.raises(RuntimeError, match="second handle refused"):
        vec_env.MPCVecEnv(blocking=False, constructors=ctors, workers=2, config=cfg, devices=[None, None])
    assert len(made) == 1 and made[0].closed
    assert len(workers) == 2
    for w in workers:
        assert not w.process.is_alive() and w.process.exitcode is not None
    for name in workers[0].shm_names:
        with pytest.raises(FileNotFoundError):
            shared_memory.SharedMemory(name=name)
    made.clear()
    state, _, _ = synthetic.make_states(B, cfg, seed=3)
    envs = [FakeGoEnv(cfg, state, b, BatchSlotController) for b in range(B)]
    with pytest.raises(RuntimeError, match="second handle refused"):
        vec_env.MPCVecEnv(envs, config=cfg, devices=[None, None, None])
    assert len(made) == 1 and made[0].closed
    assert not any(e.closed for e in envs)


def test_vec_env_refuses_a_non_repeatable_step_before_anything_is_applied(monkeypatch):
    """An env without pre_step / post_step is stepped twice per tick (capture + replay).  If its pre-controller code derives a
    different command on the second pass, the slot controller refuses INSIDE get_action -- before ApplyStepAction -- the wrapper
    is unusable from then on (the batched controller has already advanced), and split_step.one_pass is the documented fix."""
    import torch
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.gym.split_step import one_pass
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeRobotGymEnv
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    state, _, _ = synthetic.make_states(2, cfg, seed=3)

    class Drifting(FakeRobotGymEnv):
        def step(self, action, **kwargs):
            self.calls = getattr(self, "calls", 0) + 1
            return super().step((action[0] + 0.01 * self.calls, action[1], action[2]), **kwargs)   # not repeatable

    envs = [Drifting(cfg, state, b, BatchSlotController) for b in range(2)]
    venv = vec_env.MPCVecEnv(envs, config=cfg)
    with pytest.raises(RuntimeError, match="not repeatable"):
        venv.step(np.zeros((2, 3), dtype=np.float32))
    assert all(len(e.simulation.applied) == 0 for e in envs)       # nothing reached ApplyStepAction
    with pytest.raises(RuntimeError, match="unusable: an earlier step\\(\\) failed half-way"):   # the batched call had been made: fatal for the batch
        venv.step(np.zeros((2, 3), dtype=np.float32))

    Fixed = one_pass(Drifting, FakeRobotGymEnv)                    # Drifting.step's own code runs once per tick
    envs = [Fixed(cfg, state, b, BatchSlotController) for b in range(2)]
    venv = vec_env.MPCVecEnv(envs, config=cfg)
    for k in range(1, 3):
        obs, rew, done, info = venv.step(np.zeros((2, 3), dtype=np.float32))
        assert obs.shape == (2, 2) and all(len(e.simulation.applied) == k and e.calls == k for e in envs)
        assert all(abs(float(e.simulation.applied[-1][1]) - 0.01 * k) < 1e-7 for e in envs)   # the command of THAT single pass
    # alone, outside MPCVecEnv, the interceptor is a pass-through
    with pytest.raises(RuntimeError, match="outside MPCVecEnv.step"):
        envs[0].step((0.0, 0.0, 0.0))


def test_vec_env_matches_reference_batch_env_behaviour(monkeypatch):
    """MPCVecEnv against tests/golden/batch_env.json -- what the reference's own BatchEnv (agents/ppo/tools/batch_env.py:18-115,
    imported by tests/golden/make_golden.py) returned, forwarded and raised when driven with the same fake envs."""
    import json
    import torch
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeSimulation, StubRobot
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_env.json")))
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    state, _, _ = synthetic.make_states(4, cfg, seed=5)

    class Space:   # the golden's space: two components in [lo, hi]
        def __init__(self, lo, hi): self.lo, self.hi = lo, hi
        def __eq__(self, other): return isinstance(other, Space) and (self.lo, self.hi) == (other.lo, other.hi)
        def contains(self, x): return len(x) == 2 and all(self.lo <= float(v) <= self.hi for v in x)

    class Env:     # the golden's env, with the controller call of RobotGymEnv.step in the middle
        marker = "env-attribute"

        def __init__(self, k, hi=1.0):
            self.k, self.t, self.closed = k, 0, False
            self.observation_space, self.action_space = Space(-9.0, 9.0), Space(-1.0, hi)
            self.simulation = FakeSimulation(StubRobot(cfg, state, k), BatchSlotController, config=cfg)

        def step(self, action):
            self.simulation.controller.update_controller_params(action)
            self.simulation.ApplyStepAction(self.simulation.controller.get_action())
            self.t += 1
            return np.array([self.k, self.t, float(action[0])]), 0.5 * self.k, self.t >= 3, {"k": self.k}

        def reset(self):
            self.t = 0
            self.simulation.reset()
            return np.array([self.k, 0.0, 0.0])

        def close(self): self.closed = True

    envs = [Env(k) for k in range(4)]
    be = vec_env.MPCVecEnv(envs, config=cfg)
    assert len(be) == gold["len"] and (be[2] is envs[2]) == gold["getitem_is_env"]
    assert be.marker == gold["forwarded_attribute"] and (be.action_space is envs[0].action_space) == gold["forwarded_space_is_env0"]
    obs = be.reset()
    assert list(obs.shape) == gold["reset_all"]["shape"] and str(obs.dtype) == gold["reset_all"]["dtype"] and obs.tolist() == gold["reset_all"]["value"]
    actions = np.array([[0.1, 0.0], [0.2, 0.0], [0.3, 0.0], [0.4, 0.0]])
    o, r, d, i = be.step(actions)
    g = gold["step"]
    assert o.tolist() == g["obs"] and str(o.dtype) == g["obs_dtype"] and r.tolist() == g["reward"] and str(r.dtype) == g["reward_dtype"]
    assert d.tolist() == g["done"] and str(d.dtype) == g["done_dtype"] and type(i).__name__ == g["info_type"] and list(i) == g["info"]
    sub = be.reset([1, 3])
    assert list(sub.shape) == gold["reset_subset"]["shape"] and sub.tolist() == gold["reset_subset"]["value"]
    assert [e.t for e in envs] == gold["reset_subset"]["env_t_after"]
    bad = actions.copy()
    bad[2, 0] = 5.0
    with pytest.raises(ValueError) as err:
        be.step(bad)
    assert type(err.value).__name__ == gold["invalid_action"]["type"] and str(err.value) == gold["invalid_action"]["message"]
    assert [e.t for e in envs] == gold["invalid_action"]["env_t_after"]       # nothing was stepped
    with pytest.raises(ValueError):
        vec_env.MPCVecEnv([Env(0), Env(1, hi=2.0)], config=cfg)
    assert gold["space_mismatch"]["type"] == "ValueError"
    be.close()
    assert [e.closed for e in envs] == gold["close_closes_envs"]


def test_reference_env_step_fixture_and_fake_env_fidelity(monkeypatch):
    """tests/golden/env_step.json was recorded by running the REAL RobotGymEnv.step / GoEnv.step of the reference (instances made
    without PyBullet) -- alone with a recording controller, and three of them inside MPCVecEnv.  Here: (1) the fixture says
    what the north star needs (the reference's env code runs unchanged around one batched call per tick, commands clipped /
    replaced by the standing action by the ENV, update_equip honoured); (2) the fake envs the other tests use reproduce it."""
    import json
    import torch
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeGoEnv
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_step.json")))
    order = ["get_action", "ApplyStepAction", "get_observation", "reward", "termination"]
    cases = {c["name"]: c for c in gold["cases"]}
    assert cases["clipped"]["log"] == [["update_controller_params", [0.35, -0.4]]] + order                     # go_env.py:280
    assert cases["on_target"]["log"] == [["update_controller_params", [0.0, 0.0]]] + order                     # go_env.py:291-292
    assert cases["camera"]["log"] == [["update_controller_params", [0.1, 0.0]], "get_action", "ApplyStepAction", "update_equipment"] + order[2:]
    assert gold["robot_gym_env_step_log"][:4] == [["update_controller_params", [0.1, 0.2, 0.3]], "get_action", "ApplyStepAction", "update_equipment"]
    gv = gold["vec_env"]
    assert [c[0] for c in gv["batched_calls"]] == ["reset_at", "get_action", "get_action"]                       # ONE batched call per tick
    # (2) the same three envs as fakes
    calls = []

    class Recording(_RecordingBatchedController):
        def reset_at(self, t0s, idx=None): calls.append(["reset_at", list(t0s), list(idx)])
        def get_action(self, t, state):
            calls.append(["get_action", state["cmd"].numpy().T.round(6).tolist(), state["t_robot"].numpy().tolist()])
            return super().get_action(t, state)

    monkeypatch.setattr(vec_env, "BatchedMPCController", Recording)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    assert [cfg.vx_offset, cfg.vy_offset, cfg.wz_offset] == gv["offsets"]
    state, _, _ = synthetic.make_states(3, cfg, seed=9)
    envs = [FakeGoEnv(cfg, state, 0, BatchSlotController, config=cfg), FakeGoEnv(cfg, state, 1, BatchSlotController, config=cfg, on_target=True),
            FakeGoEnv(cfg, state, 2, BatchSlotController, config=cfg, follow_camera=True)]
    venv = vec_env.MPCVecEnv(envs, config=cfg)
    actions = np.array(gv["actions"], dtype=np.float32)
    for k, tick in enumerate(gv["ticks"]):
        o, r, d, i = venv.step(actions)
        assert np.asarray(o).tolist() == tick["obs"] and np.asarray(r).tolist() == tick["reward"] and np.asarray(d).tolist() == tick["done"]
        assert [e.simulation.applied[-1][:4].round(6).tolist() for e in envs] == tick["applied_row_head"]
        assert [e.simulation.robot.equipment_updates for e in envs] == tick["equipment_updates"]
    assert calls == gv["batched_calls"]
    # (3) the REAL GoEnv stepped in one pass (split_step.one_pass(GoEnv, RobotGymEnv), recorded by make_golden.py): the interceptor
    # sits after GoEnv in the MRO, GoEnv.step's own pre-controller code (show_plot on, counting _update_plot) ran ONCE per tick,
    # and the transitions, applied rows and batched calls are those of the two-pass path
    g1 = gold["vec_env_one_pass"]
    assert g1["mro"] == ["OnePassGoEnv", "GoEnv", "_InterceptRobotGymEnv", "RobotGymEnv"]
    assert g1["batched_calls"] == gv["batched_calls"]
    for k, (t1, t2) in enumerate(zip(g1["ticks"], gv["ticks"])):
        assert t1["update_plot_calls"] == [k + 1] * 3
        assert all(t1[f] == t2[f] for f in ("obs", "reward", "done", "applied_row_head", "equipment_updates"))
    # ... and the fake one-pass env reproduces it
    from robot_gym_amd.gym.split_step import one_pass
    from tests.fake_envs import FakeRobotGymEnv
    OnePass = one_pass(FakeGoEnv, FakeRobotGymEnv)
    del calls[:]
    envs = [OnePass(cfg, state, 0, BatchSlotController, config=cfg), OnePass(cfg, state, 1, BatchSlotController, config=cfg, on_target=True),
            OnePass(cfg, state, 2, BatchSlotController, config=cfg, follow_camera=True)]
    venv = vec_env.MPCVecEnv(envs, config=cfg)
    for tick in g1["ticks"]:
        o, r, d, i = venv.step(actions)
        assert np.asarray(o).tolist() == tick["obs"] and [e.simulation.applied[-1][:4].round(6).tolist() for e in envs] == tick["applied_row_head"]
        assert [e.simulation.robot.equipment_updates for e in envs] == tick["equipment_updates"]
    assert calls == g1["batched_calls"]


def test_ui_glue_of_the_controller_plugins():
    """setup_ui_params / read_ui_params (reference controllers/mpc/mpc_controller.py:68-81: three sliders Vx, Vy, Wz in [-2, 2]
    starting at 0, read back in that order; called as statics by gym/envs/go_to/go_env.py:113,136-139 and
    playground/playground.py:47,95) and get_standing_action (:111-113) on both plugin classes, with a recording stub client.
    The expected calls are those the reference's own class made when make_golden.py imported it (tests/golden/adapter.json)."""
    import json
    from robot_gym_amd.controllers.mpc.mpc_controller import MPCController
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adapter.json")))["ui_glue"]

    class Client:
        def __init__(self): self.log, self.values = [], {}
        def addUserDebugParameter(self, name, lo, hi, start):
            self.log.append(["addUserDebugParameter", name, lo, hi, start])
            self.values[len(self.values) + 10] = 0.25 * (len(self.values) + 1)
            return len(self.values) + 9
        def readUserDebugParameter(self, handle):
            self.log.append(["readUserDebugParameter", handle])
            return self.values[handle]

    for cls in (MPCController, BatchSlotController):
        c = Client()
        ui = cls.setup_ui_params(c)          # called on the CLASS, before any instance exists (go_env.py:113)
        vals = cls.read_ui_params(c, ui)
        assert list(ui) == gold["ui_handles"] and list(vals) == gold["ui_values"], cls.__name__
        assert c.log == gold["client_log"], cls.__name__
        assert list(cls.get_standing_action()) == gold["standing_action"]


def test_fake_simulation_clock_is_the_reference_clock():
    """The reference's Simulation.GetTimeSinceReset / ApplyStepAction / reset (core/simulation.py:123-127,141-142,175-179), run
    for real by make_golden.py: step_counter * 0.001 after 10 simulation steps per tick -- bit for bit what the fake simulation
    of the tests (and therefore the per-robot clocks MPCVecEnv hands the controller) produces."""
    import json
    from tests.fake_envs import FakeSimulation
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "env_step.json")))["simulation_clock"]
    assert gold["sim_steps_per_tick"] == FakeSimulation.ACTION_REPEAT == 10 and gold["reset_calls_controller_reset"] == 2 and gold["after_reset"] == 0.0

    class Ctl:
        MOTOR_CONTROL_MODE = 3
        def __init__(self, robot, clock): pass
        def reset(self): pass
    sim = FakeSimulation(object(), Ctl)
    got = []
    for _ in gold["after_each_tick_hex"]:
        sim.ApplyStepAction(np.zeros(60))
        got.append(float(sim.GetTimeSinceReset()).hex())
    assert got == gold["after_each_tick_hex"]


def test_vec_env_shards_the_batch_over_devices(monkeypatch):
    """MPCVecEnv(devices=[...]): one controller handle per shard over contiguous slices of the batch (shard_bounds), ONE pinned
    state buffer (shard s owns a contiguous [82, n_s] block of it) and ONE action slab; every shard's controller sees exactly
    its envs' state columns, clocks and commands, and resets with LOCAL indices -- a partial reset that crosses the shard
    boundary reaches both handles.  The envs see the same rows as under a single handle.  (CPU, recording controllers; the GPU
    version with two handles on one device: tests/test_gpu_boundary.py.)  API kept: reference agents/ppo/tools/batch_env.py:18-115."""
    import torch
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeGoEnv
    monkeypatch.setattr(vec_env, "BatchedMPCController", _RecordingBatchedController)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = MPCConfig.for_robot("ghost")
    B = 5
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=3)
    actions = np.array([[0.9, 0.1], [0.3, 0.2], [-0.5, -0.9], [0.2, 0.0], [0.1, 0.3]], dtype=np.float32)

    def run(devices):
        envs = [FakeGoEnv(cfg, state, b, BatchSlotController) for b in range(B)]
        venv = vec_env.MPCVecEnv(envs, config=cfg, devices=devices)
        outs = [venv.step(actions) for _ in range(3)]
        venv.reset([1, 2, 4])                     # crosses the boundary between shard 0 (envs 0, 1) and shard 1 (envs 2, 3)
        outs.append(venv.step(actions))
        return venv, envs, outs
    one, envs1, outs1 = run(None)
    three, envs3, outs3 = run([None, None, None])
    assert [c.batch for c in three.controllers] == [2, 2, 1] and len(one.controllers) == 1 and three.controller is three.controllers[0]
    assert three.batched_calls == one.batched_calls == 4
    # one pinned buffer, shard blocks back to back
    assert [sh.state.host_slab.data_ptr() - three._host_buffer.data_ptr() for sh in three._shards] == [0, 4 * 82 * 2, 4 * 82 * 4]
    lo = 0
    for ctl in three.controllers:
        n = ctl.batch
        assert ctl.resets[0] == ([0.0] * n, list(range(n)))                                           # construction: every slot, local indices
        for k, call in enumerate(ctl.calls):
            ref = one.controller.calls[k]
            for name in ("rpy", "q", "contact", "cmd", "jac"):
                assert torch.equal(call[name], ref[name][:, lo:lo + n]), (name, k)
            assert torch.equal(call["t_robot"], ref["t_robot"][lo:lo + n])
        lo += n
    assert three.controllers[0].resets[-1] == ([0.0], [1]) and three.controllers[1].resets[-1] == ([0.0], [0]) and three.controllers[2].resets[-1] == ([0.0], [0])
    assert one.controller.resets[-1] == ([0.0] * 3, [1, 2, 4])
    # the envs applied the same commands (the recording controller's rows carry its LOCAL slot index in column 0)
    for b in range(B):
        a1, a3 = envs1[b].simulation.applied, envs3[b].simulation.applied
        assert len(a1) == len(a3) == 4 and all(np.array_equal(x[1:4], y[1:4]) for x, y in zip(a1, a3))
        assert a3[-1][0] == b - [0, 0, 2, 2, 4][b]
    for o1, o3 in zip(outs1, outs3):
        assert np.array_equal(o1[0], o3[0]) and np.array_equal(o1[1], o3[1]) and np.array_equal(o1[2], o3[2])
    with pytest.raises(ValueError, match="devices for"):
        vec_env.MPCVecEnv([FakeGoEnv(cfg, state, 0, BatchSlotController)], config=cfg, devices=[None, None])
    three.close()
    assert all(c.closed for c in three.controllers) or three.controllers == []


class _FunctionBatchedController(_RecordingBatchedController):
    """... whose action rows are a function of the state it was handed (so that ranks can be compared with one process)."""

    def get_action(self, t, state):
        import torch
        act = torch.zeros(self.batch, 60)
        act[:, 0:3] = state["cmd"].T
        act[:, 3:6] = state["rpy"].T
        act[:, 6] = state["t_robot"].to(torch.float32)
        act[:, 7:19] = state["q"].T
        return act


def _sharded_env_worker(rank, world, port, tmp):
    """One process per GPU, on the CPU: rank r steps ITS shard of the envs with its own MPCVecEnv and gathers every rank's rows."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from robot_gym_amd.gym import vec_env
    from robot_gym_amd.controllers.mpc.slot_controller import BatchSlotController
    from tests.fake_envs import FakeGoEnv
    vec_env.BatchedMPCController = _FunctionBatchedController
    torch.cuda.is_available = lambda: False
    cfg = MPCConfig.for_robot("ghost")
    total = 7                                                    # uneven shards: 4 + 3
    state, cmd, t_off = synthetic.make_states(total, cfg, seed=5)
    rng = np.random.default_rng(1)
    acts = rng.uniform(-1, 1, size=(4, total, 2)).astype(np.float32)
    lo, hi = shard_bounds(total, rank, world)
    mine = vec_env.MPCVecEnv([FakeGoEnv(cfg, state, b, BatchSlotController) for b in range(lo, hi)], config=cfg)
    whole = vec_env.MPCVecEnv([FakeGoEnv(cfg, state, b, BatchSlotController) for b in range(total)], config=cfg) if rank == 0 else None
    ok = True
    for k in range(4):
        if k == 2:
            mine.reset([i - lo for i in (1, 5) if lo <= i < hi])   # env 1 lives on rank 0, env 5 on rank 1
            if whole is not None:
                whole.reset([1, 5])
        obs, rew, done, info = mine.step(acts[k, lo:hi])
        rows = torch.from_numpy(mine._act_host.numpy().copy())
        every = all_gather_actions(rows, total=total, schedule="direct" if k % 2 else "ring")   # only because every rank wants all rows
        ok = ok and tuple(every.shape) == (total, 60) and torch.equal(every[lo:hi], rows)
        if whole is not None:
            o2 = whole.step(acts[k])
            ok = ok and torch.equal(every, torch.from_numpy(whole._act_host.numpy())) and np.array_equal(o2[0][lo:hi], obs) and np.array_equal(o2[1][lo:hi], rew)
    with open(os.path.join(tmp, f"r{rank}"), "w") as f:
        f.write("ok" if ok else "bad")
    dist.destroy_process_group()


def test_sharded_env_loop_world_size_2_gloo(tmp_path):
    """BASELINE configs[3]'s gym side with one process per GPU (here: per CPU rank, gloo): each rank owns shard_bounds(total, rank,
    world) envs and one MPCVecEnv over them -- no collective on the data path --, and the optional all-gather of the action
    rows (both schedules, uneven shards) gives every rank what ONE MPCVecEnv over all envs computes, a partial reset on each
    side of the shard boundary included.  Reference API: agents/ppo/tools/batch_env.py:18-115."""
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_sharded_env_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert [open(tmp_path / f"r{r}").read() for r in range(2)] == ["ok", "ok"]
