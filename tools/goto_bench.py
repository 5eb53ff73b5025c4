"""Times the go-to-target task next to the controller + simulator tick it rides on, in one process and run: rg_goto_pre_step
alone, rg_goto_post_step alone (both on a held simulator state), the full BatchedGoEnv.step tick, and the closed-loop
controller + simulator tick of the same objects without the task, at batch 1, 1024, 4096 and 32768.  hipEvents around at
least one second of ticks after a warm-up, one synchronisation at the end of each measurement.  For the record, not a gate.

    python tools/goto_bench.py [--robot ghost] [--batches 1,1024,4096,32768] [--seconds 1.0] [--out profiles/goto_tick.json]

Every robot has its own planned path to a random target and creeps along it (vx 0.01 m/s, so a second of ticks fits on
the shortest path); the robot's command offsets are zeroed (they trim a drift the reduced model does not have) and the time,
track and progress limits are moved out of reach, so that every robot stays live for the whole measurement -- a done robot
costs the task kernel next to nothing.  `live` is the share still running at the end.

Auto-reset mode (`--auto-reset`, batch 4096, writes profiles/goto_autoreset.json with --out): (1) env.step with
auto_reset=True while no robot is done -- the cost of the empty passes -- next to env.step with auto_reset=False, the two
alternated `--repeats` times in one run; (2) a tick on which EVERY robot resets (the time limit set below one tick); (3) the
host reset(idx) of 1 % of the robots, wall clock around the call and a synchronise.

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/goto_bench.py --batches 4096
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.core import goto_abi  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.gym.batched_go_env import BatchedGoEnv  # noqa: E402
from tools.srb_bench import timed  # noqa: E402

CREEP = 0.01   # m/s


def goto_hash():
    h = hashlib.sha256()
    for rel in ("robot_gym_amd/csrc/rg_goto.hip", "robot_gym_amd/csrc/rg_goto_dev.inc", "include/rg_goto.h", "robot_gym_amd/csrc/rg_episode.hip",
                "robot_gym_amd/csrc/rg_stream_dev.inc", "include/rg_episode.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def auto_reset_mode(args, dev, cfg):
    B = 4096
    far = dict(max_time=1e9, max_track_err=10.0, progress_limit=1e9)
    off = BatchedGoEnv(B, cfg, seed=B, device=dev, **far)
    on = BatchedGoEnv(B, cfg, seed=B, device=dev, auto_reset=True, **far)
    every = BatchedGoEnv(B, cfg, seed=B, device=dev, auto_reset=True, max_time=0.005, max_track_err=10.0, progress_limit=1e9)
    action = torch.tensor([[CREEP, 0.0]], device=dev).repeat(B, 1)
    for env in (off, on, every):
        env.reset()
        for _ in range(args.warmup):
            env.step(action)
    assert int(on.done.sum()) == 0 and int(off.done.sum()) == 0 and int(every.done.sum()) == B
    assert int(every.reset_mask.sum()) == B and int(every.plan_status.sum()) == 0
    runs = dict(step_off_us=[], step_on_us=[], step_every_robot_resets_us=[])
    for _ in range(args.repeats):   # alternated: the host is shared, a drift hits all three alike
        runs["step_off_us"].append(timed(lambda: off.step(action), args.seconds)[0])
        runs["step_on_us"].append(timed(lambda: on.step(action), args.seconds)[0])
        runs["step_every_robot_resets_us"].append(timed(lambda: every.step(action), args.seconds)[0])
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    reset_only_us, _ = timed(lambda: (every.reset_on_device(ones), every.ctl.reset_masked(every.reset_mask)), args.seconds)
    idx = list(range(0, B, 100))
    host = []
    for _ in range(max(3, args.repeats)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        off.reset(idx)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e6)
    med = {k: round(statistics.median(v), 2) for k, v in runs.items()}
    row = dict(batch=B, **med, spread={k: [round(min(v), 2), round(max(v), 2)] for k, v in runs.items()},
               empty_passes_us=round(med["step_on_us"] - med["step_off_us"], 2),
               reset_of_every_robot_alone_us=round(reset_only_us, 2), host_reset_1pct_robots=len(idx),
               host_reset_1pct_us=round(statistics.median(host), 1), host_reset_1pct_spread_us=[round(min(host), 1), round(max(host), 1)],
               live_on=float((on.done == 0).float().mean()), mean_path_points=round(float(every.path_hdr[0].mean()), 1))
    for env in (off, on, every):
        env.close()
    commit, dirty = bench.git_head()
    result = dict(what="BatchedGoEnv.step at batch 4096, us per tick (median of alternated repeats, [min, max] in spread): auto_reset off; on with "
                       "no robot done (empty passes); on with every robot resetting each tick; the reset calls alone; the host reset(idx) of "
                       "1 % of the robots (wall clock)", robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(),
                  goto_source_sha256=goto_hash(), device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds,
                  repeats=args.repeats, rows=[row])
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="1,1024,4096,32768")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--auto-reset", action="store_true", help="the auto-reset measurements at batch 4096 instead of the tick table")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot, vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
    if args.auto_reset:
        result = auto_reset_mode(args, dev, cfg)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        print(json.dumps(result))
        return
    commit, dirty = bench.git_head()
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        env = BatchedGoEnv(B, cfg, seed=B, device=dev, max_time=1e9, max_track_err=10.0, progress_limit=1e9)
        env.reset()
        action = torch.tensor([[CREEP, 0.0]], device=dev).repeat(B, 1)
        for _ in range(args.warmup):
            env.step(action)
        step_us, n = timed(lambda: env.step(action), args.seconds)
        h, ts, ss = env._handle, env.task_state.data_ptr(), env.sim.state.data_ptr()
        pre_us, _ = timed(lambda: h.pre_step(ts, ss, env._paths, action.data_ptr(), env.cmd.data_ptr()), args.seconds / 4)
        post_us, _ = timed(lambda: h.post_step(ts, ss, env._paths, env._obs_cm.data_ptr(), env.reward.data_ptr(), env.done.data_ptr()), args.seconds / 4)
        live = float((env.done == 0).float().mean())
        visible = float(env.task_state[goto_abi.ROW_VISIBLE].mean())
        points = float(env.path_hdr[0].mean())
        # the tick of the parent commit: controller + simulator, the command held
        closed_us, _ = timed(lambda: (env.ctl.get_action(0.0, env.sim.obs), env.sim.step(env.ctl)), args.seconds)
        fallen = int(env.sim.fallen().sum())
        rows.append(dict(batch=B, ticks=n, pre_us=round(pre_us, 2), post_us=round(post_us, 2), step_us=round(step_us, 2),
                         closed_us=round(closed_us, 2), task_us=round(step_us - closed_us, 2),
                         task_share_of_step=round((step_us - closed_us) / step_us, 4), env_steps_per_s=round(B / step_us * 1e6),
                         live=round(live, 4), mean_path_points=round(points, 1), mean_visible_points=round(visible, 1), fallen=fallen))
        print(json.dumps(rows[-1]), flush=True)
        env.close()
    result = dict(what="go-to-target task next to the controller + simulator tick, one process and run; task_us = step_us - closed_us "
                       "(pre_step, post_step and their launch overhead)", robot=args.robot, commit=commit, dirty=dirty,
                  source_hash=bench.source_hash(), goto_source_sha256=goto_hash(), device=torch.cuda.get_device_name(0),
                  seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
