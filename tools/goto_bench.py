"""Times the go-to-target task next to the controller + simulator tick it rides on, in one process and run: rg_goto_pre_step
alone, rg_goto_post_step alone (both on a held simulator state), the full BatchedGoEnv.step tick, and the closed-loop
controller + simulator tick of the same objects without the task, at batch 1, 1024, 4096 and 32768.  hipEvents around at
least one second of ticks after a warm-up, one synchronisation at the end of each measurement.  For the record, not a gate.

    python tools/goto_bench.py [--robot ghost] [--batches 1,1024,4096,32768] [--seconds 1.0] [--out profiles/goto_tick.json]

Every robot has its own planned path to a random target and creeps along it (vx 0.01 m/s, so a second of ticks fits on
the shortest path); the robot's command offsets are zeroed (they trim a drift the reduced model does not have) and the time,
track and progress limits are moved out of reach, so that every robot stays live for the whole measurement -- a done robot
costs the task kernel next to nothing.  `live` is the share still running at the end.

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/goto_bench.py --batches 4096
"""
import argparse
import hashlib
import json
import os
import sys

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
    for rel in ("robot_gym_amd/csrc/rg_goto.hip", "include/rg_goto.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="1,1024,4096,32768")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot, vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
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
