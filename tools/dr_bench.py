"""Times the domain randomisation (include/rg_dr.h), in one process and run, at batch 64, 4096 and 32768: the three kernels
on their own (a draw for every robot with a new world, apply for every robot, the push of a tick); BatchedGoEnv.step (random
terrain, measured contact, auto-reset) without and with a randomiser that scales the body, draws worlds and pushes, alternated
twice so that the file carries the run-to-run spread, next to a randomiser whose two launches run but change nothing (unit
scales, zero amplitudes), which separates the cost of the launches from the cost of controlling disturbed robots; and a tick
after which EVERY robot is reset on the device, without and with it.  hipEvents around at least --seconds of calls after a warm-up, one synchronisation at the end of each measurement.
Every figure stands next to env.step without the randomiser from the same run.  For the record, not a gate.

    python tools/dr_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/dr_tick.json]

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/dr_bench.py --batches 4096
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.gym.batched_go_env import BatchedGoEnv  # noqa: E402
from robot_gym_amd.sim import BatchedSRBSim, DomainRandomizer, RandomTerrain  # noqa: E402
from tools.scan_bench import timed  # noqa: E402

DR_SOURCES = ("robot_gym_amd/csrc/rg_dr.hip", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_srb_handle.h", "robot_gym_amd/csrc/rg_srb_dev.inc",
              "robot_gym_amd/csrc/rg_host.h", "include/rg_dr.h")
SETTINGS = dict(mass_scale=(0.8, 1.2), inertia_scale=(0.8, 1.2), new_world_each_episode=True, push_interval=100, push_ticks=10, push_probability=0.5,
                push_force_xy=20.0, push_force_z=5.0, push_torque_xy=2.0, push_torque_z=1.0)
# both launches of a step, but unit scales, the worlds kept and zero amplitudes: the robots move exactly as without a randomiser
LAUNCHES_ONLY = dict(push_interval=100, push_ticks=10, push_probability=0.5)


def dr_hash():
    """sha256 (16 hex digits) over the unit's own sources: bench.source_hash() covers the MPC kernels only."""
    h = hashlib.sha256()
    for rel in DR_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def kernel_rows(B, dev, cfg, seconds):
    """us per call of each kernel, every robot in the mask."""
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain())
    sim.reset()
    dr = DomainRandomizer(seed=1, **SETTINGS).bind(sim)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    zeros = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {}
    out["reset_us"], out["calls"] = timed(lambda: dr.on_reset(ones), seconds)
    out["reset_nobody_us"], _ = timed(lambda: dr.on_reset(zeros), seconds)
    out["apply_us"], _ = timed(dr.apply, seconds)
    out["push_us"], _ = timed(dr.pushes, seconds)
    dr.close()
    sim.close()
    return out


def env_rows(B, dev, seconds):
    """us per BatchedGoEnv.step without a randomiser, with one whose launches run but change nothing (LAUNCHES_ONLY) and with
    the full one, alternated twice; then per tick that ends with a device reset of every robot, without and with the full one."""
    make = lambda dr: BatchedGoEnv(B, device=dev, auto_reset=True, terrain=RandomTerrain(), contact="measured", seed=3, randomizer=dr)
    plain, idle, random = make(None), make(DomainRandomizer(seed=1, **LAUNCHES_ONLY)), make(DomainRandomizer(seed=1, **SETTINGS))
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    out = {}
    for env in (plain, idle, random):
        env.reset()
    for name, env in (("step_us", plain), ("step_launches_only_us", idle), ("step_dr_us", random), ("step_again_us", plain),
                      ("step_launches_only_again_us", idle), ("step_dr_again_us", random)):
        out[name], _ = timed(lambda: env.step(action), seconds)
    out["resets_per_robot"] = round(float(random.episode_count.double().mean()), 2)
    out["fallen_plain"], out["fallen_dr"] = int(plain.sim.fallen().sum()), int(random.sim.fallen().sum())

    def reset_tick(env):
        env.step(action)
        env.reset_on_device(ones)
        env.ctl.reset_masked(env.reset_mask)

    for name, env in (("reset_tick_us", plain), ("reset_tick_dr_us", random), ("reset_tick_again_us", plain), ("reset_tick_dr_again_us", random)):
        out[name], _ = timed(lambda: reset_tick(env), seconds)
    for env in (plain, idle, random):
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="64,4096,32768")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot)
    commit, dirty = bench.git_head()
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        row = dict(batch=B)
        row.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in kernel_rows(B, dev, cfg, args.seconds).items()})
        row.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in env_rows(B, dev, args.seconds).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = dict(what="domain randomisation: rg_dr_reset (every robot, new world), the same launch with an empty mask, rg_dr_apply and rg_dr_push "
                       "on their own; BatchedGoEnv.step (random terrain, measured contact, auto-reset) without and with a randomiser (body scales, "
                       "worlds, pushes) and with one whose launches run but change nothing (unit scales, zero amplitudes), alternated twice; and a "
                       "tick followed by a device reset of every robot, without and with it",
                  settings={k: list(v) if isinstance(v, tuple) else v for k, v in SETTINGS.items()}, robot=args.robot, commit=commit, dirty=dirty,
                  source_hash=bench.source_hash(), dr_source_sha256=dr_hash(), device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds,
                  rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
