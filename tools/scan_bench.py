"""Times the terrain height scan (include/rg_scan.h), in one process and run, at batch 64, 4096 and 32768 with the default 48
points: HeightScan.observe on the plane, on the reference's random terrain and on a 256 x 256 grid; the same quantity composed
from torch operations and BatchedSRBSim.ground_height (the route a user had before the kernel); and BatchedGoEnv.step (random
terrain, measured contact, auto-reset) with and without the scan, alternated twice so that the file carries the run-to-run
spread.  hipEvents around at least --seconds of calls after a warm-up, one synchronisation at the end of each measurement.
For the record, not a gate.

    python tools/scan_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/scan_tick.json]

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/scan_bench.py --batches 4096
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
from robot_gym_amd.sim import BatchedSRBSim, GridTerrain, RandomTerrain  # noqa: E402
from robot_gym_amd.sim.height_scan import HeightScan  # noqa: E402

SCAN_SOURCES = ("robot_gym_amd/csrc/rg_scan.hip", "robot_gym_amd/csrc/rg_srb_ground.inc", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_srb_handle.h",
                "robot_gym_amd/csrc/rg_srb_dev.inc", "robot_gym_amd/csrc/rg_host.h", "include/rg_scan.h")


def timed(fn, seconds, probe=20):
    """us per call of fn() over at least `seconds` of device time: a probe sizes the run, events bracket it, one wait."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(probe):
        fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(probe):
        fn()
    stop.record()
    torch.cuda.synchronize()
    per = max(start.elapsed_time(stop) / probe, 1e-3)          # ms
    n = max(probe, int(np.ceil(1000.0 * seconds / per)))
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return 1000.0 * start.elapsed_time(stop) / n, n


def scan_hash():
    """sha256 (16 hex digits) over the scan's own sources: bench.source_hash() covers the MPC kernels only."""
    h = hashlib.sha256()
    for rel in SCAN_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def torch_scan(sim, scan, fx, fy, robot):
    """The scan of sim.state from torch operations and one ground_height launch: what rg_scan_observe_kernel fuses."""
    st = sim.state
    qx, qy, qz, qw = st[3], st[4], st[5], st[6]
    c0, s0 = 1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy + qz * qw)
    n = torch.sqrt(c0 * c0 + s0 * s0)
    ok = n > 0
    c, s = torch.where(ok, c0 / n, torch.ones_like(n)), torch.where(ok, s0 / n, torch.zeros_like(n))
    X = st[0][None, :] + (c[None, :] * fx - s[None, :] * fy)
    Y = st[1][None, :] + (s[None, :] * fx + c[None, :] * fy)
    h = sim.ground_height(torch.stack([X.reshape(-1), Y.reshape(-1)], dim=1), robot).view(X.shape)
    d = (st[2] - scan.z_offset)[None, :] - h
    return (torch.clamp(d, -scan.clip, scan.clip) * scan.scale).to(torch.float32)


def observe_rows(B, dev, cfg, seconds):
    """us per call of the kernel and of the torch composition on each ground, from the same poses."""
    rng = np.random.default_rng(B)
    xy, yaw = rng.uniform(-5.0, 5.0, (B, 2)), rng.uniform(-np.pi, np.pi, B)
    grounds = dict(plane=None, random=RandomTerrain(), grid=GridTerrain(rng.uniform(0.0, 0.06, (256, 256)), 0.05, (-6.4, -6.4)))
    out = {}
    for name, terrain in grounds.items():
        sim = BatchedSRBSim(B, cfg, device=dev, terrain=terrain)
        sim.reset(xy=xy, yaw=yaw)
        scan = HeightScan().bind(sim)
        pts = torch.as_tensor(scan.points, device=dev)
        fx, fy = pts[:, 0:1].contiguous(), pts[:, 1:2].contiguous()
        robot = torch.arange(B, dtype=torch.int32, device=dev).repeat(scan.num_points)
        buf = torch.zeros(scan.num_points, B, dtype=torch.float32, device=dev)
        worst = float((scan.observe(sim.state, out=buf) - torch_scan(sim, scan, fx, fy, robot)).abs().max())
        out[f"{name}_us"], out["calls"] = timed(lambda: scan.observe(sim.state, out=buf), seconds)
        out[f"{name}_torch_us"], _ = timed(lambda: torch_scan(sim, scan, fx, fy, robot), seconds)
        out[f"{name}_max_abs_diff"] = worst
        scan.close()
        sim.close()
    return out


def env_rows(B, dev, seconds):
    """us per BatchedGoEnv.step with and without the scan: without, with, without, with."""
    make = lambda scan: BatchedGoEnv(B, device=dev, auto_reset=True, terrain=RandomTerrain(), contact="measured", seed=3, height_scan=scan)
    plain, scanned = make(None), make(HeightScan())
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    out = {}
    for env in (plain, scanned):
        env.reset()
    for name, env in (("step_us", plain), ("step_scan_us", scanned), ("step_again_us", plain), ("step_scan_again_us", scanned)):
        out[name], _ = timed(lambda: env.step(action), seconds)
    out["resets_per_robot"] = round(float(scanned.episode_count.double().mean()), 2)
    for env in (plain, scanned):
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
        row = dict(batch=B, points=HeightScan().num_points)
        row.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in observe_rows(B, dev, cfg, args.seconds).items()})
        row.update({k: round(v, 2) for k, v in env_rows(B, dev, args.seconds).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = dict(what="terrain height scan, default 8 x 6 points: rg_scan_observe on the plane, the random terrain (amplitude 0.06, cell 0.05, one "
                       "world per robot) and a 256 x 256 grid, next to the same scan composed from torch operations and ground_height; "
                       "BatchedGoEnv.step (random terrain, measured contact, auto-reset) without and with the scan, alternated twice",
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), scan_source_sha256=scan_hash(),
                  device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
