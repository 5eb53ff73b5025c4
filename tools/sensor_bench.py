"""Times the sensor and actuator model (include/rg_sensor.h), in one process and run, at batch 64, 4096 and 32768 with D = 64
(16 path rows and 48 scan rows, both groups with every effect on), A = 2 and Lo = La = 4: the three kernels on their own (a reset
of every robot, the same launch with an empty mask, observe, act); the observe step composed from torch operations with a
torch generator standing in for the hash (the route a user had before the kernel); next to them, as yardsticks from the same
run, the randomiser's push kernel and the height scan on the random terrain; and BatchedGoEnv.step (random terrain, measured
contact, height scan, auto-reset) without a sensor model, with the default one (its launches run and copy bits) and with every
effect on, alternated twice so that the file carries the run-to-run spread.  hipEvents around at least --seconds of calls after
a warm-up, one synchronisation at the end of each measurement.  For the record, not a gate.

    python tools/sensor_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/sensor_tick.json]

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/sensor_bench.py --batches 4096
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
from robot_gym_amd.sim import BatchedSRBSim, DomainRandomizer, RandomTerrain, SensorModel  # noqa: E402
from robot_gym_amd.sim.height_scan import HeightScan  # noqa: E402
from tools.scan_bench import timed  # noqa: E402

SENSOR_SOURCES = ("robot_gym_amd/csrc/rg_sensor.hip", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_host.h", "include/rg_sensor.h")
PATH = dict(noise_sigma=0.004, bias_half_width=0.01, dropout_probability=0.05, dropout_value=0.0, quantum=0.001)
SCAN = dict(noise_sigma=0.01, bias_half_width=0.02, dropout_probability=0.02, dropout_value=1.0, quantum=0.005)
SETTINGS = dict(path=PATH, scan=SCAN, obs_delay=(0, 3), act_delay=(0, 3), act_noise_sigma=(0.02, 0.05), seed=1)
D, A, PATH_ROWS = 64, 2, 16


def sensor_hash():
    """sha256 (16 hex digits) over the unit's own sources: bench.source_hash() covers the MPC kernels only."""
    h = hashlib.sha256()
    for rel in SENSOR_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def torch_observe(clean, ring, out, ticks, delay, bias, gen):
    """The observe step from torch operations: what rg_sensor_observe_kernel fuses.  torch.rand stands in for the hash (five
    uniforms a row), the bias is stored instead of recomputed; the arithmetic is float64 like the kernel's."""
    Lo = ring.shape[0]
    x = clean.double()
    sigma, quantum, prob, dropv = (torch.cat([x.new_full((PATH_ROWS, 1), PATH[f]), x.new_full((D - PATH_ROWS, 1), SCAN[f])])
                                   for f in ("noise_sigma", "quantum", "dropout_probability", "dropout_value"))
    u = torch.rand((5,) + tuple(x.shape), dtype=torch.float64, device=x.device, generator=gen)
    x = x + bias
    x = x + sigma * ((((u[0] + u[1]) + (u[2] + u[3])) - 2.0) * 1.7320508075688772)
    x = quantum * torch.round(x / quantum)
    x = torch.where(u[4] < prob, dropv.expand_as(x), x).float()
    cols = torch.arange(x.shape[1], device=x.device)
    ring[ticks % Lo, :, cols] = x.t()
    out.copy_(ring[(ticks + Lo - delay) % Lo, :, cols].t())
    ticks += 1
    return out


def kernel_rows(B, dev, cfg, seconds):
    """us per call of each kernel, of the torch composition and of the two yardsticks."""
    sm = SensorModel(**SETTINGS).bind(B, dev, D, A, path_rows=(0, PATH_ROWS), scan_rows=(PATH_ROWS, D))
    gen = torch.Generator(device=dev).manual_seed(0)
    clean = torch.randn(D, B, device=dev, generator=gen)
    action = torch.rand(B, A, device=dev, generator=gen)
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    zeros = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {}
    out["reset_us"], out["calls"] = timed(lambda: sm.on_reset(ones, clean, prev=sm.final_obs), seconds)
    out["reset_nobody_us"], _ = timed(lambda: sm.on_reset(zeros, clean, prev=sm.final_obs), seconds)
    out["observe_us"], _ = timed(lambda: sm.observe(clean), seconds)
    out["act_us"], _ = timed(lambda: sm.act(action), seconds)
    ring, delivered = torch.zeros_like(sm.obs_ring), torch.zeros_like(sm.obs_out)
    ticks = torch.zeros(B, dtype=torch.int64, device=dev)
    delay = sm.delays[0].to(torch.int64)
    bias = torch.rand(D, B, dtype=torch.float64, device=dev, generator=gen) * 0.02 - 0.01
    out["observe_torch_us"], _ = timed(lambda: torch_observe(clean, ring, delivered, ticks, delay, bias, gen), seconds)
    sm.close()
    # yardsticks of the same run: the randomiser's push and the height scan on the random terrain
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain())
    sim.reset()
    dr = DomainRandomizer(seed=1, push_interval=100, push_ticks=10, push_probability=0.5, push_force_xy=20.0).bind(sim)
    dr.on_reset(ones)
    out["dr_push_us"], _ = timed(dr.pushes, seconds)
    scan = HeightScan().bind(sim)
    buf = torch.zeros(scan.num_points, B, dtype=torch.float32, device=dev)
    out["scan_us"], _ = timed(lambda: scan.observe(sim.state, out=buf), seconds)
    scan.close()
    dr.close()
    sim.close()
    return out


def env_rows(B, dev, seconds):
    """us per BatchedGoEnv.step without a sensor model, with the default one and with every effect on: the three, then again."""
    make = lambda sm: BatchedGoEnv(B, device=dev, auto_reset=True, terrain=RandomTerrain(), contact="measured", seed=3, height_scan=HeightScan(),   # noqa: E731
                                   sensor_model=sm)
    plain, ident, full = make(None), make(SensorModel()), make(SensorModel(**SETTINGS))
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    out = {}
    for env in (plain, ident, full):
        env.reset()
    for name, env in (("step_us", plain), ("step_default_us", ident), ("step_sensor_us", full), ("step_again_us", plain), ("step_default_again_us", ident),
                      ("step_sensor_again_us", full)):
        out[name], _ = timed(lambda: env.step(action), seconds)
    out["resets_per_robot"] = round(float(full.episode_count.double().mean()), 2)
    out["fallen_plain"], out["fallen_sensor"] = int(plain.sim.fallen().sum()), int(full.sim.fallen().sum())
    for env in (plain, ident, full):
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
    result = dict(what="sensor and actuator model: rg_sensor_reset (every robot, with prev), the same launch with an empty mask, rg_sensor_observe and "
                       "rg_sensor_act on their own at D = 64 (16 + 48 rows, both groups with every effect on), A = 2, Lo = La = 4; the observe step composed "
                       "from torch operations with torch.rand for the hash; rg_dr_push and the height scan on the random terrain as yardsticks; "
                       "BatchedGoEnv.step (random terrain, measured contact, height scan, auto-reset) without a sensor model, with the default one and "
                       "with every effect on, alternated twice",
                  settings={k: list(v) if isinstance(v, tuple) else v for k, v in SETTINGS.items()}, robot=args.robot, commit=commit, dirty=dirty,
                  source_hash=bench.source_hash(), sensor_source_sha256=sensor_hash(), device=torch.cuda.get_device_name(0),
                  seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
