"""Times the state estimator error model (include/rg_est.h), in one process and run, at batch 64, 4096 and 32768: the two kernels
on their own (a reset of every robot, the same launch with an empty mask, estimate with the default model -- every row copied --
and with every effect on); next to them, as a scale from the same run, the height scan on the random terrain and the sensor
model's observe at D = 64; and BatchedGoEnv.step (random terrain, measured contact, height scan, auto-reset) without an
estimator -- the step of the commit before this model, the same code path bit for bit -- with the default one (its launch runs
and copies bits) and with every effect on, alternated twice so that the file carries the run-to-run spread.  The extra cost of
the full model is split into the launch (default minus none) and the rest (full minus default): the kernel's own extra work
(estimate_full_us minus estimate_default_us) and the controller working on a perturbed state.  hipEvents around at least
--seconds of calls after a warm-up, one synchronisation at the end of each measurement.  For the record, not a gate.

    python tools/est_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/est_tick.json]

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/est_bench.py --batches 4096
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
from robot_gym_amd.sim import BatchedSRBSim, RandomTerrain, SensorModel, StateEstimator  # noqa: E402
from robot_gym_amd.sim.height_scan import HeightScan  # noqa: E402
from tools.scan_bench import timed  # noqa: E402
from tools.sensor_bench import D, A, PATH_ROWS, SETTINGS as SENSOR_SETTINGS  # noqa: E402

EST_SOURCES = ("robot_gym_amd/csrc/rg_est.hip", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_srb_dev.inc", "robot_gym_amd/csrc/rg_mpc_dev.h",
               "robot_gym_amd/csrc/rg_host.h", "include/rg_est.h")
FULL = dict(imu=dict(bias_half_width=(0.03, 0.03, 0.05), noise_sigma=(0.002, 0.002, 0.001)),
            gyro=dict(bias_half_width=(0.01, 0.01, 0.01), noise_sigma=(0.05, 0.05, 0.05)),
            velocity=dict(bias_half_width=(0.05, 0.05, 0.03), noise_sigma=(0.02, 0.02, 0.01)),
            encoders=dict(bias_half_width=0.01, noise_sigma=0.002, quantum=2.0 * np.pi / 4096.0),
            contact=dict(miss_probability=0.02, ghost_probability=0.005, rise_ticks=2), seed=1)


def est_hash():
    """sha256 (16 hex digits) over the unit's own sources: bench.source_hash() covers the MPC kernels only."""
    h = hashlib.sha256()
    for rel in EST_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def kernel_rows(B, dev, cfg, seconds):
    """us per call of each kernel and of the two yardsticks, on a simulator that stands after its reset."""
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain())
    sim.reset()
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    zeros = torch.zeros(B, dtype=torch.int32, device=dev)
    out = {}
    ident, full = StateEstimator().bind(sim), StateEstimator(**FULL).bind(sim)
    out["reset_us"], out["calls"] = timed(lambda: full.on_reset(ones), seconds)
    out["reset_nobody_us"], _ = timed(lambda: full.on_reset(zeros), seconds)
    ident.on_reset(ones)
    out["estimate_default_us"], _ = timed(ident.estimate, seconds)
    out["estimate_full_us"], _ = timed(full.estimate, seconds)
    ident.close()
    full.close()
    scan = HeightScan().bind(sim)
    buf = torch.zeros(scan.num_points, B, dtype=torch.float32, device=dev)
    out["scan_us"], _ = timed(lambda: scan.observe(sim.state, out=buf), seconds)
    scan.close()
    sim.close()
    sm = SensorModel(**SENSOR_SETTINGS).bind(B, dev, D, A, path_rows=(0, PATH_ROWS), scan_rows=(PATH_ROWS, D))
    clean = torch.randn(D, B, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    sm.on_reset(ones, clean)
    out["sensor_observe_us"], _ = timed(lambda: sm.observe(clean), seconds)
    sm.close()
    return out


def env_rows(B, dev, seconds):
    """us per BatchedGoEnv.step without an estimator, with the default one and with every effect on: the three, then again."""
    make = lambda est: BatchedGoEnv(B, device=dev, auto_reset=True, terrain=RandomTerrain(), contact="measured", seed=3, height_scan=HeightScan(),   # noqa: E731
                                    state_estimator=est)
    plain, ident, full = make(None), make(StateEstimator()), make(StateEstimator(**FULL))
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    out = {}
    for env in (plain, ident, full):
        env.reset()
    for name, env in (("step_us", plain), ("step_default_us", ident), ("step_est_us", full), ("step_again_us", plain), ("step_default_again_us", ident),
                      ("step_est_again_us", full)):
        out[name], _ = timed(lambda: env.step(action), seconds)
    none = 0.5 * (out["step_us"] + out["step_again_us"])
    default = 0.5 * (out["step_default_us"] + out["step_default_again_us"])
    est = 0.5 * (out["step_est_us"] + out["step_est_again_us"])
    out["extra_launch_us"], out["extra_rest_us"] = default - none, est - default
    out["resets_per_robot_plain"] = round(float(plain.episode_count.double().mean()), 2)
    out["resets_per_robot_est"] = round(float(full.episode_count.double().mean()), 2)
    out["fallen_plain"], out["fallen_est"] = int(plain.sim.fallen().sum()), int(full.sim.fallen().sum())
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
    result = dict(what="state estimator error model: rg_est_reset (every robot), the same launch with an empty mask, rg_est_estimate with the default model "
                       "(every row copied) and with every effect on; the height scan on the random terrain and the sensor model's observe (D = 64) as a "
                       "scale; BatchedGoEnv.step (random terrain, measured contact, height scan, auto-reset) without an estimator (the step of the "
                       "commit named here, which has no estimator), with the default one and with every effect on, alternated twice; extra_launch_us = "
                       "default - none and extra_rest_us = full - default, means of the two rounds.  commit is the HEAD the measured tree was built on; "
                       "est_source_sha256 is over the estimator's own sources as measured",
                  settings={g: ({k: list(v) if isinstance(v, tuple) else v for k, v in s.items()} if isinstance(s, dict) else s) for g, s in FULL.items()},
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), est_source_sha256=est_hash(),
                  device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
