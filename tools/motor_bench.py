"""Times the motor model (include/rg_srb_motor.h), in one process and run, at batch 64, 4096 and 32768: the apply kernel with the
default model (strength 1, no limit: every leg passes through) and with every leg saturated (strength 0.9: every stance leg takes
the solve), on the forces and joint angles of a trot; the draw of every robot's strengths; next to them, as the scale the other
device models use, the height scan on the random terrain; and BatchedGoEnv.step (auto-reset) without a model -- the step of the
commit before this model, the same code path -- with the default model (its launch runs and passes bits through) and with the
saturating one, alternated twice so that the file carries the run-to-run spread.  hipEvents around at least --seconds of calls
after a warm-up, one synchronisation at the end of each measurement.  For the record, not a gate: this is one launch more per tick.

    python tools/motor_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/motor_tick.json]

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/motor_bench.py --batches 4096
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
from robot_gym_amd.controllers.mpc.batched import BatchedMPCController  # noqa: E402
from robot_gym_amd.core import motor_abi  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.gym.batched_go_env import BatchedGoEnv  # noqa: E402
from robot_gym_amd.sim import BatchedSRBSim, MotorModel, RandomTerrain, rollout  # noqa: E402
from robot_gym_amd.sim.height_scan import HeightScan  # noqa: E402
from tools.scan_bench import timed  # noqa: E402

MOTOR_SOURCES = ("robot_gym_amd/csrc/rg_srb_motor.hip", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_srb_dev.inc",
                 "robot_gym_amd/csrc/rg_srb_handle.h", "robot_gym_amd/csrc/rg_mpc_dev.h", "robot_gym_amd/csrc/rg_host.h", "include/rg_srb_motor.h")
WEAK = 0.9        # the saturating model: every motor at nine tenths of its strength, so every stance leg is solved for


def motor_hash():
    """sha256 (16 hex digits) over the unit's own sources: bench.source_hash() covers the MPC kernels only."""
    h = hashlib.sha256()
    for rel in MOTOR_SOURCES:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def kernel_rows(B, dev, cfg, seconds, warmup):
    """us per call of the two kernels and of the yardstick, on the state and the held controller outputs of a trot."""
    rng = np.random.default_rng(B)
    ctl = BatchedMPCController(B, cfg, device=dev)
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain(), motors=MotorModel())
    cmd = np.stack([rng.uniform(-0.35, 0.35, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)], 1).astype(np.float32)
    sim.reset(height=cfg.body_height * rng.uniform(0.9, 1.1, B))
    ctl.reset()
    ctl.update_controller_params(torch.as_tensor(cmd, device=dev))
    rollout(ctl, sim, None, warmup)                                # into the trot: half the legs carry a force
    mot, grf = sim.motors, ctl.extra["grf"]
    out = dict(fallen_in_warmup=int(sim.fallen().sum()), legs_with_force=int((grf.view(B, 4, 3) != 0).any(2).sum()))
    out["apply_default_us"], out["calls"] = timed(lambda: mot.apply(grf), seconds)
    assert torch.equal(mot.grf, grf)
    mot.set_strength(WEAK)
    out["apply_saturated_us"], _ = timed(lambda: mot.apply(grf), seconds)
    out["legs_saturated"] = int((mot.tau != mot.tau_cmd).view(4, 3, B).any(1).sum())
    ones = torch.ones(B, dtype=torch.int32, device=dev)
    key = torch.arange(B, dtype=torch.float64, device=dev)
    draws = torch.zeros(B, dtype=torch.float64, device=dev)
    out["draw_us"], _ = timed(lambda: motor_abi.motor_draw(sim._handle, ones, key, draws, 1, 0.7, 1.0, mot.strength), seconds)
    scan = HeightScan().bind(sim)
    buf = torch.zeros(scan.num_points, B, dtype=torch.float32, device=dev)
    out["scan_us"], _ = timed(lambda: scan.observe(sim.state, out=buf), seconds)
    scan.close()
    ctl.close()
    sim.close()
    return out


def env_rows(B, dev, seconds):
    """us per BatchedGoEnv.step without a model, with the default one and with the saturating one: the three, then again."""
    make = lambda motors: BatchedGoEnv(B, device=dev, auto_reset=True, seed=3, motor_model=motors)   # noqa: E731
    plain, ident, weak = make(None), make(MotorModel()), make(MotorModel(strength=WEAK))
    action = torch.as_tensor(np.tile(np.array([[0.3, 0.1]], dtype=np.float32), (B, 1)), device=dev)
    out = {}
    for env in (plain, ident, weak):
        env.reset()
    for name, env in (("step_us", plain), ("step_default_us", ident), ("step_saturated_us", weak), ("step_again_us", plain),
                      ("step_default_again_us", ident), ("step_saturated_again_us", weak)):
        out[name], _ = timed(lambda: env.step(action), seconds)
    none = 0.5 * (out["step_us"] + out["step_again_us"])
    default = 0.5 * (out["step_default_us"] + out["step_default_again_us"])
    sat = 0.5 * (out["step_saturated_us"] + out["step_saturated_again_us"])
    out["extra_launch_us"], out["extra_rest_us"] = default - none, sat - default
    out["fallen_plain"], out["fallen_saturated"] = int(plain.sim.fallen().sum()), int(weak.sim.fallen().sum())
    for env in (plain, ident, weak):
        env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="64,4096,32768")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot)
    commit, dirty = bench.git_head()
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        row = dict(batch=B)
        row.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in kernel_rows(B, dev, cfg, args.seconds, args.warmup).items()})
        row.update({k: (round(v, 2) if k.endswith("_us") else v) for k, v in env_rows(B, dev, args.seconds).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = dict(what="motor model: rg_srb_motor_apply with the default model (every leg passes through) and with every motor at strength 0.9 (every "
                       "stance leg is solved for), on the state and held controller outputs of a trot; rg_srb_motor_draw for every robot; the height "
                       "scan on the random terrain as a scale; BatchedGoEnv.step (plane, schedule contact, auto-reset) without a model (the step of "
                       "the commit named here, which has no motor model), with the default one and with the saturating one, alternated twice; "
                       "extra_launch_us = default - none and extra_rest_us = saturated - default, means of the two rounds.  commit is the HEAD the "
                       "measured tree was built on; motor_source_sha256 is over the unit's own sources as measured",
                  strength_of_the_saturating_model=WEAK, robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(),
                  motor_source_sha256=motor_hash(), device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
