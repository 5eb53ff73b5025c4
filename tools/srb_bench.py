"""Times the single-rigid-body simulator next to the controller, in one process and run: the controller-only tick (open loop
on a fixed observation), the simulator tick alone (fixed controller outputs) and the closed-loop tick (controller +
simulator through rollout), at batch 1, 1024, 4096 and 32768.  hipEvents around at least one second of ticks after a
warm-up, one synchronisation at the end of each measurement.  For the record, not a gate.

    python tools/srb_bench.py [--robot ghost] [--batches 1,1024,4096,32768] [--seconds 1.0] [--out profiles/srb_tick.json]

    python tools/srb_bench.py --terrain [--batches 1,64,1024,4096,32768] [--out profiles/srb_terrain_tick.json]

--terrain times the tick on the reference's random terrain next to the tick on the plane, in the same run and on the same
held controller outputs (the plane before and after the terrain, so that the file carries the plane's own run-to-run spread),
and a settle of the whole batch.

    python tools/srb_bench.py --contact [--batches 4096] [--out profiles/srb_contact_tick.json]

--contact times the tick with measured foot contact (contact="measured", rg_srb_step_contact) on the random terrain next to the
schedule tick on the same terrain and the tick on the plane, in the same run, from the same state and on the same held
controller outputs (the plane before and after, for the run-to-run spread).

    python tools/srb_bench.py --friction [--batches 64,4096,32768] [--out profiles/srb_friction_tick.json]

--friction times the tick with Coulomb friction (friction=, rg_srb_step_friction, measured contact) with every mu = +inf (every
robot grips) and with every mu = 0.3 next to the measured-contact tick and the schedule tick, on the plane and on the random
terrain, in the same run, from the same state and on the same held controller outputs.  No pass/fail ratio: these are
launch-bound kernels of a few microseconds.

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/srb_bench.py --batches 4096
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.controllers.mpc.batched import BatchedMPCController  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.sim import BatchedSRBSim, rollout  # noqa: E402


CLOCK_ROWS = 500


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


def srb_hash():
    """sha256 (16 hex digits) over the simulator's own sources: bench.source_hash() covers the MPC kernels only."""
    import hashlib
    h = hashlib.sha256()
    for rel in ("robot_gym_amd/csrc/rg_srb.hip", "robot_gym_amd/csrc/rg_srb_dev.inc", "robot_gym_amd/csrc/rg_srb_tick.inc", "robot_gym_amd/csrc/rg_srb_handle.h",
                "robot_gym_amd/csrc/rg_host.h",
                "robot_gym_amd/csrc/rg_srb_terrain.hip", "robot_gym_amd/csrc/rg_srb_ground.inc", "robot_gym_amd/csrc/rg_stream_dev.inc",
                "robot_gym_amd/csrc/rg_srb_contact.hip", "robot_gym_amd/csrc/rg_srb_friction.hip", "include/rg_srb.h", "include/rg_srb_terrain.h",
                "include/rg_srb_contact.h", "include/rg_srb_friction.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def terrain_rows(args, dev, cfg):
    """Per batch: the plane's tick, the terrain's tick, the plane's again, and settle(None), us per call."""
    from robot_gym_amd.sim.terrain import RandomTerrain
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(B)
        ctl = BatchedMPCController(B, cfg, device=dev)
        flat, rough = BatchedSRBSim(B, cfg, device=dev), BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain())
        cmd = np.stack([rng.uniform(-0.35, 0.35, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)], 1).astype(np.float32)
        hs = cfg.body_height * rng.uniform(0.9, 1.1, B)
        flat.reset(height=hs)
        rough.reset(height=hs)
        ctl.reset()
        ctl.update_controller_params(torch.as_tensor(cmd, device=dev))
        rollout(ctl, rough, None, args.warmup)                  # into the trot on the terrain: feet landing at their own heights
        fallen = int(rough.fallen().sum())
        flat.state.copy_(rough.state)                           # the same robots, the same held controller outputs, either ground
        keep = rough.state.clone()
        flat_a, n = timed(lambda: flat.step(ctl), args.seconds)
        rough_us, _ = timed(lambda: rough.step(ctl), args.seconds)
        flat.state.copy_(keep)
        flat_b, _ = timed(lambda: flat.step(ctl), args.seconds)
        # settle of a freshly reset batch: the state is put back before every call (a settle raises the body each time), and the
        # copy's own time is taken off
        rough.reset(height=hs)
        fresh = rough.state.clone()
        both_us, _ = timed(lambda: (rough.state.copy_(fresh), rough.settle()), args.seconds)
        copy_us, _ = timed(lambda: rough.state.copy_(fresh), args.seconds)
        settle_us = both_us - copy_us
        rows.append(dict(batch=B, ticks=n, flat_us=round(flat_a, 2), terrain_us=round(rough_us, 2), flat_again_us=round(flat_b, 2),
                         settle_us=round(settle_us, 2), fallen_in_warmup=fallen))
        print(json.dumps(rows[-1]), flush=True)
        for h in (ctl, flat, rough):
            h.close()
    return rows


def contact_rows(args, dev, cfg):
    """Per batch: the plane's tick, the terrain's schedule tick, the measured-contact tick on the terrain, the plane's again, us per
    call; every measurement starts from the state the warm-up (closed loop with measured contact on the terrain) ended in."""
    from robot_gym_amd.sim.terrain import RandomTerrain
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(B)
        ctl = BatchedMPCController(B, cfg, device=dev)
        flat, rough = BatchedSRBSim(B, cfg, device=dev), BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain())
        measured = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain(), contact="measured")
        cmd = np.stack([rng.uniform(-0.35, 0.35, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)], 1).astype(np.float32)
        hs = cfg.body_height * rng.uniform(0.9, 1.1, B)
        for sim in (flat, rough, measured):
            sim.reset(height=hs)
        ctl.reset()
        ctl.update_controller_params(torch.as_tensor(cmd, device=dev))
        rollout(ctl, measured, None, args.warmup)               # into the trot with measured contact: feet stopping at the ground
        fallen = int(measured.fallen().sum())
        touching = int(measured.touch.sum())
        keep = measured.state.clone()
        out = {}
        for name, sim in (("flat_us", flat), ("terrain_us", rough), ("contact_us", measured), ("flat_again_us", flat)):
            sim.state.copy_(keep)
            out[name], n = timed(lambda: sim.step(ctl), args.seconds)
        rows.append(dict(batch=B, ticks=n, **{k: round(v, 2) for k, v in out.items()}, fallen_in_warmup=fallen, feet_touching_at_start=touching))
        print(json.dumps(rows[-1]), flush=True)
        for h in (ctl, flat, rough, measured):
            h.close()
    return rows


def friction_rows(args, dev, cfg):
    """Per batch and ground (the plane, the random terrain): the friction tick with every mu = +inf, the friction tick with every
    mu = 0.3, the measured-contact tick and the schedule tick, us per call; every measurement starts from the state the warm-up
    (closed loop with measured contact and friction 0.3 on that ground) ended in, on the same held controller outputs."""
    from robot_gym_amd.sim.terrain import RandomTerrain
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        for ground in ("plane", "random"):
            rng = np.random.default_rng(B)
            terrain = lambda: RandomTerrain() if ground == "random" else None
            ctl = BatchedMPCController(B, cfg, device=dev)
            schedule = BatchedSRBSim(B, cfg, device=dev, terrain=terrain())
            contact = BatchedSRBSim(B, cfg, device=dev, terrain=terrain(), contact="measured")
            grips = BatchedSRBSim(B, cfg, device=dev, terrain=terrain(), contact="measured", friction="inf")
            slippery = BatchedSRBSim(B, cfg, device=dev, terrain=terrain(), contact="measured", friction=0.3)
            sims = (schedule, contact, grips, slippery)
            cmd = np.stack([rng.uniform(-0.35, 0.35, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)], 1).astype(np.float32)
            hs = cfg.body_height * rng.uniform(0.9, 1.1, B)
            for sim in sims:
                sim.reset(height=hs)
            ctl.reset()
            ctl.update_controller_params(torch.as_tensor(cmd, device=dev))
            slid = torch.zeros(B, dtype=torch.float64, device=dev)
            rollout(ctl, slippery, None, args.warmup, on_tick=lambda k: slid.add_(slippery.slip.sum(0)))   # into the trot on the slippery floor
            fallen, sliding = int(slippery.fallen().sum()), int((slid > 0).sum())
            keep = slippery.state.clone()
            out = {}
            for name, sim in (("friction_inf_us", grips), ("friction_0p3_us", slippery), ("contact_us", contact), ("schedule_us", schedule),
                              ("friction_inf_again_us", grips)):
                sim.state.copy_(keep)
                out[name], n = timed(lambda: sim.step(ctl), args.seconds)
            rows.append(dict(batch=B, ground=ground, ticks=n, **{k: round(v, 2) for k, v in out.items()}, fallen_in_warmup=fallen,
                             robots_that_slid_in_warmup=sliding))
            print(json.dumps(rows[-1]), flush=True)
            for h in (ctl,) + sims:
                h.close()
    return rows


def closed_loop_slid(robot, dev, friction, ticks=400):
    """The closed loop of tests/test_friction_gpu.py on a floor that holds twice what the planner believes: the 32 cases of
    tests/srb_fixtures.py, measured contact on the reference's random terrain -> robots that slid at all and the worst distance a
    robot's four feet slid, added up.  For the record: how closely the ADMM lane keeps the friction cone."""
    from robot_gym_amd.sim.terrain import RandomTerrain
    from tests import contact_fixtures as CF
    from tests import srb_fixtures as F
    cfg = MPCConfig.for_robot(robot)
    cmd, hs = F.cases(robot)
    B = len(hs)
    ctl = BatchedMPCController(B, cfg, device=dev)
    sim = BatchedSRBSim(B, cfg, device=dev, terrain=RandomTerrain(CF.AMPLITUDE, CF.CELL, CF.SEED), contact="measured", friction=friction)
    sim.reset(height=cfg.body_height * hs)
    ctl.reset()
    ctl.set_raw_command(torch.as_tensor(np.ascontiguousarray(cmd.T), device=dev))
    slid = torch.zeros(B, dtype=torch.float64, device=dev)
    rollout(ctl, sim, None, ticks, on_tick=lambda k: slid.add_(sim.slip.sum(0)))
    row = dict(robot=robot, friction=friction, ticks=ticks, robots=B, fallen=int(sim.fallen().sum()), robots_that_slid=int((slid > 0).sum()),
               worst_slid_m=float(slid.max()))
    print(json.dumps(row), flush=True)
    ctl.close()
    sim.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default=None, help="default 1,1024,4096,32768 (--terrain: 1,64,1024,4096,32768)")
    ap.add_argument("--terrain", action="store_true", help="the tick on the random terrain next to the tick on the plane, and settle")
    ap.add_argument("--contact", action="store_true", help="the measured-contact tick next to the terrain tick and the plane tick (batch 4096)")
    ap.add_argument("--friction", action="store_true", help="the friction tick (mu = +inf, mu = 0.3) next to the contact tick and the schedule tick "
                                                            "(batch 64, 4096, 32768; the plane and the random terrain)")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot)
    commit, dirty = bench.git_head()
    args.batches_given = args.batches is not None
    args.batches = args.batches or ("1,64,1024,4096,32768" if args.terrain else "1,1024,4096,32768")
    rows = []
    if args.friction:
        args.batches = args.batches if args.batches_given else "64,4096,32768"
        result = dict(what="simulator tick with Coulomb friction at the stance feet (measured contact; every mu = +inf, every mu = 0.3) next to the "
                           "measured-contact tick and the schedule tick, on the plane and on the random terrain (amplitude 0.06, cell 0.05, one world "
                           "per robot): same run, same start state, same held controller outputs; the +inf tick twice, for the run-to-run spread",
                      robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), srb_source_sha256=srb_hash(),
                      device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=friction_rows(args, dev, cfg))
        result["closed_loop_friction_0p9"] = [closed_loop_slid(robot, dev, 0.9) for robot in ("ghost", "k3lso")]
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        print(json.dumps(result))
        return
    if args.contact:
        args.batches = args.batches if args.batches_given else "4096"
        result = dict(what="simulator tick with measured foot contact on the random terrain (amplitude 0.06, cell 0.05, one world per robot) next to "
                           "the schedule tick on the same terrain and the tick on the plane: same run, same start state, same held controller outputs",
                      robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), srb_source_sha256=srb_hash(),
                      device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=contact_rows(args, dev, cfg))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        print(json.dumps(result))
        return
    if args.terrain:
        result = dict(what="simulator tick on the random terrain (amplitude 0.06, cell 0.05, one world per robot) next to the tick on the plane, "
                           "same run, same held controller outputs; settle of the whole batch", robot=args.robot, commit=commit, dirty=dirty,
                      source_hash=bench.source_hash(), srb_source_sha256=srb_hash(), device=torch.cuda.get_device_name(0),
                      seconds_per_measurement=args.seconds, rows=terrain_rows(args, dev, cfg))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
        print(json.dumps(result))
        return
    for B in [int(x) for x in args.batches.split(",")]:
        rng = np.random.default_rng(B)
        ctl, sim = BatchedMPCController(B, cfg, device=dev), BatchedSRBSim(B, cfg, device=dev)
        cmd = np.stack([rng.uniform(-0.35, 0.35, B), rng.uniform(-0.2, 0.2, B), rng.uniform(-0.4, 0.4, B)], 1).astype(np.float32)
        sim.reset(height=cfg.body_height * rng.uniform(0.9, 1.1, B))
        ctl.reset()
        ctl.update_controller_params(torch.as_tensor(cmd, device=dev))
        rollout(ctl, sim, None, args.warmup)                    # into the trot: the contact mix of a running batch
        closed_us, n = timed(lambda: (ctl.get_action(0.0, sim.obs), sim.step(ctl)), args.seconds)
        fallen = int(sim.fallen().sum())
        # the simulator alone: the controller's last outputs, held (the robots coast; their state stays finite or they freeze)
        sim_us, _ = timed(lambda: sim.step(ctl), args.seconds)
        sim.reset(height=cfg.body_height * rng.uniform(0.9, 1.1, B))
        ctl.reset()
        rollout(ctl, sim, None, args.warmup)
        obs = {k: v.clone() for k, v in sim.obs.items()}
        # the observation of one moment of the trot, held; the clock goes on from a table built before the timing starts, so
        # that the timed call is the controller's launches and nothing else.  CLOCK_ROWS ticks are a whole number of gait
        # cycles (stance_duration / duty_factor = 0.5 s), so the wrap leaves the gait phase continuous.
        clocks = (obs["t_robot"][None, :] + 0.01 * torch.arange(1, CLOCK_ROWS + 1, device=dev, dtype=torch.float64)[:, None]).contiguous()
        tick = [0]

        def ctl_only():
            obs["t_robot"] = clocks[tick[0] % CLOCK_ROWS]
            tick[0] += 1
            ctl.get_action(0.0, obs)
        ctl_us, _ = timed(ctl_only, args.seconds)
        rows.append(dict(batch=B, ticks=n, sim_us=round(sim_us, 2), ctl_us=round(ctl_us, 2), closed_us=round(closed_us, 2),
                         closed_robot_steps_per_s=round(B / closed_us * 1e6), fallen_during_timing=fallen))
        print(json.dumps(rows[-1]), flush=True)
        ctl.close()
        sim.close()
    result = dict(what="single-rigid-body simulator tick next to the controller tick, one process and run", robot=args.robot,
                  commit=commit, dirty=dirty, source_hash=bench.source_hash(), srb_source_sha256=srb_hash(), device=torch.cuda.get_device_name(0),
                  seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
