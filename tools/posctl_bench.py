#!/usr/bin/env python3
"""Timing of the position-mode controllers (include/rg_posctl.h); prints one JSON line.

  bezier_us / pose_us  hipEvent time per control tick (elapsed between two events around TICKS back-to-back launches, after
                       WARMUP), params and clocks different on every tick (all staged on the device beforehand), at B = 1,
                       4096 and 32768
  robot_ticks_per_s    B / that time
  dropin_*             host wall time of the batch-1 drop-in BezierController.update_controller_params + get_action
                       (p50 and mean, microseconds), with a fake clock

Usage: python tools/posctl_bench.py [--ticks 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.controllers.bezier.batched import BatchedBezierController  # noqa: E402
from robot_gym_amd.controllers.bezier.bezier_controller import BezierController  # noqa: E402
from robot_gym_amd.controllers.pose.batched import BatchedPoseController  # noqa: E402
from robot_gym_amd.core.posctl_config import PosCtlConfig  # noqa: E402


def _inputs(B, n, dev, rng):
    params = np.empty((n, 4, B), dtype=np.float32)
    params[:, 0] = rng.uniform(-1.5, 1.5, (n, B))
    params[:, 1] = rng.uniform(-180, 180, (n, B))
    params[:, 2] = rng.uniform(-1.5, 1.5, (n, B))
    params[:, 3] = rng.uniform(0.2, 0.6, (n, B))
    clocks = 0.01 * np.arange(1, n + 1)[:, None] + rng.uniform(0, 0.005, (n, B))
    pose = rng.uniform(-0.2, 0.2, (n, 6, B)).astype(np.float32)
    return (torch.as_tensor(params, device=dev), torch.as_tensor(clocks, device=dev), torch.as_tensor(pose, device=dev))


def time_batch(B, ticks, warmup, dev):
    rng = np.random.default_rng(B)
    n = ticks + warmup
    params, clocks, pose = _inputs(B, n, dev, rng)
    bz = BatchedBezierController(B, device=dev)
    ps = BatchedPoseController(B, device=dev)
    h, hp = bz._handle, ps._handle
    sp, ap = bz.state.data_ptr(), bz._angles.data_ptr()
    pp = [(params[k].data_ptr(), clocks[k].data_ptr(), pose[k].data_ptr()) for k in range(n)]
    out = {}
    for name, call in (("bezier", lambda k: h.bezier_step(0.0, pp[k][1], pp[k][0], sp, ap)),
                       ("pose", lambda k: hp.pose(pp[k][2], ps._angles.data_ptr()))):
        for k in range(warmup):
            call(k)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for k in range(warmup, n):
            call(k)
        e1.record()
        e1.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / ticks
        out[f"{name}_us"] = round(us, 3)
        out[f"{name}_robot_ticks_per_s"] = round(B / (us * 1e-6), 1)
    assert bool(torch.isfinite(bz.state).all())
    return out


def time_dropin(ticks, warmup, dev):
    cfg = PosCtlConfig.for_robot("ghost")
    clock = types.SimpleNamespace(now=0.0)
    c = BezierController(types.SimpleNamespace(), lambda: clock.now, device=dev, config=cfg)
    rng = np.random.default_rng(3)
    samples = []
    for k in range(warmup + ticks):
        clock.now = 0.01 * (k + 1)
        p = (float(rng.uniform(-1, 1)), float(rng.uniform(-90, 90)), float(rng.uniform(-1, 1)), 0.4)
        t = time.perf_counter()
        c.update_controller_params(p)
        c.get_action()
        if k >= warmup:
            samples.append(1e6 * (time.perf_counter() - t))
    return {"dropin_p50_us": round(float(np.percentile(samples, 50)), 1), "dropin_mean_us": round(float(np.mean(samples)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posctl_bench needs a GPU")
    dev = torch.device("cuda", 0)
    res = {"what": "rg_posctl per control tick", "ticks": a.ticks, "warmup": a.warmup, "evidence": bench.evidence_header(),
           "device": torch.cuda.get_device_name(dev)}
    for B in (1, 4096, 32768):
        res[f"B{B}"] = time_batch(B, a.ticks, a.warmup, dev)
    res["dropin_batch1"] = time_dropin(a.ticks, a.warmup, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
