#!/usr/bin/env python3
"""What per-robot body rows (rg_mpc_set_body) cost the batch-4096 / horizon-10 tick: the same synthetic workload in three
states of one handle -- no rows (the config's kernels), rows equal to the config (the per-robot path, same QPs), randomised rows
(mass +-25 %, inertia diagonal +-30 %, body height 0.36-0.44, mu 0.3-0.9 per leg) -- timed back to back, each as the median of
`--reps` windows of `--steps` ticks, with the front kernel's share from the library's event timing.  Prints one JSON line.
Usage: tools/body_rows_bench.py [--batch 4096] [--steps 200] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from robot_gym_amd import synthetic
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.core.config import MPCConfig
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    B = a.batch
    cfg = MPCConfig.for_robot("ghost")
    state, cmd, t_off = synthetic.make_states(B, cfg, seed=a.seed)
    dev = torch.device("cuda:0")
    ctl = BatchedMPCController(B, cfg, device=dev, extra_outputs=False)
    ctl.reset_at(-t_off)
    ctl.update_controller_params(torch.from_numpy(cmd.T.copy()).to(dev))
    # a ring of 20 slabs of perturbed states and gait-consistent contacts, resident on the device
    ring = []
    for k in range(20):
        st = {n: np.ascontiguousarray(v) for n, v in state.items() if n != "_flip"}
        f = np.float32(1.0 + 0.1 * np.sin(0.7 * k))
        st["v_world"] = (st["v_world"] * f).astype(np.float32)
        st["contact"] = synthetic.gait_consistent_contacts(cfg, 0.01 * k + t_off, state["_flip"])
        ring.append({n: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for n, v in st.items()})

    rng = np.random.default_rng(a.seed)
    I0 = np.array(cfg.inertia, dtype=np.float64)
    inertia = np.repeat(I0[:, None], B, 1)
    for d in (0, 4, 8):
        inertia[d] *= rng.uniform(0.7, 1.3, B)
    same = dict(mass=np.full(B, cfg.mass), inertia=np.repeat(I0[:, None], B, 1), body_height=np.full(B, cfg.body_height),
                mu=np.repeat(np.array(cfg.mu, dtype=np.float64)[:, None], B, 1), hip=np.repeat(np.array(cfg.hip)[:, None], B, 1))
    rand = dict(mass=cfg.mass * rng.uniform(0.75, 1.25, B), inertia=inertia, body_height=rng.uniform(0.36, 0.44, B),
                mu=rng.uniform(0.3, 0.9, (4, B)), hip=same["hip"])
    tick = [0]

    def run(n):
        for _ in range(n):
            ctl.get_action(0.01 * tick[0], ring[tick[0] % len(ring)])
            tick[0] += 1

    def measure(label, rows):
        if rows is None:
            ctl.set_body()
        else:
            ctl.set_body(**rows)
        run(50)   # warm-up: warm starts and cost classes settle on this state
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(a.steps)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / a.steps)
        ctl._handle.profile_begin(a.steps)
        ctl._handle.profile_stride(4)
        run(a.steps)
        n, ms, _ = ctl._handle.profile_end(ctl._stream())
        stats = ctl.solver_stats()
        return {"tick_us": float(np.median(times)), "tick_us_all": [round(t, 2) for t in times], "front_us": ms[0] * 1e3,
                "plan_body": ctl._handle.plan()["body"], "failures": stats["failures"], "iters_mean": stats["iters_mean"]}

    res = {"no_rows": measure("no_rows", None), "rows_equal_config": measure("same", same), "random_rows": measure("random", rand),
           "no_rows_again": measure("no_rows", None)}
    base = 0.5 * (res["no_rows"]["tick_us"] + res["no_rows_again"]["tick_us"])
    out = {"metric": "per-robot body rows: tick time at batch %d, horizon 10" % B, "batch": B, "steps": a.steps, "reps": a.reps,
           "states": res, "rows_equal_config_ratio": res["rows_equal_config"]["tick_us"] / base,
           "random_rows_ratio": res["random_rows"]["tick_us"] / base, "audit": ctl.audit_stats()}
    ctl.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
