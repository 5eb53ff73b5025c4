#!/usr/bin/env python3
"""What saving, restoring and copying controller state costs (rg_mpc_save_state / rg_mpc_load_state / rg_mpc_copy_state): for
each batch, a handle is stepped a few ticks on the synthetic workload (so that warm starts and working sets are filled), then
every robot's row is saved to the host, loaded back, and copied on the device (a random permutation), each timed as the median
of `--reps` calls, wall clock: save and load with their host copies and the wait, copy up to a synchronisation of the stream
(the call itself does not wait).  The tick of the same handle is timed for scale.  Prints one JSON line per batch.
Usage: tools/state_bench.py [--batches 4096,32768] [--reps 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from robot_gym_amd import synthetic
    from robot_gym_amd.controllers.mpc.batched import BatchedMPCController
    from robot_gym_amd.core.config import MPCConfig
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4096,32768")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=10)
    a = ap.parse_args()
    cfg = MPCConfig.for_robot("ghost")
    dev = torch.device("cuda:0")
    for B in (int(x) for x in a.batches.split(",")):
        state, cmd, t_off = synthetic.make_states(B, cfg, seed=1)
        ctl = BatchedMPCController(B, cfg, device=dev, extra_outputs=False)
        ctl.reset_at(-t_off)
        ctl.update_controller_params(torch.from_numpy(cmd.T.copy()).to(dev))
        inp = {n: torch.from_numpy(np.ascontiguousarray(state[n])).to(dev) for n in ("rpy", "rpy_rate", "v_world", "quat", "q", "foot_pos", "jac")}
        ticks = []
        for k in range(a.ticks):
            inp["contact"] = torch.from_numpy(synthetic.gait_consistent_contacts(cfg, 0.01 * k + t_off, state["_flip"])).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctl.get_action(0.01 * k, inp)
            torch.cuda.synchronize()
            ticks.append(time.perf_counter() - t0)
        save, load, copy = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            st = ctl.save_state()
            save.append(time.perf_counter() - t0)
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctl.load_state(st)
            load.append(time.perf_counter() - t0)
        perm = np.random.default_rng(0).permutation(B)
        ctl.copy_state(perm, np.arange(B))   # first call allocates the index buffers
        torch.cuda.synchronize()
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctl.copy_state(perm, np.arange(B))
            torch.cuda.synchronize()
            copy.append(time.perf_counter() - t0)
        ctl.close()
        med = lambda v: float(np.median(v)) * 1e6
        print(json.dumps({"batch": B, "row_bytes": st.row_bytes, "bytes_total": st.row_bytes * B, "tick_us": med(ticks[2:]),
                          "save_us": med(save), "load_us": med(load), "copy_us": med(copy), "reps": a.reps}), flush=True)


if __name__ == "__main__":
    main()
