"""Times the PPO update on both paths -- DevicePPO.update (HIP kernels, include/rg_ppo.h) and PPO.update (torch autograd and
Adam) -- on one fixed rollout with the default networks and 50 + 50 epochs, at batch 64, 4096 and 32768 with T = 32, next to
one collection of that rollout.  One measurement is one whole update between two hipEvents with one synchronisation; the two
paths are alternated `--repeats` times and the medians are reported with their spread.  Every batch runs in a child
process of its own under a time limit (`--limit` seconds): a step that hangs ends there and nothing more is started.  For the
record, not a gate.

    python tools/ppo_update_bench.py [--batches 64,4096,32768] [--repeats 5] [--out profiles/ppo_update.json]

Both updates start every measurement from the same parameters and optimiser state, restored in place before the first event
(Adam's moments and step counts zeroed, the parameters copied back), so each repeat does the same arithmetic and neither
path allocates inside a measurement.  The sweep's arithmetic is counted from the shapes: a sample's multiply-adds are
sum(in * out) over a network's layers; the policy epoch runs that three times forward-and-backward (forward, dX, dW) plus
one forward-only sweep, the value epoch three times.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

T_ROLLOUT = 32


def _hash(paths):
    h = hashlib.sha256()
    for rel in paths:
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


SHARED = ("robot_gym_amd/csrc/rg_agent_dev.inc", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_host.h")   # what the agents' files include


def policy_hash():
    return _hash(("robot_gym_amd/csrc/rg_policy.hip",) + SHARED + ("include/rg_policy.h",))


def ppo_hash():
    return _hash(("robot_gym_amd/csrc/rg_ppo.hip", "robot_gym_amd/csrc/rg_ppo_dev.inc") + SHARED + ("include/rg_ppo.h",))


def _once(fn, restore):
    """ms of one fn() on the current stream: restore, event, fn, event, one synchronisation."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    restore()
    start.record()
    fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def measure(B, repeats, robot):
    from robot_gym_amd.agents.ppo import PPO, BatchedGaussianPolicy, DevicePPO, RolloutBuffer, collect
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(robot, vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
    env = BatchedGoEnv(B, cfg, seed=B, device=dev, auto_reset=True, max_time=1e9, max_track_err=10.0, progress_limit=1e9)
    env.reset()
    policy = BatchedGaussianPolicy(B, seed=B, device=dev)
    ro = RolloutBuffer(T_ROLLOUT, B, device=dev)
    collect(env, policy, ro)                      # warm-up; the rollout both updates run on is the next one
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    collect_ms = []
    for _ in range(3):
        start.record()
        collect(env, policy, ro)
        stop.record()
        torch.cuda.synchronize()
        collect_ms.append(start.elapsed_time(stop))
    device_ppo, torch_ppo = DevicePPO(policy, T_ROLLOUT), PPO(policy)
    params = (policy.policy_params.detach().clone(), policy.value_params.detach().clone())
    opt0 = device_ppo.opt_state.clone()

    def restore_device():
        with torch.no_grad():
            policy.policy_params.copy_(params[0]), policy.value_params.copy_(params[1])
        device_ppo.opt_state.copy_(opt0)

    def restore_torch():
        # in place, like the device path's: Adam's state tensors exist from the warm-up on, so no timed update allocates them
        with torch.no_grad():
            policy.policy_params.copy_(params[0]), policy.value_params.copy_(params[1])
            for opt in (torch_ppo.policy_opt, torch_ppo.value_opt):
                for state in opt.state.values():
                    for v in state.values():
                        if torch.is_tensor(v):
                            v.zero_()
                        else:
                            raise RuntimeError("this torch keeps Adam's step count outside a tensor; restore it here")
        torch_ppo.penalty = 1.0

    _once(lambda: device_ppo.update(ro), restore_device)      # warm-up of both paths
    _once(lambda: torch_ppo.update(ro), restore_torch)
    runs = dict(device_ms=[], torch_ms=[])
    for _ in range(repeats):                                  # alternated: the host is shared, a drift hits both alike
        runs["device_ms"].append(_once(lambda: device_ppo.update(ro), restore_device))
        runs["torch_ms"].append(_once(lambda: torch_ppo.update(ro), restore_torch))
    stats = device_ppo.stats_dict()
    lay = policy.layout
    macs_p = sum(i * o for i, o, _, _ in lay["policy"])
    macs_v = sum(i * o for i, o, _, _ in lay["value"])
    N = T_ROLLOUT * B
    flop = 2.0 * N * (50 * (macs_p * 4) + 50 * (macs_v * 3))
    med = {k: statistics.median(v) for k, v in runs.items()}
    cms = statistics.median(collect_ms)
    row = dict(batch=B, T=T_ROLLOUT, samples=N, device_ms=round(med["device_ms"], 3), torch_ms=round(med["torch_ms"], 3),
               spread={k: [round(min(v), 3), round(max(v), 3)] for k, v in runs.items()}, device_over_torch=round(med["device_ms"] / med["torch_ms"], 4),
               collect_ms=round(cms, 3), update_share_of_collect_plus_update=round(med["device_ms"] / (med["device_ms"] + cms), 4),
               sweep_flop=flop, device_tflops=round(flop / (med["device_ms"] * 1e-3) * 1e-12, 2), groups=device_ppo._handle.groups,
               workspace_mb=round(device_ppo._handle.workspace_bytes / 2 ** 20, 1), device=torch.cuda.get_device_name(0), stats=stats)
    env.close(), device_ppo.close(), policy.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="64,4096,32768")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a batch's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print("ROW " + json.dumps(measure(args.child, args.repeats, args.robot)), flush=True)
        return 0
    rows = []
    for B in [int(x) for x in args.batches.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", str(B), "--repeats", str(args.repeats),
               "--robot", args.robot]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
            print(f"batch {B}: exit status {res.returncode}; stopping", file=sys.stderr)
            return res.returncode
        row = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])
        print(json.dumps(row), flush=True)
        rows.append(row)
    commit, dirty = bench.git_head()
    result = dict(what="PPO update, one MI355X, ms per whole update (default networks, 50 + 50 full-batch epochs, T = 32) on one fixed rollout: "
                       "DevicePPO.update (HIP, rg_ppo.h) and PPO.update (torch), alternated, medians with [min, max] in spread; collect_ms is one "
                       "collection of the rollout; device_tflops counts 2 x samples x (50 x 4 x policy + 50 x 3 x value multiply-adds) over "
                       "device_ms.  `commit` is the commit the measured tree was based on",
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), policy_source_sha256=policy_hash(),
                  ppo_source_sha256=ppo_hash(), repeats=args.repeats, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
