"""Times the PPO agent's kernels next to the environment tick they ride on, in one process and run, at batch 1, 64, 4096 and
32768: rg_policy_act, rg_policy_record and rg_policy_returns alone; BatchedGoEnv.step alone; the collector's tick
(observation into the slot, act, env.step, record) with the act kernel; and the same tick with act replaced by the torch
path (normalize_obs + evaluate + torch.randn + the log probability, under no_grad).  hipEvents around at least `--seconds`
of calls after a warm-up, one synchronisation at the end of each measurement; the two ticks are alternated `--repeats` times
and the median is reported with its spread.  For the record, not a gate.

    python tools/policy_bench.py [--robot ghost] [--batches 1,64,4096,32768] [--seconds 0.5] [--out profiles/policy_tick.json]

The environment runs with auto-reset and its time, track and progress limits out of reach, so robots stay live under the
untrained policy's small random commands; `live` is the share not done on the last tick, `resets` the resets on the device
during the run.  The act kernel's arithmetic is counted from the shapes: multiply-adds per robot = sum of in * out over the
layers of both networks; weight bytes = 4 * the two parameter counts.

Kernel statistics come from a run of their own:  rocprofv3 --kernel-trace --stats -d DIR -- python tools/policy_bench.py --batches 4096
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.agents.ppo import BatchedGaussianPolicy, RolloutBuffer  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.gym.batched_go_env import BatchedGoEnv  # noqa: E402
from tools.srb_bench import timed  # noqa: E402

T_ROLLOUT = 32
LOG_2PI = math.log(2.0 * math.pi)


def policy_hash():
    h = hashlib.sha256()
    for rel in ("robot_gym_amd/csrc/rg_policy.hip", "robot_gym_amd/csrc/rg_agent_dev.inc", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_host.h",
                "include/rg_policy.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def torch_act(policy, obs_cm, out):
    """What rg_policy_act computes, as torch ops on the same tensors."""
    x = policy.normalize_obs(obs_cm.t())
    mean, value = policy.evaluate(x)
    logstd = policy.logstd
    eps = torch.randn(policy.batch, policy.act_dim, device=policy.device)
    torch.addcmul(mean, torch.exp(logstd), eps, out=out["action"])
    out["mean"].copy_(mean)
    out["value"].copy_(value)
    out["logprob"].copy_(-0.5 * (eps * eps).sum(-1) - logstd.sum() - 0.5 * policy.act_dim * LOG_2PI)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="1,64,4096,32768")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(args.robot, vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
    commit, dirty = bench.git_head()
    rows = []
    torch.set_grad_enabled(False)
    for B in [int(x) for x in args.batches.split(",")]:
        env = BatchedGoEnv(B, cfg, seed=B, device=dev, auto_reset=True, max_time=1e9, max_track_err=10.0, progress_limit=1e9)
        env.reset()
        policy = BatchedGaussianPolicy(B, seed=B, device=dev)
        ro = RolloutBuffer(T_ROLLOUT, B, device=dev)
        lay = policy.layout
        macs = sum(i * o for i, o, _, _ in lay["policy"] + lay["value"])
        k = [0]

        def outs(t):
            return dict(action=ro.action[t], mean=ro.mean[t], value=ro.value[t], logprob=ro.logprob[t])

        def tick(kernel):
            t = k[0] = (k[0] + 1) % T_ROLLOUT
            slot = ro.obs[t]
            slot.copy_(env.obs.t())
            if kernel:
                policy.act(slot, sample=True, out=outs(t))
            else:
                torch_act(policy, slot, outs(t))
            _, reward, done = env.step(ro.action[t])
            policy.record(slot, reward, done, None, ro_reward=ro.reward[t], ro_done=ro.done[t])

        for _ in range(args.warmup):
            tick(True)
            tick(False)
        runs = dict(tick_kernel_us=[], tick_torch_us=[])
        for _ in range(args.repeats):   # alternated: the host is shared, a drift hits both alike
            runs["tick_kernel_us"].append(timed(lambda: tick(True), args.seconds)[0])
            runs["tick_torch_us"].append(timed(lambda: tick(False), args.seconds)[0])
        live = float((env.done == 0).float().mean())
        resets = int(env.episode_count.sum())
        fallen = int(env.sim.fallen().sum())
        step_us, n = timed(lambda: env.step(ro.action[0]), args.seconds)
        obs0 = ro.obs[0]
        act_us, _ = timed(lambda: policy.act(obs0, sample=True, out=outs(0)), args.seconds / 2)
        act_torch_us, _ = timed(lambda: torch_act(policy, obs0, outs(0)), args.seconds / 2)
        record_us, _ = timed(lambda: policy.record(obs0, env.reward, env.done, None, ro_reward=ro.reward[0], ro_done=ro.done[0]), args.seconds / 2)
        returns_us, _ = timed(lambda: policy.returns(ro), args.seconds / 4)
        med = {name: round(statistics.median(v), 2) for name, v in runs.items()}
        rows.append(dict(batch=B, act_us=round(act_us, 2), act_torch_us=round(act_torch_us, 2), record_us=round(record_us, 2),
                         returns_T32_us=round(returns_us, 2), step_us=round(step_us, 2), **med,
                         spread={name: [round(min(v), 2), round(max(v), 2)] for name, v in runs.items()},
                         kernel_over_torch_tick=round(med["tick_kernel_us"] / med["tick_torch_us"], 4),
                         act_share_of_step=round(act_us / step_us, 4), act_and_record_share_of_step=round((act_us + record_us) / step_us, 4),
                         collector_robot_steps_per_s=round(B / med["tick_kernel_us"] * 1e6), macs_per_robot=macs,
                         act_gflops=round(2.0 * macs * B / act_us * 1e-3, 1), weight_bytes=4 * (lay["policy_count"] + lay["value_count"]),
                         live=round(live, 4), resets=resets, fallen=fallen))
        print(json.dumps(rows[-1]), flush=True)
        env.close()
        policy.close()
    result = dict(what="PPO agent kernels next to BatchedGoEnv.step, one process and run, us per call: act / record / returns (T = 32) alone, the "
                       "torch path of act alone, env.step alone (auto-reset, limits out of reach), and the collector's tick with the act kernel "
                       "and with the torch path (median of alternated repeats, [min, max] in spread).  `commit` is the commit the measured tree "
                       "was based on; policy_source_sha256 is the hash of rg_policy.hip, the two rg_agent_* files it includes and rg_policy.h as measured",
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), policy_source_sha256=policy_hash(),
                  device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, repeats=args.repeats, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
