"""Times the recurrent policy's kernels, in one process and run, at batch 64, 4096 and 32768: rg_rnn_act; rg_policy_act on the
default feed-forward networks; the same GRU tick as torch ops (normalize_obs, the dense layer, the cell, the head, the value
network, torch.randn and the log probability, under no_grad); rg_rnn_unroll at T = 32 next to a no-grad torch loop over the
same sequence (RecurrentGaussianPolicy.evaluate_hidden and the head); and one collect_recurrent tick (observation into the
slot, act, env.step, pending_reset, record).  hipEvents around at least `--seconds` of calls after a warm-up, one
synchronisation at the end of each measurement.  For the record, not a gate: no target time is set.

    python tools/rnn_bench.py [--robot ghost] [--batches 64,4096,32768] [--seconds 0.5] [--out profiles/rnn_tick.json]

The tick's arithmetic is counted from the shapes: multiply-adds per robot = sum of in * out over the dense layers, W_ru,
W_c, the head and the value network; weight bytes = 4 * the two parameter counts.
"""
import argparse
import hashlib
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from robot_gym_amd.agents.ppo import BatchedGaussianPolicy, RecurrentGaussianPolicy, RecurrentRolloutBuffer  # noqa: E402
from robot_gym_amd.core.config import MPCConfig  # noqa: E402
from robot_gym_amd.gym.batched_go_env import BatchedGoEnv  # noqa: E402
from tools.srb_bench import timed  # noqa: E402

T_UNROLL = 32
LOG_2PI = math.log(2.0 * math.pi)


def rnn_hash():
    h = hashlib.sha256()
    for rel in ("robot_gym_amd/csrc/rg_rnn.hip", "robot_gym_amd/csrc/rg_agent_dev.inc", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_gru_dev.inc",
                "robot_gym_amd/csrc/rg_host.h", "include/rg_rnn.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def torch_tick(policy, obs_cm, out):
    """What rg_rnn_act computes, as torch ops on the same tensors (the state advanced in place)."""
    x = policy.normalize_obs(obs_cm.t()).unsqueeze(0)
    h = policy.evaluate_hidden(x, policy.pending_reset.unsqueeze(0), policy.hidden)[0]
    W, b = policy.head
    mean = torch.tanh(h @ W + b)
    value = policy.evaluate_value(x[0])
    logstd = policy.logstd
    eps = torch.randn(policy.batch, policy.act_dim, device=policy.device)
    torch.addcmul(mean, torch.exp(logstd), eps, out=out["action"])
    out["mean"].copy_(mean)
    out["value"].copy_(value)
    out["logprob"].copy_(-0.5 * (eps * eps).sum(-1) - logstd.sum() - 0.5 * policy.act_dim * LOG_2PI)
    policy.hidden.copy_(h)
    policy.pending_reset.zero_()


def torch_unroll(policy, ro, mean_out):
    x = policy.normalize_obs(ro.obs.permute(0, 2, 1))
    W, b = policy.head
    mean_out.copy_(torch.tanh(policy.evaluate_hidden(x, ro.reset, ro.h0) @ W + b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--batches", default="64,4096,32768")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=30)
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
        policy = RecurrentGaussianPolicy(B, seed=B, device=dev)
        forward = BatchedGaussianPolicy(B, seed=B, device=dev)
        ro = RecurrentRolloutBuffer(T_UNROLL, B, device=dev)
        lay = policy.layout
        macs = sum(i * o for i, o, _, _ in lay["dense"] + [lay["w_ru"], lay["w_c"], lay["head"]] + lay["value"])
        k = [0]

        def outs(t):
            return dict(action=ro.action[t], mean=ro.mean[t], value=ro.value[t], logprob=ro.logprob[t])

        def tick():
            t = k[0] = (k[0] + 1) % T_UNROLL
            slot = ro.obs[t]
            slot.copy_(env.obs.t())
            ro.reset[t].copy_(policy.pending_reset)
            policy.act(slot, sample=True, out=outs(t))
            _, reward, done = env.step(ro.action[t])
            policy.pending_reset.copy_(done)
            policy.record(slot, reward, done, None, ro_reward=ro.reward[t], ro_done=ro.done[t])

        for _ in range(max(args.warmup, T_UNROLL)):    # fills every slot of the rollout with observations of the environment
            tick()
        tick_us, _ = timed(tick, args.seconds)
        step_us, _ = timed(lambda: env.step(ro.action[0]), args.seconds)
        obs0 = ro.obs[0]
        act_us, _ = timed(lambda: policy.act(obs0, sample=True, out=outs(0)), args.seconds / 2)
        forward_us, _ = timed(lambda: forward.act(obs0, sample=True, out=outs(0)), args.seconds / 2)
        act_torch_us, _ = timed(lambda: torch_tick(policy, obs0, outs(0)), args.seconds / 2)
        ro.h0.copy_(policy.hidden)
        mean = torch.zeros_like(ro.mean)
        unroll_us, _ = timed(lambda: policy.unroll(ro, out=dict(mean=mean)), args.seconds / 2)
        kernel_mean = mean.clone()
        unroll_torch_us, _ = timed(lambda: torch_unroll(policy, ro, mean), args.seconds / 2)
        rows.append(dict(batch=B, rnn_act_us=round(act_us, 2), forward_act_us=round(forward_us, 2), rnn_act_torch_us=round(act_torch_us, 2),
                         unroll_T32_us=round(unroll_us, 2), unroll_T32_torch_us=round(unroll_torch_us, 2), collect_tick_us=round(tick_us, 2),
                         step_us=round(step_us, 2), act_over_torch=round(act_us / act_torch_us, 4), unroll_over_torch=round(unroll_us / unroll_torch_us, 4),
                         act_over_forward=round(act_us / forward_us, 4), act_share_of_step=round(act_us / step_us, 4),
                         unroll_vs_torch_max_abs=float((kernel_mean - mean).abs().max()), macs_per_robot=macs,
                         act_gflops=round(2.0 * macs * B / act_us * 1e-3, 1), weight_bytes=4 * (lay["policy_count"] + lay["value_count"])))
        print(json.dumps(rows[-1]), flush=True)
        env.close()
        policy.close()
        forward.close()
    result = dict(what="recurrent policy kernels, one process and run, us per call: rg_rnn_act, rg_policy_act on the default feed-forward networks, "
                       "the GRU tick as torch ops, rg_rnn_unroll at T = 32 and a no-grad torch loop over the same sequence, one collect_recurrent "
                       "tick and env.step alone (auto-reset, limits out of reach).  `commit` is the commit the measured tree was based on; "
                       "rnn_source_sha256 is the hash of rg_rnn.hip, rg_agent_dev.inc, rg_stream_dev.inc, rg_gru_dev.inc and rg_host.h, which it includes, and rg_rnn.h as measured",
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), rnn_source_sha256=rnn_hash(),
                  device=torch.cuda.get_device_name(0), seconds_per_measurement=args.seconds, rows=rows)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
