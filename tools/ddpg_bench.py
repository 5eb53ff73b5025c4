"""Times the DDPG update on both paths -- BatchedDDPGAgent.update (HIP kernels, include/rg_ddpg.h) and a plain torch update
written here (autograd, clip_grad_norm_, torch.optim.Adam, lerp_ for the targets) -- with the default networks at minibatches
of 32, 256 and 4096, and one collect tick at batch 4096 with 1 and with 8 updates per tick next to the bare env.step.  A
measurement is `--updates` updates (or `--ticks` ticks) enqueued back to back on one stream between two hipEvents with one
synchronisation, after a warm-up; the two paths are alternated `--repeats` times and the medians are reported with their spread.
Every step runs in a child process of its own under a time limit (`--limit` seconds): a step that hangs ends there and nothing
more is started.  For the record, not a gate.

    python tools/ddpg_bench.py [--minibatches 32,256,4096] [--repeats 5] [--out profiles/ddpg_update.json]

The torch update runs on ONE minibatch gathered before the clock starts (s0, s1, action, reward, not-done as dense tensors):
it is not charged for sampling or for the window gather, which the device path does inside every update.  The device path
samples anew each update.  Both paths do the same arithmetic per update otherwise: critic forward and backward on M samples,
the two target forwards, the actor forward and backward through the critic, two clipped Adam steps, two soft updates.
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

RING_BATCH, RING_TICKS = 64, 256


def ddpg_hash():
    h = hashlib.sha256()
    for rel in ("robot_gym_amd/csrc/rg_ddpg.hip", "robot_gym_amd/csrc/rg_agent_dev.inc", "robot_gym_amd/csrc/rg_stream_dev.inc", "robot_gym_amd/csrc/rg_host.h",
                "include/rg_ddpg.h"):
        h.update(open(os.path.join(ROOT, rel), "rb").read())
    return h.hexdigest()[:16]


def _timed(fn, n):
    """ms per call of n calls of fn() back to back on the current stream."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(n):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / n


class TorchDDPG:
    """The same update in torch on the agent's own layout: leaf buffers, views per layer, one gathered minibatch."""

    def __init__(self, agent, M):
        dev, f = agent.device, agent.fields
        self.f, self.lay = f, agent.layout
        self.actor, self.critic = agent.actor_params.clone().requires_grad_(True), agent.critic_params.clone().requires_grad_(True)
        self.t_actor, self.t_critic = agent.target_actor_params.clone(), agent.target_critic_params.clone()
        self.opt_a = torch.optim.Adam([self.actor], lr=f["actor_lr"], betas=(f["beta1"], f["beta2"]), eps=f["adam_eps"])
        self.opt_c = torch.optim.Adam([self.critic], lr=f["critic_lr"], betas=(f["beta1"], f["beta2"]), eps=f["adam_eps"])
        W, d, C = agent.window, agent.obs_dim, agent.capacity
        gen = torch.Generator(device="cpu").manual_seed(M)
        age = torch.randint(1, C - W, (M,), generator=gen).to(dev)      # complete windows: the ring is full and holds no done
        rob = torch.randint(0, agent.batch, (M,), generator=gen).to(dev)
        head = int(agent.ring_state[0])

        def state(a):
            k = torch.arange(W - 1, -1, -1, device=dev)                   # oldest first
            slots = (head - 1 - (a[:, None] + k[None, :])) % C
            return agent.ring_obs[slots, :, rob[:, None]].reshape(M, W * d)

        slot = (head - 1 - age) % C
        self.s0, self.s1 = state(age), state(age - 1)
        self.action, self.reward = agent.ring_action[slot, rob], agent.ring_reward[slot, rob]
        self.nd = (agent.ring_done[slot, rob] == 0).float()

    def net(self, p, which, x):
        layers = self.lay[which]
        for k, (i, o, w, b) in enumerate(layers):
            x = torch.addmm(p[b:b + o], x, p[w:w + i * o].view(i, o))
            if k < len(layers) - 1:
                x = torch.relu(x)
        return torch.tanh(x) if which == "actor" else x

    def update(self):
        f = self.f
        with torch.no_grad():
            a1 = self.net(self.t_actor, "actor", self.s1)
            y = self.reward + f["gamma"] * self.nd * self.net(self.t_critic, "critic", torch.cat([a1, self.s1], dim=1))[:, 0]
        self.opt_c.zero_grad(set_to_none=True)
        q = self.net(self.critic, "critic", torch.cat([self.action, self.s0], dim=1))[:, 0]
        (0.5 * (y - q) ** 2).mean().backward()
        torch.nn.utils.clip_grad_norm_([self.critic], f["clipnorm"])
        self.opt_c.step()
        self.opt_a.zero_grad(set_to_none=True)
        mu = self.net(self.actor, "actor", self.s0)
        (-self.net(self.critic.detach(), "critic", torch.cat([mu, self.s0], dim=1))[:, 0].mean()).backward()
        torch.nn.utils.clip_grad_norm_([self.actor], f["clipnorm"])
        self.opt_a.step()
        with torch.no_grad():
            self.t_actor.lerp_(self.actor, f["tau"])
            self.t_critic.lerp_(self.critic, f["tau"])


def _filled_agent(M, dev):
    from robot_gym_amd.agents.ddpg import BatchedDDPGAgent
    agent = BatchedDDPGAgent(RING_BATCH, RING_TICKS, device=dev, minibatch=M, seed=M)
    gen = torch.Generator(device="cpu").manual_seed(1)
    agent.ring_obs.copy_(torch.randn(agent.ring_obs.shape, generator=gen) * 0.1)
    agent.ring_action.copy_(torch.rand(agent.ring_action.shape, generator=gen) * 2 - 1)
    agent.ring_reward.copy_(torch.randn(agent.ring_reward.shape, generator=gen))
    agent.ring_state.copy_(torch.tensor([0, RING_TICKS, 0, 0]))
    return agent


def measure_update(M, repeats, updates):
    dev = torch.device("cuda", 0)
    agent = _filled_agent(M, dev)
    ref = TorchDDPG(agent, M)
    _timed(lambda: agent.update(1), 20)                         # warm-up of both paths
    _timed(ref.update, 20)
    runs = dict(device_ms=[], torch_ms=[], device_chain_ms=[])
    for _ in range(repeats):                                    # alternated: the host is shared, a drift hits both alike
        runs["device_ms"].append(_timed(lambda: agent.update(1), updates))
        runs["torch_ms"].append(_timed(ref.update, updates))
        runs["device_chain_ms"].append(_timed(lambda: agent.update(updates), 1) / updates)      # one call, `updates` updates
    med = {k: statistics.median(v) for k, v in runs.items()}
    stats = agent.stats_dict()
    row = dict(minibatch=M, updates_per_measurement=updates, device_ms=round(med["device_ms"], 4), device_chain_ms=round(med["device_chain_ms"], 4),
               torch_ms=round(med["torch_ms"], 4), spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in runs.items()},
               device_over_torch=round(med["device_ms"] / med["torch_ms"], 4), groups=agent._handle.groups, lds_bytes=agent._handle.lds_bytes,
               workspace_mb=round(agent._handle.workspace_bytes / 2 ** 20, 2), device=torch.cuda.get_device_name(0), stats=stats)
    agent.close()
    return row


def measure_collect(B, repeats, ticks, robot):
    from robot_gym_amd.agents.ddpg import BatchedDDPGAgent, collect
    from robot_gym_amd.core.config import MPCConfig
    from robot_gym_amd.gym.batched_go_env import BatchedGoEnv
    dev = torch.device("cuda", 0)
    cfg = MPCConfig.for_robot(robot, vx_offset=0.0, vy_offset=0.0, wz_offset=0.0)
    env = BatchedGoEnv(B, cfg, seed=B, device=dev, auto_reset=True, max_time=1e9, max_track_err=10.0, progress_limit=1e9)
    env.reset()
    agent = BatchedDDPGAgent(B, 64, device=dev, seed=B)
    collect(env, agent, 8, updates_per_tick=1, warmup=2)        # warm-up; the ring holds transitions from here on
    action = torch.zeros(B, 2, dtype=torch.float32, device=dev)
    runs = dict(step_ms=[], tick_u1_ms=[], tick_u8_ms=[], tick_u0_ms=[])
    for _ in range(repeats):
        runs["step_ms"].append(_timed(lambda: env.step(action), ticks))
        runs["tick_u0_ms"].append(_timed(lambda: collect(env, agent, 1, updates_per_tick=0), ticks))
        runs["tick_u1_ms"].append(_timed(lambda: collect(env, agent, 1, updates_per_tick=1, warmup=0), ticks))
        runs["tick_u8_ms"].append(_timed(lambda: collect(env, agent, 1, updates_per_tick=8, warmup=0), ticks))
    med = {k: statistics.median(v) for k, v in runs.items()}
    row = dict(batch=B, ticks_per_measurement=ticks, minibatch=agent.minibatch, **{k: round(v, 4) for k, v in med.items()},
               spread={k: [round(min(v), 4), round(max(v), 4)] for k, v in runs.items()}, device=torch.cuda.get_device_name(0))
    env.close(), agent.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robot", default="ghost")
    ap.add_argument("--minibatches", default="32,256,4096")
    ap.add_argument("--collect-batch", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--updates", type=int, default=200, help="updates per measurement")
    ap.add_argument("--ticks", type=int, default=20, help="ticks per measurement of the collect step")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        kind, n = args.child.split(":")
        row = measure_update(int(n), args.repeats, args.updates) if kind == "update" else measure_collect(int(n), args.repeats, args.ticks, args.robot)
        print("ROW " + json.dumps(row), flush=True)
        return 0
    rows = dict(update=[], collect=[])
    steps = [f"update:{int(x)}" for x in args.minibatches.split(",") if x] + ([f"collect:{args.collect_batch}"] if args.collect_batch > 0 else [])
    for step in steps:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step, "--repeats", str(args.repeats),
               "--updates", str(args.updates), "--ticks", str(args.ticks), "--robot", args.robot]
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            print(res.stdout[-2000:], res.stderr[-4000:], file=sys.stderr)
            print(f"{step}: exit status {res.returncode}; stopping", file=sys.stderr)
            return res.returncode
        row = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("ROW ")][-1][4:])
        print(json.dumps(row), flush=True)
        rows[step.split(":")[0]].append(row)
    commit, dirty = bench.git_head()
    result = dict(what="DDPG update, one MI355X, ms per update with the default networks (actor 80-128-128-64-2, critic 82-256-256-128-1): "
                       "BatchedDDPGAgent.update (HIP, rg_ddpg.h; device_ms one update per call, device_chain_ms `updates` updates in one call) and a "
                       "plain torch update on one pre-gathered minibatch (autograd, clip_grad_norm_, Adam, lerp_), alternated, medians with [min, max] "
                       "in spread; collect: ms per tick at one batch for the bare env.step, for act + step + store (u0) and with 1 and 8 updates "
                       "per tick.  `commit` is the commit the measured tree was based on",
                  robot=args.robot, commit=commit, dirty=dirty, source_hash=bench.source_hash(), ddpg_source_sha256=ddpg_hash(), repeats=args.repeats,
                  update=rows["update"], collect=rows["collect"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
