"""One sha256 per output buffer of the agents' update entries at fixed seeds: two builds of librg_mpc.so (RG_MPC_LIB, as
mpc_abi.LIB_PATH takes it) that print the same lines compute the same bytes.  PPO: policy_grad, value_grad, adam on both
networks, kl; DDPG: critic_grad, actor_grad, adam on both networks, soft_update on both.  The configurations are the smallest
of the GPU tests that reach every path of the code the agents' files share: below one tile, one sample past a tile with
256-wide layers, more tiles than workgroups with a ragged tail.  Every configuration runs in a child process of its own under
a time limit (`--limit` seconds); after a failure nothing more is started.

    RG_MPC_LIB=/path/to/librg_mpc.so python tools/agent_digest.py
"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PPO_CASES = [("lopsided", 3, 5), ("limits", 1, 17), ("default", 5, 1037)]
DDPG_CASES = [("lopsided", 3, 4, 6, 5), ("limits", 3, 7, 10, 17)]


def digest(label, tensor):
    print(f"{label} {hashlib.sha256(tensor.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}", flush=True)


def ppo(name, T, B):
    import torch
    from robot_gym_amd.agents.ppo import DevicePPO
    from tests import test_ppo_update_gpu as G
    dev, tag = torch.device("cuda", 0), f"ppo {name} T={T} B={B}"
    c = G.case(name, T, B)
    pol, ro = G._policy(dev, c), G._rollout(dev, c)
    upd = DevicePPO(pol, T, **G.PPO_KW)
    upd.prepare(ro)
    for which, fn, params in (("policy", upd.policy_grad, pol.policy_params), ("value", upd.value_grad, pol.value_params)):
        grad, loss = fn(ro)
        digest(f"{tag} {which}_grad.grad", grad), digest(f"{tag} {which}_grad.loss", loss)
        upd.adam(which, grad)
        digest(f"{tag} adam.{which}_params", params)
    digest(f"{tag} adam.opt_state", upd.opt_state)
    digest(f"{tag} kl", upd.kl(ro))
    upd.close(), pol.close()


def ddpg(*cs):
    import torch
    from tests import ddpg_cases as DC
    from tests import test_ddpg_gpu as G
    dev, tag = torch.device("cuda", 0), "ddpg " + "-".join(str(v) for v in cs)
    c = DC.case(*cs)
    a = G._agent(dev, c)
    idx = G._idx(dev, c)
    for which, fn in (("critic", a.critic_grad), ("actor", a.actor_grad)):
        grad, loss = fn(idx)
        digest(f"{tag} {which}_grad.grad", grad), digest(f"{tag} {which}_grad.loss", loss)
        a.adam(which, grad)
        digest(f"{tag} adam.{which}_params", getattr(a, which + "_params"))
    digest(f"{tag} adam.opt_state", a.opt_state)
    for which in ("actor", "critic"):
        a.soft_update(which)
        digest(f"{tag} soft_update.target_{which}_params", getattr(a, f"target_{which}_params"))
    a.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=120, help="seconds a configuration's child process may take")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        agent, name, *shape = args.child.split(",")
        (ppo if agent == "ppo" else ddpg)(name, *[int(v) for v in shape])
        return 0
    for cs in [("ppo",) + c for c in PPO_CASES] + [("ddpg",) + c for c in DDPG_CASES]:
        child = ",".join(str(v) for v in cs)
        res = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", child])
        if res.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            print(f"{child}: exit status {res.returncode}; stopping", file=sys.stderr)
            return res.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
