"""One sha256 per buffer of the simulator's four ticks at fixed seeds: rg_srb_step on the plane and on a ground,
rg_srb_step_contact and rg_srb_step_friction (measured 0 and 1), each at batch 1, 5 and 67 (four lanes a robot, 64 robots a
block: 67 crosses a block edge, ends in a partial wave and has lanes past the batch) on the plane, the random terrain and a
small grid.  Every run is 40 ticks of the recorded streams of tests/srb_streams.py and the terrain, contact and friction
fixtures: pushes on half the robots, true bodies, a reset, one robot that loses its forces midway and falls, and for the
friction tick non-finite forces and a mu row mixing +inf, 0.3, 0 and NaN.

    python tools/srb_digest.py --model                        the float64 numpy models (no GPU): every tick's state and observation
    RG_MPC_LIB=/path/to/librg_mpc.so python tools/srb_digest.py    the C entries on cuda:0, replaying the models' inputs: the state,
                                                              the observation and touch / slip after the last tick

Two versions of the models, or two builds of librg_mpc.so, that print the same lines compute the same bytes.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import contact_fixtures as CF  # noqa: E402
from tests import friction_fixtures as FF  # noqa: E402
from tests import srb_streams as S  # noqa: E402
from tests import terrain_fixtures as TF  # noqa: E402

BATCHES, TICKS, FALL_TICK = (1, 5, 67), 40, 20
MU = (np.inf, 0.3, 0.0, np.nan)


def runs(cfg):
    """(tag, recording, replay on a device -> the raw simulator) for every entry, ground and batch."""
    for n, B in enumerate(BATCHES):
        fall = np.arange(B) == B // 2
        rec = S.run_model(cfg, B, TICKS, 40 + n, fall=fall, fall_tick=FALL_TICK)
        yield f"step plane B={B}", rec, lambda dev, rec=rec: S.replay(rec, dev)
        for g, kind in enumerate(CF.GROUNDS):
            rec = TF.run_model(cfg, B, TICKS, 50 + 10 * g + n, CF.stream_ground(kind, B), fall=fall, fall_tick=FALL_TICK)
            yield f"step {kind} B={B}", rec, lambda dev, rec=rec: TF.replay(rec, dev)
            rec = CF.run_model(cfg, B, 90 + 10 * g + n, kind, TICKS)
            yield f"step_contact {kind} B={B}", rec, lambda dev, rec=rec: CF.replay(rec, dev)
            for measured in (0, 1):
                rec = FF.run_model(cfg, B, FF.stream_seed(g, n, measured), kind, measured, np.resize(MU, B), TICKS)
                yield f"step_friction {kind} measured={measured} B={B}", rec, lambda dev, rec=rec: FF.replay(rec, dev)[0]


def digest(tag, name, array):
    print(f"{tag} {name} {hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest()}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", action="store_true", help="hash the numpy models' runs; nothing touches a GPU")
    args = ap.parse_args()
    from robot_gym_amd.core.config import MPCConfig
    cfg = MPCConfig.for_robot("ghost")
    dev = None
    if not args.model:
        import torch
        dev = torch.device("cuda", 0)
    for tag, rec, replay in runs(cfg):
        if args.model:
            digest("model " + tag, "state", np.stack(rec.states))
            for name in sorted(rec.obs[0]):
                digest("model " + tag, name, np.stack([o[name] for o in rec.obs]))
            for name in ("touches", "slips"):
                if hasattr(rec, name):
                    digest("model " + tag, name, np.stack(getattr(rec, name)))
            continue
        raw = replay(dev)
        state, obs = raw.numpy()
        digest(tag, "state", state)
        for name in sorted(obs):
            digest(tag, name, obs[name])
        for name in ("touch", "slip"):
            if getattr(raw, name, None) is not None:
                digest(tag, name, getattr(raw, name).cpu().numpy())
        raw.close()


if __name__ == "__main__":
    main()
