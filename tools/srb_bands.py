"""Measures what tests/srb_fixtures.py records: the worst band quantities of the CPU reference closed loop (oracle + float64
single-rigid-body model) over the fixture's 64 robots, and with --push the push-recovery ladder.  No GPU.

    python tools/srb_bands.py            # the five worst values; the bands are twice these
    python tools/srb_bands.py --push     # per push magnitude: robots outside the bands over the 2 s after the recovery time
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import srb_fixtures as F  # noqa: E402


def main():
    if "--push" in sys.argv:
        for newton in F.PUSH_LADDER:
            line = []
            for robot in F.ROBOTS:
                cmd, _ = F.cases(robot)
                traj, loop = F.run_cpu(robot, ticks=F.PUSH_RUN_TICKS, push=newton)
                worst = F.worst_in_window(F.window(traj, F.PUSH_RUN_TICKS - F.WINDOW), cmd, loop.cfg.body_height)
                line.append(f"{robot}: fallen {int(loop.model.fallen().sum())} outside {F.outside_bands(worst)} "
                            + " ".join(f"{k} {worst[k].max():.4g}" for k in F.BANDS))
            print(f"push {newton:g} N: " + " | ".join(line), flush=True)
        return
    total = {k: 0.0 for k in F.BANDS}
    for robot in F.ROBOTS:
        cmd, hs = F.cases(robot)
        traj, loop = F.run_cpu(robot)
        worst = F.worst_in_window(F.window(traj, F.TICKS - F.WINDOW), cmd, loop.cfg.body_height)
        print(robot, "fallen", int(loop.model.fallen().sum()), " ".join(f"{k} {worst[k].max():.5g} (robot {int(worst[k].argmax())})" for k in F.BANDS), flush=True)
        print(robot, "mean vy / command", float(np.mean(traj["vy"][F.TICKS - F.WINDOW:].mean(0)[16:] / cmd[16:, 1])), flush=True)
        for k in F.BANDS:
            total[k] = max(total[k], float(worst[k].max()))
    print("WORST", " ".join(f"{k} {v:.5g}" for k, v in total.items()))


if __name__ == "__main__":
    main()
