"""The float64 statement of the height scan of include/rg_scan.h in numpy, over the grounds of tests/terrain_model.py (Flat,
Random, Grid).  It restates robot_gym_amd/csrc/rg_scan.hip operation for operation -- the heading from the quaternion by
one sqrt and two divisions, the grid offsets, the rotation, the ground, the fmax / fmin clip (np.fmax / np.fmin: a NaN becomes
the lower bound, as terrain_model._lattice has it) and the rounding to float32 -- so the kernel is held to it BIT FOR BIT
(tests/test_scan_gpu.py), the masked / prev semantics included.
"""
import numpy as np

from tests import terrain_model as TM

ROW_P, ROW_QUAT = 0, 3      # RG_SRB_ROW_P, RG_SRB_ROW_QUAT
DEFAULTS = dict(nx=8, ny=6, x_first=-0.2, dx=0.1, y_first=-0.25, dy=0.1, z_offset=0.0, clip=1.0, scale=1.0)


def heading(state):
    """(c, s) [B] each: the normalised first column of the body's rotation; (1, 0) where its norm is 0 or NaN."""
    qx, qy, qz, qw = (np.asarray(state[ROW_QUAT + i], dtype=np.float64) for i in range(4))
    with np.errstate(all="ignore"):
        c0 = 1 - 2 * (qy * qy + qz * qz)
        s0 = 2 * (qx * qy + qz * qw)
        n = np.sqrt(c0 * c0 + s0 * s0)
        turned = n > 0
        return np.where(turned, c0 / n, 1.0), np.where(turned, s0 / n, 0.0)


def points(s):
    """(fx, fy) [N] each, point k = a * ny + c at grid node (a, c)."""
    a, c = np.meshgrid(np.arange(s["nx"], dtype=np.float64), np.arange(s["ny"], dtype=np.float64), indexing="ij")
    return s["x_first"] + a.ravel() * s["dx"], s["y_first"] + c.ravel() * s["dy"]


def world_points(state, settings):
    """(X, Y) [N, B] each: where the points of every robot lie in the world."""
    s = {**DEFAULTS, **settings}
    fx, fy = (v[:, None] for v in points(s))
    c, sn = (v[None, :] for v in heading(state))
    px, py = (np.asarray(state[ROW_P + i], dtype=np.float64)[None, :] for i in range(2))
    with np.errstate(all="ignore"):
        return px + (c * fx - sn * fy), py + (sn * fx + c * fy)


def scan(state, ground=None, **settings):
    """float32 [nx * ny, B]: the scan of the simulator state [43, B] (only rows 0..6 are read) on `ground` (None: the plane)."""
    s = {**DEFAULTS, **settings}
    ground = ground or TM.Flat()
    B = np.asarray(state).shape[1]
    X, Y = world_points(state, s)
    robot = np.broadcast_to(np.arange(B)[None, :], X.shape)
    pz = np.asarray(state[ROW_P + 2], dtype=np.float64)[None, :]
    with np.errstate(all="ignore"):
        h = 0.0 if ground.kind == 0 else ground.height(X, Y, robot)
        d = (pz - s["z_offset"]) - h
        d = np.broadcast_to(d, X.shape)
        if s["clip"] > 0:
            d = np.fmin(np.fmax(d, -s["clip"]), s["clip"])
        return (d * s["scale"]).astype(np.float32)


def observe(state, out, ground=None, mask=None, prev=None, **settings):
    """rg_scan_observe on numpy buffers, in place: for the robots with mask != 0 (None: all) prev, if given, takes out's
    columns, then out takes the scan; nothing else is touched.  Returns out."""
    new = scan(state, ground, **settings)
    cols = np.arange(new.shape[1]) if mask is None else np.nonzero(np.asarray(mask) != 0)[0]
    if prev is not None:
        prev[:, cols] = out[:, cols]
    out[:, cols] = new[:, cols]
    return out
