"""Host side of the go-to-target task, once per reset: the potential-field planner, the path and its tables.

Plain numpy, restated from the reference's gym/envs/go_to (path_planner/potential_field_planner.py, path_follower/path.py
and line_interpolation.py) with the same float64 arithmetic in the same order, so that plan_path and chain_sort reproduce
its recorded outputs exactly (tests/golden/goto_reference.npz).  What the reference does with shapely (arc-length
interpolation along a polyline) is restated from the documented semantics and pinned by tests/goto_model.py.

    pts = plan_path((2.0, 1.5))                 # [k,2] way points on the 0.5 m grid, the target appended
    path = build_path(pts)                      # 1 cm points, arc-length table, first_same_x, checkpoints
    rows = pack_paths([path, ...], n_max)       # the host arrays of rg_goto_set_path
"""
import math
from collections import namedtuple

import numpy as np

KP = 5.0            # attractive potential gain
ETA = 100.0         # repulsive potential gain
AREA_WIDTH = 5.0    # potential area width [m]
OSCILLATION_LENGTH = 3
GRID = 0.5
ROBOT_RADIUS = 0.25
MOTION = ((1, 0), (0, 1), (-1, 0), (0, -1), (-1, -1), (-1, 1), (1, -1), (1, 1))
SPACING = 1e-2      # path point spacing [m]
NUM_CHECKPOINTS = 100
CONTINUITY_BREAK = 30e-3

Path = namedtuple("Path", "x y s first_same_x n length checkpoints start_xy start_angle target")


MAX_WAYPOINTS = 64  # way points of a plan at most, start and target included (RG_EPISODE_MAX_WAYPOINTS)


def _potential_map(gx, gy, ox, oy, reso, rr, sx, sy, kp=KP, eta=ETA, area_width=AREA_WIDTH):
    minx = min(min(ox), sx, gx) - area_width / 2.0
    miny = min(min(oy), sy, gy) - area_width / 2.0
    maxx = max(max(ox), sx, gx) + area_width / 2.0
    maxy = max(max(oy), sy, gy) + area_width / 2.0
    xw = int(round((maxx - minx) / reso))
    yw = int(round((maxy - miny) / reso))
    X = (np.arange(xw) * reso + minx)[:, None]
    Y = (np.arange(yw) * reso + miny)[None, :]
    pmap = 0.5 * kp * np.hypot(X - gx, Y - gy)
    # the nearest obstacle of every cell; `dmin >= d` lets the last of equally near obstacles win
    dmin = np.full((xw, yw), np.inf)
    for k in range(len(ox)):
        d = np.hypot(X - ox[k], Y - oy[k])
        dmin = np.where(dmin >= d, d, dmin)
    for ix, iy in zip(*np.nonzero(dmin <= rr)):
        dq = dmin[ix, iy]
        if dq <= 0.1:
            dq = 0.1
        pmap[ix, iy] = pmap[ix, iy] + 0.5 * eta * (1.0 / dq - 1.0 / rr) ** 2
    return pmap, minx, miny


def plan_path(target_xy, obstacles=(), *, kp=KP, eta=ETA, area_width=AREA_WIDTH, grid=GRID, robot_radius=ROBOT_RADIUS,
              oscillation_length=OSCILLATION_LENGTH, max_waypoints=MAX_WAYPOINTS):
    """Way points from the origin to target_xy: steepest descent on the potential grid over the 8 neighbours (the first of
    equally low neighbours wins), stopped within one cell of the target or when the last `oscillation_length` cells hold a
    repeat, with the target appended.  obstacles: [(x, y), ...]; none puts the reference's dummy obstacle outside the area.
    The keyword settings are the planner's fields of rg_episode_config (include/rg_episode.h), their defaults this module's
    constants.  Returns [k,2].  Raises ValueError in the two cases that are RG_EPISODE_PLAN_WAYPOINTS on the device: the plan
    would hold more than max_waypoints way points, or no neighbour of a cell has a finite potential."""
    gx, gy = float(target_xy[0]), float(target_xy[1])
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 2)
    if len(obstacles) == 0:
        ox, oy = [area_width + 1.0], [area_width + 1.0]
    else:
        ox, oy = list(obstacles[:, 0]), list(obstacles[:, 1])
    sx, sy, reso = 0.0, 0.0, grid
    pmap, minx, miny = _potential_map(gx, gy, ox, oy, reso, robot_radius, sx, sy, kp, eta, area_width)
    d = np.hypot(sx - gx, sy - gy)
    ix = round((sx - minx) / reso)
    iy = round((sy - miny) / reso)
    rx, ry = [sx], [sy]
    previous = []
    while d >= reso:
        if len(rx) + 2 > max_waypoints:   # the next cell and the target would not fit
            raise ValueError(f"plan_path: more than max_waypoints = {max_waypoints} way points to {(gx, gy)}")
        minp, minix, miniy = float("inf"), -1, -1
        for mx, my in MOTION:
            inx, iny = int(ix + mx), int(iy + my)
            if inx >= pmap.shape[0] or iny >= pmap.shape[1] or inx < 0 or iny < 0:
                p = float("inf")
            else:
                p = pmap[inx, iny]
            if minp > p:
                minp, minix, miniy = p, inx, iny
        if minix < 0:
            raise ValueError(f"plan_path: no finite neighbour of cell {(int(ix), int(iy))} on the way to {(gx, gy)}")
        ix, iy = minix, miniy
        xp = ix * reso + minx
        yp = iy * reso + miny
        d = np.hypot(gx - xp, gy - yp)
        rx.append(xp)
        ry.append(yp)
        previous.append((ix, iy))
        if len(previous) > oscillation_length:
            previous.pop(0)
        if len(set(previous)) < len(previous):
            break
    rx.append(gx)
    ry.append(gy)
    return np.stack((np.asarray(rx, dtype=np.float64), np.asarray(ry, dtype=np.float64)), axis=-1)


def arc_table(points):
    """Cumulative arc length s[i] of a polyline [n,2]: s[0] = 0, s[i] = s[i-1] + sqrt(dx*dx + dy*dy), summed in order."""
    points = np.asarray(points, dtype=np.float64)
    s = np.zeros(len(points))
    for i in range(1, len(points)):
        dx, dy = points[i, 0] - points[i - 1, 0], points[i, 1] - points[i - 1, 1]
        s[i] = s[i - 1] + math.sqrt(dx * dx + dy * dy)
    return s


def interpolate_along(points, s, t):
    """The point at arc length t of the polyline: the last point for t >= s[-1], else on the first segment k with
    t < s[k+1], at points[k] + (t - s[k]) / (s[k+1] - s[k]) * (points[k+1] - points[k])."""
    last = len(points) - 1
    if t >= s[last]:
        return float(points[last, 0]), float(points[last, 1])
    k = 0
    while k < last - 1 and not t < s[k + 1]:
        k += 1
    fr = (t - s[k]) / (s[k + 1] - s[k])
    return (float(points[k, 0] + fr * (points[k + 1, 0] - points[k, 0])),
            float(points[k, 1] + fr * (points[k + 1, 1] - points[k, 1])))


def interpolate_points(points, nb_out_points):
    """nb_out_points points at equal arc length along the polyline: i * (length / (nb_out_points - 1)), stopping at the
    first that lies more than 1e-6 past the length.  One input point gives that point; a polyline of zero length gives
    None (the reference raises there)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    if nb_out_points < 1:
        raise ValueError("nb_out_points must be greater than 0")
    if len(points) == 0:
        raise ValueError("point array is empty")
    if nb_out_points == 1 or len(points) < 2:
        return points[:1].copy()
    s = arc_table(points)
    length = s[-1]
    if not length > 0.0:
        return None
    seg = length / (nb_out_points - 1)
    out = []
    for i in range(nb_out_points):
        t = i * seg
        if t > length + 1e-6:
            break
        out.append(interpolate_along(points, s, t))
    return np.array(out)


def chain_sort(points, origin=(0.0, 0.0), continuity_break=CONTINUITY_BREAK):
    """sort_points: start at the point nearest `origin`, then repeatedly take the nearest remaining point; strict <, so the
    first in input order wins a tie; stop before the first link longer than continuity_break.  The distances
    sqrt(dx*dx + dy*dy) are compared, as the reference compares them: the two neighbours of a point on a 1 cm path differ by
    an ulp squared and tie after the root.  Returns (sorted points [m,2], their input indices [m])."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    free = list(range(len(points)))
    order = []
    tx, ty = float(origin[0]), float(origin[1])
    while free:
        best, bd = -1, math.inf
        for i in free:
            dx, dy = points[i, 0] - tx, points[i, 1] - ty
            d = math.sqrt(dx * dx + dy * dy)
            if d < bd:
                best, bd = i, d
        if best < 0 or (order and bd > continuity_break):
            break
        order.append(best)
        free.remove(best)
        tx, ty = points[best, 0], points[best, 1]
    order = np.asarray(order, dtype=np.int64)
    return points[order], order


def build_path(points, num_checkpoints=NUM_CHECKPOINTS, target=None, spacing=SPACING, n_max=None):
    """Path.__init__: n = int(len / spacing) points (the reference's 1e-2) at equal arc length along the way points,
    `length` of the INTERPOLATED polyline, checkpoints at i * length / num_checkpoints, start_xy, start_angle in [0, 2 pi)
    from the first segment -- and the tables the kernel reads: cumulative arc length s and first_same_x[i], the first j
    with x[j] == x[i].  ValueError for n < 2 and, with n_max given, for n > n_max (RG_EPISODE_PLAN_SHORT / _LONG on the
    device)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = int(arc_table(points)[-1] / spacing)
    if n < 2:
        raise ValueError(f"build_path: the way points span {n} path points, at least 2 are needed")
    if n_max is not None and n > n_max:
        raise ValueError(f"build_path: the way points span {n} path points, n_max is {n_max}")
    pts = interpolate_points(points, n)
    x, y = np.ascontiguousarray(pts[:, 0]), np.ascontiguousarray(pts[:, 1])
    s = arc_table(pts)
    first, fsx = {}, np.zeros(len(x), dtype=np.int32)
    for i, v in enumerate(x):
        fsx[i] = first.setdefault(float(v), i)
    length = float(s[-1])
    checkpoints = np.array([i * (length / num_checkpoints) for i in range(1, num_checkpoints + 1)])
    vx, vy = x[1] - x[0], y[1] - y[0]
    norm = math.sqrt(vx * vx + vy * vy)
    vx, vy = (vx / norm, vy / norm) if norm > 0.0 else (1.0, 0.0)
    ang = math.atan2(vy, vx)
    if ang < 0.0:
        ang += 2 * math.pi
    tgt = points[-1] if target is None else np.asarray(target, dtype=np.float64)
    return Path(x, y, s, fsx, len(x), length, checkpoints, (float(x[0]), float(y[0])), ang, (float(tgt[0]), float(tgt[1])))


def length_between_idx(path, idx1, idx2):
    """Path.length_between_idx(shortest=True) on the tables, the path closed into a loop, its sign rules as written."""
    if idx1 == idx2:
        return 0.0
    first, second = (idx1, idx2) if idx1 < idx2 else (idx2, idx1)
    len_1 = path.s[second] - path.s[first]
    gx, gy = path.x[second] - path.x[first], path.y[second] - path.y[first]
    len_2 = path.s[first] + math.sqrt(gx * gx + gy * gy) + (path.s[path.n - 1] - path.s[second])
    if len_1 < len_2:
        return float(len_1 if idx1 < idx2 else -len_1)
    return float(-len_2 if idx1 < idx2 else len_2)


def random_target(rng):
    """go_env.py:163-175: uniform on +-2.5, rounded to 0.01, pushed out of (-1, 1).  rng: a numpy Generator.  An exact 0.0 is
    not pushed (as in the reference); the one draw in ~250000 that gives (0.0, 0.0) -- a target on the start, no path -- is
    drawn again."""
    while True:
        out = []
        for _ in range(2):
            v = round(float(rng.uniform(-2.5, 2.5)), 2)
            if 1.0 > v > 0:
                v = 1.0
            if -1.0 < v < 0:
                v = -1.0
            out.append(v)
        if out[0] != 0.0 or out[1] != 0.0:
            return tuple(out)


def pack_paths(paths, n_max):
    """The host arrays of rg_goto_set_path for a list of Path: dict of npts [n] int32, length [n], target [2,n],
    x / y / s [n,n_max] float64 and first_same_x [n,n_max] int32 (zero past each path's end)."""
    n = len(paths)
    out = dict(npts=np.zeros(n, dtype=np.int32), length=np.zeros(n), target=np.zeros((2, n)),
               x=np.zeros((n, n_max)), y=np.zeros((n, n_max)), s=np.zeros((n, n_max)), first_same_x=np.zeros((n, n_max), dtype=np.int32))
    for k, p in enumerate(paths):
        if p.n > n_max:
            raise ValueError(f"pack_paths: path {k} has {p.n} points, n_max is {n_max}")
        out["npts"][k], out["length"][k] = p.n, p.length
        out["target"][:, k] = p.target
        out["x"][k, :p.n], out["y"][k, :p.n], out["s"][k, :p.n], out["first_same_x"][k, :p.n] = p.x, p.y, p.s, p.first_same_x
    return out
