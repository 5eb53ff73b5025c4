"""A float64 model of the go-to-target task of include/rg_goto.h: rg_goto_pre_step, rg_goto_post_step and rg_goto_observe for
ONE robot at a time, in plain numpy and Python floats, written for clarity.

It restates robot_gym_amd/csrc/rg_goto.hip operation for operation: every product and sum is formed in the kernel's order,
nothing is contracted, and what the library precomputes on the host (1 / max_track_err, the reward per checkpoint, the step
limit) is precomputed here the same way.  What remains different is the device's atan2 / sincos / sqrt / division against
libm's.  The pieces the reference does with shapely -- arc-length interpolation, closed point-in-polygon, minimum
point-to-point distance, rigid moves -- have documented semantics and are pinned by this model only.

Each tick also reports the MARGINS that make a comparison with another implementation meaningful: how far every decision
of the tick was from flipping (`margins`, by name; `margin` is the smallest).  They fall in two groups.  The window test,
the chain's arg-mins and its continuity check work on values that went through sin / cos / atan2 of the yaw, where two
correct implementations differ by an ulp: `margin_frame` is the smallest of those, and a comparison may leave a robot-tick
out when it is below the comparison's threshold.  The nearest path point, the checkpoint loop and every threshold of the
reward and the termination work on sums, products, square roots and quotients of the inputs only, which IEEE arithmetic
fixes to the bit in a fixed order: two implementations of this file's order agree there even at an exact tie (and on a
1 cm path whose length is a round number the progress DOES sit exactly on a checkpoint), so those margins are reported but
are no ground to leave anything out.

Exact ties.  A path may hold the same point more than once (the reference's planner repeats coordinates).  Copies of a point
have bitwise equal robot-frame coordinates and so tie exactly in the chain's arg-min: `margin_frame` is 0 there although
nothing is in doubt -- the lowest index wins on both sides, and either copy puts the same coordinates into the chain.
`margin_frame_ties_ok` is margin_frame with the arg-min gap taken over the candidates that are NOT bitwise copies of the
winner; a comparison built on it compares the tie ticks too.  The nearest-point arg-min (`nearest`, `nearest_prev`) is not
among FRAME_MARGINS: it is compared even at a tie, and this model takes the lowest index there as the kernel does (np.argmin
returns the first minimum; tests/test_goto_model_cpu.py holds it to that).
"""
import math

import numpy as np

from robot_gym_amd.core import goto_abi
from robot_gym_amd.core.goto_abi import (ROW_CHAIN, ROW_DONE, ROW_ENV_STEPS, ROW_LATCHED, ROW_NEXT_CP, ROW_OBS, ROW_OVERFLOW,
                                         ROW_PATH_DONE, ROW_POS, ROW_POT, ROW_PREV, ROW_PROGRESS, ROW_REASON, ROW_TRACK_ERR,
                                         ROW_VISIBLE, STATE_ROWS)

FRAME_MARGINS = ("window_edge", "chain_argmin", "continuity")
REASON = {name: k for k, name in enumerate(goto_abi.REASONS)}
INF = math.inf


def config(mpc_cfg=None, **task):
    """The configuration as the kernels see it: goto_abi.task_fields plus the host-side precomputations of rg_goto_create."""
    c = dict(goto_abi.task_fields(mpc_cfg, **task))
    c["inv_max_err"] = 1.0 / c["max_track_err"]
    c["cp_reward"] = c["checkpoint_reward_total"] / float(c["num_checkpoints"])
    c["max_steps"] = c["max_time"] / (c["dt_sim"] * float(c["substeps"]))
    c["off"] = np.asarray(c["cmd_offset"], dtype=np.float32)
    return c


def new_state():
    """The task state column rg_goto_set_path leaves: all zero."""
    return np.zeros(STATE_ROWS)


def yaw_of(quat):
    x, y, z, w = (float(v) for v in quat)
    return math.atan2(2 * (x * y + z * w), 1 - 2 * (y * y + z * z))


def pre_step(c, state, path, sim_xy, action):
    """-> the offset-corrected command (vx, vy, wz) as float32 [3]."""
    a = [float(np.float32(action[0])), float(np.float32(action[1]))]
    for i in range(2):
        if a[i] != a[i]:
            a[i] = 0.0
        lo, hi = c["action_low"][i], c["action_high"][i]
        a[i] = lo if a[i] < lo else (hi if a[i] > hi else a[i])
    stand = state[ROW_DONE] != 0.0 or path is None or path.n < 2
    if not stand:
        tx, ty = float(sim_xy[0]) - path.target[0], float(sim_xy[1]) - path.target[1]
        stand = math.sqrt(tx * tx + ty * ty) <= c["target_radius"]
    if stand:
        a = [0.0, 0.0]
    off = c["off"]
    return np.array([np.float32(a[0]) + off[0], np.float32(0.0) + off[1], np.float32(a[1]) + off[2]], dtype=np.float32)


def window_corners(c, px, py, sn, cz):
    d, h, wt, wb = c["window_distance"], c["window_height"], c["window_top_width"], c["window_bottom_width"]
    lcx = (d + h, d + h, d, d)
    lcy = (wt / 2, -(wt / 2), -(wb / 2), wb / 2)
    return ([px + (cz * lcx[e] - sn * lcy[e]) for e in range(4)], [py + (sn * lcx[e] + cz * lcy[e]) for e in range(4)])


def _argmin2(d):
    """(lowest index of the minimum, gap to the second best) of a float array."""
    i = int(np.argmin(d))
    if len(d) < 2:
        return i, INF
    rest = np.delete(d, i)
    return i, float(rest.min() - d[i])


def _same_point(lx, ly, w):
    """Mask of the points whose coordinates are BITWISE those of point w."""
    bx, by = np.ascontiguousarray(lx).view(np.int64), np.ascontiguousarray(ly).view(np.int64)
    return (bx == bx[w]) & (by == by[w])


def chain_points(lx, ly, continuity_break):
    """sort_points as the kernel does it, on points (lx, ly) seen from the origin: start at the nearest, chain the nearest
    free point, distances compared after the root with the lowest index winning a tie, stop before the first link above
    continuity_break.  -> (chain [(x, y)], cumulative length per chain point, total length, the smallest gap between the
    best and the second best of an arg-min, the smallest distance of a link from the break, and the smallest gap once more
    with the candidates left out whose coordinates are bitwise the winner's: a copy of the winner is at the same distance
    in any IEEE arithmetic, the lowest index takes it, and whichever copy is taken the chain holds the same coordinates)."""
    nvis = len(lx)
    chain, cs, acc = [], [], 0.0
    free = np.ones(nvis, dtype=bool)
    tx, ty = 0.0, 0.0
    chain_gap, brk_margin, gap_ties_ok = INF, INF, INF
    while len(chain) < nvis:
        a, b = lx - tx, ly - ty
        d = np.where(free, np.sqrt(a * a + b * b), INF)
        w, g = _argmin2(d)
        if chain:
            dist = float(d[w])
            brk_margin = min(brk_margin, abs(dist - continuity_break))
            if dist > continuity_break:
                break
            acc = acc + dist
        chain_gap = min(chain_gap, g)
        rivals = d[free & ~_same_point(lx, ly, w)]
        if len(rivals):
            gap_ties_ok = min(gap_ties_ok, float(rivals.min() - d[w]))
        tx, ty = float(lx[w]), float(ly[w])
        free[w] = False
        chain.append((tx, ty))
        cs.append(acc)
    return chain, cs, acc, chain_gap, brk_margin, gap_ties_ok


def post_step(c, state, path, sim_xy, quat, sim_status=0.0, sim_steps=0.0, observe_only=False):
    """One tick on `state` (modified in place).  Returns a dict: obs float32 [2 num_cam_pts], reward float32, done int,
    margin (metres / reward units: the distance of the tick's nearest decision from flipping) and its parts."""
    ncp = c["num_cam_pts"]
    out = dict(margin=INF, margin_frame=INF, margin_frame_ties_ok=INF, zero_links=0, margins={})
    n = 0 if path is None else min(path.n, c["n_max"])
    if state[ROW_DONE] != 0.0 or n < 2:
        out.update(obs=state[ROW_OBS:ROW_OBS + 2 * ncp].astype(np.float32), reward=np.float32(0.0), done=1, frozen=True)
        return out
    out["frozen"] = False
    marg = out["margins"]
    # 1. pose
    ox, oy, oyaw = (float(v) for v in state[ROW_POS:ROW_POS + 3])
    px, py, yaw = float(sim_xy[0]), float(sim_xy[1]), yaw_of(quat)
    bad = not (math.isfinite(px) and math.isfinite(py) and math.isfinite(yaw))
    if bad:
        px, py, yaw = ox, oy, oyaw
    fallen = bad or sim_status != 0.0
    sn, cz = math.sin(yaw), math.cos(yaw)
    wx, wy = window_corners(c, px, py, sn, cz)
    # 2a. the scan
    X, Y = path.x[:n], path.y[:n]
    dx, dy = X - px, Y - py
    dn = np.sqrt(dx * dx + dy * dy)
    ex, ey = X - ox, Y - oy
    en = np.sqrt(ex * ex + ey * ey)
    bi, gap = _argmin2(dn)
    bpi, gap_prev = _argmin2(en)
    vis = np.ones(n, dtype=bool)
    edge_margin = INF
    for e in range(4):
        f = (e + 1) & 3
        ax, ay = wx[f] - wx[e], wy[f] - wy[e]
        cr = ax * (Y - wy[e]) - ay * (X - wx[e])
        vis &= cr <= 0.0
        edge_margin = min(edge_margin, float(np.abs(cr).min()) / math.hypot(ax, ay))
    marg["window_edge"] = edge_margin
    idx = np.nonzero(vis)[0]
    count = len(idx)
    idx = idx[:c["max_visible"]]
    lx = cz * dx[idx] + sn * dy[idx]
    ly = cz * dy[idx] - sn * dx[idx]
    nvis = len(idx)
    # 2b. sort_points
    chain, cs, acc, chain_gap, brk_margin, gap_ties_ok = chain_points(lx, ly, c["continuity_break"])
    if brk_margin < INF:
        marg["continuity"] = brk_margin
    marg["chain_argmin"] = chain_gap
    clen = len(chain)
    # 2c. interpolate_points
    fresh = clen >= 2 and acc > 0.0
    if fresh:
        seg = acc / float(ncp - 1) if ncp > 1 else 0.0
        for j in range(ncp):
            t = float(j) * seg
            if t > acc + 1e-6:
                continue
            if t >= acc:
                qx, qy = chain[-1]
            else:
                k = 0
                while k < clen - 2 and not t < cs[k + 1]:
                    k += 1
                fr = (t - cs[k]) / (cs[k + 1] - cs[k])
                qx = chain[k][0] + fr * (chain[k + 1][0] - chain[k][0])
                qy = chain[k][1] + fr * (chain[k + 1][1] - chain[k][1])
            state[ROW_OBS + 2 * j], state[ROW_OBS + 2 * j + 1] = qx, qy
    state[ROW_PREV:ROW_PREV + 3] = ox, oy, oyaw
    state[ROW_POS:ROW_POS + 3] = px, py, yaw
    if count > c["max_visible"]:
        state[ROW_OVERFLOW] = 1.0
    state[ROW_VISIBLE], state[ROW_CHAIN], state[ROW_LATCHED] = float(count), float(clen), 1.0 if fresh else 0.0
    out["obs"] = state[ROW_OBS:ROW_OBS + 2 * ncp].astype(np.float32)
    out.update(visible=count, chain=clen, latched=int(fresh), nearest=bi, nearest_prev=bpi)
    out["margin_frame"] = min(marg[k] for k in FRAME_MARGINS if k in marg)
    out["margin_frame_ties_ok"] = min([gap_ties_ok] + [marg[k] for k in FRAME_MARGINS if k in marg and k != "chain_argmin"])
    out["zero_links"] = sum(1 for k in range(1, clen) if cs[k] == cs[k - 1])      # chain links of length zero: copies of a point
    if observe_only:
        out["margin"] = min(marg.values())
        return out
    # 3. reward
    last = n - 1
    i1 = min(max(int(path.first_same_x[bpi]), 0), last)
    i2 = min(max(int(path.first_same_x[bi]), 0), last)
    S = path.s
    track_err = float(dn[bi])
    marg["nearest"], marg["nearest_prev"] = gap, gap_prev
    err_norm = track_err * c["inv_max_err"]
    dl = 0.0
    if i1 != i2:
        first, second = (i1, i2) if i1 < i2 else (i2, i1)
        len1 = S[second] - S[first]
        gx, gy = X[second] - X[first], Y[second] - Y[first]
        len2 = S[first] + math.sqrt(gx * gx + gy * gy) + (S[last] - S[second])
        marg["loop_side"] = abs(len1 - len2)
        if len1 < len2:
            dl = len1 if i1 < i2 else -len1
        else:
            dl = -len2 if i1 < i2 else len2
        dl = float(dl)
    pot = float(state[ROW_POT]) + dl
    progress = float(state[ROW_PROGRESS])
    nci = int(state[ROW_NEXT_CP])
    path_done = state[ROW_PATH_DONE] != 0.0
    r = 0.0
    k = 0
    marg["progress_window"] = abs((pot - progress) - c["progress_window"])
    if pot - progress < c["progress_window"]:
        if not path_done:
            if pot > progress:
                progress = pot
            per = path.length / float(c["num_checkpoints"])
            while k < c["num_checkpoints"]:
                marg["checkpoint"] = min(marg.get("checkpoint", INF), abs(progress - float(nci + 1) * per))
                if not progress >= float(nci + 1) * per:
                    break
                nci += 1
                k += 1
                if nci >= c["num_checkpoints"] - 1:
                    path_done = True
                    break
        u = 1.0 - err_norm
        r = r + float(k) * c["cp_reward"] * (u * u)
    r = r - c["time_penalty"]
    off_progress = abs(pot - progress) > c["progress_limit"]
    off_track = track_err > c["max_track_err"]
    marg["progress_limit"] = abs(abs(pot - progress) - c["progress_limit"])
    marg["track_limit"] = abs(track_err - c["max_track_err"])
    if off_progress or off_track:
        r = goto_abi.LIMIT_REWARD
    # 4. termination
    tgx, tgy = px - path.target[0], py - path.target[1]
    tdist = math.sqrt(tgx * tgx + tgy * tgy)
    marg["on_target"] = abs(tdist - c["target_radius"])
    marg["time"] = abs(float(sim_steps) - c["max_steps"])
    if fallen:
        reason = REASON["fallen"]
    elif path_done:
        reason = REASON["path_done"]
    elif tdist <= c["target_radius"]:
        reason = REASON["on_target"]
    elif off_progress:
        reason = REASON["progress"]
    elif off_track:
        reason = REASON["track"]
    elif float(sim_steps) > c["max_steps"]:
        reason = REASON["time"]
    else:
        reason = REASON["none"]
    state[ROW_POT], state[ROW_PROGRESS], state[ROW_NEXT_CP], state[ROW_PATH_DONE] = pot, progress, float(nci), 1.0 if path_done else 0.0
    state[ROW_ENV_STEPS] += 1.0
    state[ROW_DONE], state[ROW_REASON], state[ROW_TRACK_ERR] = (1.0 if reason else 0.0), float(reason), track_err
    out.update(reward=np.float32(r), reward64=r, done=int(reason != 0), reason=reason, track_err=track_err, checkpoints=k,
               position_on_track=pot, first_same=(i1, i2))
    out["margin"] = min(marg.values())
    return out
