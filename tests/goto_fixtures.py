"""Shared inputs of the go-to-target tests: planned paths, synthetic pose sequences near them, and the model run over them.

RawTask is the task's handle on caller-owned buffers between guard rows (torch is imported when one is made, so this module
loads without it).

A pose sequence is written straight into a simulator state, so no controller takes part: robot r starts at a random arc
position of its own planned path and moves along it at its own speed, with a lateral offset up to 0.12 m and a heading up
to 0.6 rad off the tangent, both slowly varying.  A few robots are teleported 0.6 m ahead at some tick, a few fall.  Tick 0
is the pose of the reset (rg_goto_observe); ticks 1..T are rg_goto_post_step.
"""
import math
import multiprocessing
import os
from concurrent.futures import ProcessPoolExecutor

import numpy as np

from robot_gym_amd.core import goto_abi, srb_abi
from robot_gym_amd.gym import goto_path
from tests import goto_model

POSE_ROWS = 6   # x, y, quat z, quat w, simulator sub-steps, simulator status
# every field off its default: a lopsided trapezoid, 5 camera points, other thresholds, a short time limit, a non-zero offset
CONFIG_B = dict(window_height=0.21, window_top_width=0.19, window_bottom_width=0.26, window_distance=0.07, max_track_err=0.085,
                progress_window=0.33, progress_limit=0.45, target_radius=0.22, time_penalty=0.4, checkpoint_reward_total=730.0,
                max_time=6.0, continuity_break=0.024, action_low=(0.05, -0.3), action_high=(0.3, 0.25), cmd_offset=(0.01, -0.02, 0.03),
                dt_sim=0.002, substeps=5, num_cam_pts=5, num_checkpoints=37, n_max=640, max_visible=24)
assert all(CONFIG_B[k] != v for k, v in goto_abi.DEFAULTS.items()) and set(CONFIG_B) == set(goto_abi.DEFAULTS)


def planned_paths(batch, seed, num_checkpoints=100):
    """One planned path per robot, targets from GoEnv's distribution; equal targets share one Path object."""
    rng = np.random.default_rng(seed)
    cache, out = {}, []
    for _ in range(batch):
        t = goto_path.random_target(rng)
        if t not in cache:
            cache[t] = goto_path.build_path(goto_path.plan_path(t), num_checkpoints, target=t)
        out.append(cache[t])
    return out


def pose_sequence(path, ticks, rng, substeps=10):
    """[ticks + 1, POSE_ROWS] float64 for one robot."""
    T = ticks + 1
    k = np.arange(T)
    speed = rng.uniform(0.004, 0.02)
    s = rng.uniform(0.0, 0.6) * path.length + np.cumsum(np.r_[0.0, speed * rng.uniform(0.5, 1.5, ticks)])
    if rng.uniform() < 0.03:
        s[int(rng.integers(2, T)):] += 0.6
    s = np.minimum(s, path.length)
    amp = rng.uniform(0.0, 0.12)
    if rng.uniform() < 0.5:
        amp *= 0.5   # more robots that stay on the track to the end
    lat = amp * np.sin(rng.uniform(0, 2 * np.pi) + k * rng.uniform(0.01, 0.08))
    head = rng.uniform(0.0, 0.6) * np.sin(rng.uniform(0, 2 * np.pi) + k * rng.uniform(0.01, 0.1))
    x, y = np.interp(s, path.s, path.x), np.interp(s, path.s, path.y)
    j = np.clip(np.searchsorted(path.s, s, side="right") - 1, 0, path.n - 2)
    tang = np.arctan2(path.y[j + 1] - path.y[j], path.x[j + 1] - path.x[j])
    yaw = tang + head
    out = np.zeros((T, POSE_ROWS))
    out[:, 0], out[:, 1] = x - lat * np.sin(tang), y + lat * np.cos(tang)
    out[:, 2], out[:, 3] = np.sin(0.5 * yaw), np.cos(0.5 * yaw)
    out[:, 4] = substeps * k
    if rng.uniform() < 0.02:
        out[int(rng.integers(2, T)):, 5] = 1.0
    return out


def pose_sequences(paths, ticks, seed, substeps=10):
    """[ticks + 1, POSE_ROWS, B]."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([pose_sequence(p, ticks, rng, substeps) for p in paths], axis=-1))


GUARD = 777


class RawTask:
    """The task's handle and caller-owned buffers without controller or simulator: poses are written into `sim`."""

    def __init__(self, paths, dev, packed=None, **task):
        """packed: the host arrays handed to set_path in place of goto_path.pack_paths(paths, n_max) (a test that changes them)."""
        import torch
        B = self.batch = len(paths)
        self.torch = torch
        self.handle = goto_abi.GotoHandle(B, None, dev, **task)
        f = self.handle.fields
        n_max, self.ncp = f["n_max"], f["num_cam_pts"]
        z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
        self._guarded = []

        def g(rows, dtype=torch.float64):
            """rows x B zeros between two guard rows of GUARD that the kernels must leave as they are"""
            back = torch.full((rows + 2, B), GUARD, dtype=dtype, device=dev)
            back[1:-1] = 0
            self._guarded.append(back)
            return back[1:-1]
        self.state, self.sim = g(goto_abi.STATE_ROWS), z(srb_abi.STATE_ROWS, B)
        self.px, self.py, self.ps, self.pf, self.hdr = z(B, n_max), z(B, n_max), z(B, n_max), z(B, n_max, dtype=torch.int32), z(goto_abi.HDR_ROWS, B)
        self.ptrs = goto_abi.CPathPtrs(self.px.data_ptr(), self.py.data_ptr(), self.ps.data_ptr(), self.pf.data_ptr(), self.hdr.data_ptr())
        self.obs, self.reward, self.done = g(2 * self.ncp, torch.float32), g(1, torch.float32)[0], g(1, torch.int32)[0]
        self.action, self.cmd = z(B, 2, dtype=torch.float32), g(3, torch.float32)
        self.handle.set_path(self.ptrs, self.state.data_ptr(), None, **(packed or goto_path.pack_paths(paths, n_max)))

    def set_path(self, idx, paths):
        """New paths for robots idx (rg_goto_set_path with an index list)."""
        self.handle.set_path(self.ptrs, self.state.data_ptr(), idx, **goto_path.pack_paths(paths, self.handle.n_max))

    def guards_intact(self):
        return all(bool((t[0] == GUARD).all()) and bool((t[-1] == GUARD).all()) for t in self._guarded)

    def pose(self, rows):
        """rows [POSE_ROWS, B] host array -> the simulator state rows the task reads."""
        t = self.torch.as_tensor(rows, device=self.sim.device)
        self.sim[srb_abi.ROW_P:srb_abi.ROW_P + 2] = t[0:2]
        self.sim[srb_abi.ROW_QUAT + 2:srb_abi.ROW_QUAT + 4] = t[2:4]
        self.sim[srb_abi.ROW_STEPS], self.sim[srb_abi.ROW_STATUS] = t[4], t[5]

    def observe(self):
        self.handle.observe(self.state.data_ptr(), self.sim.data_ptr(), self.ptrs, self.obs.data_ptr())

    def post(self):
        self.handle.post_step(self.state.data_ptr(), self.sim.data_ptr(), self.ptrs, self.obs.data_ptr(), self.reward.data_ptr(), self.done.data_ptr())

    def pre(self):
        self.handle.pre_step(self.state.data_ptr(), self.sim.data_ptr(), self.ptrs, self.action.data_ptr(), self.cmd.data_ptr())


RECORD = ("visible", "chain", "latched", "next_cp", "done", "reason", "reward", "margin", "margin_frame", "frozen", "overflow",
          "margin_frame_ties_ok", "zero_links")


def run_model_robot(c, path, poses):
    """The model over one robot's pose sequence [T + 1, POSE_ROWS] -> dict of per-tick arrays [T] and obs [T, 2 ncp]
    (tick 0, the observe of the reset, is not recorded, but its observation seeds the latch)."""
    st = goto_model.new_state()
    T = len(poses) - 1
    rec = {k: np.zeros(T) for k in RECORD}
    obs = np.zeros((T, 2 * c["num_cam_pts"]), dtype=np.float32)
    p = poses[0]
    first = goto_model.post_step(c, st, path, p[0:2], (0.0, 0.0, p[2], p[3]), p[5], p[4], observe_only=True)
    obs0, margin0, margin0_ties_ok = first["obs"], first["margin_frame"], first["margin_frame_ties_ok"]
    for t in range(1, T + 1):
        p = poses[t]
        r = goto_model.post_step(c, st, path, p[0:2], (0.0, 0.0, p[2], p[3]), p[5], p[4])
        k = t - 1
        obs[k] = r["obs"]
        rec["visible"][k], rec["chain"][k], rec["latched"][k] = st[goto_abi.ROW_VISIBLE], st[goto_abi.ROW_CHAIN], st[goto_abi.ROW_LATCHED]
        rec["next_cp"][k], rec["done"][k], rec["reason"][k] = st[goto_abi.ROW_NEXT_CP], r["done"], st[goto_abi.ROW_REASON]
        rec["reward"][k], rec["margin"][k], rec["frozen"][k], rec["overflow"][k] = r["reward"], r["margin"], r["frozen"], st[goto_abi.ROW_OVERFLOW]
        rec["margin_frame"][k], rec["margin_frame_ties_ok"][k], rec["zero_links"][k] = r["margin_frame"], r["margin_frame_ties_ok"], r["zero_links"]
    rec["obs"], rec["obs0"], rec["margin0"], rec["margin0_ties_ok"] = obs, obs0, margin0, margin0_ties_ok
    return rec


def _chunk(args):
    c, paths, poses = args
    return [run_model_robot(c, p, poses[:, :, k]) for k, p in enumerate(paths)]


def run_model(c, paths, poses, workers=None):
    """The model over every robot -> dict of [T, B] arrays, obs [T, 2 ncp, B], obs0 [2 ncp, B] and margin0 [B].  With more
    than one worker the robots are split over a pool of SPAWNED processes (at most 15: the children import this module
    afresh and inherit nothing of the parent, a GPU it may hold open included -- a forked child would)."""
    B = len(paths)
    workers = workers or min(15, os.cpu_count() or 1, max(1, B // 8))
    bounds = np.linspace(0, B, workers * 4 + 1).astype(int) if workers > 1 else np.array([0, B])
    jobs = [(c, paths[a:b], poses[:, :, a:b]) for a, b in zip(bounds[:-1], bounds[1:]) if b > a]
    if workers > 1:
        with ProcessPoolExecutor(workers, mp_context=multiprocessing.get_context("spawn")) as ex:
            parts = list(ex.map(_chunk, jobs))
    else:
        parts = [_chunk(j) for j in jobs]
    recs = [r for part in parts for r in part]
    out = {k: np.stack([r[k] for r in recs], axis=-1) for k in RECORD + ("obs", "obs0")}
    out["margin0"] = np.array([r["margin0"] for r in recs])
    out["margin0_ties_ok"] = np.array([r["margin0_ties_ok"] for r in recs])
    return out


def excluded(model, threshold=1e-9, ties_ok=False):
    """(tick, obs): two bool [T, B] masks of the robot-ticks a comparison may leave out.  ties_ok: judge by
    margin_frame_ties_ok, which does not count the exact tie between copies of one path point, so that those ticks are compared.
    tick: a rounding-sensitive decision of THAT tick (goto_model's margin_frame: window edge, chain arg-min, continuity
    break) lay within `threshold` of flipping -- every output of the tick may be left out.
    obs: the same ticks, and after such a tick (or such a reset observation) the following ticks for as long as the model
    keeps the latch (latched == 0, or the robot is frozen): the observation they show is the doubtful one carried on.
    Nothing else is carried: reward, checkpoints, done and its cause do not depend on those decisions."""
    tick = model["margin_frame_ties_ok" if ties_ok else "margin_frame"] < threshold
    kept = (model["latched"] == 0) | (model["frozen"] != 0)
    obs = np.zeros_like(tick)
    carry = model["margin0_ties_ok" if ties_ok else "margin0"] < threshold
    for t in range(len(tick)):
        carry = tick[t] | (carry & kept[t])
        obs[t] = carry
    return tick, obs
