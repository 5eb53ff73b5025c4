#!/usr/bin/env python3
"""Golden vectors of the go-to-target task, recorded by RUNNING THE REFERENCE'S FUNCTIONS (authoring machine only).

    RG_REFERENCE=/path/to/robot-gym python tests/golden/make_goto_golden.py

Writes tests/golden/goto_reference.npz.  Nothing of the reference's source travels: only seeded inputs and the outputs its
code produced.  The two modules are loaded by file, so nothing else of the reference is imported:

  planner_*   potential_field_planner.get_path (numpy only; `matplotlib.pyplot` is stubbed when it is absent) on N_TARGETS
              targets from GoEnv's own distribution (go_env.py:163-175) plus N_OBSTACLE cases with obstacles: targets,
              obstacles, and the returned way points, stored flat with offsets
  sort_*      line_interpolation.sort_points (pure numpy; `shapely.geometry` is stubbed for the module-level import only and
              never called) on N_CLOUDS point clouds: 1 cm polylines seen from a nearby origin, shuffled, some with a gap
              above the 30 mm continuity break: the clouds and the returned points, flat with offsets

The authoring machine has no shapely, so Path, Follower and CameraWindow cannot be run; what they do with it (arc-length
interpolation, closed point-in-polygon, minimum point-to-point distance, rigid moves) has documented semantics and is pinned
by tests/goto_model.py alone.  On a machine WITH shapely, `--shapely` additionally records
interpolate_points and Path on the planner cases into goto_reference_shapely.npz, for a comparison with
robot_gym_amd.gym.goto_path.build_path.

The file is compared with the committed one before it is replaced, and the script says whether its arrays are identical.
"""
import importlib.util
import os
import sys
import types

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
N_TARGETS, N_OBSTACLE, N_CLOUDS = 200, 8, 200
GO_TO = os.path.join("robot_gym", "gym", "envs", "go_to")


def _stub(name, **attrs):
    try:
        __import__(name)
    except ImportError:
        parts = name.split(".")
        for k in range(1, len(parts) + 1):
            sub = ".".join(parts[:k])
            if sub not in sys.modules:
                sys.modules[sub] = types.ModuleType(sub)
                if k > 1:
                    setattr(sys.modules[".".join(parts[:k - 1])], parts[k - 1], sys.modules[sub])
        for k, v in attrs.items():
            setattr(sys.modules[name], k, v)


def _load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, GO_TO, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _never(*a, **k):
    raise RuntimeError("the shapely stub was called: this recording must not depend on shapely")


def _target(rng):
    out = []
    for _ in range(2):
        v = round(float(rng.uniform(-2.5, 2.5)), 2)
        if 1.0 > v > 0:
            v = 1.0
        if -1.0 < v < 0:
            v = -1.0
        out.append(v)
    return out


def _flat(arrays):
    off = np.cumsum([0] + [len(a) for a in arrays]).astype(np.int64)
    return (np.concatenate(arrays, axis=0) if arrays else np.zeros((0, 2))), off


def record(ref):
    _stub("matplotlib.pyplot")
    _stub("shapely.geometry", LineString=_never)
    planner = _load(ref, os.path.join("path_planner", "potential_field_planner.py"), "ref_potential_field_planner")
    interp = _load(ref, os.path.join("path_follower", "line_interpolation.py"), "ref_line_interpolation")
    planner.print = lambda *a, **k: None   # "outside potential!" / "Oscillation detected" chatter
    rng = np.random.default_rng(20240611)
    targets, obstacles, paths = [], [], []
    for k in range(N_TARGETS + N_OBSTACLE):
        t = _target(rng)
        obs = np.zeros((0, 2))
        if k >= N_TARGETS:   # a few obstacles near the straight line, none on the start or the target
            m = int(rng.integers(1, 4))
            lam = rng.uniform(0.3, 0.7, m)
            obs = np.round(np.outer(lam, t) + rng.uniform(-0.3, 0.3, (m, 2)), 2)
        x, y = planner.get_path(t[0], t[1], list(obs[:, 0]), list(obs[:, 1]))
        targets.append(t)
        obstacles.append(obs)
        paths.append(np.stack((np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)), axis=-1))
    clouds, chains = [], []
    for k in range(N_CLOUDS):
        m = int(rng.integers(2, 40))
        ang = np.cumsum(rng.uniform(-0.15, 0.15, m)) + rng.uniform(-np.pi, np.pi)
        step = np.full(m, 0.01)
        if k % 4 == 0 and m > 4:
            step[int(rng.integers(2, m - 1))] = rng.uniform(0.031, 0.06)   # a continuity break
        pts = np.cumsum(np.stack((step * np.cos(ang), step * np.sin(ang)), axis=-1), axis=0) + rng.uniform(-0.05, 0.05, 2)
        pts = pts[rng.permutation(m)]
        clouds.append(pts)
        chains.append(np.asarray(interp.sort_points(pts), dtype=np.float64).reshape(-1, 2))
    out = dict(planner_targets=np.asarray(targets))
    out["planner_obstacles"], out["planner_obstacles_off"] = _flat(obstacles)
    out["planner_paths"], out["planner_paths_off"] = _flat(paths)
    out["sort_clouds"], out["sort_clouds_off"] = _flat(clouds)
    out["sort_chains"], out["sort_chains_off"] = _flat(chains)
    return out


def _save(name, **arrays):
    """Write tests/golden/<name>, and say whether its arrays equal the ones of the file it replaces."""
    path = os.path.join(OUT, name)
    verdict = "new file"
    if os.path.exists(path):
        old = np.load(path)
        same = sorted(old.files) == sorted(arrays) and all(np.array_equal(old[k], arrays[k]) for k in arrays)
        verdict = "arrays identical to the committed file" if same else "ARRAYS CHANGED"
    np.savez_compressed(path, **arrays)
    print(f"{name}: {os.path.getsize(path)} bytes, {verdict}")
    return verdict


def record_shapely(ref, golden):
    """With shapely installed: interpolate_points as Path.__init__ calls it, on the recorded planner cases."""
    import shapely.geometry  # noqa: F401  (the real one; fails where it is absent)
    interp = _load(ref, os.path.join("path_follower", "line_interpolation.py"), "ref_line_interpolation_real")
    from shapely.geometry import LineString
    pts_all, off = [], golden["planner_paths_off"]
    for k in range(len(off) - 1):
        pts = golden["planner_paths"][off[k]:off[k + 1]]
        n = int(LineString(pts).length / 1e-2)
        pts_all.append(np.asarray(interp.interpolate_points(np.array(pts), n)))
    out = {}
    out["path_points"], out["path_points_off"] = _flat(pts_all)
    return out


if __name__ == "__main__":
    ref = os.environ.get("RG_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, GO_TO)):
        sys.exit("set RG_REFERENCE to a checkout of the reference (it holds " + GO_TO + ")")
    if "--shapely" in sys.argv:
        _save("goto_reference_shapely.npz", **record_shapely(ref, np.load(os.path.join(OUT, "goto_reference.npz"))))
    else:
        _save("goto_reference.npz", **record(ref))
