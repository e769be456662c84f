#!/usr/bin/env python3
"""Writes tests/golden/ndt_tiny_models.npz: the Euler-angle model (tools/ndt_euler_ref.sweep_euler) and PCL's f64 class (tools/ndt_pcl_ref.sweep_pcl)
evaluated on the tiny scenes of tests/ndt_ref.py -- a 4 x 4 x 4-cell target, so out-of-grid points, a NaN row and grid-face cells, 37 m and 580 m
from the origin -- for tests/test_tiny_scene_models_gpu.py.  Every hit of the Euler model is evaluated in Python: a case costs seconds, hence a
fixture; tests/test_tiny_scene_models_cpu.py regenerates cases of it word for word.

  euler/<scene>/<pose>/<n>/<search>/<order>/{score, g, H, hits}      search: direct1, direct7, direct26, kdtree; order: the f32 sum order
  pcl/<scene>/<pose>/<n>/{score, g, H, hits}

Run:  python tests/golden/make_tiny_models.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import ndt_ref as R  # noqa: E402

FIXTURE = os.path.join(HERE, "ndt_tiny_models.npz")
SCENES = ("mid", "far")
SIZES = (1, 64, 65, 513)                      # one lane, one tile, a tile and one point, an item (512 points) and one point
ANGLES = {"yaw": (0.0, 0.0, 0.02), "rpy": (0.12, 0.15, 0.2)}          # roll, pitch, yaw about the block's centre
OUTLIER_RATIO = 0.55


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


P = _load("ndt_pcl_ref")
E = P.E
mg = E.mg
SEARCHES = {"direct1": E.DIRECT1, "direct7": E.DIRECT7, "direct26": E.DIRECT26, "kdtree": E.KDTREE}
_grids = {}


def pose_vector(scene_name, pose_name):
    """[x, y, z, roll, pitch, yaw] of the rotation Rx Ry Rz about the centre c of the scene's block: t = c - R c"""
    c = R.named_scene(scene_name).centre
    a = np.array(ANGLES[pose_name], np.float64)
    return np.concatenate([c - E.rot64(np.concatenate([np.zeros(3), a])) @ c, a])


def source(scene_name, n):
    """the scene's first n source points as they lie (from 8 points on: three of them outside the grid, one NaN row), f32"""
    return R.named_scene(scene_name).source64(n).astype(np.float32)


def grid_of(scene_name):
    if scene_name not in _grids:
        sc = R.named_scene(scene_name)
        _grids[scene_name] = mg.build_grid(np.array(sc.target), sc.leaf)
    return _grids[scene_name]


def euler_case(scene_name, pose_name, n, search, order):
    d1, d2, _ = mg.gauss_constants(OUTLIER_RATIO, R.named_scene(scene_name).leaf)
    return E.sweep_euler(grid_of(scene_name), source(scene_name, n), pose_vector(scene_name, pose_name), d1, d2, SEARCHES[search], order)


def pcl_case(scene_name, pose_name, n):
    d1, d2, _ = mg.gauss_constants(OUTLIER_RATIO, R.named_scene(scene_name).leaf)
    return P.sweep_pcl(P.Cells(grid_of(scene_name)), source(scene_name, n), pose_vector(scene_name, pose_name), d1, d2)


def euler_key(scene_name, pose_name, n, search, order):
    return f"euler/{scene_name}/{pose_name}/{n}/{search}/{order}"


def pcl_key(scene_name, pose_name, n):
    return f"pcl/{scene_name}/{pose_name}/{n}"


def _job(args):
    return args, (euler_case(*args) if len(args) == 5 else pcl_case(*args))


def make_fixture(path=FIXTURE, procs=None):
    import multiprocessing as mp
    cases = [(s, p, n) for s in SCENES for p in ANGLES for n in SIZES]
    jobs = [c + (m, o) for c in cases for m in SEARCHES for o in (0, 1)] + cases
    jobs.sort(key=lambda j: -j[2])                                   # the long ones first
    out = {}
    with mp.Pool(procs or min(8, os.cpu_count() or 1)) as pool:
        for args, r in pool.imap_unordered(_job, jobs):
            E._pack_sweep(out, euler_key(*args) if len(args) == 5 else pcl_key(*args), r)
            print(args, "hits", r[3], flush=True)
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(path, os.path.getsize(path), "B")


if __name__ == "__main__":
    make_fixture()
