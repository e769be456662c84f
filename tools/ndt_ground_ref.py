#!/usr/bin/env python3
"""Restatement of pclomp_ground::NormalDistributionsTransformGround (include/ndt_omp/ndt_ground.h, ndt_ground_impl.hpp) in NumPy: the
contract the engine's MI355NDT_OPT_GROUND_CLASS is held to.  Independent of the library: nothing here loads it.

The class is ndt_omp model 0 (ndt_omp_impl2.hpp) on the same pclomp::VoxelGridCovariance.  Everything shared is imported, unchanged, from
tests/golden/make_golden.py: the grid build, the neighbourhoods of the DIRECT searches, transform_point, point_derivatives,
update_derivatives (ndt_ground_impl.hpp's is impl2's but for the class name and the flag_class argument), the Gauss constants, se3_exp /
se3_log.  What is restated here, line by line:

  leaf_normal              make_golden.Leaf has no evecs slot: the covariance is recomputed from (C, S, n) by make_golden.build_grid's own
                           formula (vgc:329-330), un-inflated, and decomposed as there (lower triangle, ascending); evecs_.col(0).
  leaf_angle               ndt_ground_impl.hpp:503-507: the normal normalised again, acos(|n_z|) * 180 / 3.1415926.
  sweep_ground             computeDerivatives_seg, :484-567: every hit evaluated TWICE into the point's gradient and Hessian (:519, :522),
                           the second call's return value alone into the score; the point's sums added under the class of the LAST
                           neighbour in the search's order (:527-544; a point without neighbours keeps angle2xy = 0); rows and columns
                           zeroed after the sum (:554-567).
  align_ground             computeTransformation, :87-180, with computeStepLengthMT up to the dead More-Thuente loop: impl2's, except
                           that the convergence test (:173) has no `nr_iterations_ &&` guard.

flag_class is the reference's own number: 0 every point and no mask, 1 horizontal leaves (angle2xy < 10), 2 vertical leaves (> 80).
MI355NDT_OPT_GROUND_CLASS = 1 / 2 / 3 are flag_class 1 / 2 / 0 (OPTION_OF_FLAG).

Run:  python tools/ndt_ground_ref.py            rewrites tests/golden/ndt_ground.npz (minutes: every hit is evaluated in Python, twice)
      python tools/ndt_ground_ref.py choose     prints, for candidate scenes and aligns, whether they satisfy the fixture's conditions
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402

f32, f64 = np.float32, np.float64
DIRECT1, DIRECT7, DIRECT26 = mg.DIRECT1, mg.DIRECT7, mg.DIRECT26
FIXTURE = os.path.join(ROOT, "tests", "golden", "ndt_ground.npz")
OPTION_OF_FLAG = {1: 1, 2: 2, 0: 3}                                  # flag_class -> MI355NDT_OPT_GROUND_CLASS
FLAGS = (1, 2, 0)
MIN_ANGLE_MARGIN = 0.5                                               # degrees between any valid leaf's angle and either threshold
MIN_EIGEN_GAP = 1e-6                                                 # (ev1 - ev0) / ev2 of any valid leaf


# ----------------------------------------------------------------------------- leaves
def leaf_normal(L):
    """(evecs_.col(0), evals) of the un-inflated covariance (vgc:329-335)"""
    n = L.n_pushed
    cov = (L.C - 2 * np.outer(L.S, L.mean)) / n + np.outer(L.mean, L.mean)      # vgc:329
    cov = cov * ((n - 1.0) / n)                                                 # vgc:330
    low = np.tril(cov) + np.tril(cov, -1).T
    ev, V = np.linalg.eigh(low)
    return V[:, 0], ev


def leaf_angle(L):
    """ndt_ground_impl.hpp:503-507"""
    nrm, _ = leaf_normal(L)
    nrm = nrm / np.linalg.norm(nrm)                                             # normal.normalize()
    return float(np.arccos(np.fabs(nrm[2])) * 180 / 3.1415926)


def class_code(angle):
    """the engine's code of a live leaf: 1 = angle2xy < 10, 2 = angle2xy > 80, 3 = neither (0 = not a neighbour)"""
    return 1 if angle < 10 else (2 if angle > 80 else 3)


def records(grid):
    """the leaves applyFilter pushed (>= min_points then), in cell order: the engine's leaf records"""
    return [L for _, L in sorted(grid["leaves"].items()) if L.n_pushed >= grid["min_points"]]


def leaf_codes(grid):
    """one code per record"""
    return np.array([0 if L.n == -1 else class_code(leaf_angle(L)) for L in records(grid)], np.uint8)


def scene_conditions(grid):
    """(smallest distance of a valid leaf's angle from 10 and from 80 degrees, smallest (ev1 - ev0) / ev2 of a valid leaf)"""
    ang, gap = [], []
    for L in records(grid):
        if L.n == -1:
            continue
        ang.append(leaf_angle(L))
        ev = leaf_normal(L)[1]
        gap.append((ev[1] - ev[0]) / ev[2])
    ang = np.array(ang)
    return float(np.abs(ang - 10).min()), float(np.abs(ang - 80).min()), float(np.min(gap))


def assert_scene(grid, what):
    m10, m80, gap = scene_conditions(grid)
    assert m10 >= MIN_ANGLE_MARGIN and m80 >= MIN_ANGLE_MARGIN, (what, m10, m80)
    assert gap >= MIN_EIGEN_GAP, (what, gap)
    return m10, m80, gap


# ----------------------------------------------------------------------------- sweep
def passes(flag, angle2xy):
    """:527-544"""
    return flag == 0 or (flag == 1 and angle2xy < 10) or (flag == 2 and angle2xy > 80)


def sweep_ground(grid, src, T32, M32, d1, d2, mode, flags=FLAGS, angles=None):
    """computeDerivatives_seg, :484-567, for every flag_class of `flags` in one pass over the points (a point's sums do not depend on the flag,
    only whether they are added).  Returns {flag: (score, g, H, hits, points_added)}; hits = the evaluated hits of the points added."""
    angles = {} if angles is None else angles
    acc = {f: [0.0, np.zeros(6), np.zeros((6, 6)), 0, 0] for f in flags}
    for p in np.asarray(src, f32):
        if not np.isfinite(p).all():
            continue
        xt = mg.transform_point(T32, p)
        if not np.isfinite(xt).all():
            continue
        s_pt, g_pt, H_pt = 0.0, np.zeros(6), np.zeros((6, 6))
        angle2xy, nh = 0.0, 0                                                   # :495
        for L in mg.neighbourhood(grid, xt, mode):
            x_trans = xt.astype(f64) - L.mean
            J, Hp = mg.point_derivatives(p, M32)
            if id(L) not in angles:
                angles[id(L)] = leaf_angle(L)
            angle2xy = angles[id(L)]                                            # :503-507: overwritten by every neighbour
            mg.update_derivatives(g_pt, H_pt, J, Hp, x_trans, L.icov, d1, d2)   # :519
            s_pt += mg.update_derivatives(g_pt, H_pt, J, Hp, x_trans, L.icov, d1, d2)   # :522
            nh += 1
        for f in flags:
            if passes(f, angle2xy):                                             # :527-544
                a = acc[f]
                a[0] += s_pt; a[1] += g_pt; a[2] += H_pt; a[3] += nh; a[4] += 1
    out = {}
    for f in flags:
        score, g, H, hits, used = acc[f]
        if f == 1:                                                              # :554-560
            H[:, 0] = 0; H[:, 1] = 0; H[:, 5] = 0; H[0, :] = 0; H[1, :] = 0; H[5, :] = 0
            g[0] = 0; g[1] = 0; g[5] = 0
        if f == 2:                                                              # :561-567
            H[:, 2] = 0; H[:, 3] = 0; H[:, 4] = 0; H[2, :] = 0; H[3, :] = 0; H[4, :] = 0
            g[2] = 0; g[3] = 0; g[4] = 0
        out[f] = (score, g, H, hits, used)
    return out


def deciding_codes(grid, src, T32, mode):
    """per source point: (code of the first live neighbour, code of the last one), 0 0 without neighbours"""
    out = []
    for p in np.asarray(src, f32):
        hood = mg.neighbourhood(grid, mg.transform_point(T32, p), mode)
        out.append((class_code(leaf_angle(hood[0])), class_code(leaf_angle(hood[-1]))) if hood else (0, 0))
    return np.array(out, np.int64)


# ----------------------------------------------------------------------------- align
def solve_newton(H, g):
    """JacobiSVD(H).solve(-g): the thresholded pseudo-inverse (as make_golden.align_dead_mt); returns (delta_p, rank)"""
    U, S, Vt = np.linalg.svd(H)
    rank = int((S >= max(S[0] * 6 * np.finfo(f64).eps, np.finfo(f64).tiny)).sum()) if S[0] > 0 else 0
    return Vt[:rank].T @ ((U[:, :rank].T @ (-g)) / S[:rank]), rank


def align_ground(grid, src, guess32, prm, flag):
    """computeTransformation, ndt_ground_impl.hpp:87-180 (flag_class hard-coded to 1 there; any of the three here)"""
    assert prm["step_size"] - prm["trans_epsilon"] / 2 > 0
    d1, d2, _ = mg.gauss_constants(prm["outlier_ratio"], prm["resolution"])
    eps, step, mode = prm["trans_epsilon"], prm["step_size"], prm["neighbor_mode"]
    angles = {}
    final = np.array(guess32, f32)
    p = mg.se3_log(final.astype(f64))
    score, g, H, hits, _ = sweep_ground(grid, src, final, mg.se3_exp(p).astype(f32), d1, d2, mode, (flag,), angles)[flag]
    inc = prev_inc = np.eye(4, dtype=f32)
    it, sweeps, steps, ranks = 0, 1, [], []
    while True:
        prev_inc = inc
        dp, rank = solve_newton(H, g)
        n = np.linalg.norm(dp)
        if n == 0 or n != n:
            return dict(final=final, iterations=it, converged=bool(n == n), score=score, hits=hits, sweeps=sweeps, inc=inc, prev_inc=prev_inc,
                        steps=np.array(steps), ranks=np.array(ranks, np.int64), p=p)
        dp = dp / n
        dphi0 = -(g @ dp)
        if dphi0 >= 0 and dphi0 == 0:
            a = 0.0
        else:
            if dphi0 >= 0:
                dp = -dp
            a = max(min(n, step), eps / 2)
            xt = p + dp * a
            final = mg.se3_exp(xt).astype(f32)
            score, g, H, hits, _ = sweep_ground(grid, src, final, final, d1, d2, mode, (flag,), angles)[flag]
            sweeps += 1
        dpv = dp * a
        inc = mg.se3_exp(dpv).astype(f32)                                       # transformation_
        p = mg.se3_log(mg.se3_exp(dpv) @ mg.se3_exp(p))
        steps.append(a); ranks.append(rank)
        conv = it > prm["max_iterations"] or abs(a) < eps                       # :173: no `nr_iterations_ &&`
        it += 1
        if conv:
            return dict(final=final, iterations=it, converged=True, score=score, hits=hits, sweeps=sweeps, inc=inc, prev_inc=prev_inc,
                        steps=np.array(steps), ranks=np.array(ranks, np.int64), p=p)


# ----------------------------------------------------------------------------- hand-made scenes
def _patch(cx, cy, cz, normal, n=8, r=0.2):
    """n points on a small disc around (cx, cy, cz) in the plane with the given normal, slightly off it so that no eigenvalue is zero"""
    nrm = np.asarray(normal, f64) / np.linalg.norm(normal)
    a = np.cross(nrm, [1.0, 0.3, 0.2]); a /= np.linalg.norm(a)
    b = np.cross(nrm, a)
    k = np.arange(n)
    th = 2 * np.pi * k / n + 0.3
    rad = r * (0.5 + 0.5 * ((k * 3) % n) / n)
    off = 0.004 * np.where(k % 2 == 0, 1.0, -1.0) * (1 + 0.3 * (k % 3))
    return (np.array([cx, cy, cz]) + rad[:, None] * (np.cos(th)[:, None] * a + np.sin(th)[:, None] * b) + off[:, None] * nrm).astype(f32)


def three_leaf_scene():
    """(target, expected codes): a flat patch, a wall and a 45 degree ramp of 8 points each in three cells of a 1 m grid, and 5 points in a
    fourth cell, which is no record at all"""
    flat = _patch(0.5, 0.5, 0.5, (0, 0, 1))
    wall = _patch(2.5, 0.5, 0.5, (1, 0, 0))
    ramp = _patch(4.5, 0.5, 0.5, (1, 0, 1))
    few = _patch(6.5, 0.5, 0.5, (0, 0, 1), n=5)
    return np.concatenate([flat, wall, ramp, few]), [1, 2, 3]


def floor_wall_scene():
    """(target, source): a floor cell (0, 0, 0) with a wall cell above it (0, 0, 1) and beside it (1, 0, 0), a ramp further on, a cell with ONE
    point at (6, 0, 0), 1 m grid, min_points_per_voxel = 1 (HAND_MIN_POINTS): the one-point cell is a record and a dead leaf (its covariance
    is zero, vgc:330, 337-341).  Source points, at the identity pose:
      in the floor cell       DIRECT7 neighbours: floor, wall beside (+x), wall above (+z) -- first horizontal, last vertical
      in the wall cell above  DIRECT7: wall above, floor (-z) -- first vertical, last horizontal
      in the wall cell beside DIRECT7: wall beside, floor (-x) -- first vertical, last horizontal
      in the dead cell        its only neighbour is the dead leaf: no neighbour at all
      next to the dead cell   (5, 0, 0): DIRECT7 reaches the dead leaf alone
      far outside the grid    no neighbour"""
    floor = _patch(0.5, 0.5, 0.5, (0, 0, 1), n=10)
    above = _patch(0.5, 0.5, 1.5, (1, 0, 0), n=9)
    beside = _patch(1.5, 0.5, 0.5, (0, 1, 0), n=9)
    ramp = _patch(3.5, 0.5, 0.5, (1, 0, 1), n=8)
    dead = np.array([[6.5, 0.5, 0.5]], f32)
    tgt = np.concatenate([floor, above, beside, ramp, dead])
    src = np.array([[0.4, 0.6, 0.45], [0.6, 0.4, 0.55], [0.45, 0.5, 1.4], [0.55, 0.45, 1.6], [1.4, 0.5, 0.6], [1.6, 0.55, 0.4],
                    [3.4, 0.5, 0.6], [6.4, 0.5, 0.5], [5.5, 0.5, 0.5], [40.0, 40.0, 40.0], [-30.0, 0.5, 0.5]], f32)
    return tgt, src


IDENTITY_P = np.zeros(6)
HAND_MIN_POINTS = 1


def floor_wall_grid():
    return mg.build_grid(floor_wall_scene()[0], 1.0, min_points=HAND_MIN_POINTS)


def hand_sweeps(mode):
    """the floor-next-to-wall scene's sums at the identity pose, resolution 1.0: {flag: (score, g, H, hits, points_added)}"""
    _, src = floor_wall_scene()
    grid = floor_wall_grid()
    d1, d2, _ = mg.gauss_constants(0.55, 1.0)
    T = mg.se3_exp(IDENTITY_P).astype(f32)
    return sweep_ground(grid, src, T, T, d1, d2, mode)


# ----------------------------------------------------------------------------- fixture
PRM = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, trans_epsilon=0.01, max_iterations=64, neighbor_mode=DIRECT7, variant=0,
           min_points_per_voxel=6, min_covar_eigvalue_mult=0.01)
SHAPE_PAIR, SHAPE_RES, SHAPE_SIZES = 2, 1.0, (1, 64, 65, 513, 2049)
SHAPE_START = 26                                                      # the first source point that meets a leaf (tools/ndt_euler_ref.py)
LAST_N = 500
# name -> (pair, resolution, search): the scenes of the "last neighbour decides" sweeps; chosen with `choose`
LAST_SCENES = {"direct7": (2, 1.0, DIRECT7), "direct26": (5, 2.0, DIRECT26)}
MIN_DIFFERING = 20                                                    # source points whose first and last live neighbours have different codes
ALIGN_N = 500
# (pair, resolution, search, flag_class): chosen with `choose` so that no step length lies within 5 % of trans_epsilon and the scene
# conditions hold; the first is the nodelet's ground_s2k configuration, the second ends after ONE iteration with a step of 0.0064 (the rule of
# :173; ndt_omp's rule would not end there).  Pair 1 at resolution 1.0 ends after one iteration too, but its grid has a leaf 0.059 degrees from
# a threshold, so it is no fixture scene.
ALIGNS = [(1, 10.0, DIRECT1, 1), (5, 1.0, DIRECT1, 1), (2, 1.0, DIRECT1, 2), (2, 1.0, DIRECT1, 0), (2, 1.0, DIRECT7, 1), (2, 1.0, DIRECT7, 2),
          (2, 1.0, DIRECT7, 0)]


def clouds(k):
    from lv_slam_amd import synth
    tgt, src, _ = synth.make_pair(k, 256, n_beams=32)
    return tgt.numpy(), src.numpy()


def default_guess():
    from lv_slam_amd import synth
    return synth.default_guess()


def subsample(src, n):
    return src[:: max(1, len(src) // n)][:n]


def sweep_pose():
    """(p, T32): the pose of the fixture's sweeps -- the tangent of default_guess(), and the f32 matrix mi355ndt_derivatives moves the cloud by"""
    p = mg.se3_log(default_guess().astype(f64))
    return p, mg.se3_exp(p).astype(f32)


def shape_source(n):
    _, src = clouds(SHAPE_PAIR)
    return subsample(src[SHAPE_START:], n)


def shape_case(n):
    tgt, _ = clouds(SHAPE_PAIR)
    grid = mg.build_grid(tgt, SHAPE_RES)
    d1, d2, _ = mg.gauss_constants(0.55, SHAPE_RES)
    _, T = sweep_pose()
    return sweep_ground(grid, shape_source(n), T, T, d1, d2, DIRECT1)


def last_source(name):
    _, src = clouds(LAST_SCENES[name][0])
    return subsample(src, LAST_N)


def last_case(name):
    pair, res, mode = LAST_SCENES[name]
    tgt, _ = clouds(pair)
    grid = mg.build_grid(tgt, res)
    d1, d2, _ = mg.gauss_constants(0.55, res)
    _, T = sweep_pose()
    s = last_source(name)
    codes = deciding_codes(grid, s, T, mode)
    differing = int((codes[:, 0] != codes[:, 1]).sum())
    return sweep_ground(grid, s, T, T, d1, d2, mode), differing


def align_inputs(i):
    pair, res, mode, flag = ALIGNS[i]
    tgt, src = clouds(pair)
    return tgt, subsample(src, ALIGN_N), default_guess(), res, mode, flag


def align_case(i):
    tgt, s, G, res, mode, flag = align_inputs(i)
    return align_ground(mg.build_grid(tgt, res), s, G, dict(PRM, resolution=res, neighbor_mode=mode), flag)


def steps_clear(steps, eps=PRM["trans_epsilon"]):
    return bool((np.abs(np.asarray(steps) - eps) > 0.05 * eps).all())


def fixture_scenes():
    """every (pair, resolution) a fixture case builds a grid for"""
    return sorted({(SHAPE_PAIR, SHAPE_RES)} | {(p, r) for p, r, _ in LAST_SCENES.values()} | {(p, r) for p, r, _, _ in ALIGNS})


def _pack_sweeps(out, key, by_flag):
    for f, (score, g, H, hits, used) in by_flag.items():
        k = f"{key}/{OPTION_OF_FLAG[f]}"
        out[k + "/score"] = np.float64(score); out[k + "/g"] = g; out[k + "/H"] = H; out[k + "/hits"] = np.int64(hits); out[k + "/used"] = np.int64(used)


def _pack_align(out, key, r):
    for f in ("final", "inc", "prev_inc", "steps", "ranks", "p"):
        out[key + "/" + f] = r[f]
    for f in ("iterations", "converged", "sweeps", "hits"):
        out[key + "/" + f] = np.int64(r[f])
    out[key + "/score"] = np.float64(r["score"])


def scene_case(arg):
    pair, res = arg
    tgt, _ = clouds(pair)
    grid = mg.build_grid(tgt, res)
    return assert_scene(grid, arg), leaf_codes(grid)


def _job(job):
    kind, arg = job
    return job, {"shape": shape_case, "last": last_case, "align": align_case, "scene": scene_case}[kind](arg)


def make_fixture(path=FIXTURE, procs=None):
    import multiprocessing as mp
    out = {}
    # (every cloud is made inside a worker: the parent starts no thread pool of its own before the workers fork)
    jobs = [("align", i) for i in range(len(ALIGNS))] + [("shape", n) for n in SHAPE_SIZES[::-1]] + [("last", k) for k in LAST_SCENES] + \
           [("scene", s) for s in fixture_scenes()]
    with mp.Pool(procs or min(16, os.cpu_count() or 1)) as pool:
        for (kind, arg), r in pool.imap_unordered(_job, jobs):
            if kind == "scene":
                out["codes/%d/%s" % arg] = r[1]
                out["scene/%d/%s" % arg] = np.array(r[0])
            elif kind == "shape":
                _pack_sweeps(out, f"shape/{arg}", r)
            elif kind == "last":
                assert r[1] >= MIN_DIFFERING, (arg, r[1])
                _pack_sweeps(out, f"last/{arg}", r[0])
                out[f"last/{arg}/differing"] = np.int64(r[1])
            else:
                assert steps_clear(r["steps"]), (arg, r["steps"])
                _pack_align(out, f"align/{arg}", r)
            print(kind, arg, "done", flush=True)
    assert int(out["align/1/iterations"]) == 1 and ALIGNS[1] == (5, 1.0, DIRECT1, 1)      # ndt_omp's rule would not end there
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(path, os.path.getsize(path), "B")


def _choose_scene(args):
    pair, res = args
    tgt, src = clouds(pair)
    grid = mg.build_grid(tgt, res)
    _, T = sweep_pose()
    s = subsample(src, LAST_N)
    diff = {m: int((lambda c: (c[:, 0] != c[:, 1]).sum())(deciding_codes(grid, s, T, m))) for m in (DIRECT7, DIRECT26)}
    return args, scene_conditions(grid), diff


def _choose_align(a):
    global ALIGNS
    ALIGNS = [a]
    return a, align_case(0)


def choose():
    """scene conditions of candidate (pair, resolution) grids, and iterations / step lengths of candidate aligns, by the restatement alone"""
    import multiprocessing as mp
    scenes = [(k, r) for k in range(1, 7) for r in (1.0, 2.0, 10.0)]
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        ok = set()
        for (pair, res), (m10, m80, gap), diff in pool.imap(_choose_scene, scenes):
            good = m10 >= MIN_ANGLE_MARGIN and m80 >= MIN_ANGLE_MARGIN and gap >= MIN_EIGEN_GAP
            if good:
                ok.add((pair, res))
            print(f"scene pair {pair} resolution {res}: margins {m10:.3f} {m80:.3f} gap {gap:.3e} eligible {good}; points whose first and last codes differ: "
                  f"DIRECT7 {diff[DIRECT7]} DIRECT26 {diff[DIRECT26]}", flush=True)
        cands = [(p, r, m, f) for (p, r) in sorted(ok) if r != 2.0 for m in (DIRECT1, DIRECT7) for f in FLAGS]
        for a, r in pool.imap(_choose_align, cands):
            print(a, "iterations", r["iterations"], "converged", r["converged"], "hits", r["hits"], "ranks", r["ranks"], "clear of eps", steps_clear(r["steps"]),
                  np.round(r["steps"], 5), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "choose":
        choose()
    else:
        make_fixture()
