#!/usr/bin/env python3
"""Restatement of pcl::NormalDistributionsTransform<PointXYZI, PointXYZI> (registration_method = NDT, the fall-back of
select_registration_method) in NumPy: the contract the engine's MI355NDT_OPT_NDT_CLASS = 1 is held to.  Independent of the library: nothing
here loads it.

PCL is not part of the reference tree.  include/ndt_omp/ndt_omp_impl.hpp is PCL 1.8's ndt.hpp with OpenMP and f32 substitutions, and it keeps
PCL's f64 originals beside them; the class is restated as that file with the substitutions undone (parity unpinned):

  computeTransformation   impl.hpp:81-171 as it stands -- align_pcl is tools/ndt_euler_ref.align_euler over sweep_pcl.
  computeStepLengthMT     up to impl.hpp:831 (line 803's always-true interval_converged: the More-Thuente loop and computeHessian are dead).
  computeDerivatives      one neighbourhood, radiusSearch(x_trans_pt, resolution_): make_golden.radius_search's rule, vectorised (all_pairs).
  computePointDerivatives the f64 overload, impl.hpp:442-479: 3x6 and 18x6 doubles from the f64 rows (ndt_euler_ref.angle_rows64, snap kept),
                          applied to the original point widened.
  updateDerivatives       the structure of impl.hpp:482-535 with every quantity a double; the Hessian terms are those updateHessian writes in f64
                          (impl.hpp:598-640).  x_trans = the f32 transformPointCloud result widened, minus the leaf's f64 mean.

The sums over (point, leaf) hits are taken by NumPy over all hits at once, not point by point in the search's order: f64 sums of a few thousand
terms, order-dependent at ~1e-13 of the largest entry, two orders inside the bar (1e-11) the device is held to.  No f32 inner product is left, so
MI355NDT_OPT_F32_SUM_ORDER has nothing to order: the moved point (transform_point) and the radius test are written in one order.

Run:  python tools/ndt_pcl_ref.py            rewrites tests/golden/ndt_pcl.npz
      python tools/ndt_pcl_ref.py choose     prints, for candidate pairs, whether an align keeps clear of a convergence decision
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
_spec = importlib.util.spec_from_file_location("ndt_euler_ref", os.path.join(ROOT, "tools", "ndt_euler_ref.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)
mg = E.mg

f32, f64 = np.float32, np.float64
FIXTURE = os.path.join(ROOT, "tests", "golden", "ndt_pcl.npz")


# ----------------------------------------------------------------------------- the radius search, all points at once
class Cells:
    """the leaves radiusSearch can return (pushed by applyFilter: >= min_points at that time, eigen-failed ones included), as arrays"""

    def __init__(self, grid):
        cand = [L for _, L in sorted(grid["leaves"].items()) if L.n_pushed >= grid["min_points"]]
        self.grid = grid
        self.cen = np.array([L.cen for L in cand], f32).reshape(-1, 3)
        self.mean = np.array([L.mean for L in cand], f64).reshape(-1, 3)
        self.icov = np.array([L.icov for L in cand], f64).reshape(-1, 3, 3)


def move_cloud(T32, src):
    """PCL 1.8 transformPointCloud, scalar form, f32 (make_golden.transform_point over the whole cloud)"""
    T = np.asarray(T32, f32)
    s = np.asarray(src, f32)
    return np.stack([(((T[a, 0] * s[:, 0]).astype(f32) + (T[a, 1] * s[:, 1]).astype(f32)).astype(f32) + (T[a, 2] * s[:, 2]).astype(f32)).astype(f32) + T[a, 3]
                     for a in range(3)], axis=1).astype(f32)


def all_pairs(cells, xt, radius):
    """(point index, leaf index) of every hit of radiusSearch(xt[i], radius): squared distance to the f32 centroid in f32, (dx^2 + dy^2) + dz^2,
    strictly below float(radius * radius) -- make_golden.radius_search for every point (tests/test_ndt_pcl_cpu.py compares the two)"""
    if len(cells.cen) == 0 or len(xt) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    d = (xt[:, None, :].astype(f32) - cells.cen[None, :, :]).astype(f32)
    d2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32)
    return np.nonzero(d2 < f32(float(radius) * float(radius)))


# ----------------------------------------------------------------------------- sweep
def point_derivatives64(x64, j_ang, h_ang):
    """the f64 computePointDerivatives (impl.hpp:442-479) for n points: J (n, 3, 6), Hp (n, 18, 6)"""
    n = len(x64)
    xj, xh = x64 @ j_ang.T, x64 @ h_ang.T
    J = np.zeros((n, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1
    J[:, 1, 3] = xj[:, 0]; J[:, 2, 3] = xj[:, 1]
    J[:, 0, 4] = xj[:, 2]; J[:, 1, 4] = xj[:, 3]; J[:, 2, 4] = xj[:, 4]
    J[:, 0, 5] = xj[:, 5]; J[:, 1, 5] = xj[:, 6]; J[:, 2, 5] = xj[:, 7]
    z = np.zeros(n)
    a = [z, xh[:, 0], xh[:, 1]]; b = [z, xh[:, 2], xh[:, 3]]; c = [z, xh[:, 4], xh[:, 5]]
    d = [xh[:, 6], xh[:, 7], xh[:, 8]]; e = [xh[:, 9], xh[:, 10], xh[:, 11]]; f = [xh[:, 12], xh[:, 13], xh[:, 14]]
    Hp = np.zeros((n, 18, 6))
    for blk, col, v in ((3, 3, a), (4, 3, b), (5, 3, c), (3, 4, b), (4, 4, d), (5, 4, e), (3, 5, c), (4, 5, e), (5, 5, f)):
        for r in range(3):
            Hp[:, 3 * blk + r, col] = v[r]
    return J, Hp


def sweep_pcl(cells, src, p, d1, d2, T32=None, exact_move=False, hood_pose=None):
    """computeDerivatives of pcl::NormalDistributionsTransform at pose vector p: the cloud moved by T32 (default: convertTransform(p) in f32), the
    rows from p, the Hessian always.  Returns (score, g, H, hits); every (point, leaf) pair the search returns is a hit, rejected or not.
    exact_move / hood_pose (the finite-difference test alone): the moved point is Rx Ry Rz x + t in f64 and the hits are those of the cloud
    moved (in f32) by hood_pose, so that a difference quotient sees a FIXED set of (point, leaf) pairs and a smooth function."""
    p = np.asarray(p, f64)
    src = np.asarray(src, f32)
    T32 = E.convert_transform_f32(p if hood_pose is None else np.asarray(hood_pose, f64)) if T32 is None else np.asarray(T32, f32)
    src = src[np.isfinite(src).all(axis=1)]
    xt = move_cloud(T32, src)
    keep = np.isfinite(xt).all(axis=1)
    src, xt = src[keep], xt[keep]
    pi, li = all_pairs(cells, xt, float(cells.grid["leaf"]))
    x64 = src[pi].astype(f64)
    moved = (x64 @ E.rot64(p).T + p[:3]) if exact_move else xt[pi].astype(f64)
    u = moved - cells.mean[li]                                                   # impl.hpp:259-262
    C = cells.icov[li]
    j_ang, h_ang = E.angle_rows64(p)
    J, Hp = point_derivatives64(x64, j_ang, h_ang)
    with np.errstate(invalid="ignore", over="ignore"):
        e0 = np.exp(-d2 * np.einsum("ni,nij,nj->n", u, C, u) / 2)
        e1 = d2 * e0
        ok = ~((e1 > 1) | (e1 < 0) | (e1 != e1))                                 # impl.hpp:504
    u, C, J, Hp, e0, e1 = u[ok], C[ok], J[ok], Hp[ok], e0[ok], e1[ok]
    score = float(np.sum(-d1 * e0))
    e = e1 * d1
    uC = np.einsum("ni,nij->nj", u, C)
    v = np.einsum("nj,njk->nk", uC, J)                                           # x . (C J_i)
    g = np.einsum("n,nk->k", e, v)
    t2 = np.einsum("na,niak->nik", uC, Hp.reshape(-1, 6, 3, 6))                  # x . (C H_ij)
    t3 = np.einsum("nak,nab,nbi->nik", J, C, J)                                  # J_j . (C J_i), at [i, j]
    H = np.einsum("n,nik->ik", e, -d2 * v[:, :, None] * v[:, None, :] + t2 + t3)
    return score, g, H, int(len(pi))


# ----------------------------------------------------------------------------- align
def align_pcl(cells, src, guess32, prm):
    """computeTransformation (impl.hpp:81-171) + computeStepLengthMT up to :831: ndt_euler_ref.align_euler over sweep_pcl"""
    assert prm["step_size"] - prm["trans_epsilon"] / 2 > 0
    d1, d2, _ = mg.gauss_constants(prm["outlier_ratio"], prm["resolution"])
    eps, step = prm["trans_epsilon"], prm["step_size"]
    final = np.array(guess32, f32)
    p = np.concatenate([final[:3, 3].astype(f64), E.euler_angles_012(final).astype(f64)])   # impl.hpp:107-111
    score, g, H, hits = sweep_pcl(cells, src, p, d1, d2, T32=final)                          # the cloud moved by the guess itself (:95-101, 119)
    inc = prev_inc = np.eye(4, dtype=f32)
    it, sweeps, steps = 0, 1, []
    while True:
        prev_inc = inc                                                                      # :124
        dp = E.solve_newton(H, g)
        n = np.linalg.norm(dp)
        if n == 0 or n != n:                                                                # :134-139
            return dict(final=final, iterations=it, converged=bool(n == n), score=score, hits=hits, sweeps=sweeps, inc=inc, prev_inc=prev_inc,
                        steps=np.array(steps), p=p)
        dp = dp / n
        dphi0 = -(g @ dp)
        if dphi0 >= 0 and dphi0 == 0:                                                       # :768-772
            a = 0.0
        else:
            if dphi0 >= 0:
                dp = -dp                                                                    # :776-777
            a = max(min(n, step), eps / 2)                                                  # :805-807
            x_t = p + dp * a                                                                # :809
            final = E.convert_transform_f32(x_t)                                            # :811-814
            score, g, H, hits = sweep_pcl(cells, src, x_t, d1, d2, T32=final)                # :817-821
            sweeps += 1
        delta = dp * a                                                                      # :143
        inc = E.convert_transform_f32(delta)                                                # :146-149
        p = p + delta                                                                       # :152
        steps.append(a)
        conv = it > prm["max_iterations"] or (it and abs(a) < eps)                          # :158-159
        it += 1
        if conv:
            return dict(final=final, iterations=it, converged=True, score=score, hits=hits, sweeps=sweeps, inc=inc, prev_inc=prev_inc,
                        steps=np.array(steps), p=p)


# ----------------------------------------------------------------------------- fixture
# the factory's settings (registrations.cpp:64-72): epsilon 0.01, 64 iterations, ndt_resolution; PCL's constructor: step 0.1, outlier ratio 0.55
PRM = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, trans_epsilon=0.01, max_iterations=64, min_points_per_voxel=6, min_covar_eigvalue_mult=0.01)
SHAPE_PAIR, SHAPE_SIZES, SHAPE_START, SHAPE_POSE = E.SHAPE_PAIR, E.SHAPE_SIZES, E.SHAPE_START, E.SHAPE_POSE
SHAPE_RES = 1.0
POSE_PAIR, POSE_N, POSE_RES = E.POSE_PAIR, E.POSE_N, 2.0                # (the resolution at which 500 points meet > 1000 leaves)
ALIGN_N = 500
FACTORY_RES, FACTORY_N = 0.5, 500                                      # the factory's ndt_resolution (registrations.cpp:63), on a target dense enough (1024 x 64
FACTORY_SCAN = (1024, 64)                                              # beams instead of 256 x 32) that most source points meet a leaf of 0.5 m
# (pair, rotation axis or None, angle, resolution, source points): chosen with `choose` so that no step length lies within 5 % of trans_epsilon
ALIGNS = [(1, None, 0.0, 1.0, ALIGN_N), (2, None, 0.0, 1.0, ALIGN_N), (6, None, 0.0, 1.0, ALIGN_N), (7, None, 0.0, 1.0, ALIGN_N),
          (1, (1, 0, 0), -0.3, 1.0, ALIGN_N), (2, (0, 0, 1), 1.3, 1.0, ALIGN_N), (3, None, 0.0, FACTORY_RES, FACTORY_N)]

_cells = {}


def clouds(pair, res):
    """(target, source) of a synthetic pair: ndt_euler_ref.clouds, at the factory's resolution the dense scan"""
    if res != FACTORY_RES:
        return E.clouds(pair)
    from lv_slam_amd import synth
    tgt, src, _ = synth.make_pair(pair, FACTORY_SCAN[0], n_beams=FACTORY_SCAN[1])
    return tgt.numpy(), src.numpy()


def cells_of(pair, res):
    """the target grid of a synthetic pair at a resolution (built once per process)"""
    if (pair, res) not in _cells:
        _cells[(pair, res)] = Cells(mg.build_grid(clouds(pair, res)[0], res))
    return _cells[(pair, res)]


def shape_source(n):
    return E.shape_source(n)


def shape_case(n):
    d1, d2, _ = mg.gauss_constants(0.55, SHAPE_RES)
    return sweep_pcl(cells_of(SHAPE_PAIR, SHAPE_RES), shape_source(n), SHAPE_POSE, d1, d2)


def pose_cases():
    """name -> (source, pose): ndt_euler_ref.pose_cases (zero, snapped, unsnapped, roll near pi, pitch 1.5)"""
    return E.pose_cases()


def pose_case(name):
    d1, d2, _ = mg.gauss_constants(0.55, POSE_RES)
    s, p = pose_cases()[name]
    return sweep_pcl(cells_of(POSE_PAIR, POSE_RES), s, p, d1, d2)


def pose_case_f32(name):
    """the same case by the f32 restatement (ndt_euler_ref.sweep_euler, KDTREE): what a device that merely ran model 1 with KDTREE would give"""
    d1, d2, _ = mg.gauss_constants(0.55, POSE_RES)
    s, p = pose_cases()[name]
    return E.sweep_euler(cells_of(POSE_PAIR, POSE_RES).grid, s, p, d1, d2, E.KDTREE)


def shape_case_f32(n):
    d1, d2, _ = mg.gauss_constants(0.55, SHAPE_RES)
    return E.sweep_euler(cells_of(SHAPE_PAIR, SHAPE_RES).grid, shape_source(n), SHAPE_POSE, d1, d2, E.KDTREE)


def align_inputs(i):
    """(target, source, guess, resolution) of align case i"""
    k, axis, angle, res, n = ALIGNS[i]
    tgt, src = clouds(k, res)
    s, G = E.turned(E.subsample(src, n), axis, angle)
    return tgt, s, G, res


def align_case(i):
    k, _, _, res, _ = ALIGNS[i]
    _, s, G, _ = align_inputs(i)
    return align_pcl(cells_of(k, res), s, G, dict(PRM, resolution=res))


def sources_with_hits(i):
    """source points of align case i that meet at least one leaf at the guess"""
    k, _, _, res, _ = ALIGNS[i]
    _, s, G, _ = align_inputs(i)
    pi, _ = all_pairs(cells_of(k, res), move_cloud(G, s), res)
    return len(np.unique(pi)), len(s)


def make_fixture(path=FIXTURE):
    out = {}
    for n in SHAPE_SIZES:
        E._pack_sweep(out, f"shape/{n}", shape_case(n))
        E._pack_sweep(out, f"shape_f32/{n}", shape_case_f32(n))
        print("shape", n, "done", flush=True)
    for name in pose_cases():
        E._pack_sweep(out, f"pose/{name}", pose_case(name))
        E._pack_sweep(out, f"pose_f32/{name}", pose_case_f32(name))
        print("pose", name, "done", flush=True)
    for i in range(len(ALIGNS)):
        E._pack_align(out, f"align/{i}", align_case(i))
        with_hits, n = sources_with_hits(i)
        out[f"align/{i}/points_with_hits"] = np.int64(with_hits)
        print("align", i, "done", flush=True)
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(path, os.path.getsize(path), "B")


def choose():
    """for candidate pairs: iterations and the distance of every step length from trans_epsilon, by the restatement alone"""
    global ALIGNS
    ALIGNS = [(k, None, 0.0, 1.0, ALIGN_N) for k in range(1, 9)] + [(k, (1, 0, 0), -0.3, 1.0, ALIGN_N) for k in range(1, 5)] + \
             [(k, (0, 0, 1), 1.3, 1.0, ALIGN_N) for k in range(1, 5)] + [(k, None, 0.0, FACTORY_RES, FACTORY_N) for k in range(1, 7)]
    if len(sys.argv) > 2:
        ALIGNS = [a for a in ALIGNS if a[3] == float(sys.argv[2])]                         # `choose 0.5`: the candidates at one resolution
    for i in range(len(ALIGNS)):
        r = align_case(i)
        clear = bool((np.abs(r["steps"] - 0.01) > 0.05 * 0.01).all())
        print(ALIGNS[i], "iterations", r["iterations"], "converged", r["converged"], "hits", r["hits"], "points with hits", sources_with_hits(i), "clear of eps", clear,
              np.round(r["steps"], 5), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "choose":
        choose()
    else:
        make_fixture()
