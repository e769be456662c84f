#!/usr/bin/env python3
"""Restatement of the Euler-angle pclomp::NormalDistributionsTransform (include/ndt_omp/ndt_omp_impl.hpp, the implementation a host gets
by changing the include line of src/ndt_omp/ndt_omp.cpp) in NumPy: the contract the engine's MI355NDT_OPT_POSE_MODEL = 1 is held to.
Independent of the library: nothing here loads it.

Everything the variant shares with ndt_omp_impl2.hpp is imported, unchanged, from tests/golden/make_golden.py: the grid build, the
neighbourhoods of all four search modes, mm32, update_derivatives (impl.hpp:483-535 is impl2's, operation for operation),
transform_point, the Gauss constants and convert_transform.  What is restated here, line by line:

  euler_angles_012         Eigen 3.3 MatrixBase::eulerAngles(0, 1, 2) in f32 (third-party, restated from its published form; parity
                           unpinned).  A guess with negative roll starts in the chart near roll = pi.
  convert_transform_f32    Translation3f * AngleAxisf(X) * AngleAxisf(Y) * AngleAxisf(Z) the way Eigen 3.3 evaluates it in f32
                           (AngleAxis::toRotationMatrix, coefficient-wise 3x3 products, a 3-term sum reduced as t0 + (t1 + t2)): the
                           operations of mi355ndt_convert_transform.  make_golden.convert_transform is the same composition in f64,
                           cast at the end; the two agree to f32 rounding (tests/test_ndt_euler_cpu.py).
  angle_derivatives        computeAngleDerivatives, impl.hpp:288-393: sin / cos in f64, |angle| < 10e-5 -> c = 1, s = 0, rows cast to f32.
  point_derivatives_euler  the f32 computePointDerivatives, impl.hpp:397-438, on the ORIGINAL point.
  sweep_euler              computeDerivatives, impl.hpp:180-284.
  align_euler              computeTransformation, impl.hpp:81-171, with computeStepLengthMT up to :831 (line 803 holds the always-true
                           interval_converged at the factory's settings: the More-Thuente loop and computeHessian are dead).

f32 sines, cosines and arc tangents are the f64 function of the f32 argument rounded to f32 (a correctly rounded f32 function but for
double rounding), on both sides.  `order` = MI355NDT_OPT_F32_SUM_ORDER: 0 sums a 4-wide f32 inner product left to right, 1 pairs it as
(t0 + t2) + (t1 + t3), Eigen 3.3's SSE predux; every inner product of the evaluation is 4 wide with a structural zero.

Run:  python tools/ndt_euler_ref.py            rewrites tests/golden/ndt_euler.npz (minutes: every hit is evaluated in Python)
      python tools/ndt_euler_ref.py choose     prints, for candidate pairs, whether an align keeps clear of a convergence decision
"""
from __future__ import annotations

import contextlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402

f32, f64 = np.float32, np.float64
FIXTURE = os.path.join(ROOT, "tests", "golden", "ndt_euler.npz")
KDTREE, DIRECT26, DIRECT7, DIRECT1 = mg.KDTREE, mg.DIRECT26, mg.DIRECT7, mg.DIRECT1


# ----------------------------------------------------------------------------- f32 helpers
def sin32(a):
    return f32(np.sin(f64(f32(a))))


def cos32(a):
    return f32(np.cos(f64(f32(a))))


def atan2_32(a, b):
    return f32(np.arctan2(f64(f32(a)), f64(f32(b))))


def mm32_pair(A, B):
    """mm32 with Eigen 3.3's SSE predux pairing of a 4-wide inner product: (t0 + t2) + (t1 + t3)"""
    A = np.asarray(A, f32)
    B = np.asarray(B, f32)
    n, k = A.shape
    assert k == 4 and B.shape[0] == 4
    out = np.zeros((n, B.shape[1]), f32)
    for i in range(n):
        for j in range(B.shape[1]):
            t = [f32(A[i, q] * B[q, j]) for q in range(4)]
            out[i, j] = f32(f32(t[0] + t[2]) + f32(t[1] + t[3]))
    return out


@contextlib.contextmanager
def sum_order(order):
    """make_golden's update_derivatives with its inner products in the given order (it reads the module's mm32 when it runs)"""
    keep = mg.mm32
    mg.mm32 = mm32_pair if order == 1 else keep
    try:
        yield mg.mm32
    finally:
        mg.mm32 = keep


# ----------------------------------------------------------------------------- pose
def euler_angles_012(M):
    """Eigen 3.3 eulerAngles(0, 1, 2) of the 3x3 block of M, f32 throughout"""
    m = np.asarray(M, f32)
    r0 = atan2_32(m[1, 2], m[2, 2])
    c2 = f32(np.sqrt(f32(f32(m[0, 0] * m[0, 0]) + f32(m[0, 1] * m[0, 1]))))
    if r0 > 0:
        r0 = f32(r0 - f32(np.pi))
        r1 = atan2_32(-m[0, 2], -c2)
    else:
        r1 = atan2_32(-m[0, 2], c2)
    s1, c1 = sin32(r0), cos32(r0)
    r2 = atan2_32(f32(f32(s1 * m[2, 0]) - f32(c1 * m[1, 0])), f32(f32(c1 * m[1, 1]) - f32(s1 * m[2, 1])))
    return np.array([-r0, -r1, -r2], f32)


def _aa_matrix(angle, axis):
    """Eigen 3.3 AngleAxisf(angle, unit axis).toRotationMatrix()"""
    ax = np.zeros(3, f32)
    ax[axis] = 1
    sn, c = sin32(angle), cos32(angle)
    sa = (sn * ax).astype(f32)
    c1 = (f32(f32(1) - c) * ax).astype(f32)
    R = np.zeros((3, 3), f32)
    tmp = f32(c1[0] * ax[1])
    R[0, 1] = f32(tmp - sa[2]); R[1, 0] = f32(tmp + sa[2])
    tmp = f32(c1[0] * ax[2])
    R[0, 2] = f32(tmp + sa[1]); R[2, 0] = f32(tmp - sa[1])
    tmp = f32(c1[1] * ax[2])
    R[1, 2] = f32(tmp - sa[0]); R[2, 1] = f32(tmp + sa[0])
    for a in range(3):
        R[a, a] = f32(f32(c1[a] * ax[a]) + c)
    return R


def _mul33(A, B):
    C = np.zeros((3, 3), f32)
    for r in range(3):
        for c in range(3):
            C[r, c] = f32(f32(A[r, 0] * B[0, c]) + f32(f32(A[r, 1] * B[1, c]) + f32(A[r, 2] * B[2, c])))
    return C


def convert_transform_f32(x):
    """ndt_omp.h:209-228 / impl.hpp:146-149, 811-814 as Eigen 3.3 evaluates them in f32"""
    L = _mul33(_mul33(_aa_matrix(f32(x[3]), 0), _aa_matrix(f32(x[4]), 1)), _aa_matrix(f32(x[5]), 2))
    M = np.eye(4, dtype=f32)
    M[:3, :3] = L
    M[:3, 3] = [f32(v) for v in x[:3]]
    return M


def angle_rows64(p, snap=True):
    """the 8 + 15 rows of impl.hpp:328-391 in f64 (C evaluation order)"""
    def sc(a):
        if snap and abs(a) < 10e-5:
            return 1.0, 0.0
        return float(np.cos(f64(a))), float(np.sin(f64(a)))
    cx, sx = sc(p[3]); cy, sy = sc(p[4]); cz, sz = sc(p[5])
    j = [[(-sx * sz + cx * sy * cz), (-sx * cz - cx * sy * sz), (-cx * cy)],
         [(cx * sz + sx * sy * cz), (cx * cz - sx * sy * sz), (-sx * cy)],
         [(-sy * cz), sy * sz, cy],
         [sx * cy * cz, (-sx * cy * sz), sx * sy],
         [(-cx * cy * cz), cx * cy * sz, (-cx * sy)],
         [(-cy * sz), (-cy * cz), 0],
         [(cx * cz - sx * sy * sz), (-cx * sz - sx * sy * cz), 0],
         [(sx * cz + cx * sy * sz), (cx * sy * cz - sx * sz), 0]]
    h = [[(-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), sx * cy],          # a2
         [(-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), (-cx * cy)],       # a3
         [(cx * cy * cz), (-cx * cy * sz), (cx * sy)],                             # b2
         [(sx * cy * cz), (-sx * cy * sz), (sx * sy)],                             # b3
         [(-sx * cz - cx * sy * sz), (sx * sz - cx * sy * cz), 0],                 # c2
         [(cx * cz - sx * sy * sz), (-sx * sy * cz - cx * sz), 0],                 # c3
         [(-cy * cz), (cy * sz), (sy)],                                            # d1
         [(-sx * sy * cz), (sx * sy * sz), (sx * cy)],                             # d2
         [(cx * sy * cz), (-cx * sy * sz), (-cx * cy)],                            # d3
         [(sy * sz), (sy * cz), 0],                                                # e1
         [(-sx * cy * sz), (-sx * cy * cz), 0],                                    # e2
         [(cx * cy * sz), (cx * cy * cz), 0],                                      # e3
         [(-cy * cz), (cy * sz), 0],                                               # f1
         [(-cx * sz - sx * sy * cz), (-cx * cz + sx * sy * sz), 0],                # f2
         [(-sx * sz + cx * sy * cz), (-cx * sy * sz - sx * cz), 0]]                # f3
    return np.array(j, f64), np.array(h, f64)


def angle_derivatives(p):
    """computeAngleDerivatives (impl.hpp:288-393): j_ang (8x3) and h_ang (15x3), f32"""
    j, h = angle_rows64(p)
    return j.astype(f32), h.astype(f32)


def _place(xj, xh, dtype, rows):
    """the patterns of impl.hpp:405-436 (rows = 4: the f32 overload's padded blocks; 3: plain)"""
    J = np.zeros((rows, 6), dtype)
    J[0, 0] = J[1, 1] = J[2, 2] = 1
    J[1, 3] = xj[0]; J[2, 3] = xj[1]                       # (0, 3) is a structural zero
    J[0, 4] = xj[2]; J[1, 4] = xj[3]; J[2, 4] = xj[4]
    J[0, 5] = xj[5]; J[1, 5] = xj[6]; J[2, 5] = xj[7]
    a = [0, xh[0], xh[1]]; b = [0, xh[2], xh[3]]; c = [0, xh[4], xh[5]]
    d = [xh[6], xh[7], xh[8]]; e = [xh[9], xh[10], xh[11]]; f = [xh[12], xh[13], xh[14]]
    Hp = np.zeros((6 * rows, 6), dtype)
    for blk, col, v in ((3, 3, a), (4, 3, b), (5, 3, c), (3, 4, b), (4, 4, d), (5, 4, e), (3, 5, c), (4, 5, e), (5, 5, f)):
        Hp[blk * rows:blk * rows + 3, col] = v
    return J, Hp


def point_derivatives_euler(x, j_ang, h_ang):
    """the f32 computePointDerivatives (impl.hpp:397-438): J = 4x6, Hp = 24x6, from the ORIGINAL point x"""
    x4 = np.array([[x[0]], [x[1]], [x[2]], [0.0]], f32)
    j4 = np.zeros((8, 4), f32); j4[:, :3] = j_ang
    h4 = np.zeros((15, 4), f32); h4[:, :3] = h_ang
    return _place(mg.mm32(j4, x4)[:, 0], mg.mm32(h4, x4)[:, 0], f32, 4)


# ----------------------------------------------------------------------------- sweep
def sweep_euler(grid, src, p, d1, d2, mode, order=0, T32=None):
    """computeDerivatives (impl.hpp:180-284) at pose vector p: the cloud moved by T32 (default: convertTransform(p) in f32), the rows
    from p.  Returns (score, g, H, hits)."""
    p = np.asarray(p, f64)
    T32 = convert_transform_f32(p) if T32 is None else np.asarray(T32, f32)
    j_ang, h_ang = angle_derivatives(p)
    score, g, H, hits = 0.0, np.zeros(6), np.zeros((6, 6)), 0
    with sum_order(order):
        for x in np.asarray(src, f32):
            if not np.isfinite(x).all():
                continue
            xt = mg.transform_point(T32, x)
            if not np.isfinite(xt).all():
                continue
            s_pt, g_pt, H_pt = 0.0, np.zeros(6), np.zeros((6, 6))
            for L in mg.neighbourhood(grid, xt, mode):
                x_trans = xt.astype(f64) - L.mean                          # impl.hpp:259-262
                J, Hp = point_derivatives_euler(x, j_ang, h_ang)           # impl.hpp:267
                s_pt += mg.update_derivatives(g_pt, H_pt, J, Hp, x_trans, L.icov, d1, d2)
                hits += 1
            score += s_pt; g += g_pt; H += H_pt
    return score, g, H, hits


def rot64(p):
    """Rx Ry Rz in f64"""
    cx, sx, cy, sy, cz, sz = np.cos(p[3]), np.sin(p[3]), np.cos(p[4]), np.sin(p[4]), np.cos(p[5]), np.sin(p[5])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def sweep_euler_f64(grid, src, p, d1, d2, mode, hessian=False, hood_pose=None):
    """The same evaluation in plain f64 (no f32 rounding anywhere; the snap of impl.hpp:292-325 kept): the restatement against itself, for the
    finite-difference test.  The neighbourhoods are those of the point moved (in f32) by `hood_pose` (default: p): the gradient differentiates
    the score over a FIXED set of (point, leaf) pairs, so a difference quotient must not let a point change cell between its two ends."""
    p = np.asarray(p, f64)
    R, t = rot64(p), p[:3]
    hp = p if hood_pose is None else np.asarray(hood_pose, f64)
    T32 = convert_transform_f32(hp)                                   # (the cells sweep_euler finds)
    j_ang, h_ang = angle_rows64(p)
    score, g, H = 0.0, np.zeros(6), np.zeros((6, 6))
    for x in np.asarray(src, f32):
        x64 = x.astype(f64)
        J, Hp = _place(j_ang @ x64, h_ang @ x64, f64, 3)
        for L in mg.neighbourhood(grid, mg.transform_point(T32, x), mode):
            u = (R @ x64 + t) - L.mean
            C = L.icov
            e0 = np.exp(-d2 * (u @ C @ u) / 2)
            if d2 * e0 > 1 or d2 * e0 < 0:
                continue
            score += -d1 * e0
            e = d2 * e0 * d1
            v = u @ C @ J
            g += e * v
            if hessian:
                for i in range(6):
                    for k in range(6):
                        H[i, k] += e * (-d2 * v[i] * v[k] + u @ C @ Hp[3 * i:3 * i + 3, k] + J[:, k] @ C @ J[:, i])
    return score, g, H


# ----------------------------------------------------------------------------- align
def solve_newton(H, g):
    """JacobiSVD(H).solve(-g): the thresholded pseudo-inverse (as make_golden.align_dead_mt)"""
    U, S, Vt = np.linalg.svd(H)
    rank = int((S >= max(S[0] * 6 * np.finfo(f64).eps, np.finfo(f64).tiny)).sum()) if S[0] > 0 else 0
    return Vt[:rank].T @ ((U[:, :rank].T @ (-g)) / S[:rank])


def align_euler(grid, src, guess32, prm, order=0):
    """computeTransformation (impl.hpp:81-171) + computeStepLengthMT up to :831, dead More-Thuente loop (step_size > eps / 2)."""
    assert prm["step_size"] - prm["trans_epsilon"] / 2 > 0
    d1, d2, _ = mg.gauss_constants(prm["outlier_ratio"], prm["resolution"])
    eps, step, mode = prm["trans_epsilon"], prm["step_size"], prm["neighbor_mode"]
    final = np.array(guess32, f32)
    p = np.concatenate([final[:3, 3].astype(f64), euler_angles_012(final).astype(f64)])     # impl.hpp:107-111
    score, g, H, hits = sweep_euler(grid, src, p, d1, d2, mode, order, T32=final)            # the cloud moved by the guess itself (:95-101, 119)
    inc = prev_inc = np.eye(4, dtype=f32)
    it, sweeps, steps = 0, 1, []
    while True:
        prev_inc = inc                                                                      # :124
        dp = solve_newton(H, g)
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
                dp = -dp                                                                    # :776-777 (step_dir is a reference)
            a = max(min(n, step), eps / 2)                                                  # :805-807
            x_t = p + dp * a                                                                # :809
            final = convert_transform_f32(x_t)                                              # :811-814
            score, g, H, hits = sweep_euler(grid, src, x_t, d1, d2, mode, order, T32=final)  # :817-821
            sweeps += 1
        delta = dp * a                                                                      # :143
        inc = convert_transform_f32(delta)                                                  # :146-149
        p = p + delta                                                                       # :152
        steps.append(a)
        conv = it > prm["max_iterations"] or (it and abs(a) < eps)                          # :158-159
        it += 1
        if conv:
            return dict(final=final, iterations=it, converged=True, score=score, hits=hits, sweeps=sweeps, inc=inc, prev_inc=prev_inc,
                        steps=np.array(steps), p=p)


# ----------------------------------------------------------------------------- fixture
PRM = dict(resolution=1.0, step_size=0.1, outlier_ratio=0.55, trans_epsilon=0.01, max_iterations=64, neighbor_mode=DIRECT7, variant=0,
           min_points_per_voxel=6, min_covar_eigvalue_mult=0.01)
SHAPE_PAIR, SHAPE_SIZES = 2, (1, 64, 65, 513, 2049)
SHAPE_START = 26                                                      # the first source point that meets a leaf: the one-point case has a hit
SHAPE_POSE = np.array([1.0, 0.0, 0.0, 0.12, 0.15, 0.2])             # every angle in (0.1, 1)
POSE_PAIR, POSE_N = 4, 500
POSE_MODES = {"direct7": (DIRECT7, 1.0), "direct26": (DIRECT26, 2.0), "kdtree": (KDTREE, 2.0)}   # (resolutions at which 500 points meet > 1000 leaves)
POSES = {"zero": [1.0, 0, 0, 0, 0, 0], "snapped": [1.0, 0, 0, 0, 5e-5, 0], "unsnapped": [1.0, 0, 0, 0, 2e-4, 0]}
ALIGN_N = 500
# (pair, rotation axis or None, angle, search): chosen with `choose` so that no step length lies within 5 % of trans_epsilon
ALIGNS = [(1, None, 0.0, DIRECT7), (2, None, 0.0, DIRECT7), (6, None, 0.0, DIRECT7), (7, None, 0.0, DIRECT7),
          (1, (1, 0, 0), -0.3, DIRECT1), (2, (0, 0, 1), 1.3, DIRECT1)]


def clouds(k):
    from lv_slam_amd import synth
    tgt, src, _ = synth.make_pair(k, 256, n_beams=32)
    return tgt.numpy(), src.numpy()


def subsample(src, n):
    """n points strided over the cloud (as make_golden.make_case)"""
    return src[:: max(1, len(src) // n)][:n]


def rotation(axis, angle):
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def turned(src, axis, angle):
    """(Q^-1 src as f32, default_guess() Q as f32): the geometry of the plain pair presented turned (tests/test_large_rotation_gpu.turned)"""
    from lv_slam_amd import synth
    if axis is None:
        return src, synth.default_guess()
    R = rotation(axis, angle)
    Q = np.eye(4); Q[:3, :3] = R
    return (src.astype(f64) @ R).astype(f32), (synth.default_guess().astype(f64) @ Q).astype(f32)


def turned_pose(axis, angle):
    """pose vector whose convertTransform is default_guess() Q, in the chart eulerAngles(0, 1, 2) gives"""
    _, G = turned(np.zeros((1, 3), f32), axis, angle)
    return np.concatenate([G[:3, 3].astype(f64), euler_angles_012(G).astype(f64)])


def shape_source(n):
    """n points of the shapes pair turned against SHAPE_POSE's rotation, so that the moved cloud is the plain pair's at default_guess()"""
    _, src = clouds(SHAPE_PAIR)
    return (subsample(src[SHAPE_START:], n).astype(f64) @ rot64(SHAPE_POSE)).astype(f32)


def shape_case(n):
    tgt, _ = clouds(SHAPE_PAIR)
    grid = mg.build_grid(tgt, 1.0)
    d1, d2, _ = mg.gauss_constants(0.55, 1.0)
    return sweep_euler(grid, shape_source(n), SHAPE_POSE, d1, d2, DIRECT1)


def pose_cases():
    """name -> (source, pose): the three poses of POSES on the plain source; roll near pi (the chart a guess with roll -0.3 starts in) and
    pitch 1.5 on the source turned the other way, so that the moved cloud is the plain pair's"""
    _, src = clouds(POSE_PAIR)
    s = subsample(src, POSE_N)
    out = {k: (s, np.array(v, f64)) for k, v in POSES.items()}
    out["roll_pi"] = (turned(s, (1, 0, 0), -0.3)[0], turned_pose((1, 0, 0), -0.3))
    out["pitch_1.5"] = (turned(s, (0, 1, 0), 1.5)[0], turned_pose((0, 1, 0), 1.5))
    return out


def pose_case(args):
    mode_name, pose_name, order = args
    mode, res = POSE_MODES[mode_name]
    tgt, _ = clouds(POSE_PAIR)
    grid = mg.build_grid(tgt, res)
    d1, d2, _ = mg.gauss_constants(0.55, res)
    s, p = pose_cases()[pose_name]
    return sweep_euler(grid, s, p, d1, d2, mode, order)


def align_inputs(i):
    """(target, source, guess, search mode) of align case i"""
    k, axis, angle, mode = ALIGNS[i]
    tgt, src = clouds(k)
    s, G = turned(subsample(src, ALIGN_N), axis, angle)
    return tgt, s, G, mode


def align_case(i):
    tgt, s, G, mode = align_inputs(i)
    return align_euler(mg.build_grid(tgt, 1.0), s, G, dict(PRM, neighbor_mode=mode))


def _pack_sweep(out, key, r):
    out[key + "/score"] = np.float64(r[0]); out[key + "/g"] = r[1]; out[key + "/H"] = r[2]; out[key + "/hits"] = np.int64(r[3])


def _pack_align(out, key, r):
    for f in ("final", "inc", "prev_inc", "steps", "p"):
        out[key + "/" + f] = r[f]
    for f in ("iterations", "converged", "sweeps", "hits"):
        out[key + "/" + f] = np.int64(r[f])
    out[key + "/score"] = np.float64(r["score"])


def _job(job):
    kind, arg = job
    return job, {"shape": shape_case, "pose": pose_case, "align": align_case}[kind](arg)


def make_fixture(path=FIXTURE, procs=None):
    import multiprocessing as mp
    jobs = [("align", i) for i in range(len(ALIGNS))] + [("pose", (m, p, o)) for m in POSE_MODES for p in list(POSES) + ["roll_pi", "pitch_1.5"] for o in (0, 1)] + \
           [("shape", n) for n in SHAPE_SIZES]
    out = {}
    with mp.Pool(procs or min(8, os.cpu_count() or 1)) as pool:
        for (kind, arg), r in pool.imap_unordered(_job, jobs):
            if kind == "shape":
                _pack_sweep(out, f"shape/{arg}", r)
            elif kind == "pose":
                _pack_sweep(out, "pose/%s/%s/%d" % arg, r)
            else:
                _pack_align(out, f"align/{arg}", r)
            print(kind, arg, "done", flush=True)
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    print(path, os.path.getsize(path), "B")


def choose():
    """for candidate pairs: iterations and the distance of every step length from trans_epsilon, by the restatement alone"""
    import multiprocessing as mp
    global ALIGNS
    ALIGNS = [(k, None, 0.0, DIRECT7) for k in range(1, 9)] + [(k, (1, 0, 0), -0.3, DIRECT1) for k in range(1, 7)] + [(k, (0, 0, 1), 1.3, DIRECT1) for k in range(1, 7)]
    with mp.Pool(min(8, os.cpu_count() or 1), initializer=_set_aligns, initargs=(ALIGNS,)) as pool:
        for i, r in enumerate(pool.map(align_case, range(len(ALIGNS)))):
            clear = bool((np.abs(r["steps"] - 0.01) > 0.05 * 0.01).all())
            print(ALIGNS[i], "iterations", r["iterations"], "converged", r["converged"], "hits", r["hits"], "clear of eps", clear, np.round(r["steps"], 5), flush=True)


def _set_aligns(a):
    global ALIGNS
    ALIGNS = a


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "choose":
        choose()
    else:
        make_fixture()
