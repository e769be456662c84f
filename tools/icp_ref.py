"""Restatement of pcl::IterativeClosestPoint as the loop-closure factory sets it up for registration_method = ICP
(src/global_graph/registrations.cpp:21-29) in NumPy / plain Python, by brute force: the contract the engine's ICP surface (mi355ndt_icp_*,
lv_slam_amd/csrc/ndt_icp.hpp, icp_outer.hpp, ndt_host_icp.hpp) is held to.  Independent of the library: nothing here loads it.

PCL is not in the reference tree: computeTransformation, CorrespondenceEstimation::determineCorrespondences, TransformationEstimationSVD
(Eigen::umeyama without scaling) and DefaultConvergenceCriteria::hasConverged are RESTATED AS RECALLED from PCL 1.8.  Parity unpinned:
INTEGRATION.md section 5.

  moves            every move of the working cloud is an f32 product, each coordinate ((a x + b y) + c z) + d; the cloud is moved cumulatively
                   and never recomputed from the source; final = transformation * final in f32, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3.
  correspondences  exhaustive 1-NN over the target's finite points, d2 = (dx*dx + dy*dy) + dz*dz in f32, a tie to the lower point id (the
                   engine's rule); kept iff (double)d2 <= corr_dist_threshold^2; a point that is not finite before or after the move
                   matches nothing.
  sums             sixteen f64 sums over the matches of f64 products of the f32 coordinates (p the moved point, q its target point):
                   sum p [0..2], sum q [3..5], sum q_r p_c [6 + 3 r + c], sum d2 [15], over the engine's fixed tree: 256 points per chunk
                   (64 lanes by halving, four wave sums in wave order), chunk c into slot c % 256 in ascending c, the 256 slots by halving.
                   Eigen's own sums are f32 and vectorised in an order nobody can observe.
  estimate         Sigma = (sum q p' - (sum q)(sum p)' / m) / m = U S V' (jacobi_svd3: ndt_math.hpp's two-sided Jacobi, operation for
                   operation in Python floats); s = -1 iff det U det V < 0; R = U diag(1, 1, s) V'; t = cq - R cp; cast to f32.
  criteria         iterations >= max_iterations (converged: ICP reports true at the cap); cos >= 1 - eps and the SQUARED translation <=
                   eps (PCL's slip: the unsquared epsilon); |mse - prev| < 1e-12; |mse - prev| / prev < euclidean_fitness_epsilon.
"""
import math

import numpy as np

F32 = np.float32
ROWS = 512
DBL_MAX = 1.7976931348623157e308
DBL_MIN = 2.2250738585072014e-308
EPS = 2.220446049250313e-16
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
STATE_NAMES = ["NOT_CONVERGED", "ITERATIONS", "TRANSFORM", "ABS_MSE", "REL_MSE", "NO_CORRESPONDENCES"]

DEFAULTS = dict(transformation_epsilon=0.0, max_iterations=10, euclidean_fitness_epsilon=-DBL_MAX, corr_dist_threshold=math.sqrt(DBL_MAX),
                min_number_correspondences=3, use_reciprocal_correspondences=0)          # pcl::Registration's constructor
FACTORY = dict(DEFAULTS, transformation_epsilon=0.01, max_iterations=64, use_reciprocal_correspondences=0)   # registrations.cpp:21-29


def cloud(points):
    return np.ascontiguousarray(points, F32).reshape(-1, 3)


def move_f32(T, p):
    """rows of p moved by the 4x4 f32 T: ((a x + b y) + c z) + d per coordinate"""
    T = np.asarray(T, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def mul4_f32(A, B):
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    out = np.zeros((4, 4), F32)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return out


def d2_rows(p, q):
    """[len(q), len(p)] f32 squared distances, (dx*dx + dy*dy) + dz*dz"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def _nearest_exhaustive(ts, q):
    """(position in ts, f32 d2) of the nearest row of ts for every row of q: the first minimum, i.e. the lower id on a tie"""
    best = np.zeros(len(q), np.int64)
    dmin = np.full(len(q), np.inf, F32)
    for r0 in range(0, len(q), ROWS):
        d2 = d2_rows(ts, q[r0:r0 + ROWS])
        with np.errstate(invalid="ignore"):
            d2 = np.where(np.isnan(d2), F32(np.inf), d2)
        b = np.argmin(d2, axis=1)
        best[r0:r0 + ROWS] = b
        dmin[r0:r0 + ROWS] = d2[np.arange(len(b)), b]
    return best, dmin


def _nearest_screened(ts, q, tree, k=4):
    """the same answer as _nearest_exhaustive, found among the k nearest rows of an f64 kd-tree wherever that provably loses nothing: the
    f32 distance of a row is within 1e-5 (relative) of its f64 distance, so when the k-th f64 distance exceeds the best f32 distance among
    the k by more than that, no row outside the k can win or tie.  Every other query goes through the exhaustive search."""
    k = min(k, len(ts))
    d64, cand = tree.query(q.astype(np.float64), k=k)
    d64, cand = d64.reshape(len(q), k), np.sort(cand.reshape(len(q), k), axis=1)      # candidates in id order: argmin takes the lower id
    c = ts[cand]
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy, dz = q[:, None, 0] - c[:, :, 0], q[:, None, 1] - c[:, :, 1], q[:, None, 2] - c[:, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
    b = np.argmin(d2, axis=1)
    dmin = d2[np.arange(len(q)), b]
    best = cand[np.arange(len(q)), b]
    far = d64.max(axis=1)
    unsure = ~(far * far * (1.0 - 1e-5) > dmin.astype(np.float64)) if k < len(ts) else np.zeros(len(q), bool)
    if unsure.any():
        best[unsure], dmin[unsure] = _nearest_exhaustive(ts, q[unsure])
    return best, dmin


_TREES = {}


def correspondences(W, src_finite, tgt, corr_dist_threshold=DEFAULTS["corr_dist_threshold"], exhaustive=True):
    """the working cloud W against the target: (idx [n] int32, -1 = none; d2 [n] f32, 0 where unmatched; m).  exhaustive=False screens
    the candidates with SciPy's kd-tree (the same result, see _nearest_screened; needs SciPy)"""
    t = cloud(tgt)
    tid = np.flatnonzero(np.isfinite(t).all(axis=1))
    ts = t[tid]
    live = np.asarray(src_finite, bool) & np.isfinite(W).all(axis=1)
    idx = np.full(len(W), -1, np.int32)
    d2o = np.zeros(len(W), F32)
    with np.errstate(over="ignore"):
        thr2 = np.float64(corr_dist_threshold) * np.float64(corr_dist_threshold)
    lv = np.flatnonzero(live)
    if len(tid) and len(lv):
        if exhaustive:
            best, dmin = _nearest_exhaustive(ts, W[lv])
        else:
            from scipy.spatial import cKDTree
            key = (len(ts), hash(ts.tobytes()))
            if key not in _TREES:
                _TREES.clear()
                _TREES[key] = cKDTree(ts.astype(np.float64))
            best, dmin = _nearest_screened(ts, W[lv], _TREES[key])
        ok = dmin.astype(np.float64) <= thr2
        idx[lv[ok]] = tid[best[ok]]
        d2o[lv[ok]] = dmin[ok]
    return idx, d2o, int((idx >= 0).sum())


def terms(W, tgt, idx, d2):
    """[n, 16] f64: the sixteen terms of every point, zeros where unmatched"""
    t = cloud(tgt)
    out = np.zeros((len(W), 16), np.float64)
    mt = np.flatnonzero(idx >= 0)
    p = W[mt].astype(np.float64)
    q = t[idx[mt]].astype(np.float64)
    out[mt, 0:3] = p
    out[mt, 3:6] = q
    for r in range(3):
        for c in range(3):
            out[mt, 6 + 3 * r + c] = q[:, r] * p[:, c]
    out[mt, 15] = d2[mt].astype(np.float64)
    return out


def tree_sum(v):
    """the engine's fixed tree over [n, NS] f64 terms -> [NS]"""
    v = np.asarray(v, np.float64)
    n, ns = v.shape
    chunks = max((n + 255) // 256, 1)
    a = np.zeros((chunks * 256, ns), np.float64)
    a[:n] = v
    a = a.reshape(chunks, 4, 64, ns)
    o = 32
    while o:                                                           # 64 lanes by shuffle-xor 32 .. 1: lane 0 holds the halving tree
        a = a[:, :, :o] + a[:, :, o:2 * o]
        o >>= 1
    w = a[:, :, 0]
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]                   # the four wave sums in wave order
    slots = np.zeros((256, ns), np.float64)
    for c0 in range(0, chunks, 256):                                   # chunk c into slot c % 256, ascending c
        blk = part[c0:c0 + 256]
        slots[:len(blk)] = slots[:len(blk)] + blk
    o = 128
    while o:
        slots = slots[:o] + slots[o:2 * o]
        o >>= 1
    return slots[0]


def step_sums(W, tgt, idx, d2):
    """(sums [16], the sums of the absolute terms [16])"""
    t = terms(W, tgt, idx, d2)
    return tree_sum(t), np.abs(t).sum(axis=0)


def jacobi_svd3(A):
    """ndt_math.hpp jacobi_svd3, operation for operation: (U, S, V) as lists, A = U diag(S) V'"""
    A = [[float(A[i][j]) for j in range(3)] for i in range(3)]
    scale = 0.0
    for i in range(3):
        for j in range(3):
            scale = abs(A[i][j]) if abs(A[i][j]) > scale else scale
    if scale == 0.0:
        scale = 1.0
    M = [[A[i][j] / scale for j in range(3)] for i in range(3)]
    u = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    v = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    maxdiag = 0.0
    for i in range(3):
        maxdiag = abs(M[i][i]) if abs(M[i][i]) > maxdiag else maxdiag
    for _ in range(60):
        rotated = False
        for p in range(1, 3):
            for q in range(p):
                thr = 2.0 * EPS * maxdiag
                if thr < DBL_MIN:
                    thr = DBL_MIN
                off = abs(M[p][q]) if abs(M[p][q]) > abs(M[q][p]) else abs(M[q][p])
                if not off > thr:
                    continue
                rotated = True
                a, b, c, d = M[q][q], M[q][p], M[p][q], M[p][p]
                c1, s1 = 1.0, 0.0
                t, dd = a + d, c - b
                if dd != 0.0:
                    w = t / dd
                    tmp = math.sqrt(1.0 + w * w)
                    s1, c1 = 1.0 / tmp, w / tmp
                x, y, z = c1 * a + s1 * c, c1 * b + s1 * d, -s1 * b + c1 * d
                cj, sj = 1.0, 0.0
                if y != 0.0:
                    tau = (x - z) / (2.0 * y)
                    w = math.sqrt(1.0 + tau * tau)
                    tj = -1.0 / (tau + w if tau >= 0.0 else tau - w)
                    cj = 1.0 / math.sqrt(1.0 + tj * tj)
                    sj = tj * cj
                cl, sl = cj * c1 + sj * s1, cj * s1 - sj * c1
                for j in range(3):
                    mq, mp = M[q][j], M[p][j]
                    M[q][j], M[p][j] = cl * mq + sl * mp, -sl * mq + cl * mp
                for i in range(3):
                    mq, mp = M[i][q], M[i][p]
                    M[i][q], M[i][p] = cj * mq - sj * mp, sj * mq + cj * mp
                    vq, vp = v[i][q], v[i][p]
                    v[i][q], v[i][p] = cj * vq - sj * vp, sj * vq + cj * vp
                    uq, up = u[i][q], u[i][p]
                    u[i][q], u[i][p] = cl * uq + sl * up, -sl * uq + cl * up
                maxdiag = abs(M[q][q]) if abs(M[q][q]) > maxdiag else maxdiag
                maxdiag = abs(M[p][p]) if abs(M[p][p]) > maxdiag else maxdiag
        if not rotated:
            break
    s = [0.0] * 3
    for j in range(3):
        s[j] = abs(M[j][j])
        if M[j][j] < 0.0:
            for i in range(3):
                u[i][j] = -u[i][j]
    for j in range(2):
        k = j
        for l in range(j + 1, 3):
            k = l if s[l] > s[k] else k
        if k != j:
            s[j], s[k] = s[k], s[j]
            for i in range(3):
                u[i][j], u[i][k] = u[i][k], u[i][j]
                v[i][j], v[i][k] = v[i][k], v[i][j]
    return u, [s[i] * scale for i in range(3)], v


def det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])) + \
        M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])


def rigid_from_sigma(Sg, cp, cq):
    """(R, t) in Python floats from the covariance and the centroids: umeyama without scaling"""
    U, _, V = jacobi_svd3(Sg)
    s = -1.0 if det3(U) * det3(V) < 0.0 else 1.0
    R = [[(U[r][0] * V[c][0] + U[r][1] * V[c][1]) + (U[r][2] * s) * V[c][2] for c in range(3)] for r in range(3)]
    t = [cq[r] - ((R[r][0] * cp[0] + R[r][1] * cp[1]) + R[r][2] * cp[2]) for r in range(3)]
    return R, t


def estimate(sums, m):
    """the 4x4 f32 transformation from the sixteen sums over m matches"""
    v = [float(x) for x in sums]
    m = float(m)
    cp = [v[r] / m for r in range(3)]
    cq = [v[3 + r] / m for r in range(3)]
    Sg = [[(v[6 + 3 * r + c] - v[3 + r] * v[c] / m) / m for c in range(3)] for r in range(3)]
    R, t = rigid_from_sigma(Sg, cp, cq)
    T = np.eye(4, dtype=F32)
    for r in range(3):
        for c in range(3):
            T[r, c] = F32(R[r][c])
        T[r, 3] = F32(t[r])
    return T


def criteria(T, nr, mse, prev_mse, prm):
    """DefaultConvergenceCriteria::hasConverged: (state or NOT_CONVERGED, the new prev_mse, cos, tr2)"""
    T = np.asarray(T, F32)
    cos = 0.5 * (((float(T[0, 0]) + float(T[1, 1])) + float(T[2, 2])) - 1.0)
    tr2 = (float(T[0, 3]) * float(T[0, 3]) + float(T[1, 3]) * float(T[1, 3])) + float(T[2, 3]) * float(T[2, 3])
    eps = float(prm["transformation_epsilon"])
    if nr >= prm["max_iterations"]:
        return ITERATIONS, prev_mse, cos, tr2
    if cos >= 1.0 - eps and tr2 <= eps:                              # (the squared translation against the unsquared epsilon: PCL's slip)
        return TRANSFORM, prev_mse, cos, tr2
    if abs(mse - prev_mse) < 1e-12:
        return ABS_MSE, prev_mse, cos, tr2
    with np.errstate(all="ignore"):
        rel = float(np.float64(abs(mse - prev_mse)) / np.float64(prev_mse))
    if rel < prm["euclidean_fitness_epsilon"]:
        return REL_MSE, prev_mse, cos, tr2
    return NOT_CONVERGED, mse, cos, tr2


def one_step(src, tgt, guess, T=None, corr_dist_threshold=DEFAULTS["corr_dist_threshold"], exhaustive=True):
    """mi355ndt_icp_correspondences: a fresh working cloud T (guess p): dict W, idx, d2, m, sums, abs_sums"""
    s = cloud(src)
    W = move_f32(np.eye(4, dtype=F32) if T is None else T, move_f32(guess, s))
    idx, d2, m = correspondences(W, np.isfinite(s).all(axis=1), tgt, corr_dist_threshold, exhaustive)
    sums, abss = step_sums(W, tgt, idx, d2)
    return dict(W=W, idx=idx, d2=d2, m=m, sums=sums, abs_sums=abss)


def align(src, tgt, guess, params=None, transformations=None, exhaustive=True):
    """computeTransformation.  dict: final, converged, iterations, state, matches, mse, aligned (the working cloud after the last move),
    trace (per iteration: T, m, mse, prev_mse, cos, tr2, state).  `transformations`: use these estimates instead of the restatement's own
    (the test of the fused move feeds the engine's)."""
    prm = dict(DEFAULTS, **(params or {}))
    if prm["use_reciprocal_correspondences"]:
        raise ValueError("use_reciprocal_correspondences is not served")
    s = cloud(src)
    fin = np.isfinite(s).all(axis=1)
    final = np.array(guess, F32)
    W = move_f32(final, s)
    nr, prev_mse, mse, m = 0, DBL_MAX, 0.0, 0
    state, converged, trace = NOT_CONVERGED, False, []
    while True:
        idx, d2, m = correspondences(W, fin, tgt, prm["corr_dist_threshold"], exhaustive)
        sums, _ = step_sums(W, tgt, idx, d2)
        mse = float(sums[15]) / m if m > 0 else 0.0
        if m < prm["min_number_correspondences"] or m < 1:
            state, converged = NO_CORRESPONDENCES, False
            break
        T = estimate(sums, m) if transformations is None else np.asarray(transformations[nr], F32)
        W = move_f32(T, W)
        final = mul4_f32(T, final)
        nr += 1
        before = prev_mse
        state, prev_mse, cos, tr2 = criteria(T, nr, mse, prev_mse, prm)
        trace.append(dict(T=T, m=m, mse=mse, prev_mse=before, cos=cos, tr2=tr2, state=state))
        if state != NOT_CONVERGED:
            converged = True
            break
    return dict(final=final, converged=converged, iterations=nr, state=state, matches=int(m), mse=mse, aligned=W, trace=trace)


def margin(res, params=None):
    """how far the deciding quantity of the last two iterations is from its threshold, as a fraction of the threshold (inf where the exit
    does not hang on a comparison of floating-point results: ITERATIONS, NO_CORRESPONDENCES).  TRANSFORM exits and the iterations that
    did not exit on it: |tr2 - eps| / eps (and cos against 1 - eps); ABS_MSE: |(|mse - prev|) - 1e-12| / 1e-12."""
    prm = dict(DEFAULTS, **(params or {}))
    eps = float(prm["transformation_epsilon"])
    out = math.inf
    for it in res["trace"][-2:]:
        if it["state"] == ITERATIONS:
            continue
        if eps > 0.0:
            if it["cos"] >= 1.0 - eps or it["state"] == TRANSFORM:       # the rotation test passes: the translation decides
                out = min(out, abs(it["tr2"] - eps) / eps)
            else:                                                          # the rotation test fails: it decides
                out = min(out, abs(it["cos"] - (1.0 - eps)) / eps)
        if it["state"] != TRANSFORM:
            out = min(out, abs(abs(it["mse"] - it["prev_mse"]) - 1e-12) / 1e-12)
    return out
