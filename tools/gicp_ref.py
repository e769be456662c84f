"""Restatement of pclomp::GeneralizedIterativeClosestPoint (include/ndt_omp/gicp_omp.h, gicp_omp_impl.hpp) in NumPy / plain Python, by
brute force: the contract the engine's GICP surface (mi355ndt_gicp_*, lv_slam_amd/csrc/ndt_gicp.hpp, ndt_host_gicp.hpp, gicp_bfgs.hpp) is
held to.  Independent of the library: nothing here loads it.

  covariances      computeCovariances (:60-133).  Searchable points have three finite coordinates; squared distance f32,
                   (dx*dx + dy*dy) + dz*dz; the k nearest searchable points, the point itself included, ascending by (d2, point id) -- the
                   engine's tie rule, FLANN's is not observable; mean and lower triangle accumulated in f64 in that order, the products
                   pt.r * pt.c in f32; cyclic Jacobi (the engine's eigen_sym3, restated below) where the reference runs Eigen::JacobiSVD;
                   cov = (c0 c0' + c1 c1') + (eps c2) c2' over the eigenvectors by descending eigenvalue, equal ones in column order.  A non-finite point gets zeros.
  correspondences  (:415-466)  q = T (G p), two f32 products of the form ((a x + b y) + c z) + d; exhaustive 1-NN, a tie to the lower id;
                   matched iff (double)d2 < threshold^2; R = the 3x3 block of the f64 product T G; M = (R C1 R' + C2)^-1, each 3x3 product
                   entry as (a0 b0 + a1 b1) + a2 b2, the inverse by cofactors over the determinant (Eigen 3.3 compute_inverse).
  cost             operator(), df, fdf (:255-378): thirteen sums over the matched points -- the restatement sums in index order, the engine
                   by a fixed tree; the tests bound the difference by 1e-11 of the sum of the absolute terms.
  BFGS             PCL's bfgs.h = GSL's vector_bfgs2, RESTATED AS RECALLED (neither is in the reference tree): the same statements as
                   lv_slam_amd/csrc/gicp_bfgs.hpp, in Python floats, word for word.
  align            computeTransformation (:380-515), the composition final = [R_t R_g | t_t + t_g] and the two different ways the guess
                   enters (matching: T (G p); cost: applyState(G, x)) included.
Unpinned: INTEGRATION.md section 5.
"""
import math

import numpy as np

F32 = np.float32
ROWS = 512
NEG_GRADIENT_EPS, NOT_STARTED, RUNNING, SUCCESS, NO_PROGRESS = -3, -2, -1, 0, 1
EPS = 2.2204460492503131e-16

DEFAULTS = dict(k_correspondences=20, gicp_epsilon=1e-3, rotation_epsilon=2e-3, transformation_epsilon=5e-4, max_iterations=200,
                max_inner_iterations=20, corr_dist_threshold=5.0)                       # gicp_omp.h:110-120
FACTORY = dict(DEFAULTS, transformation_epsilon=0.01, max_iterations=64, k_correspondences=20, max_inner_iterations=20)   # registrations.cpp:47-51


def searchable(points):
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    return p, np.isfinite(p).all(axis=1)


def d2_rows(p, q):
    """[len(q), len(p)] f32 squared distances, FLANN L2_Simple accumulation order"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def knn(points, k):
    """(ids [n_searchable, k] into points, d2 [n_searchable, k], idx of the searchable points): ascending by (d2, id)"""
    p, fin = searchable(points)
    idx = np.flatnonzero(fin)
    s = p[idx]
    ids = np.zeros((len(idx), k), np.int64)
    d2k = np.zeros((len(idx), k), F32)
    for r0 in range(0, len(idx), ROWS):
        d2 = d2_rows(s, s[r0:r0 + ROWS])
        # the k smallest by (d2, id): where no other point shares the k-th distance, the k smallest are a set -- put them in id order and
        # sort stably by distance; the rows with a tie at the edge go through a stable sort of the whole row
        part = np.sort(np.argpartition(d2, k - 1, axis=1)[:, :k], axis=1)
        dk = np.take_along_axis(d2, part, axis=1)
        order = np.take_along_axis(part, np.argsort(dk, axis=1, kind="stable"), axis=1)
        tied = np.flatnonzero((d2 <= dk.max(axis=1, keepdims=True)).sum(axis=1) != k)
        if len(tied):
            order[tied] = np.argsort(d2[tied], axis=1, kind="stable")[:, :k]
        ids[r0:r0 + ROWS] = idx[order]
        d2k[r0:r0 + ROWS] = np.take_along_axis(d2, order, axis=1)
    return ids, d2k, idx


def eigen_sym3(A):
    """the engine's cyclic Jacobi (ndt_math.hpp eigen_sym3): A 3x3 symmetric (lower triangle read) -> (ascending eigenvalues, V columns)"""
    a = [[float(A[0][0]), float(A[1][0]), float(A[2][0])], [float(A[1][0]), float(A[1][1]), float(A[2][1])],
         [float(A[2][0]), float(A[2][1]), float(A[2][2])]]
    v = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for sweep in range(64):
        off = abs(a[0][1]) + abs(a[0][2]) + abs(a[1][2])
        if off == 0.0:
            break
        for k in range(3):
            p = 1 if k == 2 else 0
            q = 1 if k == 0 else 2
            r = 3 - p - q
            apq = a[p][q]
            if apq == 0.0:
                continue
            g = 100.0 * abs(apq)
            if sweep > 3 and abs(a[p][p]) + g == abs(a[p][p]) and abs(a[q][q]) + g == abs(a[q][q]):
                a[p][q] = a[q][p] = 0.0
                continue
            h = a[q][q] - a[p][p]
            if abs(h) + g == abs(h):
                t = apq / h
            else:
                theta = 0.5 * h / apq
                t = 1.0 / (abs(theta) + math.sqrt(1.0 + theta * theta))
                if theta < 0.0:
                    t = -t
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = t * c
            tau = s / (1.0 + c)
            hh = t * apq
            a[p][p] -= hh
            a[q][q] += hh
            a[p][q] = a[q][p] = 0.0
            arp, arq = a[r][p], a[r][q]
            a[r][p] = a[p][r] = arp - s * (arq + arp * tau)
            a[r][q] = a[q][r] = arq + s * (arp - arq * tau)
            for i in range(3):
                vip, viq = v[i][p], v[i][q]
                v[i][p] = vip - s * (viq + vip * tau)
                v[i][q] = viq + s * (vip - viq * tau)
    d = [a[0][0], a[1][1], a[2][2]]
    o = [0, 1, 2]
    if d[o[1]] < d[o[0]]:
        o[0], o[1] = o[1], o[0]
    if d[o[2]] < d[o[1]]:
        o[1], o[2] = o[2], o[1]
    if d[o[1]] < d[o[0]]:
        o[0], o[1] = o[1], o[0]
    return [d[o[j]] for j in range(3)], [[v[i][o[j]] for j in range(3)] for i in range(3)]


def covariances(points, k=20, gicp_epsilon=1e-3, return_eigenvalues=False):
    """[n, 9] f64 (row-major 3x3 per point); ValueError when k exceeds the number of searchable points (the reference prints an error and
    reads unsized storage)"""
    p, fin = searchable(points)
    n = len(p)
    if k < 1 or k > 64:
        raise ValueError("k outside 1..64")
    if k > int(fin.sum()):
        raise ValueError("fewer searchable points than k")
    ids, _, idx = knn(p, k)
    mean = np.zeros((len(idx), 3), np.float64)
    low = np.zeros((len(idx), 6), np.float64)                         # (0,0) (1,0) (1,1) (2,0) (2,1) (2,2)
    for j in range(k):
        pt = p[ids[:, j]]
        x, y, z = pt[:, 0], pt[:, 1], pt[:, 2]
        mean[:, 0] += x.astype(np.float64); mean[:, 1] += y.astype(np.float64); mean[:, 2] += z.astype(np.float64)
        for c, v in enumerate((x * x, y * x, y * y, z * x, z * y, z * z)):      # f32 products, as the reference writes them
            low[:, c] += v.astype(np.float64)
    kd = np.float64(k)
    mean = mean / kd
    pos = {(0, 0): 0, (1, 0): 1, (1, 1): 2, (2, 0): 3, (2, 1): 4, (2, 2): 5}
    out = np.zeros((n, 9), np.float64)
    evs = np.zeros((n, 3), np.float64)
    eps = float(gicp_epsilon)
    for row, i in enumerate(idx):
        A = [[0.0] * 3 for _ in range(3)]
        for (r, c), at in pos.items():
            A[r][c] = A[c][r] = float(low[row, at] / kd - mean[row, r] * mean[row, c])
        ev, V = eigen_sym3(A)
        o = [0, 1, 2]                                                 # descending eigenvalue, equal ones in column order
        if ev[o[1]] > ev[o[0]]:
            o[0], o[1] = o[1], o[0]
        if ev[o[2]] > ev[o[1]]:
            o[1], o[2] = o[2], o[1]
        if ev[o[1]] > ev[o[0]]:
            o[0], o[1] = o[1], o[0]
        c0, c1, c2 = ([V[r][o[s]] for r in range(3)] for s in range(3))
        for r in range(3):
            for c in range(3):
                out[i, 3 * r + c] = (c0[r] * c0[c] + c1[r] * c1[c]) + (eps * c2[r]) * c2[c]
        evs[i] = ev
    return (out, evs) if return_eigenvalues else out


# ---- f32 pose arithmetic ---------------------------------------------------------------------------------------
def move_f32(T, p):
    """rows of p moved by the 4x4 f32 T: ((a x + b y) + c z) + d per coordinate"""
    T = np.asarray(T, F32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def _q_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def apply_state(t, x):
    """applyState (:517-528): AngleAxisf(x5, Z) * AngleAxisf(x4, Y) * AngleAxisf(x3, X) -- Eigen multiplies angle-axes as quaternions --
    in front of t's rotation, the translation added; all f32.  Returns a new 4x4 f32."""
    t = np.array(t, F32)
    qs = []
    for angle, axis in ((x[5], 2), (x[4], 1), (x[3], 0)):
        ha = F32(0.5) * F32(angle)
        w, s = F32(math.cos(float(ha))), F32(math.sin(float(ha)))
        v = [F32(0.0)] * 3
        v[axis] = s
        qs.append((w, v[0], v[1], v[2]))
    w, qx, qy, qz = _q_mul(_q_mul(qs[0], qs[1]), qs[2])
    two = F32(2.0)
    tx, ty, tz = two * qx, two * qy, two * qz
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    one = F32(1.0)
    R = [[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]]
    out = t.copy()
    for r in range(3):
        for c in range(3):
            out[r, c] = (R[r][0] * t[0, c] + R[r][1] * t[1, c]) + R[r][2] * t[2, c]
        out[r, 3] = t[r, 3] + F32(x[r])
    return out


def _mat3_mul(A, B, transpose_b=False):
    """[m, 3, 3] products, entry (r, c) = (a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c"""
    out = np.zeros(np.broadcast_shapes(A.shape, B.shape), np.float64)
    for r in range(3):
        for c in range(3):
            b = (lambda k: B[..., c, k]) if transpose_b else (lambda k: B[..., k, c])
            out[..., r, c] = (A[..., r, 0] * b(0) + A[..., r, 1] * b(1)) + A[..., r, 2] * b(2)
    return out


def _mat3_inverse(m):
    """Eigen 3.3 compute_inverse<Matrix3d>, as ndt_math.hpp mat3_inverse states it"""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return m[..., i1, j1] * m[..., i2, j2] - m[..., i1, j2] * m[..., i2, j1]
    c0, c1, c2 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c0 * m[..., 0, 0] + c1 * m[..., 1, 0]) + c2 * m[..., 2, 0]
    with np.errstate(all="ignore"):
        invdet = 1.0 / det
    out = np.zeros_like(m)
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in range(3):
                out[..., a, b] = (c0, c1, c2)[b] * invdet if a == 0 else cof(b, a) * invdet
    return out


def transform_R(T, G):
    """the 3x3 block of the f64 product T G (:423-429), k ascending"""
    T, G = np.asarray(T, F32).astype(np.float64), np.asarray(G, F32).astype(np.float64)
    R = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            s = 0.0
            for k in range(4):
                s = s + float(T[i, k]) * float(G[k, j])
            R[i, j] = s
    return R


def correspondences(src, tgt, cov_src, cov_tgt, guess, T, corr_dist_threshold=5.0):
    """(idx [n_src] int32 (-1: none), M [n_src, 9] f64 (zeros where unmatched), m)"""
    s, sfin = searchable(src)
    t, tfin = searchable(tgt)
    q = move_f32(T, move_f32(guess, s))
    live = sfin & np.isfinite(q).all(axis=1)
    idx = np.full(len(s), -1, np.int32)
    thr2 = np.float64(corr_dist_threshold) * np.float64(corr_dist_threshold)
    tid = np.flatnonzero(tfin)
    ts = t[tid]
    if len(tid):
        for r0 in range(0, len(s), ROWS):
            d2 = d2_rows(ts, q[r0:r0 + ROWS])
            with np.errstate(invalid="ignore"):
                d2 = np.where(np.isnan(d2), F32(np.inf), d2)
            best = np.argmin(d2, axis=1)                               # the first minimum: the lower id
            dmin = d2[np.arange(len(best)), best]
            ok = live[r0:r0 + ROWS] & (dmin.astype(np.float64) < thr2)
            idx[r0:r0 + ROWS] = np.where(ok, tid[best], -1)
    M = np.zeros((len(s), 3, 3), np.float64)
    mt = np.flatnonzero(idx >= 0)
    if len(mt):
        R = transform_R(T, guess)
        C1 = np.asarray(cov_src, np.float64).reshape(-1, 3, 3)[mt]
        C2 = np.asarray(cov_tgt, np.float64).reshape(-1, 3, 3)[idx[mt]]
        M1 = _mat3_mul(R[None], C1)
        temp = _mat3_mul(M1, R[None], transpose_b=True)
        temp = temp + C2
        M[mt] = _mat3_inverse(temp)
    return idx, M.reshape(-1, 9), int(len(mt))


def seq_sum(v):
    v = np.asarray(v, np.float64)
    return float(np.add.accumulate(v)[-1]) if v.size else 0.0


def cost_sums(src, tgt, idx, M, x, base):
    """the thirteen sums over the matched points, in index order, and the sums of their absolute terms: f, g_t[3], Rm[9] (row-major)"""
    s, _ = searchable(src)
    t, _ = searchable(tgt)
    mt = np.flatnonzero(np.asarray(idx) >= 0)
    Tx = apply_state(base, x)
    p = s[mt]
    pp = move_f32(Tx, p)
    res = (pp - t[np.asarray(idx)[mt]]).astype(np.float64)             # an f32 subtraction, widened
    Mm = np.asarray(M, np.float64).reshape(-1, 3, 3)[mt]
    temp = np.stack([(Mm[:, r, 0] * res[:, 0] + Mm[:, r, 1] * res[:, 1]) + Mm[:, r, 2] * res[:, 2] for r in range(3)], axis=1)
    bp = move_f32(base, p).astype(np.float64)
    terms = [(res[:, 0] * temp[:, 0] + res[:, 1] * temp[:, 1]) + res[:, 2] * temp[:, 2]]
    terms += [temp[:, c] for c in range(3)]
    terms += [bp[:, r] * temp[:, c] for r in range(3) for c in range(3)]
    return np.array([seq_sum(v) for v in terms]), np.array([seq_sum(np.abs(v)) for v in terms]), len(mt)


def r_derivative(x, R, g):
    """computeRDerivative (:134-187): g[3..5] = tr(dR/dangle' R), matricesInnerProd's order (gicp_omp.h:320-329)"""
    phi, theta, psi = float(x[3]), float(x[4]), float(x[5])
    cphi, sphi, ctheta, stheta, cpsi, spsi = math.cos(phi), math.sin(phi), math.cos(theta), math.sin(theta), math.cos(psi), math.sin(psi)
    dphi = [[0.0, sphi * spsi + cphi * cpsi * stheta, cphi * spsi - cpsi * sphi * stheta],
            [0.0, -cpsi * sphi + cphi * spsi * stheta, -cphi * cpsi - sphi * spsi * stheta],
            [0.0, cphi * ctheta, -ctheta * sphi]]
    dtheta = [[-cpsi * stheta, cpsi * ctheta * sphi, cphi * cpsi * ctheta],
              [-spsi * stheta, ctheta * sphi * spsi, cphi * ctheta * spsi],
              [-ctheta, -sphi * stheta, -cphi * stheta]]
    dpsi = [[-ctheta * spsi, -cphi * cpsi - sphi * spsi * stheta, cpsi * sphi - cphi * spsi * stheta],
            [cpsi * ctheta, -cphi * spsi + cpsi * sphi * stheta, sphi * spsi + cphi * cpsi * stheta],
            [0.0, 0.0, 0.0]]
    for at, D in ((3, dphi), (4, dtheta), (5, dpsi)):
        r = 0.0
        for i in range(3):
            for j in range(3):
                r += D[j][i] * float(R[i][j])
        g[at] = r


def cost_from_sums(sums, m, x):
    """(f, g[6]) from the thirteen sums: f /= m, g_t *= 2/m, Rm *= 2/m, computeRDerivative"""
    f = float(sums[0]) / float(m)
    w = 2.0 / m
    g = [float(sums[1]) * w, float(sums[2]) * w, float(sums[3]) * w, 0.0, 0.0, 0.0]
    R = [[float(sums[4 + 3 * r + c]) * w for c in range(3)] for r in range(3)]
    r_derivative(x, R, g)
    return f, g


def cost(src, tgt, idx, M, x, base):
    sums, _, m = cost_sums(src, tgt, idx, M, x, base)
    return cost_from_sums(sums, m, x)


# ---- BFGS (gicp_bfgs.hpp, statement for statement) ------------------------------------------------------------
def dot(a, b):
    s = a[0] * b[0]
    for i in range(1, 6):
        s = s + a[i] * b[i]
    return s


def norm(a):
    return math.sqrt(dot(a, a))


def solve_quadratic(a, b, c):
    if a == 0:
        if b == 0:
            return 0, 0.0, 0.0
        return 1, -c / b, 0.0
    disc = b * b - 4 * a * c
    if disc > 0:
        if b == 0:
            r = math.sqrt(-c / a)
            return 2, -r, r
        sgnb = 1.0 if b > 0 else -1.0
        temp = -0.5 * (b + sgnb * math.sqrt(disc))
        r1, r2 = temp / a, c / temp
        return (2, r1, r2) if r1 < r2 else (2, r2, r1)
    if disc == 0:
        return 2, -0.5 * b / a, -0.5 * b / a
    return 0, 0.0, 0.0


def interp_quad(f0, fp0, f1, zl, zh):
    fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0))
    fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0))
    c = 2 * (f1 - f0 - fp0)
    zmin, fmin = zl, fl
    if fh < fmin:
        zmin, fmin = zh, fh
    if c > 0:
        z = -fp0 / c
        if zl < z < zh:
            f = f0 + z * (fp0 + z * (f1 - f0 - fp0))
            if f < fmin:
                zmin, fmin = z, f
    return zmin


def cubic(c0, c1, c2, c3, z):
    return c0 + z * (c1 + z * (c2 + z * c3))


def interp_cubic(f0, fp0, f1, fp1, zl, zh):
    eta = 3 * (f1 - f0) - 2 * fp0 - fp1
    xi = fp0 + fp1 - 2 * (f1 - f0)
    c0, c1, c2, c3 = f0, fp0, eta, xi
    zmin, fmin = zl, cubic(c0, c1, c2, c3, zl)

    def check(z, zmin, fmin):
        y = cubic(c0, c1, c2, c3, z)
        return (z, y) if y < fmin else (zmin, fmin)
    zmin, fmin = check(zh, zmin, fmin)
    n, z0, z1 = solve_quadratic(3 * c3, 2 * c2, c1)
    if n == 2:
        if zl < z0 < zh:
            zmin, fmin = check(z0, zmin, fmin)
        if zl < z1 < zh:
            zmin, fmin = check(z1, zmin, fmin)
    elif n == 1:
        if zl < z0 < zh:
            zmin, fmin = check(z0, zmin, fmin)
    return zmin


def interpolate(a, fa, fpa, b, fb, fpb, xmin, xmax, order):
    zmin, zmax = (xmin - a) / (b - a), (xmax - a) / (b - a)
    if zmin > zmax:
        zmin, zmax = zmax, zmin
    if order > 2 and math.isfinite(fpb):
        z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax)
    else:
        z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax)
    return a + z * (b - a)


class BFGS:
    """fn: an object with f(x) -> float, df(x) -> list of 6, fdf(x) -> (float, list of 6); x: lists of 6 Python floats"""

    def __init__(self, fn, sigma=0.01, rho=0.01, tau1=9.0, tau2=0.05, tau3=0.5, step_size=1.0, order=3):
        self.fn = fn
        self.sigma, self.rho, self.tau1, self.tau2, self.tau3, self.step_size, self.order = sigma, rho, tau1, tau2, tau3, step_size, order

    # the function along the line
    def moveto(self, alpha):
        if alpha == self.x_key:
            return
        self.x_alpha = [self.wx[i] + alpha * self.p[i] for i in range(6)]
        self.x_key = alpha

    def slope(self):
        return dot(self.g_alpha, self.p)

    def wrap_f(self, alpha):
        if alpha == self.f_key:
            return self.f_alpha
        self.moveto(alpha)
        self.f_alpha = self.fn.f(self.x_alpha)
        self.f_key = alpha
        return self.f_alpha

    def wrap_df(self, alpha):
        if alpha == self.df_key:
            return self.df_alpha
        self.moveto(alpha)
        if alpha != self.g_key:
            self.g_alpha = list(self.fn.df(self.x_alpha))
            self.g_key = alpha
        self.df_alpha = self.slope()
        self.df_key = alpha
        return self.df_alpha

    def wrap_fdf(self, alpha):
        if alpha == self.f_key and alpha == self.df_key:
            return self.f_alpha, self.df_alpha
        if alpha == self.f_key or alpha == self.df_key:
            return self.wrap_f(alpha), self.wrap_df(alpha)
        self.moveto(alpha)
        f, g = self.fn.fdf(self.x_alpha)
        self.f_alpha, self.g_alpha = f, list(g)
        self.f_key = self.g_key = alpha
        self.df_alpha = self.slope()
        self.df_key = alpha
        return self.f_alpha, self.df_alpha

    def reset_line(self, x, g):
        self.wx = x
        self.x_alpha, self.x_key = list(x), 0.0
        self.f_key = 0.0
        self.g_alpha, self.g_key = list(g), 0.0
        self.df_alpha, self.df_key = self.slope(), 0.0

    def line_search(self, alpha1):
        """(status, alpha or None): None = *alpha_new was not written"""
        rho, sigma, tau1, tau2, tau3, order = self.rho, self.sigma, self.tau1, self.tau2, self.tau3, self.order
        alpha, alpha_prev = alpha1, 0.0
        a, b, fb, fpb = 0.0, alpha, 0.0, 0.0
        i = 0
        f0, fp0 = self.wrap_fdf(0.0)
        falpha_prev, fpalpha_prev = f0, fp0
        fa, fpa = f0, fp0
        while i < 100:
            i += 1
            falpha = self.wrap_f(alpha)
            if falpha > f0 + alpha * rho * fp0 or falpha >= falpha_prev:
                a, fa, fpa = alpha_prev, falpha_prev, fpalpha_prev
                b, fb, fpb = alpha, falpha, math.nan
                break
            fpalpha = self.wrap_df(alpha)
            if abs(fpalpha) <= -sigma * fp0:
                return SUCCESS, alpha
            if fpalpha >= 0:
                a, fa, fpa = alpha, falpha, fpalpha
                b, fb, fpb = alpha_prev, falpha_prev, fpalpha_prev
                break
            delta = alpha - alpha_prev
            lower, upper = alpha + delta, alpha + tau1 * delta
            alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, lower, upper, order)
            alpha_prev, falpha_prev, fpalpha_prev = alpha, falpha, fpalpha
            alpha = alpha_next
        else:
            i += 1                                                       # (`while (i++ < n)`: the failed test increments as well)
        while i < 100:
            i += 1
            delta = b - a
            lower, upper = a + tau2 * delta, b - tau3 * delta
            alpha = interpolate(a, fa, fpa, b, fb, fpb, lower, upper, order)
            falpha = self.wrap_f(alpha)
            if (a - alpha) * fpa <= EPS:
                return NO_PROGRESS, None
            if falpha > f0 + rho * alpha * fp0 or falpha >= fa:
                b, fb, fpb = alpha, falpha, math.nan
            else:
                fpalpha = self.wrap_df(alpha)
                if abs(fpalpha) <= -sigma * fp0:
                    return SUCCESS, alpha
                if ((b - a) >= 0 and fpalpha >= 0) or ((b - a) <= 0 and fpalpha <= 0):
                    b, fb, fpb = a, fa, fpa
                    a, fa, fpa = alpha, falpha, fpalpha
                else:
                    a, fa, fpa = alpha, falpha, fpalpha
        return SUCCESS, None

    def minimize_init(self, x):
        self.iter, self.step, self.delta_f = 0, self.step_size, 0.0
        self.f, g = self.fn.fdf(x)
        self.gradient = list(g)
        self.x0, self.g0 = list(x), list(g)
        self.g0norm = norm(self.g0)
        with np.errstate(all="ignore"):
            inv = float(np.float64(-1.0) / np.float64(self.g0norm))      # (-1 / 0 = -inf, as in C)
            self.p = [float(np.float64(self.gradient[i]) * np.float64(inv)) for i in range(6)]
        self.pnorm = norm(self.p)
        self.fp0 = -self.g0norm
        self.f_alpha = self.f
        self.reset_line(x, self.gradient)
        return NOT_STARTED

    def minimize_one_step(self, x):
        """x is updated in place; returns the status"""
        f0 = self.f
        if self.pnorm == 0.0 or self.g0norm == 0.0 or self.fp0 == 0:
            return NO_PROGRESS
        if self.delta_f < 0:
            d, e = -self.delta_f, 10 * EPS * abs(f0)
            dl = d if d > e else e
            t = 2.0 * dl / (-self.fp0)
            alpha1 = t if t < 1.0 else 1.0
        else:
            alpha1 = abs(self.step)
        self.wx = x
        status, alpha = self.line_search(alpha1)
        if status != SUCCESS:
            return status
        if alpha is None:
            alpha = 0.0
        self.f, _ = self.wrap_fdf(alpha)
        x[:] = self.x_alpha
        g = self.gradient = list(self.g_alpha)
        self.delta_f = self.f - f0
        dx0 = [x[i] - self.x0[i] for i in range(6)]
        dg0 = [g[i] - self.g0[i] for i in range(6)]
        dxg, dgg, dxdg, dgnorm = dot(dx0, g), dot(dg0, g), dot(dx0, dg0), norm(dg0)
        if dxdg != 0:
            B = dxg / dxdg
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg
        else:
            A = B = 0.0
        p = [(g[i] - A * dx0[i]) - B * dg0[i] for i in range(6)]
        self.g0, self.x0 = list(g), list(x)
        self.g0norm = norm(self.g0)
        self.pnorm = norm(p)
        pg = dot(p, g)
        direction = -1.0 if pg >= 0.0 else 1.0
        with np.errstate(all="ignore"):
            scale = float(np.float64(direction) / np.float64(self.pnorm))
            self.p = [float(np.float64(p[i]) * np.float64(scale)) for i in range(6)]
        self.pnorm = norm(self.p)
        self.fp0 = dot(self.p, self.g0)
        self.reset_line(x, g)
        self.iter += 1
        return SUCCESS

    def test_gradient(self, epsabs):
        if epsabs < 0:
            return NEG_GRADIENT_EPS
        return SUCCESS if norm(self.gradient) < epsabs else RUNNING


def minimize(bfgs, x, gradient_tol, max_inner_iterations, trace=None):
    """the driver loop of estimateRigidTransformationBFGS (:229-241): (last status, inner iterations); x in place"""
    inner = 0
    bfgs.minimize_init(x)
    while True:
        inner += 1
        result = bfgs.minimize_one_step(x)
        if trace is not None:
            trace(inner, result, x, bfgs)
        if result:
            break
        result = bfgs.test_gradient(gradient_tol)
        if not (result == RUNNING and inner < max_inner_iterations):
            break
    return result, inner


def accepted(result, inner, max_inner_iterations):
    return result == NO_PROGRESS or result == SUCCESS or inner == max_inner_iterations


# ---- the outer loop ------------------------------------------------------------------------------------------
class _Functor:
    def __init__(self, src, tgt, idx, M, base):
        self.a = (src, tgt, idx, M)
        self.base = base
        self.evaluations = 0

    def fdf(self, x):
        self.evaluations += 1
        return cost(*self.a, x, self.base)

    def f(self, x):
        return self.fdf(x)[0]

    def df(self, x):
        return self.fdf(x)[1]


def state_of(T):
    """the start of the optimiser from transformation_ (:204-210); the angles are taken in f64 from the f32 entries"""
    T = np.asarray(T, F32)
    return [float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), math.atan2(float(T[2, 1]), float(T[2, 2])), math.asin(-float(T[2, 0])),
            math.atan2(float(T[1, 0]), float(T[0, 0]))]


def compose_final(prev, guess):
    """final = [R_t R_g | t_t + t_g] (:508-511), f32"""
    prev, guess = np.asarray(prev, F32), np.asarray(guess, F32)
    out = np.eye(4, dtype=F32)
    for r in range(3):
        for c in range(3):
            out[r, c] = (prev[r, 0] * guess[0, c] + prev[r, 1] * guess[1, c]) + prev[r, 2] * guess[2, c]
        out[r, 3] = prev[r, 3] + guess[r, 3]
    return out


def align(src, tgt, guess, params=None, cov_src=None, cov_tgt=None):
    """computeTransformation (:380-515).  dict: final, converged, iterations, inner_status, n_matched, delta, deltas, aligned"""
    prm = dict(DEFAULTS, **(params or {}))
    guess = np.asarray(guess, F32)
    if cov_tgt is None:
        cov_tgt = covariances(tgt, prm["k_correspondences"], prm["gicp_epsilon"])
    if cov_src is None:
        cov_src = covariances(src, prm["k_correspondences"], prm["gicp_epsilon"])
    T = np.eye(4, dtype=F32)
    prev = T.copy()
    nr, converged, delta, deltas, status, m = 0, False, 0.0, [], NOT_STARTED, 0
    while not converged:
        idx, M, m = correspondences(src, tgt, cov_src, cov_tgt, guess, T, prm["corr_dist_threshold"])
        prev = T.copy()
        if m < 4:                                                        # NotEnoughPointsException -> break, unconverged
            break
        x = state_of(T)
        fn = _Functor(src, tgt, idx, M, guess)
        status, inner = minimize(BFGS(fn), x, 1e-2, prm["max_inner_iterations"])
        if not accepted(status, inner, prm["max_inner_iterations"]):     # SolverDidntConvergeException -> break, unconverged
            break
        T = apply_state(np.eye(4, dtype=F32), x)
        delta = 0.0
        for k in range(4):
            for l in range(4):
                ratio = 1.0 / prm["rotation_epsilon"] if (k < 3 and l < 3) else 1.0 / prm["transformation_epsilon"]
                c_delta = ratio * float(abs(prev[k, l] - T[k, l]))     # an f32 difference
                if c_delta > delta:
                    delta = c_delta
        deltas.append(delta)
        nr += 1
        if nr >= prm["max_iterations"] or delta < 1:
            converged = True
            prev = T.copy()
    final = compose_final(prev, guess)
    s, _ = searchable(src)
    return dict(final=final, converged=converged, iterations=nr, inner_status=int(status), n_matched=int(m), delta=delta, deltas=deltas,
                aligned=move_f32(final, s))
