"""Brute-force restatement, in NumPy, of the exact k-nearest and radius search over a resident keyframe (mi355ndt_keyframe_knn / _knn_ids /
_radius_search).  This file is the contract the library is held to, word for word: ids and counts as integers, d2 as bit patterns.

  searchable points   three finite coordinates; a point's id is its position in the keyframe
  the query           a point, optionally moved by a 4x4 f32 pose: ((T0 x + T1 y) + T2 z) + T3, every operation rounded on its own; a query
                      that is not finite before or after the move finds nothing (count 0)
  squared distance    f32, (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
  the order           ascending (d2, id): a tie goes to the lower point id (FLANN's order among equals is not observable and not emulated)
  k-NN                the k first searchable points in that order, kept iff (double)d2 <= max_range * max_range (inclusive); counts = the
                      filled slots
  radius              within iff d2 < r2, r2 = (float)(radius * radius), strict; counts = ALL the searchable points within, the lists hold the
                      max_nn nearest of them in the order above
  unused slots        id -1, d2 +inf
"""
import numpy as np

ROWS = 256       # queries of the all-pairs matrix held at once


def searchable(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return p, np.isfinite(p).all(axis=1)


def as_queries(queries):
    """[n,3] f32: x, y, z of [n,>=3] records (or of one point)"""
    a = np.asarray(queries, np.float32)
    if a.size == 0:
        return np.zeros((0, 3), np.float32)
    a = a.reshape(-1, a.shape[-1]) if a.ndim >= 2 else a.reshape(-1, 3)
    return np.ascontiguousarray(a[:, :3])


def move(queries, T=None):
    """(moved [n,3] f32, live [n]): the queries moved by T (4x4, used as f32), and which of them search at all"""
    q = as_queries(queries)
    live = np.isfinite(q).all(axis=1)
    if T is not None:
        M = np.asarray(T, np.float32).reshape(4, 4)
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.stack([((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3] for a in range(3)], axis=1).astype(np.float32)
        live &= np.isfinite(q).all(axis=1)
    return q, live


def d2_rows(p, q):
    """[len(q), len(p)] f32 squared distances, every operation rounded on its own"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def _ordered(points, queries, T):
    """per block of queries: (rows, live, d2 sorted ascending by (d2, id) [rows, m], ids in that order [rows, m]) over the m searchable points"""
    p, fin = searchable(points)
    idx = np.flatnonzero(fin).astype(np.int64)
    s = p[idx]
    q, live = move(queries, T)
    for r0 in range(0, len(q), ROWS):
        rows = slice(r0, min(r0 + ROWS, len(q)))
        d2 = d2_rows(s, q[rows])
        order = np.argsort(d2, axis=1, kind="stable")          # stable over ascending ids: a tie goes to the lower id
        yield rows, live[rows], np.take_along_axis(d2, order, axis=1), idx[order]


def knn(points, queries, k, max_range=np.inf, T=None):
    """(ids [n,k] int32, d2 [n,k] float32, counts [n] int32)"""
    n = len(as_queries(queries))
    ids = np.full((n, k), -1, np.int32)
    out = np.full((n, k), np.inf, np.float32)
    cnt = np.zeros(n, np.int32)
    if n == 0:
        return ids, out, cnt
    with np.errstate(over="ignore"):
        thr2 = np.float64(max_range) * np.float64(max_range)
    for rows, live, d2, pid in _ordered(points, queries, T):
        m = min(k, d2.shape[1])
        keep = (d2[:, :m].astype(np.float64) <= thr2) & live[:, None]
        # (ascending: the kept ones are a prefix of the row)
        ids[rows, :m] = np.where(keep, pid[:, :m], -1)
        out[rows, :m] = np.where(keep, d2[:, :m], np.float32(np.inf))
        cnt[rows] = keep.sum(axis=1)
    return ids, out, cnt


def radius_search(points, queries, radius, max_nn, T=None):
    """(ids [n,max_nn] int32, d2 [n,max_nn] float32, counts [n] int32): counts take in every searchable point within the radius"""
    n = len(as_queries(queries))
    ids = np.full((n, max_nn), -1, np.int32)
    out = np.full((n, max_nn), np.inf, np.float32)
    cnt = np.zeros(n, np.int32)
    if n == 0:
        return ids, out, cnt
    with np.errstate(over="ignore"):
        r2 = np.float32(np.float64(radius) * np.float64(radius))
    for rows, live, d2, pid in _ordered(points, queries, T):
        inside = (d2 < r2) & live[:, None]
        cnt[rows] = inside.sum(axis=1)
        m = min(max_nn, d2.shape[1])
        ids[rows, :m] = np.where(inside[:, :m], pid[:, :m], -1)
        out[rows, :m] = np.where(inside[:, :m], d2[:, :m], np.float32(np.inf))
    return ids, out, cnt
