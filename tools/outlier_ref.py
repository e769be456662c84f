"""Restatement of the prefiltering nodelet's outlier removal (prefiltering_nodelet.cpp:61-78, 150-161) in NumPy, by brute force.

The rules are PCL 1.8's StatisticalOutlierRemoval::applyFilterIndices and RadiusOutlierRemoval and FLANN's L2_Simple, as recalled (neither
library is available to pin them; INTEGRATION.md lists what to pin).  This file is the contract mi355ndt_prefilter_outliers is held to, word
for word:

  searchable points   three finite coordinates (the kd-tree drops the others)
  squared distance    f32, (dx*dx + dy*dy) + dz*dz, every operation rounded on its own
  STATISTICAL         per point, in input order: non-finite, or fewer than mean_k + 1 searchable points -> dist = 0, not valid.  Otherwise the
                      mean_k + 1 smallest squared distances over all searchable points (itself included), ascending, the first dropped;
                      s (f64) += (double)sqrtf(d2) in that order; dist = (float)(s / mean_k).  Then, f64, strictly in index order over every
                      dist (zeros included): sum += dist, sq += dist * dist; mean = sum / n_valid; var = (sq - sum * sum / n_valid) /
                      (n_valid - 1); threshold = mean + stddev_mul * sqrt(var); removed iff (double)dist > threshold.
  RADIUS              r2 = (float)(radius * radius); kept iff at least min_neighbors searchable points other than itself have d2 < r2
                      (strict); non-finite points are removed.  The reference builds this filter and never runs it (:71-78).
"""
import numpy as np

ROWS = 512       # rows of the all-pairs matrix held at once


def searchable(points):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    return p, np.isfinite(p).all(axis=1)


def _d2_rows(p, q):
    """[len(q), len(p)] f32 squared distances, FLANN L2_Simple accumulation order"""
    with np.errstate(over="ignore", invalid="ignore"):
        dx = q[:, None, 0] - p[None, :, 0]
        dy = q[:, None, 1] - p[None, :, 1]
        dz = q[:, None, 2] - p[None, :, 2]
        return (dx * dx + dy * dy) + dz * dz


def seq_sum(v):
    """f64 sum strictly in index order (np.sum is pairwise)"""
    v = np.asarray(v, np.float64)
    return np.float64(np.add.accumulate(v)[-1]) if v.size else np.float64(0.0)


def mean_distances(points, mean_k):
    """(dist [N] f32, n_valid): StatisticalOutlierRemoval's first pass"""
    p, fin = searchable(points)
    n = len(p)
    dist = np.zeros(n, np.float32)
    idx = np.flatnonzero(fin)
    if len(idx) < mean_k + 1:
        return dist, 0
    s = p[idx]
    for r0 in range(0, len(idx), ROWS):
        d2 = _d2_rows(s, s[r0:r0 + ROWS])
        near = np.sort(np.partition(d2, mean_k, axis=1)[:, :mean_k + 1], axis=1)[:, 1:]     # k + 1 smallest, ascending, the first dropped
        acc = np.zeros(len(near), np.float64)
        for c in range(mean_k):
            acc += np.sqrt(near[:, c]).astype(np.float64)                                    # sqrtf, widened, ascending order
        dist[idx[r0:r0 + ROWS]] = (acc / np.float64(mean_k)).astype(np.float32)
    return dist, len(idx)


def statistics(dist, n_valid, stddev_mul):
    d = np.asarray(dist, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        total, sq = seq_sum(d), seq_sum(d * d)
        nv = np.float64(n_valid)
        mean = total / nv
        var = (sq - total * total / nv) / (nv - np.float64(1.0))
        stddev = np.sqrt(var)
        threshold = mean + np.float64(stddev_mul) * stddev
    return dict(n_in=len(d), n_valid=int(n_valid), mean=mean, stddev=stddev, threshold=threshold)


def statistical(points, mean_k=20, stddev_mul=1.0):
    """dict: dist, n_in, n_valid, mean, stddev, threshold, kept (indices, ascending)"""
    dist, n_valid = mean_distances(points, mean_k)
    out = statistics(dist, n_valid, stddev_mul)
    with np.errstate(invalid="ignore"):
        removed = dist.astype(np.float64) > out["threshold"]
    out.update(dist=dist, kept=np.flatnonzero(~removed))
    return out


def radius(points, radius=0.8, min_neighbors=2):
    """dict: kept (indices, ascending); dist and the statistics are zeros, as the library returns them"""
    p, fin = searchable(points)
    n = len(p)
    r2 = np.float32(np.float64(radius) * np.float64(radius))
    idx = np.flatnonzero(fin)
    keep = np.zeros(n, bool)
    s = p[idx]
    for r0 in range(0, len(idx), ROWS):
        inside = _d2_rows(s, s[r0:r0 + ROWS]) < r2
        rows = np.arange(inside.shape[0])
        inside[rows, r0 + rows] = False                                                      # the point itself
        keep[idx[r0:r0 + ROWS]] = inside.sum(axis=1) >= min_neighbors
    return dict(dist=np.zeros(n, np.float32), n_in=n, n_valid=0, mean=0.0, stddev=0.0, threshold=0.0, kept=np.flatnonzero(keep))


def remove_outliers(points, method="STATISTICAL", mean_k=20, stddev_mul=1.0, radius_m=0.8, min_neighbors=2):
    """the survivors, in order, and the dict above"""
    p, _ = searchable(points)
    r = statistical(p, mean_k, stddev_mul) if method == "STATISTICAL" else radius(p, radius_m, min_neighbors)
    return p[r["kept"]], r
