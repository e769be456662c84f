"""CPU restatement of the window map of GlobalGraphNodelet::cloud_callback (src/global_graph/global_graph_nodelet.cpp:202-244): the scans
between two keyframe decisions moved into the window's first frame, appended in scan order, and the whole window down-sampled with
pcl::VoxelGrid when it closes.  The checker of mi355ndt_window_keyframe (tests/test_window_map_*.py, tools/window_map_timing.py); not part of
the product package.

Written from PCL 1.8.1's documented behaviour and this project's prefilter recipe (ndt_prefilter.hpp, oracle ora_prefilter).  PCL is not in
the reference tree and NONE OF THIS HAS MET A PCL BUILD: the parity is pinned to this restatement, not to a reference binary.

1. Window (global_graph_nodelet.cpp:206, :232, :241-242): scan 0 as it is (`w_cloud = *cloud`); scan k > 0 through
   pcl::transformPointCloud<PointT, double>(cloud, out, (w_odom.inverse() * odom_k).matrix()) (common/impl/transforms.hpp, the Scalar =
   double instantiation): per coordinate a,  (float)(((T(a,0) x + T(a,1) y) + T(a,2) z) + T(a,3))  with x, y, z widened to f64 first --
   f64 products and sums, left to right, no fused multiply-add, ONE rounding to f32 at the end.  In a cloud that is not dense PCL leaves a
   point with a non-finite coordinate as it is; it is restated that way, and step 2 drops such points either way.  `w_cloud += transformed`
   appends in scan order.  The intensity rides along unchanged.
2. pcl::VoxelGrid(leaf) over the window (:214-218; filters/impl/voxel_grid.hpp applyFilter): points with a non-finite x, y or z are skipped;
   f32 minimum and maximum of the others (getMinMax3D); inv = 1.0f / leaf; the "Leaf size is too small for the input dataset" guard --
   (int64((max - min) * inv) + 1) multiplied over the axes exceeds INT32_MAX -- returns the input undown-sampled (here: its finite points in
   order, as the prefilter's restatement has it); min_b = int(floorf(min * inv)), max_b likewise, div_b = max_b - min_b + 1, divb_mul =
   (1, div_b[0], div_b[0] * div_b[1]); cell index of a point = sum over axes of int(floorf(p[a] * inv) - float(min_b[a])) * divb_mul[a];
   the points sorted by cell index; per cell the centroid (common/centroid.h CentroidPoint: AccumulatorXYZ and AccumulatorIntensity add in
   f32, divide by float(n)); output in ascending cell index.  PCL's std::sort is not stable; the order of a cell's points is the INPUT
   order here, as in the prefilter.
3. leaf <= 0: no down-sampling -- the finite points of the window in order.
"""
import numpy as np

INT32_MAX = 2147483647


def transform(scan, T):
    """Step 1 for one scan: [N,>=3] f32 records moved by the 4x4 f64 matrix T; columns past z are carried unchanged."""
    P = np.array(np.asarray(scan, np.float32), copy=True, order="C")
    M = np.asarray(T, np.float64)
    fin = np.isfinite(P[:, :3]).all(axis=1)
    x, y, z = (P[fin, a].astype(np.float64) for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            P[fin, a] = (((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]).astype(np.float32)
    return P


def window_points(scans, rel_poses, intensity=False):
    """Step 1: the window as one [N, 3 or 4] f32 array in scan order (rel_poses[0] is ignored: scan 0 is the window's frame)."""
    w = 4 if intensity else 3
    parts = []
    for k, s in enumerate(scans):
        s = np.asarray(s, np.float32)
        if s.ndim != 2 or s.shape[1] < w:
            raise ValueError("intensity=True needs [N,>=4] records")
        parts.append(np.ascontiguousarray(s[:, :w]) if k == 0 else transform(s[:, :w], rel_poses[k]))
    return np.concatenate(parts) if parts else np.zeros((0, w), np.float32)


def _grid_too_big(mn, mx, inv):
    prod = 1
    for a in range(3):
        e = np.float32(np.float32(mx[a] - mn[a]) * inv)
        if not (e < np.float32(2147483648.0)):
            return True
        prod *= int(e) + 1
    return prod > INT32_MAX


def _cells(P, leaf):
    """(finite mask, cell index of every finite point) or (finite mask, None) when nothing is to be down-sampled."""
    fin = np.isfinite(P[:, :3]).all(axis=1)
    if not (leaf > 0) or not fin.any():
        return fin, None
    Q = P[fin, :3]
    mn, mx = Q.min(axis=0), Q.max(axis=0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = np.float32(1.0) / np.float32(leaf)
        if _grid_too_big(mn, mx, inv):
            return fin, None
        min_b = [int(np.floor(np.float32(mn[a] * inv))) for a in range(3)]
        max_b = [int(np.floor(np.float32(mx[a] * inv))) for a in range(3)]
        mul = (1, max_b[0] - min_b[0] + 1, (max_b[0] - min_b[0] + 1) * (max_b[1] - min_b[1] + 1))
        idx = np.zeros(Q.shape[0], np.int64)
        for a in range(3):
            ijk = (np.floor(Q[:, a] * inv) - np.float32(min_b[a])).astype(np.float32).astype(np.int32)
            idx += ijk.astype(np.int64) * mul[a]
    return fin, idx


def voxel_grid(P, leaf):
    """Steps 2-3 on [N, C] f32 points (C = 3, or 4 with the intensity): [M, C] f32."""
    P = np.ascontiguousarray(np.asarray(P, np.float32))
    fin, idx = _cells(P, leaf)
    Q = P[fin]
    if idx is None:
        return Q.copy()
    order = np.argsort(idx, kind="stable")
    si = idx[order]
    heads = np.nonzero(np.concatenate([[True], si[1:] != si[:-1]]))[0]
    lens = np.diff(np.concatenate([heads, [len(si)]]))
    S = np.zeros((len(heads), P.shape[1]), np.float32)
    for r in range(int(lens.max())):                  # the r-th point of every cell that has one, added in f32: input order within a cell
        live = lens > r
        S[live] += Q[order[heads[live] + r]]
    with np.errstate(invalid="ignore", over="ignore"):
        return (S / lens.astype(np.float32)[:, None]).astype(np.float32)


def window_map(scans, rel_poses, leaf=0.1, intensity=False):
    """The keyframe cloud of a closed window: [M, 3] f32 (or [M, 4] with the intensity)."""
    return voxel_grid(window_points(scans, rel_poses, intensity), leaf)


def run_lengths(scans, rel_poses, leaf=0.1):
    """Points per occupied voxel of the window, in ascending cell index (empty when the window is not down-sampled)."""
    P = window_points(scans, rel_poses)
    _, idx = _cells(P, leaf)
    if idx is None:
        return np.zeros(0, np.int64)
    return np.unique(idx, return_counts=True)[1]
