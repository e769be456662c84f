"""The restatement mi355ndt_batch_prefilter / mi355ndt_prefilter_p are held to for the two nodelet options the VoxelGrid oracle does not cover
(PrefilteringNodelet, src/lidar_odometry/prefiltering_nodelet.cpp): downsample_method = APPROX_VOXELGRID (:48-52) and
use_angle_calibration (:88, :118-122, :183-220).  NumPy, no GPU.

  approx_voxel_grid(xyz, leaf)   pcl::ApproximateVoxelGrid as recalled from PCL 1.8.1 approximate_voxel_grid.hpp, the literal sequential loop
  angle_calibration(xyz, rad)    vertical_angle_calibration, Eigen 3.3's operations one by one in f64
  prefilter(xyz, params)         base_link move -> calibration -> gate -> down-sampling, cloud_callback's order; VOXELGRID and NONE
                                 (leaf <= 0) go through oracle.oracle_py.prefilter

Neither PCL nor Eigen is available to pin these against; INTEGRATION.md section 5 lists the rules a PCL host has to confirm."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HISTSIZE = 512                                  # histsize_
MULTIPLIERS = (7171, 3079, 4231)
ANGLE_RAD = 0.11 * math.pi / 180                # "detal" (:190)
DEFAULTS = dict(distance_near=0.5, distance_far=100.0, leaf=0.1, use_distance_filter=True, transform=None, downsample_method="VOXELGRID",
                angle_calibration=False)


def _xyz(xyz):
    a = np.asarray(xyz, np.float32)
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1] if a.ndim == 2 else 3)[:, :3])


def cells(xyz, leaf):
    """(floor(coord * inv) as f32 [N,3], inv): inv = 1.0f / leaf, the products f32"""
    inv = np.float32(1.0) / np.float32(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor(_xyz(xyz) * inv), inv


def cells_overflow(xyz, leaf):
    """some |floor(coord * inv)| >= 2^31 (PCL's cast to int is undefined behaviour there): the cloud is left un-down-sampled"""
    f, _ = cells(xyz, leaf)
    return bool(len(f)) and not bool(np.all(np.abs(f) < np.float32(2147483648.0)))


def approx_voxel_grid(xyz, leaf):
    """pcl::ApproximateVoxelGrid::applyFilter over x, y, z.  Non-finite points are dropped.  Returns [M,3] f32 in PCL's output order; a cloud
    whose cell indices do not fit an int comes back as its finite points in input order (cells_overflow tells)."""
    p = _xyz(xyz)
    p = p[np.isfinite(p).all(axis=1)]
    if cells_overflow(p, leaf):
        return p.copy()
    f, _ = cells(p, leaf)
    idx = f.astype(np.int64)
    hist_cell = [None] * HISTSIZE
    hist_count = [0] * HISTSIZE
    hist_sum = [np.zeros(3, np.float32) for _ in range(HISTSIZE)]
    out = []

    def flush(h):
        out.append(hist_sum[h] / np.float32(hist_count[h]))          # centroid / (float)count, f32 per component
        hist_count[h] = 0
        hist_sum[h] = np.zeros(3, np.float32)

    for i in range(len(p)):
        ix, iy, iz = (int(v) for v in idx[i])
        h = (ix * MULTIPLIERS[0] + iy * MULTIPLIERS[1] + iz * MULTIPLIERS[2]) & (HISTSIZE - 1)   # (low 9 bits: wrap-around in int is harmless)
        if hist_count[h] and hist_cell[h] != (ix, iy, iz):
            flush(h)
        hist_cell[h] = (ix, iy, iz)
        hist_count[h] += 1
        hist_sum[h] = hist_sum[h] + p[i]                              # centroid += p: f32 sums from zero, in input order
    for h in range(HISTSIZE):
        if hist_count[h]:
            flush(h)
    return np.array(out, np.float32).reshape(-1, 3)


def angle_calibration(xyz, rad=ANGLE_RAD):
    """vertical_angle_calibration: every point, widened to f64, turned by `rad` about normalize(p x (0,0,1)), cast to f32.  Eigen 3.3 restated:
    cross(), normalize() (divides only when the squared norm is > 0), AngleAxisd::toRotationMatrix(), the 3x3 product; every operation is one
    NumPy ufunc call, so each is rounded on its own.  Rows with a non-finite coordinate are left as they are."""
    p32 = _xyz(xyz)
    out = p32.copy()
    fin = np.isfinite(p32).all(axis=1)
    x, y, z = (p32[fin, a].astype(np.float64) for a in range(3))
    a0, a1, a2 = y * 1.0 - z * 0.0, z * 0.0 - x * 1.0, x * 0.0 - y * 0.0
    s = (a0 * a0 + a1 * a1) + a2 * a2
    pos = s > 0
    r = np.sqrt(s, where=pos, out=np.ones_like(s))
    a0, a1, a2 = (np.where(pos, np.divide(a, r), a) for a in (a0, a1, a2))
    sn, cs = math.sin(rad), math.cos(rad)
    s0, s1, s2 = sn * a0, sn * a1, sn * a2
    k = 1.0 - cs
    c0, c1, c2 = k * a0, k * a1, k * a2
    t = c0 * a1
    r01, r10 = t - s2, t + s2
    t = c0 * a2
    r02, r20 = t + s1, t - s1
    t = c1 * a2
    r12, r21 = t - s0, t + s0
    r00, r11, r22 = c0 * a0 + cs, c1 * a1 + cs, c2 * a2 + cs
    out[fin, 0] = ((r00 * x + r01 * y) + r02 * z).astype(np.float32)
    out[fin, 1] = ((r10 * x + r11 * y) + r12 * z).astype(np.float32)
    out[fin, 2] = ((r20 * x + r21 * y) + r22 * z).astype(np.float32)
    return out


def move(xyz, T):
    """pcl::transformPointCloud(in, out, Eigen::Matrix4f): ((T(a,0) x + T(a,1) y) + T(a,2) z) + T(a,3) in f32; non-finite rows stay"""
    p = _xyz(xyz)
    T = np.asarray(T, np.float32)
    out = p.copy()
    fin = np.isfinite(p).all(axis=1)
    x, y, z = (p[fin, a] for a in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            out[fin, a] = ((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]
    return out


def gate(xyz, distance_near, distance_far, use_distance_filter=True):
    """distance_filter (:163-181, the f32 norm compared as double) and the finite test every down-sampling applies"""
    p = _xyz(xyz)
    keep = np.isfinite(p).all(axis=1)
    if use_distance_filter:
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(np.float64)
            keep &= (d > float(distance_near)) & (d < float(distance_far))
    return p[keep]


def prefilter(xyz, params=None, **kw):
    """The nodelet's chain for one cloud.  params / keywords: DEFAULTS' keys (Engine.batch_prefilter's keywords, `leaf` for
    downsample_resolution); angle_calibration: False, True (ANGLE_RAD) or radians.  Returns [M,3] f32."""
    q = dict(DEFAULTS, **(params or {}), **kw)
    unknown = sorted(set(q) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"unknown parameter(s) {unknown}")
    if q["downsample_method"] not in ("VOXELGRID", "APPROX_VOXELGRID"):
        raise ValueError("downsample_method must be VOXELGRID or APPROX_VOXELGRID")
    p = _xyz(xyz)
    if q["transform"] is not None:
        p = move(p, q["transform"])
    cal = q["angle_calibration"]
    if isinstance(cal, (bool, np.bool_)):
        if cal:
            p = angle_calibration(p, ANGLE_RAD)
    else:
        p = angle_calibration(p, float(cal))
    if q["downsample_method"] == "APPROX_VOXELGRID" and q["leaf"] > 0:
        return approx_voxel_grid(gate(p, q["distance_near"], q["distance_far"], q["use_distance_filter"]), q["leaf"])
    from oracle import oracle_py as O
    return O.prefilter(p, q["distance_near"], q["distance_far"], q["leaf"], q["use_distance_filter"])
