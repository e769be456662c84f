"""The [N,4] restatement of the prefiltering nodelet's whole chain (PrefilteringNodelet::cloud_callback, src/lidar_odometry/
prefiltering_nodelet.cpp) for pcl::PointXYZI: what mi355ndt_prefilter_p, mi355ndt_batch_prefilter, mi355ndt_prefilter_outliers and
mi355ndt_batch_remove_outliers are held to, word for word, when they carry an intensity (mi355ndt_prefilter_params_ex2).  NumPy, no GPU.

It is composed from the restatements the xyz surfaces are held to and adds only the fourth column:

  move          prefilter_options_ref.move on x, y, z; pcl::transformPointCloud copies the point and rewrites x, y, z: the intensity is
                untouched, also for a point left alone because a coordinate is non-finite
  calibration   prefilter_options_ref.angle_calibration on x, y, z; vertical_angle_calibration builds a fresh PointT and assigns x, y, z only
                (:207-210), and the PointXYZI constructor leaves intensity = 0: EVERY intensity becomes +0.0f.  A quirk of the reference.
  gate          prefilter_options_ref.gate's rule as a mask: a dropped point takes its intensity with it, a kept point's non-finite
                intensity is kept
  VOXELGRID     window_map_ref.voxel_grid on the [N,4] points: CentroidPoint<PointXYZI>, AccumulatorIntensity -- the f32 sum of the
                voxel's intensities in input order, divided by (float)count
  APPROX_VOXELGRID   prefilter_options_ref.approx_voxel_grid's walk with downsample_all_data_: the history entry's VectorXf holds x, y, z and
                intensity (centroid_size 4), starts from zero, adds in input order and is divided by (float)count at every flush
  NONE, or a leaf too small for the extent   the kept point's own intensity
  outliers      outlier_ref.remove_outliers on x, y, z; the survivors keep their intensity

PCL 1.8.1's rules as recalled; none of it has met a PCL build."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import outlier_ref as OR                 # noqa: E402
import prefilter_options_ref as PR       # noqa: E402
import window_map_ref as WR              # noqa: E402

DEFAULTS = dict(PR.DEFAULTS, outlier=None)


def _xyzi(cloud):
    a = np.asarray(cloud, np.float32)
    if a.ndim != 2 or a.shape[1] < 4:
        raise ValueError("[N,>=4] records: x, y, z, intensity")
    return np.ascontiguousarray(a[:, :4])


def gate_mask(xyz, distance_near, distance_far, use_distance_filter=True):
    """prefilter_options_ref.gate's rule as a mask over the rows"""
    p = PR._xyz(xyz)
    keep = np.isfinite(p).all(axis=1)
    if use_distance_filter:
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(np.float64)
            keep &= (d > float(distance_near)) & (d < float(distance_far))
    return keep


def approx_voxel_grid(P, leaf):
    """pcl::ApproximateVoxelGrid over [N,4] points with downsample_all_data_: prefilter_options_ref.approx_voxel_grid's loop, the entry's
    sum four floats wide.  Non-finite x, y or z: dropped.  [M,4] f32 in PCL's output order."""
    P = _xyzi(P)
    P = P[np.isfinite(P[:, :3]).all(axis=1)]
    if PR.cells_overflow(P[:, :3], leaf):
        return P.copy()
    f, _ = PR.cells(P[:, :3], leaf)
    idx = f.astype(np.int64)
    cell = [None] * PR.HISTSIZE
    count = [0] * PR.HISTSIZE
    total = [np.zeros(4, np.float32) for _ in range(PR.HISTSIZE)]
    out = []

    def flush(h):
        with np.errstate(invalid="ignore", over="ignore"):
            out.append(total[h] / np.float32(count[h]))
        count[h] = 0
        total[h] = np.zeros(4, np.float32)

    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(P)):
            ix, iy, iz = (int(v) for v in idx[i])
            h = (ix * PR.MULTIPLIERS[0] + iy * PR.MULTIPLIERS[1] + iz * PR.MULTIPLIERS[2]) & (PR.HISTSIZE - 1)
            if count[h] and cell[h] != (ix, iy, iz):
                flush(h)
            cell[h] = (ix, iy, iz)
            count[h] += 1
            total[h] = total[h] + P[i]
    for h in range(PR.HISTSIZE):
        if count[h]:
            flush(h)
    return np.array(out, np.float32).reshape(-1, 4)


def remove_outliers(P, **kw):
    """outlier_ref.remove_outliers over x, y, z of [N,4] points: the surviving rows, whole, and its dict"""
    P = _xyzi(P)
    _, r = OR.remove_outliers(P[:, :3], **kw)
    return P[r["kept"]], r


def prefilter(cloud, params=None, **kw):
    """The nodelet's chain for one [N,>=4] cloud.  params / keywords: prefilter_options_ref.DEFAULTS' keys and `outlier` (None, or a dict
    of outlier_ref.remove_outliers' keywords: the third stage).  Returns [M,4] f32."""
    q = dict(DEFAULTS, **(params or {}), **kw)
    unknown = sorted(set(q) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"unknown parameter(s) {unknown}")
    if q["downsample_method"] not in ("VOXELGRID", "APPROX_VOXELGRID"):
        raise ValueError("downsample_method must be VOXELGRID or APPROX_VOXELGRID")
    P = _xyzi(cloud).copy()
    if q["transform"] is not None:
        P[:, :3] = PR.move(P[:, :3], q["transform"])
    cal = q["angle_calibration"]
    if not isinstance(cal, (bool, np.bool_)) or cal:
        P[:, :3] = PR.angle_calibration(P[:, :3], PR.ANGLE_RAD if isinstance(cal, (bool, np.bool_)) else float(cal))
        P[:, 3] = np.float32(0.0)                    # the fresh PointXYZI's intensity
    P = P[gate_mask(P[:, :3], q["distance_near"], q["distance_far"], q["use_distance_filter"])]
    if q["downsample_method"] == "APPROX_VOXELGRID" and q["leaf"] > 0:
        P = approx_voxel_grid(P, q["leaf"])
    else:
        P = WR.voxel_grid(P, q["leaf"])
    if q["outlier"] is not None:
        P, _ = remove_outliers(P, **q["outlier"])
    return P
