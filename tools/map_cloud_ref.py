"""CPU restatement of MapCloudGenerator::generate (src/global_graph/map_cloud_generator.cpp:17-55): every keyframe's points moved by
its pose, fed in order into a pcl::octree::OctreePointCloud(resolution), the occupied voxel centres returned depth first.  The checker
of mi355ndt_map_cloud (tests/test_map_cloud_*.py, tools/map_cloud_timing.py); not part of the product package.

Restated from PCL 1.8 octree_pointcloud.hpp and Eigen 3.3's fixed-size product; neither library is present, so the parity is pinned to
this restatement and not to a reference binary (README "parity unpinned").

1. Transform: M = pose.cast<float>(), each coordinate ((M[a][0]*x + M[a][1]*y) + M[a][2]*z) + M[a][3], every f32 operation rounded
   on its own (Eigen's lazy 4x4 * 4x1 product under SSE without FMA; w = 1).
2. Points whose transformed x, y or z is not finite are skipped (addPointsFromInputCloud's isFinite).
3. The first finite point p defines the box (adoptBoundingBoxToPoint, then getKeyBitSize while leaf_count_ == 0), all in f64 with
   eps = (double)FLT_EPSILON: min = p - r/2, max = p + r/2; max_key = (unsigned)((max - min) / r); depth = ceil(log(max(max_key, 2))
   / log(2) - eps); side = 2^depth * r - eps; over = (side - (max - min)) / 2; min -= over, max += over.
4. Every finite point q (the first one too) then grows the box while, on any axis, q < min or q >= max: on each axis where q is not at
   or above max, min -= 2^depth * r (the old root becomes child (!upX << 2) | (!upY << 1) | !upZ of the new one); depth += 1;
   max = min + (2^depth * r - eps).  The box depends on the order of the points.
5. Key of q: (unsigned)((q - min) / r) per axis, an f64 division.
6. Output: every occupied leaf once, depth first with children 0..7, i.e. ascending Morton order of the key with x the most significant
   of each level's three bits; centre = (float)(((double)key + 0.5) * r + min) with the final min.

Step 5 is evaluated in the box AS IT STANDS WHEN q IS ADDED (after q's own growth), not in the final box, because that is what PCL
does.  addPointIdx computes genOctreeKeyforPoint right after adoptBoundingBoxToPoint and
walks createLeafRecursive with the depth mask of that moment; a later growth never re-keys a leaf, it only hangs the old root below a new
one.  q's leaf in the final tree therefore has key  (key_t & (2^depth_t - 1)) + shift_t,  where shift_t (per axis) is the sum of 2^d over
the later growth levels d that extended that axis downwards.  In exact arithmetic this equals the key in the final box; in f64 the two
can differ by one voxel when q lies within rounding of a voxel face (min_final = min_t - sum of 2^d r is rounded).  The mask is what
createLeafRecursive does with a key bit above the depth (release builds: the assert is compiled out).

Limit of the engine (not of PCL): a final depth above 21 (Morton code wider than 63 bits) raises MapCloudDepthError.
"""
import numpy as np

EPS = float(np.finfo(np.float32).eps)
MAX_DEPTH = 21


class MapCloudDepthError(ValueError):
    """The octree would need more than MAX_DEPTH levels (2^21 voxels per axis) for these points at this resolution."""


def transform(cloud, pose):
    """[N,3] f32 points moved by a 4x4 f64 pose, step 1 (explicit f32 operations, no fused multiply-add)."""
    P = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    out = np.empty_like(P)
    with np.errstate(over="ignore", invalid="ignore"):             # non-finite inputs / a pose beyond f32 range: IEEE results, as in Eigen
        M = np.asarray(pose, np.float64).astype(np.float32)
        for a in range(3):
            out[:, a] = ((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]
    return out


class Box:
    """The octree's bounding box and depth as OctreePointCloud keeps them (f64), with the growth history needed for the keys."""

    def __init__(self, r):
        self.r = float(r)
        self.defined = False
        self.min = [0.0, 0.0, 0.0]
        self.max = [0.0, 0.0, 0.0]
        self.depth = 0
        self.down = [0, 0, 0]          # sum of 2^d over the growth levels that extended each axis downwards so far
        self.last_child = None         # child index the old root took in the last growth

    def define(self, p):
        r = self.r
        self.min = [float(p[a]) - r / 2 for a in range(3)]
        self.max = [float(p[a]) + r / 2 for a in range(3)]
        max_key = [int((self.max[a] - self.min[a]) / r) for a in range(3)]
        max_vox = max(max(max_key), 2)
        self.depth = min(32, int(np.ceil(np.log(float(max_vox)) / np.log(2.0) - EPS)))
        side = float(1 << self.depth) * r - EPS
        for a in range(3):
            over = (side - (self.max[a] - self.min[a])) / 2.0
            self.min[a] -= over
            self.max[a] += over
        self.defined = True

    def violates(self, q):
        return any(float(q[a]) < self.min[a] or float(q[a]) >= self.max[a] for a in range(3))

    def adopt(self, q):
        """adoptBoundingBoxToPoint(q); raises MapCloudDepthError past MAX_DEPTH."""
        if not self.defined:
            self.define(q)
        while self.violates(q):
            up = [float(q[a]) >= self.max[a] for a in range(3)]
            side = float(1 << self.depth) * self.r
            for a in range(3):
                if not up[a]:
                    self.min[a] -= side
                    self.down[a] += 1 << self.depth
            self.last_child = (int(not up[0]) << 2) | (int(not up[1]) << 1) | int(not up[2])
            self.depth += 1
            if self.depth > MAX_DEPTH:
                raise MapCloudDepthError(f"map cloud: the points need an octree deeper than {MAX_DEPTH} levels at resolution {self.r}")
            side = float(1 << self.depth) * self.r - EPS
            for a in range(3):
                self.max[a] = self.min[a] + side


def _first_violator(Q, lo, hi, start):
    """Index >= start of the first row of Q (f64) outside [lo, hi), or -1; windows that double in size keep one pass over Q."""
    n, w = Q.shape[0], 1 << 14
    i = start
    while i < n:
        blk = Q[i:i + w]
        v = np.any((blk < lo) | (blk >= hi), axis=1)
        if v.any():
            return i + int(np.argmax(v))
        i += w
        w *= 2
    return -1


def morton(kx, ky, kz, depth):
    """Codes whose bit 3l+2 / 3l+1 / 3l is bit l of kx / ky / kz (uint64)."""
    kx, ky, kz = (np.asarray(k, np.uint64) for k in (kx, ky, kz))
    code = np.zeros(kx.shape, np.uint64)
    for lvl in range(depth):
        s = np.uint64(lvl)
        code |= ((kx >> s) & np.uint64(1)) << np.uint64(3 * lvl + 2)
        code |= ((ky >> s) & np.uint64(1)) << np.uint64(3 * lvl + 1)
        code |= ((kz >> s) & np.uint64(1)) << np.uint64(3 * lvl)
    return code


def unmorton(code, depth):
    code = np.asarray(code, np.uint64)
    k = [np.zeros(code.shape, np.uint64) for _ in range(3)]
    for lvl in range(depth):
        for a in range(3):
            k[a] |= ((code >> np.uint64(3 * lvl + 2 - a)) & np.uint64(1)) << np.uint64(lvl)
    return k


def octree_points(P, r, return_box=False):
    """Steps 2-6 on [N,3] f32 points in their insertion order: [M,3] f32 voxel centres (and the final Box with return_box)."""
    if not (r > 0) or not np.isfinite(r):
        raise ValueError("resolution must be finite and > 0")
    P = np.ascontiguousarray(np.asarray(P, np.float32).reshape(-1, 3))
    fin = np.isfinite(P).all(axis=1)
    idx = np.nonzero(fin)[0]
    box = Box(r)
    if idx.size == 0:
        out = np.zeros((0, 3), np.float32)
        return (out, box) if return_box else out
    Q = P[idx].astype(np.float64)
    # epochs: the box after each point that changed it; points from one epoch start to the next are keyed in that epoch's box
    epochs = []
    i = 0
    while i >= 0:
        box.adopt(Q[i])
        epochs.append((i, list(box.min), box.depth, list(box.down)))
        i = _first_violator(Q, np.array(box.min), np.array(box.max), i + 1)
    keys = np.zeros((Q.shape[0], 3), np.uint64)
    for e, (s, mn, d, down) in enumerate(epochs):
        t = epochs[e + 1][0] if e + 1 < len(epochs) else Q.shape[0]
        for a in range(3):
            k = ((Q[s:t, a] - mn[a]) / r).astype(np.uint64)               # (unsigned)((q - min) / r), q >= min
            k &= np.uint64((1 << d) - 1)                                    # createLeafRecursive reads `depth` key bits
            keys[s:t, a] = k + np.uint64(box.down[a] - down[a])            # the growth levels after this epoch
    codes = np.unique(morton(keys[:, 0], keys[:, 1], keys[:, 2], box.depth))
    kk = unmorton(codes, box.depth)
    out = np.empty((codes.size, 3), np.float32)
    for a in range(3):
        out[:, a] = ((kk[a].astype(np.float64) + 0.5) * r + box.min[a]).astype(np.float32)
    return (out, box) if return_box else out


def map_cloud(clouds, poses, resolution, return_box=False):
    """MapCloudGenerator::generate(keyframes, resolution): None for no keyframes, else the [M,3] f32 centres."""
    if len(clouds) != len(poses):
        raise ValueError("one pose per cloud")
    if len(clouds) == 0:
        return None
    P = np.concatenate([transform(c, T) for c, T in zip(clouds, poses)]) if clouds else np.zeros((0, 3), np.float32)
    return octree_points(P, resolution, return_box)
