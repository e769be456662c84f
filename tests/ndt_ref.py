"""A plain float64 statement of one derivative sweep (updateDerivatives, ndt_omp_impl2.hpp:566-619; ndt_pca_impl2.hpp:294-296), with an entrywise
majorant, and the tiny scenes the entrywise sweep tests run on (tests/test_sweep_entries_cpu.py, tests/test_sweep_entries_gpu.py).

The oracle (oracle/ndt_oracle.c) restates the reference's f32 recipe step by step and the kernels are held to the oracle; this module is the
mathematics alone.  Only what decides WHICH leaves a point meets is taken in f32, in the reference's rounding order: the moved point x', r = Rj p
and the cell floor(x' / leaf).  From there on x', r, the leaf's f64 mean and its f32 inverse covariance (symmetrised) are inputs and every formula
is evaluated in f64:

    J = [I | -[r]x]    y = C u    q = u . y    e0 = exp(-d2 q / 2)    s = -d1 e0    e = d1 d2 e0    v = J^T y
    score += s         g += e v   H += e (-d2 v v^T + J^T C J + Z),     Z = [0 0; 0 r y^T - (y . r) I]

The majorant is the same evaluation on absolute values, times k = 1 + |d2 q / 2| (the condition number of the exponential's argument): one
rounding of relative size eps anywhere in an evaluation moves entry a by at most about eps * majorant[a], so errors are stated per entry, in units
of 2^-24 * majorant -- not as a fraction of the largest of the 43 numbers, which leaves the translation block of H unchecked once |r| is large."""
import functools

import numpy as np

from oracle import oracle_py as O

EPS32 = 2.0 ** -24
EPS64 = 2.0 ** -53
OFFSETS7 = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)   # the oracle's order (impl:423-430)
# DIRECT26 (impl:413-414: pcl::getAllNeighborCellIndices): the 13 offsets of the lower half -- the nine of z = -1, the three of (y, z) = (-1, 0),
# then (-1, 0, 0), x running slowest -- followed by their negations.  The centre cell is NOT among them: a point meets at most 26 leaves.
_HALF13 = [(i, j, -1) for i in (-1, 0, 1) for j in (-1, 0, 1)] + [(i, -1, 0) for i in (-1, 0, 1)] + [(-1, 0, 0)]
OFFSETS26 = np.array(_HALF13 + [(-i, -j, -k) for i, j, k in _HALF13], np.int64)
CELL_OFFSETS = {1: OFFSETS7[:1], 7: OFFSETS7, 26: OFFSETS26}
# K, the cells a search probes, names the search: 1 = DIRECT1, 7 = DIRECT7, 26 = DIRECT26, 27 = KDTREE (the radius search: the 3 x 3 x 3 block)
MODE_OF_K = {1: O.DIRECT1, 7: O.DIRECT7, 26: O.DIRECT26, 27: O.KDTREE}


def _skew_neg(r):
    """-[r]x for rows r: [n, 3, 3]"""
    z = np.zeros(len(r))
    return np.stack([np.stack([z, r[:, 2], -r[:, 1]], -1), np.stack([-r[:, 2], z, r[:, 0]], -1), np.stack([r[:, 1], -r[:, 0], z], -1)], 1)


def _row(s, g, H):
    return np.concatenate([s[:, None], g, H.reshape(len(s), 36)], 1)


def _radius_slots(leaves, params, xt, ok, tie_last_first):
    """KDTREE (VoxelGridCovariance::radiusSearch, voxel_grid_covariance_omp.h:505-534; impl2:251-253): every leaf that had min_points points when
    the grid was filtered -- eigen- or inverse-failed ones included, there is no nr_points re-check -- whose f32 centroid lies within `resolution`
    of x'.  Squared distance in f32 as (dx dx + dy dy) + dz dz, against float(resolution * resolution), strictly less.  Hits come in ascending
    squared distance, ties by leaf index (tie_last_first: the opposite tie rule, for the scene that shows the rule matters).
    One slot per rank: (leaf position, hit mask)."""
    cen = np.ascontiguousarray(leaves["centroid"], np.float32)
    cand = np.asarray(leaves["n_pushed"]) >= params.min_points_per_voxel
    res = float(params.resolution)
    r2 = np.float32(res * res)
    d = xt[:, None, :] - cen[None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    assert d2.dtype == np.float32
    within = ok[:, None] & cand[None, :] & (d2 < r2)
    key = np.where(within, d2, np.float32(np.inf))
    if tie_last_first:
        order = key.shape[1] - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable")
    else:
        order = np.argsort(key, axis=1, kind="stable")
    count = within.sum(1)
    return [(order[:, k], k < count) for k in range(int(count.max(initial=0)))]


def _lookup(leaves, bounds, params, src_f32, T_f32, Rj_f32, K, tie_last_first=False):
    """The f32 part: x', r (as f64 values, 0 for rows that are not finite) and, per probed cell in the oracle's order (KDTREE: per rank of the
    radius search's result), (leaf position, hit mask)."""
    assert K in MODE_OF_K
    src = np.ascontiguousarray(src_f32, np.float32)
    T = np.asarray(T_f32, np.float32)
    Rj = np.asarray(Rj_f32, np.float32)
    px, py, pz = src[:, 0], src[:, 1], src[:, 2]
    with np.errstate(invalid="ignore"):
        # f32, one rounding per operation, left to right (PCL's scalar transformPointCloud; impl2:507-508)
        xt = np.stack([((T[a, 0] * px + T[a, 1] * py) + T[a, 2] * pz) + T[a, 3] for a in range(3)], 1)
        r32 = np.stack([(Rj[a, 0] * px + Rj[a, 1] * py) + Rj[a, 2] * pz for a in range(3)], 1)
    assert xt.dtype == np.float32 and r32.dtype == np.float32
    ok = np.isfinite(src).all(1) & np.isfinite(xt).all(1)
    xt = np.where(ok[:, None], xt, np.float32(0))
    cell = np.floor(xt / np.float32(params.resolution)).astype(np.int64)                     # f32 divide, then floor
    min_b, max_b, div_b = (np.asarray(b, np.int64) for b in bounds)
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    l_idx = np.asarray(leaves["idx"], np.int64)
    assert np.all(np.diff(l_idx) > 0)
    slots = _radius_slots(leaves, params, xt, ok, tie_last_first) if K == 27 else []
    for k in range(0 if K == 27 else K):
        c = cell + CELL_OFFSETS[K][k]
        inb = ok & np.all((c >= min_b) & (c <= max_b), 1)
        idx = np.where(inb, (c - min_b) @ mul, -1)
        pos = np.clip(np.searchsorted(l_idx, idx), 0, len(l_idx) - 1)
        slots.append((pos, inb & (l_idx[pos] == idx) & (leaves["n"][pos] >= params.min_points_per_voxel)))
    return xt.astype(np.float64), np.where(ok[:, None], r32, np.float32(0)).astype(np.float64), slots


def hit_leaves(leaves, bounds, params, src_f32, T_f32, Rj_f32, K):
    """positions (into `leaves`) of every leaf met, one per hit"""
    return np.concatenate([pos[hit] for pos, hit in _lookup(leaves, bounds, params, src_f32, T_f32, Rj_f32, K)[2]])


def ref_sweep(leaves, bounds, params, src_f32, T_f32, Rj_f32, K, tie_last_first=False, hessian_R64=None):
    """leaves: the records of Grid.leaves() (idx ascending, n, mean f64, icov, weight, centroid f32, n_pushed); bounds: (min_b, max_b, div_b);
    K: 1, 7 or 26 cells probed, 27 = the radius search.  Returns (sums[43] = score, g[6], H[36] row-major; majorant[43]; hits; hits_per_point[n]).
    ndt_pca's weight is the leaf's `weight` field under every search: 0 for an eigen-failed leaf, the dimension weight where only the inverse
    failed afterwards -- what the radius search's path reads (kd_weight, k_voxels); the direct searches never meet such a leaf.
    hessian_R64 (3x3 f64, the rotation of exp(p)): the recipe of computeHessian / updateHessian instead (impl2:622-714), whose H block is the
    same mathematics on other inputs -- r = R x in f64 from the f64 rotation (impl2:535-563), the leaf's f64 inverse covariance, d2 unrounded,
    no ndt_pca weights; x' is still the f32-moved point, and the caller passes K = 27: the neighbourhoods come from the radius search whatever the
    search method is.  Score and g of that call are by-products no reference function computes."""
    x, r, slots = _lookup(leaves, bounds, params, src_f32, T_f32, Rj_f32, K, tie_last_first)
    n = len(x)
    d1, d2 = (float(v) for v in O.gauss_constants(params.outlier_ratio, params.resolution)[:2])
    pca = params.variant == O.VARIANT_PCA
    if hessian_R64 is None:
        d2 = float(np.float32(d2))                                                           # impl2:578
    else:
        pca = False
        r = np.where((r != 0).any(1)[:, None] | np.isfinite(np.asarray(src_f32, np.float64)).all(1)[:, None],
                     np.nan_to_num(np.asarray(src_f32, np.float32).astype(np.float64)) @ np.asarray(hessian_R64, np.float64).T, 0.0)

    J = np.concatenate([np.broadcast_to(np.eye(3), (n, 3, 3)), _skew_neg(r)], 2)            # [n, 3, 6]
    aJ = np.abs(J)
    ar = np.abs(r)
    sums = np.zeros((n, 43))
    maj = np.zeros((n, 43))
    hits_pp = np.zeros(n, np.int64)
    eye3 = np.eye(3)
    for pos, hit in slots:
        L = leaves[pos]
        hits_pp += hit
        u = x - L["mean"]
        C = (L["icov"].astype(np.float32).astype(np.float64) if hessian_R64 is None else L["icov"]).reshape(n, 3, 3)
        if hessian_R64 is None:
            C = 0.5 * (C + C.transpose(0, 2, 1))
        # (written for a C that need not be symmetric, as updateHessian reads its f64 inverse covariance: y = u^T C, H[a][b] has J_b^T C J_a;
        #  far from the origin that inverse is asymmetric by ~1e-9 of its entries, 1e-4 units of 2^-24 and thousands of units of 2^-53)
        aC = np.abs(C)
        y = np.einsum("nba,nb->na", C, u)
        q = np.einsum("na,na->n", u, y)
        e0 = np.exp(-d2 * q / 2)
        s = -d1 * e0
        e1 = d2 * e0
        live = hit & ~((e1 > 1) | (e1 < 0) | np.isnan(e1))                                  # impl2:588-589: a gated hit is still a hit
        e = d1 * d2 * e0
        v = np.einsum("nak,na->nk", J, y)
        Z = np.zeros((n, 6, 6))
        Z[:, 3:, 3:] = r[:, :, None] * y[:, None, :] - np.einsum("na,na->n", y, r)[:, None, None] * eye3
        H = e[:, None, None] * (-d2 * v[:, :, None] * v[:, None, :] + np.einsum("nak,nab,nbl->nlk", J, C, J) + Z)
        term = _row(s, e[:, None] * v, H)
        # the same on absolute values
        yh = np.einsum("nba,nb->na", aC, np.abs(u))
        vh = np.einsum("nak,na->nk", aJ, yh)
        kk = 1 + np.abs(d2 * q / 2)
        Zh = np.zeros((n, 6, 6))
        Zh[:, 3:, 3:] = ar[:, :, None] * yh[:, None, :] + np.einsum("na,na->n", yh, ar)[:, None, None] * eye3
        ke = kk * np.abs(e)
        Hh = ke[:, None, None] * (abs(d2) * vh[:, :, None] * vh[:, None, :] + np.einsum("nak,nab,nbl->nkl", aJ, aC, aJ) + Zh)
        termh = _row(kk * np.abs(s), ke[:, None] * vh, Hh)
        term = np.where(live[:, None], term, 0.0)
        termh = np.where(live[:, None], termh, 0.0)
        if pca:
            # ndt_pca_impl2.hpp:295-296, literally: after every hit the point's running sums are multiplied by that leaf's weight
            w = np.where(hit, L["weight"], 1).astype(np.float64)[:, None]
            sums = (sums + term) * w
            maj = (maj + termh) * np.abs(w)
        else:
            sums = sums + term
            maj = maj + termh
    return sums.sum(0), maj.sum(0), int(hits_pp.sum()), hits_pp


def ref_calculate_score(leaves, params, cloud_f32, gauss=None):
    """calculateScore (impl2:1006-1040) of an ALREADY MOVED f32 cloud, in f64: the radius search's hits; per hit -d1 exp(-d2 u^T C u / 2) - d3 with
    the leaf's f64 inverse covariance, divided by the number of hits of its point; the sum divided by the number of rows of the cloud, finite or
    not.  This is not ref_sweep's score term (the d3 offset, the division per neighbourhood, f64 covariances, d2 unrounded).
    Returns (score, majorant, hits): the majorant is the sum of |term| (1 + |d2 q / 2|) / hits of the point / rows."""
    cloud = np.ascontiguousarray(cloud_f32, np.float32)
    ok = np.isfinite(cloud).all(1)
    xt = np.where(ok[:, None], cloud, np.float32(0))
    d1, d2, d3 = (float(v) for v in (O.gauss_constants(params.outlier_ratio, params.resolution) if gauss is None else gauss))
    slots = _radius_slots(leaves, params, xt, ok, False)
    count = sum(hit.astype(np.int64) for _, hit in slots) if slots else np.zeros(len(cloud), np.int64)
    score = maj = 0.0
    for pos, hit in slots:
        L = leaves[pos]
        u = xt.astype(np.float64) - L["mean"]
        C = L["icov"].reshape(len(cloud), 3, 3)
        q = np.einsum("na,nab,nb->n", u, 0.5 * (C + C.transpose(0, 2, 1)), u)
        aq = np.einsum("na,nab,nb->n", np.abs(u), np.abs(C), np.abs(u))
        e = np.exp(-d2 * q / 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            score += np.where(hit, (-d1 * e - d3) / count, 0.0).sum()
            maj += np.where(hit, ((1 + np.abs(d2 * aq / 2)) * np.abs(d1 * e) + abs(d3)) / count, 0.0).sum()
    return score / len(cloud), maj / len(cloud), int(count.sum())


def units(got, want, majorant):
    """|got - want| entry by entry, in units of 2^-24 * majorant (0 where both the difference and the majorant vanish)"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d == 0, 0.0, d / (EPS32 * majorant))


def as_row(res):
    """(score, g, H, hits) of a derivative hook -> (row[43], hits)"""
    s, g, H, hits = res
    return np.concatenate([[s], np.asarray(g, np.float64).ravel(), np.asarray(H, np.float64).ravel()]), int(hits)


# ------------------------------------------------------------------------------------------------------------------------- scenes
N_SRC = (1, 63, 64, 65, 511, 512, 513, 2049)           # across the 64-point tile, the 512-point work item and the 2048-point chunk
N_POOL = max(N_SRC)
SEED = 20240917
OFFSETS = {"origin": (0.0, 0.0, 0.0), "around0": (-2.0, -2.0, -2.0), "mid": (37.5, 12.25, -3.0), "far": (500.0, -300.0, 40.0)}
SCENES = {name: (off, 1.0) for name, off in OFFSETS.items()}
SCENES["mid_r0.7"] = (OFFSETS["mid"], 0.7)              # leaf size not a power of two: the lookup's divide path
BIG_SCENE = "mid"                                       # the one scene that also runs n_src = 2049
POSES = ("near", "turned")


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


class Scene:
    """target: 4 x 4 x 4 grid cells, 12 points in the inner [0.1, 0.9] of each; the block starts at the cell that holds `offset`.
    pool: source points uniform in offset + leaf * [0.3, 3.7]^3 -- points of the block's outer cells meet fewer than 7 leaves, and where `offset`
    is no multiple of the leaf size the pool overhangs the block, so some points meet 1 to 3."""

    def __init__(self, seed, offset, leaf):
        rng = np.random.default_rng(seed)
        self.leaf = float(leaf)
        self.offset = np.asarray(offset, np.float64)
        cell0 = np.floor(self.offset / leaf)
        ijk = np.stack(np.meshgrid(range(4), range(4), range(4), indexing="ij"), -1).reshape(-1, 3)
        self.target = ((cell0 + np.repeat(ijk, 12, 0) + rng.uniform(0.1, 0.9, (64 * 12, 3))) * leaf).astype(np.float32)
        self.pool = self.offset + leaf * rng.uniform(0.3, 3.7, (N_POOL, 3))
        # three points that meet no leaf: far outside the grid's bounds, and diagonally off two corners of the block (every probed cell out of bounds)
        self.outside = (cell0 + np.array([[14.5, 1.5, 2.5], [-0.5, -0.5, 1.5], [4.5, 4.5, 2.5]])) * leaf
        self.centre = (cell0 + 2.0) * leaf
        self.target.setflags(write=False)

    def source64(self, n):
        """the first n pool points; from 8 points on, three of them are replaced by the outside points and one row is NaN"""
        s = self.pool[:n].copy()
        if n >= 8:
            s[[1, n // 3, n - 2]] = self.outside
            s[n // 2] = np.nan
        return s

    def pose(self, name, n):
        """(source f32 [n, 3], T f32 4x4, Rj f32 3x3).  near: a 0.02 rad yaw about the block's centre plus (0.05, -0.03, 0.02).
        turned: the same geometry presented turned by 2.5 rad about (1, 2, 3) -- source Q^-1 s, pose T Q (tests/test_large_rotation_gpu.py)."""
        A, B, M = np.eye(4), np.eye(4), np.eye(4)
        A[:3, 3] = self.centre + np.array([0.05, -0.03, 0.02])
        B[:3, 3] = -self.centre
        M[:3, :3] = rotation((0, 0, 1), 0.02)
        T = A @ M @ B
        s = self.source64(n)
        if name == "turned":
            R = rotation((1, 2, 3), 2.5)
            Q = np.eye(4)
            Q[:3, :3] = R
            s = s @ R                                      # rows: (R^T x)^T
            T = T @ Q
        else:
            assert name == "near"
        T = T.astype(np.float32)
        return s.astype(np.float32), T, T[:3, :3].copy()


@functools.lru_cache(maxsize=None)
def _scene(seed, offset, leaf):
    return Scene(seed, offset, leaf)


def scene(seed, offset, leaf=1.0):
    """the committed inputs of one scene, built once"""
    return _scene(int(seed), tuple(float(v) for v in offset), float(leaf))


class TieScene:
    """The order rule of ndt_pca + KDTREE: two target leaves whose f32 centroids are mirror images about a source point, exactly, with
    different integer ndt_pca weights -- the radius search returns them at EQUAL f32 squared distance and the lower leaf index goes first;
    (sums + term) * w does not commute, so the other tie rule gives other sums (tests/test_sweep_entries_cpu.py shows by how much).
    Every coordinate is a multiple of 1/32 and a leaf has 16 points, +-d in pairs about its centre: the f32 coordinate sums, the division by 16
    and the f64 mean are all exact.  Leaves A and B have centres c -+ (0.5, 0, 0), |c -+ .| = 9.78 and 10.77; two more leaves give the other
    source points something to meet.  The pose is the identity (pose name "exact": x' = x with no rounding)."""
    leaf = 1.0
    TIE_ROW, EDGE_ROW = 0, 3
    TIE_POINT = (10.25, 0.5, 0.5)
    EDGE_POINT = (10.75, 1.5, 0.5)

    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        centres = np.array([[9.75, 0.5, 0.5], [10.75, 0.5, 0.5], [10.5, 1.5, 0.5], [9.5, 0.5, 1.5]])
        tgt = []
        for c in centres:
            d = rng.integers(-7, 8, (8, 3)) / 32.0
            tgt.append(np.concatenate([c + d, c - d]))
        self.target = np.concatenate(tgt).astype(np.float32)
        assert np.array_equal(self.target.astype(np.float64) * 32, np.round(self.target.astype(np.float64) * 32))
        # the tie point, two ordinary points (one meets A, B and a third leaf at unequal distances), the edge point -- exactly 1 m from B's
        # centroid, f32 squared distance == float(resolution^2): the radius test is strict, so B is NOT met --, a point outside the grid, a NaN row
        self.source = np.array([self.TIE_POINT, [10.3125, 0.9375, 0.40625], [9.6875, 0.59375, 1.21875], self.EDGE_POINT, [24.5, 0.5, 0.5], [np.nan] * 3],
                               np.float32)
        self.target.setflags(write=False)
        self.source.setflags(write=False)

    def pose(self, name, n):
        assert name == "exact"
        T = np.eye(4, dtype=np.float32)
        return self.source[:n].copy(), T, T[:3, :3].copy()


TIE = "tie"
TIE_CASE = (TIE, "exact", 6)


@functools.lru_cache(maxsize=None)
def named_scene(name):
    if name == TIE:
        return TieScene(SEED)
    off, leaf = SCENES[name]
    return scene(SEED, off, leaf)


def cases(tie=False):
    """(scene name, pose name, n_src) of every committed sweep; tie: with the order-rule scene (the searches past DIRECT1 / DIRECT7 run it)"""
    return [(sn, pn, n) for sn in SCENES for pn in POSES for n in N_SRC if n != N_POOL or sn == BIG_SCENE] + ([TIE_CASE] if tie else [])


@functools.lru_cache(maxsize=None)
def oracle_grid(scene_name, variant, K):
    """(Grid, leaves, bounds, params) of a scene's target under the oracle"""
    sc = named_scene(scene_name)
    prm = O.default_params(resolution=sc.leaf, variant=variant, neighbor_mode=MODE_OF_K[K])
    grid = O.Grid(sc.target, prm)
    assert grid.ok
    return grid, grid.leaves(), grid.bounds(), prm


def sweep_inputs(scene_name, pose_name, n):
    return named_scene(scene_name).pose(pose_name, n)


@functools.lru_cache(maxsize=None)
def _ref_rows(scene_name, pose_name, n, variant, K):
    _, leaves, bounds, prm = oracle_grid(scene_name, variant, K)
    row, maj, hits, hpp = ref_sweep(leaves, bounds, prm, *sweep_inputs(scene_name, pose_name, n), K)
    for a in (row, maj, hpp):
        a.setflags(write=False)
    return row, maj, hits, hpp


@functools.lru_cache(maxsize=None)
def _oracle_rows(scene_name, pose_name, n, variant, K, order):
    grid = oracle_grid(scene_name, variant, K)[0]
    O.lib().ora_set_variant(order, 256)                    # the oracle's matching f32 sum order (ORA_VAR_SUM3_02_1)
    try:
        orow, ohits = as_row(O.derivatives(grid, *sweep_inputs(scene_name, pose_name, n)))
    finally:
        O.lib().ora_set_variant(0, 256)
    orow.setflags(write=False)
    return orow, ohits


def reference(scene_name, pose_name, n, variant, K, order=0):
    """ref_sweep and the oracle's sweep of one case (order: the oracle's three-term f32 sum order, as MI355NDT_OPT_F32_SUM_ORDER), computed
    once and shared, read-only: (ref row, majorant, ref hits, hits per point, oracle row, oracle hits)"""
    return _ref_rows(scene_name, pose_name, n, variant, K) + _oracle_rows(scene_name, pose_name, n, variant, K, order)


# ------------------------------------------------------------------------------------- computeHessian and calculateScore on the scenes
HESSIAN_SIZES = (1, 65, 513)


@functools.lru_cache(maxsize=None)
def tangent_case(scene_name, pose_name, n):
    """A case for the hooks that take a tangent: p = log of the case's f32 pose (tests/se3_ref.py, f64), and what follows from p alone --
    (source f32, p, T32 = f32(exp(p)), R64 = the f64 rotation of exp(p), the cloud moved by T32 in f32 as transformPointCloud moves it)"""
    import se3_ref as S
    src, T, _ = sweep_inputs(scene_name, pose_name, n)
    p = S.eval_log(S.F64, T[:3, :3].astype(np.float64).ravel(), T[:3, 3].astype(np.float64))["p"]
    M = S.eval_exp(S.F64, p)["M"]
    R64 = M[:9].reshape(3, 3).copy()
    T32 = np.eye(4, dtype=np.float32)
    T32[:3, :3], T32[:3, 3] = R64, M[9:]
    with np.errstate(invalid="ignore"):
        cloud = np.stack([((T32[a, 0] * src[:, 0] + T32[a, 1] * src[:, 1]) + T32[a, 2] * src[:, 2]) + T32[a, 3] for a in range(3)], 1)
    assert cloud.dtype == np.float32
    for a in (src, p, T32, R64, cloud):
        a.setflags(write=False)
    return src, p, T32, R64, cloud


def tangent_cases():
    return [(sn, pn, n) for sn in SCENES for pn in POSES for n in HESSIAN_SIZES]


@functools.lru_cache(maxsize=None)
def hessian_reference(scene_name, pose_name, n, variant):
    """(ref H[36], majorant[36], hits, oracle H[36]) of computeHessian at the case's tangent: ref_sweep's H block under the Hessian recipe"""
    grid, leaves, bounds, prm = oracle_grid(scene_name, variant, 27)
    src, p, T32, R64, _ = tangent_case(scene_name, pose_name, n)
    row, maj, hits, _ = ref_sweep(leaves, bounds, prm, src, T32, T32[:3, :3], 27, hessian_R64=R64)
    out = (row[7:].copy(), maj[7:].copy(), hits, O.compute_hessian(grid, src, p).ravel())
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def score_reference(scene_name, pose_name, n, variant):
    """(ref score, majorant, hits, oracle score) of calculateScore on the case's moved cloud, with the Gauss constants of the grid's parameters"""
    grid, leaves, _, prm = oracle_grid(scene_name, variant, 27)
    cloud = tangent_case(scene_name, pose_name, n)[4]
    return ref_calculate_score(leaves, prm, cloud) + (O.calculate_score(grid, cloud),)
