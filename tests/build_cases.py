"""The inputs of the stage tests of the target build (test_build_stages_cpu.py, test_build_stages_gpu.py): batches of point clouds, each made for
one edge of one kernel of lv_slam_amd/csrc/ndt_build.hpp.  A case plants counts per cell; run lengths and positions in the sorted order follow
from the cell order, NaN rows and the pitch's padding form the unbinned tail.  What a case claims to reach is asserted from the reference's own
outputs in test_build_stages_cpu.py.

mode "set": batch_reserve + batch_set_target (the pitch is the largest cloud rounded up to 64 rows).  mode "bind": batch_bind_device on rows
laid out here, for what the upload path cannot make -- an odd pitch (rows 1, 2 and later targets then start off a 16-byte boundary), a cloud
that fills a pitch that is no multiple of 64, and padding rows with huge finite values that must never be read."""
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
PAD = (F32(1e30), F32(-1e30), F32(3e38))         # what a bound buffer holds past a cloud's rows
ORIGINS = ((0, 0, 0), (37, -20, 5), (580, -410, 33))
MM_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 3071, 3072, 3073, 3077, 12289)
MIN_POINTS = (1, 2, 6, 12)
LEAF_SIZES = (63, 64, 65, 128, 129, 200, 1000)
N_VOXELS = (1, 3, 4, 5, 255, 256, 257, 600)
XCD_K = (1, 7, 8, 9, 17)


@dataclass
class Case:
    name: str
    group: str
    clouds: list                  # [n_i, 3] f32 each
    leaf: float = 1.0
    min_points: int = 6
    pitch: int = 0                # 0: mode "set"
    model: bool = False           # the voxel model of every leaf is compared with the mpmath evaluation
    note: dict = field(default_factory=dict)

    @property
    def mode(self):
        return "bind" if self.pitch else "set"

    @property
    def eff_pitch(self):
        return self.pitch or max(64, -(-max(len(c) for c in self.clouds) // 64) * 64)

    def rows(self):
        """[(rows [pitch, 3], n)]: the clouds in their pitch, padded with huge finite values"""
        P = self.eff_pitch
        out = []
        for c in self.clouds:
            r = np.empty((P, 3), F32)
            r[:] = np.array(PAD, F32)[np.arange(P) % 3][:, None]
            r[:len(c)] = c
            out.append((r, len(c)))
        return out


def _rng(*key):
    return np.random.default_rng([20261020] + [int(k) for k in key])


def box(rng, n, lo=(-3.5, -2.5, -1.5), size=(8, 6, 3)):
    return (np.asarray(lo) + rng.random((n, 3)) * np.asarray(size)).astype(F32)


def plant(rng, cells, leaf=1.0, shape="iso", shuffle=True):
    """cells: [((i, j, k), count)] -> the points, shuffled: `count` points inside cell (i, j, k), away from its faces.
    shape: iso = anywhere in the cell's middle; plane = a sheet 1e-3 leaf thick; line = a needle; same = one point, repeated"""
    out = []
    for (ijk, cnt) in cells:
        u = 0.125 + 0.75 * rng.random((cnt, 3))
        if shape == "plane":
            u[:, 2] = 0.5 + 1e-3 * (rng.random(cnt) - 0.5)
        elif shape == "line":
            u[:, 1:] = 0.5 + 1e-3 * (rng.random((cnt, 2)) - 0.5)
        elif shape == "same":
            u[:] = u[0]
        out.append(((np.asarray(ijk, np.float64) + u) * float(F32(leaf))).astype(F32))
    P = np.concatenate(out) if out else np.zeros((0, 3), F32)
    return P[rng.permutation(len(P))] if shuffle else P


def line(counts, origin=(0, 0, 0)):
    """cells along x from `origin`, cell k with counts[k] points (0: an empty cell)"""
    return [((origin[0] + k, origin[1], origin[2]), int(c)) for k, c in enumerate(counts) if c > 0]


def with_nans(rng, P, m):
    """m rows with one non-finite coordinate each, scattered through the cloud"""
    bad = box(rng, m)
    bad[np.arange(m), rng.integers(0, 3, m)] = np.array([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, m)]
    Q = np.concatenate([P, bad])
    return Q[rng.permutation(len(Q))]


# ------------------------------------------------------------------------------------------------ k_minmax
def minmax_cases():
    out = []
    for n in MM_SIZES:
        rng = _rng(1, n)
        out.append(Case(f"minmax_n{n}_K1", "minmax", [box(rng, n)], min_points=1, pitch=n))
        # ragged, with an empty and an all-NaN cloud; the odd pitch puts rows 1 and 2 and targets 1 and 2 off the 16-byte boundary
        out.append(Case(f"minmax_n{n}_K3", "minmax", [np.full((n // 2 + 1, 3), np.nan, F32), np.zeros((0, 3), F32), box(rng, n)], min_points=1,
                        pitch=n + 1 if n % 2 == 0 else n + 2))
    # where the extreme sits: per axis, min and max apart; n = 3075 is one full trip of one block (3072) and a quad that straddles n
    n = 3075
    spots = {"first": 0, "last": n - 1, "straddle": 3073, "group2": 1024 + 5, "group3": 2048 + 7}
    clouds, what = [], []
    for a in range(3):
        for sgn in (-1, 1):
            for nm, r in spots.items():
                P = box(_rng(2, a, sgn + 1, r), n)
                P[r, a] = F32(sgn * 50.0)
                clouds.append(P)
                what.append((a, sgn, r))
    out.append(Case("minmax_extreme_spots", "minmax", clouds, min_points=1, pitch=n + 2, note={"spots": what}))
    # a row whose one coordinate is NaN or +-inf and whose other two would be the extremes is dropped whole
    clouds = []
    for a in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            P = box(_rng(3, a), 37)
            for r, s in ((0, 1000.0), (36, -1000.0)):
                P[r] = F32(s)
                P[r, a] = F32(bad)
            clouds.append(P)
    out.append(Case("minmax_dropped_rows", "minmax", clouds, min_points=1, pitch=39))
    z = np.zeros((5, 3), F32)
    zeros = z.copy(); zeros[1::2] = F32(-0.0)
    den = z.copy(); den[1] = F32(1e-40); den[3] = F32(-1e-40)
    big = z.copy(); big[2] = FLT_MAX; big[4] = -FLT_MAX
    out.append(Case("minmax_special_values", "minmax", [zeros, den, big], min_points=1, pitch=7))
    return out


# ------------------------------------------------------------------------------------------------ k_griddesc
def griddesc_cases():
    out = []
    for leaf in (1.0, 0.5, 0.3):
        rng = _rng(4, int(leaf * 10))
        k = np.arange(-2, 3)
        lattice = np.stack([F32(k) * F32(leaf), F32(k[::-1]) * F32(leaf), F32(k // 2) * F32(leaf)], axis=1).astype(F32)   # exactly on k * leaf
        A = np.concatenate([box(rng, 300, lo=(-2.9, -2.2, -0.8), size=(5.5, 4.1, 1.7)), lattice])
        B = np.concatenate([box(rng, 200, lo=(-7.3, -6.1, -2.2), size=(3, 3, 2)), lattice - F32(3) * F32(leaf)])        # all coordinates negative
        out.append(Case(f"griddesc_leaf{leaf}", "griddesc", [A[rng.permutation(len(A))], B], leaf=leaf, min_points=2))
    rng = _rng(5)
    out.append(Case("griddesc_cells_63_64_65", "griddesc", [plant(rng, line([2] + [0] * (nc - 2) + [1], origin=(-30, 4, -2))) for nc in (63, 64, 65)],
                    min_points=1, note={"ncells": (63, 64, 65)}))
    ok = box(rng, 100)
    out.append(Case("griddesc_statuses", "griddesc",
                    [np.full((3, 3), np.nan, F32), np.array([[0, 0, 0], [1e30, 0, 0]], F32), np.array([[0, 0, 0], [400, 400, 400], [1, 1, 1]], F32), ok,
                     np.zeros((0, 3), F32)], min_points=1, note={"status": (1, 2, 3, 0, 1)}))
    return out


# ------------------------------------------------------------------------------------------------ k_mark / k_rank
def run_lengths(mp):
    return [v for v in dict.fromkeys([mp, 1, mp - 1, mp + 1, 63, 64, 65, 255, 256, 257, 600]) if v > 0]


def markrank_cases():
    out = []
    for mp in MIN_POINTS:
        rng = _rng(6, mp)
        L = run_lengths(mp)
        t0 = plant(rng, line(L))                                            # a leaf's head at position 0; t1: a run of mp - 1 there, and NaN rows
        t1 = with_nans(rng, plant(rng, line([mp - 1] + L[::-1] + [0, 0, 3], origin=(-5, 2, 1))), 9)
        n0 = max(len(t0), len(t1))
        pitch = n0 + 3 if (n0 + 3) % 256 else n0 + 4                        # no multiple of 256 (nor of 64: the last slice is a short one)
        clouds = [t0, t1]
        if mp > 1:
            # a head in one slice whose mp-th entry is in the next: a run of mp from 257 - mp, then a longer one from 513 - mp, then one of mp - 1
            clouds.append(plant(rng, line([257 - mp, mp, 256 - mp, mp + 3, mp - 1, 2 * mp])))
            # the pitch's last run: exactly mp entries ending at pitch - 1 (a leaf), and mp - 1 (none); all rows finite, n == pitch
            clouds.append(plant(rng, line([pitch - 70 - mp, 70, mp])))
            clouds.append(plant(rng, line([pitch - 70 - (mp - 1), 70, mp - 1])))
            # ... followed by a target whose sorted keys START with that run's key (cell 2): a head test that looks one entry past the pitch sees the
            # run go on there and makes a leaf of it
            clouds.append(plant(rng, [((2, 0, 0), 4), ((0, 1, 0), 3)]))
        else:
            clouds.append(plant(rng, line([pitch - 70 - 1, 70, 1])))
        out.append(Case(f"markrank_mp{mp}", "markrank", clouds, min_points=mp, pitch=pitch, note={"straddle": 2 if mp > 1 else None, "full": 3 if mp > 1 else 2}))
    # the same through the upload path: the pitch a multiple of 64 and not of 256
    rng = _rng(7)
    L = run_lengths(6)
    t0 = plant(rng, line(L))
    pitch = -(-len(t0) // 64) * 64
    if pitch % 256 == 0:
        pitch += 64
    out.append(Case("markrank_set_mode", "markrank", [t0, plant(rng, line([pitch - 70 - 6, 70, 6])), plant(rng, line([pitch - 70 - 5, 70, 5]))], min_points=6,
                    note={"full": 2, "pitch": pitch}))
    # 131,072 + 256 rows, all finite: 513 slices, the head loop's second trip
    n = 131072 + 256
    cells = rng.integers(0, (40, 40, 20), size=(n, 3))
    P = ((cells + 0.125 + 0.75 * rng.random((n, 3)))).astype(F32)
    out.append(Case("markrank_two_head_trips", "markrank", [P], min_points=6, note={"slices": 513}))
    return out


# ------------------------------------------------------------------------------------------------ bitmaps
def bitmap_cases():
    out = []
    rng = _rng(8)
    counts = rng.integers(0, 6, 130)                                         # under min_points: occupied, no leaf
    counts[[0, 63, 64, 129]] = (6, 7, 6, 9)
    counts[[1, 62, 65, 128]] = (5, 0, 5, 0)
    out.append(Case("bitmap_word_edges", "bitmap", [plant(rng, line(counts, origin=(-64, 0, 0)))], min_points=6, note={"leaves": (0, 63, 64, 129)}))
    for div, nm in (((128, 64, 33), "262144"), ((128, 64, 65), "524288")):
        c = rng.integers(0, div, size=(60, 3))
        cells = [((0, 0, 0), 6), ((div[0] - 1, div[1] - 1, div[2] - 1), 6)] + [(tuple(int(v) for v in r), int(rng.integers(1, 9))) for r in c]
        out.append(Case(f"bitmap_sparse_over_{nm}_cells", "bitmap", [plant(rng, cells)], min_points=6, note={"min_cells": int(nm)}))
    return out


# ------------------------------------------------------------------------------------------------ leaf sums and the voxel model
def leafsum_cases():
    out = []
    for oi, org in enumerate(ORIGINS):
        rng = _rng(9, oi)
        sizes = [6] + list(LEAF_SIZES)
        P = plant(rng, line(sizes, origin=org))                             # the last leaf (1000 entries) ends at pitch - 1
        out.append(Case(f"leafsum_sizes_at_{org[0]}m", "leafsum", [P], min_points=6, pitch=len(P), model=True, note={"sizes": sizes}))
        shapes = []
        for sh in ("iso", "plane", "line", "same"):
            # (4 m leaves of 200 .. 400 points: the Identity seed adds 1 / n to every eigenvalue, and below ~130 points of a 4 m leaf that alone keeps
            # the smallest one above a hundredth of the largest)
            shapes.append(plant(rng, [((org[0] // 4 + i, org[1] // 4 + j, org[2] // 4), int(c)) for i, j, c in zip(range(12), rng.integers(0, 3, 12), rng.integers(200, 400, 12))],
                                leaf=4.0, shape=sh))
        out.append(Case(f"leafsum_shapes_at_{org[0]}m", "leafsum", shapes, leaf=4.0, min_points=6, model=True, note={"shapes": ("iso", "plane", "line", "same")}))
    rng = _rng(10)
    org = ORIGINS[1]
    out.append(Case("leafsum_n_voxels", "leafsum", [plant(rng, line(rng.integers(6, 9, nv), origin=(org[0] - nv // 2, org[1], org[2]))) for nv in N_VOXELS],
                    min_points=6, model=True, note={"n_voxels": N_VOXELS}))
    for K in XCD_K:
        clouds = [plant(rng, line(rng.integers(3, 70, 6), origin=ORIGINS[k % 3])) for k in range(K)]
        out.append(Case(f"leafsum_K{K}", "leafsum", clouds, min_points=6, model=(K == 9), note={"K": K}))
    for mp in (1, 2, 12):
        out.append(Case(f"leafsum_mp{mp}", "leafsum", [plant(rng, line([mp, mp + 1, 1, 63, 64, 65, max(1, mp - 1), 129], origin=ORIGINS[1]))], min_points=mp,
                        model=True))
    return out


def wordoff_cases():
    rng = _rng(11)
    return [Case("wordoff_1025_targets", "wordoff", [box(rng, 1) for _ in range(1025)], min_points=1, note={"K": 1025})]


def all_cases():
    return minmax_cases() + griddesc_cases() + markrank_cases() + bitmap_cases() + leafsum_cases() + wordoff_cases()


_REF = {}


def reference(case):
    """build_ref.build_batch of a case, computed once: (targets, cb, word_off, total_words, largest)"""
    import build_ref as R
    if case.name not in _REF:
        _REF[case.name] = R.build_batch(case.rows(), case.eff_pitch, case.leaf, case.min_points)
    return _REF[case.name]


# ------------------------------------------------------------------------------------------------ k_voxels alone: synthetic sums and counts
DISTANCES = (0.0, 37.0, 580.0, 5000.0)
EIG_MULTS = (0.01, 0.1)


def sums_for(n, mu, cov):
    """the nine sums (S0 S1 S2 C00 C01 C02 C11 C12 C22) whose one-pass covariance ((C - 2 S mu^T) / n + mu mu^T) (n - 1) / n is `cov` about `mu`,
    up to their rounding to f64 (the reference is evaluated from the rounded sums, so that rounding is part of the input)"""
    mu, cov = np.asarray(mu, np.float64), np.asarray(cov, np.float64)
    C = n * (cov * (n / (n - 1.0)) + np.outer(mu, mu))
    return np.array([n * mu[0], n * mu[1], n * mu[2], C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]], np.float64)


def voxel_cases():
    """[(name, count, sums[9], expect)]: expect "model" = what build_ref.model says, "bad_inverse" = alive through the eigenvalue test, inverse not finite"""
    rng = _rng(12)
    out = []
    shapes = {"isotropic": (0.04, 0.05, 0.06), "planar": (1e-5, 0.04, 0.05), "collinear": (1e-5, 2e-5, 0.05)}
    for d in DISTANCES:
        mu = d * np.array([0.6, -0.7, 0.3872983346207417]) + np.array([0.3, 0.2, 0.1])     # (off the origin: scale * |mu| is truncated to an integer)
        for nm, ev in shapes.items():
            Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
            out.append((f"{nm}_{d:g}m", 50, sums_for(50, mu, Q @ np.diag(ev) @ Q.T), "model"))
        out.append((f"two_equal_{d:g}m", 50, sums_for(50, mu, np.diag([0.03, 0.03, 0.06])), "model"))
        out.append((f"three_equal_{d:g}m", 50, sums_for(50, mu, np.diag([0.04, 0.04, 0.04])), "model"))
        out.append((f"min_points_{d:g}m", 6, sums_for(6, mu, np.diag([0.02, 0.05, 0.03])), "model"))
        Q = np.linalg.qr(rng.standard_normal((3, 3)))[0]
        out.append((f"negative_eigenvalue_{d:g}m", 50, sums_for(50, mu, Q @ np.diag([-0.01, 0.04, 0.05]) @ Q.T), "model"))
        p = (mu + np.array([0.25, 0.5, 0.125])).astype(F32).astype(np.float64)
        for n in (1, 9):                                                 # n copies of one point: the Identity seed alone (n = 1: f = 0, no covariance at all)
            S, C = n * p, np.eye(3) + n * np.outer(p, p)
            out.append((f"identical_points_n{n}_{d:g}m", n, np.array([S[0], S[1], S[2], C[0, 0], C[0, 1], C[0, 2], C[1, 1], C[1, 2], C[2, 2]]), "model"))
    out.append(("zero_largest_eigenvalue", 50, np.zeros(9), "model"))
    out.append(("inverse_not_finite", 50, sums_for(50, np.zeros(3), np.diag([1e-200, 2e-200, 3e-200])), "bad_inverse"))
    return out


def build_check_cases():
    """k_build_check alone: (name, n_pairs, plan_words, plan_cb, total words, largest grid); fits iff total <= plan_words and (plan_cb >= 31 or
    largest + 1 <= 2^plan_cb)"""
    return [("fits", 5, 4096, 12, 4096, 4095), ("too_few_words", 5, 4095, 12, 4096, 100), ("cell_field_too_narrow", 5, 4096, 12, 100, 4096),
            ("plan_cb_31", 5, 4096, 31, 4096, (1 << 25)), ("plan_cb_32", 3, 10, 32, 10, 0xFFFFFFFF), ("fits_300_pairs", 300, 70000, 8, 69999, 255),
            ("misfit_300_pairs", 300, 70000, 8, 70001, 255), ("misfit_257_pairs", 257, 9, 8, 10, 3), ("misfit_1_pair", 1, 9, 1, 9, 2)]
