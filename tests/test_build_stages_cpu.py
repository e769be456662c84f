"""CPU: the reference and the inputs of the stage tests of the target build are themselves checked here (tests/build_ref.py, tests/build_cases.py;
the device side is tests/test_build_stages_gpu.py).

* build_ref against the oracle on every chain case: bounds, every occupied cell and its count (n_pushed) exactly, means and centroids bit for
  bit, cov and icov inside the bar K_ICOV * majorant (build_ref.icov_majorant) -- K_ICOV is MEASURED here, on the oracle, never on the device.
* the inputs separate right from wrong: five deliberately wrong references each change the expected output of a named case.
* the generator reaches the edges it claims, read off the reference's own outputs.
* at most 1 % of the model leaves sit on a discontinuity (build_ref.ModelRef.near_guard), none of them in a named case."""
import numpy as np
import pytest

import build_cases as BC
import build_ref as R
from oracle import oracle_py as O

CASES = BC.all_cases()
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def oracle_params(case, pca=True):
    return O.default_params(resolution=case.leaf, min_points_per_voxel=case.min_points, variant=1 if pca else 0)


def model_rows(case):
    """(target, leaf index, TargetRef, ModelRef) of every leaf of a model case, mpmath evaluated once per process"""
    T = BC.reference(case)[0]
    return [(b, v, t, R.model_cached(t.sums[v], int(t.counts[v]), 0.01, True)) for b, t in enumerate(T) for v in range(t.n_voxels)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_matches_the_oracle(case):
    T, cb, word_off, total, largest = BC.reference(case)
    assert total == sum(t.grid.nwords for t in T) and largest == max(t.grid.ncells for t in T)
    for b, (t, cloud) in enumerate(zip(T, case.clouds)):
        if t.grid.status == R.GRID_CAP:
            continue                                                     # (the oracle has no cell cap: it would build the 64 M-cell grid)
        G = O.Grid(cloud, oracle_params(case)) if len(cloud) else None
        if t.grid.status != R.GRID_OK:
            assert G is None or not G.ok, (case.name, b)
            continue
        mn, mx, dv = G.bounds()
        assert np.array_equal(mn, t.grid.min_b) and np.array_equal(mx, t.grid.max_b) and np.array_equal(dv, t.grid.div_b), (case.name, b)
        lv = G.leaves()
        assert np.array_equal(lv["idx"], t.all_cells) and np.array_equal(lv["n_pushed"], t.all_counts), (case.name, b)
        v = lv[lv["n_pushed"] >= case.min_points]
        assert np.array_equal(v["idx"], t.leaf_cells) and np.array_equal(v["n_pushed"], t.counts)
        assert (v["mean"] == t.sums[:, :3] / t.counts[:, None]).all(), (case.name, b)          # bit for bit
        assert v["centroid"].tobytes() == t.cent.tobytes(), (case.name, b)


def oracle_model_ratios():
    """worst |oracle - mpmath| / majorant over every model leaf that sits on no discontinuity: cov, icov as f64, icov rounded to f32"""
    worst = {"cov": 0.0, "icov64": 0.0, "icov32": 0.0}
    n = near = 0
    for case in CASES:
        if not case.model:
            continue
        rows = model_rows(case)
        leaves = [O.Grid(c, oracle_params(case)).leaves() for c in case.clouds]
        leaves = [lv[lv["n_pushed"] >= case.min_points] for lv in leaves]
        for b, v, t, m in rows:
            L = leaves[b][v]
            n += 1
            assert (L["n"] == -1) == m.dead or m.near_guard, (case.name, b, v)
            if m.near_guard:
                near += 1
                continue
            if m.dead:
                continue
            assert L["label"] == m.label and L["weight"] == int(m.dim2d), (case.name, b, v)
            ic = L["icov"].reshape(3, 3)
            u64, u32 = R.icov_majorant(m.icov, m.a, m.kappa, False), R.icov_majorant(m.icov, m.a, m.kappa, True)
            worst["icov64"] = max(worst["icov64"], float((np.abs(ic - m.icov) / u64).max()))
            worst["icov32"] = max(worst["icov32"], float((np.abs(ic.astype(np.float32).astype(np.float64) - m.icov) / u32).max()))
            worst["cov"] = max(worst["cov"], float((np.abs(L["cov"].reshape(3, 3) - m.cov) / R.cov_majorant(m.cov, m.a, m.kappa)).max()))
    return worst, n, near


def test_the_bar_of_the_inverse_covariance_is_measured_on_the_oracle():
    worst, n, near = oracle_model_ratios()
    print(f"oracle vs mpmath, worst |diff| / majorant over {n} leaves ({near} left out): " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    w = max(worst["icov64"], worst["icov32"])
    assert 2 * w <= R.K_ICOV <= 4 * w, (worst, R.K_ICOV)                  # K = the next power of two at or above twice the oracle's worst ratio
    assert worst["cov"] <= R.K_ICOV
    assert (worst["icov64"], worst["icov32"]) == pytest.approx((R.ORACLE_WORST["icov64"], R.ORACLE_WORST["icov32"]), rel=0.05)
    assert near <= 0.01 * n                                              # the left-out share
    assert near == 0                                                     # ... and every model case is a named one: none may be left out


WRONG = [("min_points off by one", R.Rules(min_points_off=1), "markrank_mp6", 3, "leaf_cells"),
         ("< for <= in the head rule", R.Rules(head_strict=True), "markrank_mp6", 3, "leaf_cells"),
         ("truncation for floorf", R.Rules(truncate=True), "griddesc_leaf1.0", 0, "min_b"),
         ("rows with one non-finite coordinate kept", R.Rules(keep_partial=True), "minmax_dropped_rows", 0, "mm"),
         ("pairwise sums", R.Rules(pairwise=True), "leafsum_sizes_at_580m", 0, "sums")]


@pytest.mark.parametrize("what,rules,name,b,field", WRONG, ids=[w[0] for w in WRONG])
def test_inputs_tell_a_wrong_build_from_a_right_one(what, rules, name, b, field):
    case = BY_NAME[name]
    right = BC.reference(case)[0][b]
    wrong = R.build_batch(case.rows(), case.eff_pitch, case.leaf, case.min_points, rules)[0][b]
    pick = {"leaf_cells": lambda t: t.leaf_cells, "min_b": lambda t: t.grid.min_b, "mm": lambda t: np.concatenate(t.mm), "sums": lambda t: t.sums}[field]
    assert not np.array_equal(pick(right), pick(wrong)), what
    if field == "leaf_cells":                                            # the run of exactly min_points entries that ends the pitch is what differs
        assert set(right.leaf_cells) - set(wrong.leaf_cells) == {right.leaf_cells[-1]}
    if field == "sums":
        assert len(wrong.sums) == len(right.sums) and (np.abs(wrong.sums - right.sums) <= 1e-12 * np.abs(right.sums)).all()   # wrong in the last bits only


def run_of(t, v):
    return int(t.seg_start[v]), int(t.counts[v])


def all_runs(t, cb):
    """(start, length, is_leaf) of every binned run of the sorted order"""
    k = t.keys[t.keys != (1 << cb) - 1]
    start = np.flatnonzero(np.r_[True, k[1:] != k[:-1]]) if len(k) else np.zeros(0, int)
    length = np.diff(np.r_[start, len(k)])
    return start, length, np.isin(start, t.seg_start)


@pytest.mark.parametrize("mp", BC.MIN_POINTS)
def test_mark_and_rank_cases_reach_their_edges(mp):
    case = BY_NAME[f"markrank_mp{mp}"]
    T, cb = BC.reference(case)[:2]
    P = case.eff_pitch
    assert P % 256 != 0 and case.mode == "bind"
    s, l, leaf = all_runs(T[0], cb)
    assert set(l) == set(BC.run_lengths(mp)) and (leaf == (l >= mp)).all()
    assert s[0] == 0 and leaf[0]                                         # a head at position 0
    assert len(case.clouds[0]) < P                                       # an unbinned tail of padding ...
    assert (~np.isfinite(case.clouds[1])).any() and (T[1].keys == (1 << cb) - 1).sum() == P - len(case.clouds[1]) + 9   # ... and of NaN rows
    if mp > 1:
        s1, l1, leaf1 = all_runs(T[1], cb)
        assert s1[0] == 0 and l1[0] == mp - 1 and not leaf1[0]
        s2, l2, leaf2 = all_runs(T[case.note["straddle"]], cb)
        straddles = [(a, n) for a, n, f in zip(s2, l2, leaf2) if f and a // 256 != (a + mp - 1) // 256]
        assert any(n == mp for a, n in straddles) and any(n > mp for a, n in straddles)
    full = T[case.note["full"]]
    assert len(case.clouds[case.note["full"]]) == P and np.isfinite(case.clouds[case.note["full"]]).all()
    assert run_of(full, full.n_voxels - 1) == (P - mp, mp)               # exactly min_points entries ending at pitch - 1: a leaf
    if mp > 1:
        short = T[case.note["full"] + 1]
        s3, l3, leaf3 = all_runs(short, cb)
        assert len(case.clouds[case.note["full"] + 1]) == P and s3[-1] + l3[-1] == P and l3[-1] == mp - 1 and not leaf3[-1]
        assert T[case.note["full"] + 2].keys[0] == short.keys[-1] == 2      # the next target's first key goes on where the short run ends


def test_the_other_cases_reach_their_edges():
    ref = lambda n: BC.reference(BY_NAME[n])
    T = ref("markrank_set_mode")[0]
    P = BY_NAME["markrank_set_mode"].eff_pitch
    assert P % 64 == 0 and P % 256 != 0 and run_of(T[1], T[1].n_voxels - 1) == (P - 6, 6)
    s, l, leaf = all_runs(T[2], ref("markrank_set_mode")[1])
    assert s[-1] + l[-1] == P and l[-1] == 5 and not leaf[-1]
    t = ref("markrank_two_head_trips")[0][0]
    assert len(t.head_cnt) == 513 and t.head_cnt[512] > 0 and t.head_cnt[:512].sum() > 0        # more than 512 slices: the head loop's second trip
    t = ref("bitmap_word_edges")[0][0]
    assert t.grid.ncells == 130 and tuple(t.leaf_cells) == (0, 63, 64, 129) and len(t.all_cells) > 60
    for name, words in (("bitmap_sparse_over_262144_cells", 4096), ("bitmap_sparse_over_524288_cells", 8192)):
        t = ref(name)[0][0]
        assert t.grid.nwords > words + 1 and t.leaf_cells[0] == 0 and t.leaf_cells[-1] == t.grid.ncells - 1 and len(BY_NAME[name].clouds[0]) < 400
        assert (t.leaf_cells // 64 >= words).any() and t.prefix[words] > 0                      # the word loop's later trips carry a prefix in
    T = ref("griddesc_cells_63_64_65")[0]
    assert [(t.grid.ncells, t.grid.nwords) for t in T] == [(63, 2), (64, 2), (65, 3)]
    assert tuple(t.grid.status for t in ref("griddesc_statuses")[0]) == (R.GRID_EMPTY, R.GRID_OVERFLOW, R.GRID_CAP, R.GRID_OK, R.GRID_EMPTY)
    for leaf in (1.0, 0.5, 0.3):
        T = ref(f"griddesc_leaf{leaf}")[0]
        assert (T[0].grid.min_b < 0).all() and (T[0].grid.max_b > 0).all() and (T[1].grid.max_b < 0).all()
    case = BY_NAME["minmax_extreme_spots"]
    for t, cloud, (a, sgn, r) in zip(ref(case.name)[0], case.clouds, case.note["spots"]):
        assert (np.argmax(cloud[:, a]) if sgn > 0 else np.argmin(cloud[:, a])) == r and t.mm[sgn > 0][a] == 50.0 * sgn
    for n in BC.MM_SIZES:
        assert tuple(t.grid.status for t in ref(f"minmax_n{n}_K3")[0]) == (R.GRID_EMPTY, R.GRID_EMPTY, R.GRID_OK)
        assert BY_NAME[f"minmax_n{n}_K3"].eff_pitch % 2 == 1 and BY_NAME[f"minmax_n{n}_K1"].eff_pitch == n
    for t in ref("minmax_dropped_rows")[0]:
        assert np.abs(np.concatenate(t.mm)).max() < 10                   # the +-1000 of the dropped rows are no extremes
    T = ref("minmax_special_values")[0]
    assert T[0].grid.ncells == 1 and tuple(T[1].grid.min_b) == (-1, -1, -1) and T[2].grid.status == R.GRID_OVERFLOW
    for org in BC.ORIGINS:
        case = BY_NAME[f"leafsum_sizes_at_{org[0]}m"]
        t = ref(case.name)[0][0]
        assert list(t.counts) == case.note["sizes"] and run_of(t, 7) == (case.eff_pitch - 1000, 1000)
        assert tuple(t.grid.min_b) == org
    assert tuple(t.n_voxels for t in ref("leafsum_n_voxels")[0]) == BC.N_VOXELS
    for K in BC.XCD_K:
        T = ref(f"leafsum_K{K}")[0]
        assert len(T) == K and all(t.n_voxels > 0 for t in T)
    T, cb, word_off, total, largest = ref("wordoff_1025_targets")
    assert len(T) == 1025 and total == 2050 and largest == 1 and np.array_equal(word_off, 2 * np.arange(1025))


def test_the_shapes_reach_every_branch_of_the_model():
    """isotropic leaves are not inflated, sheets have one inflated eigenvalue, needles two, a repeated point leaves the Identity seed alone (isotropic),
    a one-point leaf is dead; all three pca labels occur"""
    labels = set()
    for org in BC.ORIGINS:
        case = BY_NAME[f"leafsum_shapes_at_{org[0]}m"]
        by_target = {}
        for b, v, t, m in model_rows(case):
            by_target.setdefault(b, []).append(m)
            labels.add(m.label)
        assert [set(m.inflated for m in by_target[b]) for b in range(4)] == [{0}, {1}, {2}, {0}], case.name
        for m, n in zip(by_target[3], BC.reference(case)[0][3].counts):
            assert np.allclose(m.cov, np.eye(3) * (n - 1) / n ** 2, rtol=0, atol=1e-6)
    assert labels == {1, 2, 3}
    dead = [m.dead for b, v, t, m in model_rows(BY_NAME["leafsum_mp1"]) if t.counts[v] == 1]
    assert dead and all(dead)


def test_the_synthetic_voxel_cases_reach_every_guard():
    """k_voxels alone (tests/hip/build_check): per eig_mult, no / one / two inflated eigenvalues, the three pca labels, dead leaves by a negative and by a
    zero eigenvalue and by n = 1, every distance, and no case on a discontinuity"""
    VC = BC.voxel_cases()
    assert len({name for name, _, _, _ in VC}) == len(VC)
    for em in BC.EIG_MULTS:
        M = {name: R.model_cached(s, n, em, True) for name, n, s, expect in VC if expect == "model"}
        assert not any(m.near_guard for m in M.values())
        assert {m.inflated for m in M.values() if not m.dead} == {0, 1, 2} and {m.label for m in M.values() if not m.dead} == {1, 2, 3}
        for d in BC.DISTANCES:
            assert [M[f"{k}_{d:g}m"].inflated for k in ("isotropic", "planar", "collinear", "two_equal", "three_equal")] == [0, 1, 2, 0, 0]
            assert [M[f"{k}_{d:g}m"].label for k in ("collinear", "planar", "isotropic")] == [1, 2, 3]
            assert M[f"negative_eigenvalue_{d:g}m"].dead and M[f"identical_points_n1_{d:g}m"].dead and not M[f"identical_points_n9_{d:g}m"].dead
            assert np.allclose(M[f"identical_points_n9_{d:g}m"].cov, np.eye(3) * 8 / 81, rtol=0, atol=1e-5)      # the Identity seed alone
            assert abs(np.linalg.norm(M[f"isotropic_{d:g}m"].mean) - d) < 0.5
        assert M["zero_largest_eigenvalue"].dead
    name, n, s, expect = VC[-1]
    assert expect == "bad_inverse" and not R.model_cached(s, n, 0.01, True).dead                  # mathematically invertible; f64's cofactors underflow


def test_the_build_check_cases_cover_both_reasons_and_a_ragged_grid():
    C = {c[0]: c for c in BC.build_check_cases()}
    fits = lambda c: c[4] <= c[2] and (c[3] >= 31 or c[5] + 1 <= (1 << c[3]))
    assert fits(C["fits"]) and fits(C["plan_cb_31"]) and fits(C["plan_cb_32"]) and fits(C["fits_300_pairs"])
    assert C["too_few_words"][4] > C["too_few_words"][2] and C["too_few_words"][5] + 1 <= 1 << C["too_few_words"][3]
    assert C["cell_field_too_narrow"][4] <= C["cell_field_too_narrow"][2] and C["cell_field_too_narrow"][5] + 1 > 1 << C["cell_field_too_narrow"][3]
    assert not any(fits(C[k]) for k in C if k.startswith("misfit")) and C["plan_cb_31"][5] + 1 > 1 << 12
    assert {C[k][1] % 256 for k in ("misfit_300_pairs", "misfit_257_pairs", "misfit_1_pair")} == {44, 1}
