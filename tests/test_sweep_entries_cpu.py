"""CPU: the float64 reference of one derivative sweep (tests/ndt_ref.py) against the oracle, entry by entry, on the tiny scenes of
tests/test_sweep_entries_gpu.py -- the guard of the reference itself and the anchor of that file's bars.

The oracle evaluates the reference's f32 recipe, ref_sweep the mathematics in f64, so what separates them is the recipe's own rounding: every one of
the 43 numbers (score, g, H) must agree within K_EXACT * 2^-24 * majorant of THAT entry.  The scenes are also shown not to be vacuous, on the
reference alone: partial neighbourhoods, ndt_pca weights of 0 and of >= 100, Hessian entries far below the largest one, the asymmetry of H."""
import os
import re
import subprocess

import numpy as np
import pytest

import ndt_ref as R
import sweep_matrix as M
from conftest import ROOT
from oracle import oracle_py as O

K_EXACT = 4          # measured maximum over all cases: 2.34 (a one-hit sweep; glibc exp); 4 leaves room for another libm's last bit in exp
VARIANTS = (O.VARIANT_OMP, O.VARIANT_PCA)


@pytest.mark.parametrize("K", [7, 1])
@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_agrees_with_the_f64_reference_entry_by_entry(variant, K):
    worst = (0.0,)
    for sn, pn, n in R.cases():
        row, maj, hits, hpp, orow, ohits = R.reference(sn, pn, n, variant, K)
        assert hits == ohits, (sn, pn, n)
        assert np.all(np.isfinite(row)) and np.all(np.isfinite(orow)) and np.all(maj >= np.abs(row))
        u = R.units(orow, row, maj)
        worst = max(worst, (float(u.max()), int(u.argmax()), sn, pn, n))
        assert np.all(np.abs(orow - row) <= K_EXACT * R.EPS32 * maj), (sn, pn, n, float(u.max()), int(u.argmax()))
    print(f"variant {variant} K {K}: largest |oracle - ref| / (2^-24 majorant) = {worst[0]:.3f} at entry {worst[1]} of {worst[2:]}")
    assert worst[0] > 0.01            # (the two do differ: the oracle is not the reference in disguise)


@pytest.mark.parametrize("pose", R.POSES)
def test_the_scenes_are_not_vacuous(pose):
    """on the reference alone, for each pose"""
    n = 513
    per_point = np.concatenate([R.reference(sn, pose, n, O.VARIANT_OMP, 7)[3] for sn in R.SCENES])
    assert (per_point == 7).any() and ((per_point >= 1) & (per_point <= 3)).any() and (per_point == 0).any()
    for sn in R.SCENES:                                   # every scene: full and partial neighbourhoods, the four rows that meet nothing
        hpp = R.reference(sn, pose, n, O.VARIANT_OMP, 7)[3]
        assert (hpp == 7).any() and ((hpp > 0) & (hpp < 7)).any() and (hpp == 0).sum() >= 4, sn
        assert R.reference(sn, pose, 1, O.VARIANT_OMP, 1)[2] == 1, sn          # (the one-point sweep is one hit, not none)
    # ndt_pca: a leaf of weight 0 and a leaf of weight >= 100 are both met, and a weight of 0 does wipe what its point had gathered
    met = []
    for sn in R.SCENES:
        src, T, Rj = R.sweep_inputs(sn, pose, n)
        _, leaves, bounds, prm = R.oracle_grid(sn, O.VARIANT_PCA, 1)
        met.append(leaves["weight"][R.hit_leaves(leaves, bounds, prm, src, T, Rj, 1)])
    met = np.concatenate(met)
    assert (met == 0).any() and (met >= 100).any()
    pca = R.reference("origin", pose, n, O.VARIANT_PCA, 7)
    omp = R.reference("origin", pose, n, O.VARIANT_OMP, 7)
    assert pca[2] == omp[2] and not np.allclose(pca[0], omp[0])
    # away from the origin the rotation block of H dwarfs the translation block: the smallest |H| entry is far below 1e-5 of the largest, which
    # is the whole of what a bar stated as a fraction of the largest entry checks
    for sn in ("mid", "far", "mid_r0.7"):
        for variant in VARIANTS:
            H = np.abs(R.reference(sn, pose, n, variant, 7)[0][7:])
            assert 0 < H.min() < 1e-4 * H.max(), (sn, variant, H.min() / H.max())
    # H is not symmetric (impl2:522-530, 607: z = r y^T - (y . r) I), by more than the bar: a symmetric rotation block would fail
    seen = 0
    for sn in R.SCENES:
        for variant in VARIANTS:
            row, maj = R.reference(sn, pose, n, variant, 7)[:2]
            H, mH = row[7:].reshape(6, 6), maj[7:].reshape(6, 6)
            seen += abs(H[3, 4] - H[4, 3]) > 64 * K_EXACT * R.EPS32 * (mH[3, 4] + mH[4, 3])
    assert seen >= 1


# ------------------------------------------------------------------------------------------------- DIRECT26 and the radius search
# The same bar for the two searches past DIRECT1 / DIRECT7.  Measured maximum over all cases, the "tie" scene included: 2.31 (ndt_pca + KDTREE, entry
# H[4][4] of the one-point sweep of "mid", pose "near"); DIRECT26 1.76, omp + KDTREE 1.74.  Under 4: K_EXACT holds for all four searches.
NEW_K = (26, 27)


@pytest.mark.parametrize("K", NEW_K)
@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_agrees_with_the_f64_reference_under_direct26_and_kdtree(variant, K):
    worst = (0.0,)
    for sn, pn, n in R.cases(tie=True):
        row, maj, hits, hpp, orow, ohits = R.reference(sn, pn, n, variant, K)
        assert hits == ohits, (sn, pn, n)
        assert np.all(np.isfinite(row)) and np.all(np.isfinite(orow)) and np.all(maj >= np.abs(row))
        u = R.units(orow, row, maj)
        worst = max(worst, (float(u.max()), int(u.argmax()), sn, pn, n))
        assert np.all(np.abs(orow - row) <= K_EXACT * R.EPS32 * maj), (sn, pn, n, float(u.max()), int(u.argmax()))
    print(f"variant {variant} K {K}: largest |oracle - ref| / (2^-24 majorant) = {worst[0]:.3f} at entry {worst[1]} of {worst[2:]}")
    assert worst[0] > 0.01


@pytest.mark.parametrize("pose", R.POSES)
def test_the_scenes_are_not_vacuous_for_direct26_and_kdtree(pose):
    """on the reference alone.  DIRECT26 probes the 26 cells AROUND the point's own (no centre cell: ndt_ref.OFFSETS26), so a full neighbourhood is
    26 leaves; a point of a corner cell of the block meets 7."""
    n = 513
    for sn in R.SCENES:
        hpp = R.reference(sn, pose, n, O.VARIANT_OMP, 26)[3]
        assert (hpp == 26).any() and ((hpp > 0) & (hpp < 9)).any() and (hpp == 0).any(), sn
        # KDTREE: some leaf of the 3 x 3 x 3 block around a point is rejected by the radius, some point meets more than DIRECT7 could, some none
        src, T, Rj = R.sweep_inputs(sn, pose, n)
        _, leaves, bounds, prm = R.oracle_grid(sn, O.VARIANT_OMP, 27)
        kd = R.reference(sn, pose, n, O.VARIANT_OMP, 27)[3]
        block = R.reference(sn, pose, n, O.VARIANT_OMP, 26)[3] + R.reference(sn, pose, n, O.VARIANT_OMP, 1)[3]
        assert np.all(kd <= block) and (kd < block).any() and (kd > 7).any() and (kd == 0).any(), sn
        # and the radius is decided close to its edge: some accepted and some rejected leaf within 2 % of the squared radius
        x = R._lookup(leaves, bounds, prm, src, T, Rj, 1)[0]
        d2 = ((x[:, None, :] - leaves["centroid"][None].astype(np.float64)) ** 2).sum(2) / (R.named_scene(sn).leaf ** 2)
        assert ((d2 > 0.98) & (d2 < 1)).any() and ((d2 > 1) & (d2 < 1.02)).any(), sn


def test_the_tie_scene_decides_the_order_rule():
    """ndt_pca + KDTREE on "tie": two leaves at the SAME f32 squared distance from the first source point, weights 9 and 10.  With the tie broken
    the other way at least one entry moves by more than 100 x the widest bar any sweep test holds it to (K_EXACT 2^-24 majorant)."""
    _, leaves, bounds, prm = R.oracle_grid(R.TIE, O.VARIANT_PCA, 27)
    src, T, Rj = R.sweep_inputs(*R.TIE_CASE)
    x, _, slots = R._lookup(leaves, bounds, prm, src, T, Rj, 27)
    assert np.array_equal(x[0], np.float64(R.TieScene.TIE_POINT))
    (a, hit_a), (b, hit_b) = slots[0], slots[1]
    assert hit_a[0] and hit_b[0] and a[0] < b[0] and not any(hit[0] for _, hit in slots[2:])
    ca, cb = leaves["centroid"][a[0]], leaves["centroid"][b[0]]
    assert ca.dtype == np.float32 and np.array_equal(src[0] - ca, cb - src[0])                # mirror images, exactly, in f32
    d2 = [np.float32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) for d in (src[0] - ca, src[0] - cb)]
    assert d2[0] == d2[1] < np.float32(1)
    wa, wb = int(leaves["weight"][a[0]]), int(leaves["weight"][b[0]])
    assert wa != wb and wa > 0 and wb > 0
    row, maj, hits, hpp = R.ref_sweep(leaves, bounds, prm, src, T, Rj, 27)
    swapped = R.ref_sweep(leaves, bounds, prm, src, T, Rj, 27, tie_last_first=True)
    assert hits == swapped[2] and np.array_equal(hpp, swapped[3]) and list(hpp) == [2, 3, 2, 1, 0, 0]
    # the edge point: B's centroid at an f32 squared distance EQUAL to float(resolution^2) -- not met, the test being strict; `<=` would meet it
    e = R.TieScene.EDGE_ROW
    de = src[e] - cb
    assert np.float32((de[0] * de[0] + de[1] * de[1]) + de[2] * de[2]) == np.float32(float(prm.resolution) * float(prm.resolution))
    assert b[0] not in [int(pos[e]) for pos, hit in slots if hit[e]] and hpp[e] == 1
    moved = np.abs(row - swapped[0]) / (K_EXACT * R.EPS32 * maj)
    print(f"tie rule reversed: entries move by up to {moved.max():.3g} x the bar (entry {int(moved.argmax())})")
    assert moved.max() > 100
    # the oracle takes the lower leaf index first
    orow = R.reference(*R.TIE_CASE, O.VARIANT_PCA, 27)[4]
    assert np.all(np.abs(orow - row) <= K_EXACT * R.EPS32 * maj) and not np.all(np.abs(orow - swapped[0]) <= 100 * K_EXACT * R.EPS32 * maj)
    # ndt_omp sums without weights: there the rule moves nothing past rounding
    _, lo, bo, po = R.oracle_grid(R.TIE, O.VARIANT_OMP, 27)
    assert np.allclose(R.ref_sweep(lo, bo, po, src, T, Rj, 27)[0], R.ref_sweep(lo, bo, po, src, T, Rj, 27, tie_last_first=True)[0], rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------- computeHessian and calculateScore
# Both are f64 throughout on both sides, so the oracle meets the reference within the f64 bar of tests/test_sweep_entries_gpu.py,
# (2 hits + 2 x 27) 2^-53 majorant (measured: 0.042 of it for H, 0.014 for the score); in units of 2^-24 majorant that is ~5e-9, and K_EXACT
# needs no second constant for the Hessian's recipe.  What the recipe changes is its INPUTS: the leaf's f64 inverse covariance, which far from the origin
# is asymmetric by ~1e-9 of its entries (cov(a, b) is computed from S[a] mu[b], not S[b] mu[a]) -- ref_sweep therefore reads it as
# updateHessian does, unsymmetrised; symmetrising it first moves H by 160 of these bars at offset (500, -300, 40).
def f64_bar(hits, maj):
    return (2 * hits + 2 * 27) * R.EPS64 * maj


@pytest.mark.parametrize("variant", VARIANTS)
def test_compute_hessian_and_calculate_score_oracle_against_the_reference(variant):
    worst_h, worst_s, hits_seen = (0.0,), (0.0,), set()
    for case in R.tangent_cases():
        H, mH, hits, Ho = R.hessian_reference(*case, variant)
        assert hits > 0 and np.all(np.isfinite(H)) and np.all(mH >= np.abs(H))
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.where(Ho == H, 0.0, np.abs(Ho - H) / f64_bar(hits, mH))
        worst_h = max(worst_h, (float(u.max()), int(u.argmax())) + case)
        assert np.all(np.abs(Ho - H) <= f64_bar(hits, mH)), (case, float(u.max()))
        s, ms, shits, so = R.score_reference(*case, variant)
        assert shits == hits and ms >= abs(s) > 0                      # the radius search of both hooks is the same search
        worst_s = max(worst_s, (abs(so - s) / f64_bar(shits, ms),) + case)
        assert abs(so - s) <= f64_bar(shits, ms), (case, s, so)
        hits_seen.add(hits)
        # the Hessian's recipe is not the sweep's: against the sweep's own H block (f32 covariances, f32 r) it is off by far more than this bar
        src, _, T32, _, _ = R.tangent_case(*case)
        sweep_H = R.ref_sweep(*R.oracle_grid(case[0], O.VARIANT_OMP, 27)[1:], src, T32, T32[:3, :3], 27)[0][7:]
        assert not np.all(np.abs(sweep_H - H) <= 100 * f64_bar(hits, mH))
    print(f"variant {variant}: computeHessian |oracle - ref| / f64 bar <= {worst_h[0]:.3f} at entry {worst_h[1]} of {worst_h[2:]}; "
          f"calculateScore <= {worst_s[0]:.3f} of {worst_s[1:]}")
    assert len(hits_seen) > 6


# ------------------------------------------------------------------------------------------------- the matrix is the predicate
CSRC = os.path.join(ROOT, "lv_slam_amd", "csrc")


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """tests/cpp/sweep_matrix_main.cpp, built with the sanitizers on that program alone: the rows for which each predicate says yes"""
    exe = str(tmp_path_factory.mktemp("sweep_matrix") / "sweep_matrix_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "sweep_matrix_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    t = {"sweep": set(), "euler": set(), "lean": set(), "asked": {"sweep": 0, "euler": 0, "lean": 0}}
    for l in run.stdout.splitlines():
        w = l.split()
        if w[0] == "const":
            t["it_batch"] = int(w[1])
            continue
        t["asked"][w[0]] += 1
        if int(w[-1]):
            t[w[0]].add(tuple(int(x) for x in w[1:-1]))
    return t


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_test_matrices_are_the_predicates(table):
    assert table["asked"] == {"sweep": 2 * 11 * 5 * 7, "euler": 11 * 5, "lean": 2 * 11 * 5} and table["it_batch"] == M.IT_BATCH
    assert len(set(M.SWEEP_ROWS)) == len(M.SWEEP_ROWS) == 42 and set(M.SWEEP_ROWS) == table["sweep"]
    assert len(set(M.EULER_ROWS)) == len(M.EULER_ROWS) == 8 and set(M.EULER_ROWS) == table["euler"]
    # k_align_async: every batch-mode row of sweep_exists, plus the lean bodies
    align = {(pca, K, o, 0) for pca, K, o, it in table["sweep"] if it == table["it_batch"]} | {(pca, K, o, 1) for pca, K, o in table["lean"]}
    assert len(set(M.ALIGN_ROWS)) == len(M.ALIGN_ROWS) == 20 and set(M.ALIGN_ROWS) == align
    # the two kernels outside the predicates: ndt_pca + KDTREE is exactly the row sweep_exists leaves out of an otherwise full K = 27 column,
    # and PCL's class has the one kernel
    assert M.PCA_KD_ROWS == [0, 1] and all((0, 27, o, 8) in table["sweep"] and (1, 27, o, 8) not in table["sweep"] for o in M.PCA_KD_ROWS)
    assert M.PCL_ROWS == [(27, 0)]
    assert len(M.SWEEP_ROWS) + len(M.PCA_KD_ROWS) + len(M.EULER_ROWS) + len(M.PCL_ROWS) + len(M.ALIGN_ROWS) == 73
    # the GPU tests' families are the matrix, each row once
    assert sorted(M.EXACT_BATCH + M.TOLERANCE_BATCH + M.FINE) == sorted(M.SWEEP_ROWS)


# ------------------------------------------------------------------------------------------------- the table is the matrix, the code, the binary
TABLE_HPP = os.path.join(CSRC, "ndt_sweep_exists.hpp")
KERNELS = r"\b(k_sweep_pca_kd|k_sweep|k_align_async)"


def _rows(macro):
    """the rows of one X-macro row list of the table header, as tuples of ints, in the order written: a parser of the test's own (the body of
    `#define <macro>(R)` up to the first line that does not end in a backslash, comments aside, every R(...) of it)"""
    m = re.search(r"^#define %s\(R\)((?:[^\n]*\\\n)*[^\n]*)\n" % macro, open(TABLE_HPP).read(), flags=re.M)
    body = _strip_comments(m.group(1)).replace("\\\n", " ")
    val = {"true": 1, "false": 0}
    rows = [tuple(val[x] if x in val else int(x) for x in (a.strip() for a in args.split(","))) for args in re.findall(r"\bR\(([^()]*)\)", body)]
    assert re.sub(r"\bR\([^()]*\)", "", body).strip() == "", "something in the list that is no row"
    return rows


@pytest.fixture(scope="module")
def rows():
    r = {"sweep": _rows("NDT_SWEEP_ROWS"), "kd": _rows("NDT_KD_ROWS"), "align": _rows("NDT_ALIGN_ROWS")}
    for name, width in (("sweep", 6), ("kd", 1), ("align", 4)):
        assert all(len(x) == width for x in r[name]) and len(set(r[name])) == len(r[name]), f"{name}: a row is listed twice"
    return r


@pytest.fixture(scope="module")
def tag_table(tmp_path_factory):
    """`sweep_matrix_main tags`, sanitizers on: sweep_exists(SweepTag) and align_exists(AlignTag) over every tag of a wide box, ground_sweep_exists"""
    exe = str(tmp_path_factory.mktemp("sweep_tags") / "sweep_matrix_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + CSRC, os.path.join(ROOT, "tests", "cpp", "sweep_matrix_main.cpp"), "-o", exe])
    run = subprocess.run([exe, "tags"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    t = {"tag": set(), "align": set(), "ground": set(), "asked": {"tag": 0, "align": 0, "ground": 0}}
    for l in run.stdout.splitlines():
        w = l.split()
        t["asked"][w[0]] += 1
        if int(w[-1]):
            t[w[0]].add(tuple(int(x) for x in w[1:-1]))
    return t


def _matrix_sweep_rows():
    """tests/sweep_matrix.py's four k_sweep families as rows of the table: (pca, K, it, ord, pm, gate)"""
    return ([(pca, K, it, o, 0, 0) for pca, K, o, it in M.SWEEP_ROWS] + [(0, K, M.IT_BATCH, o, 1, 0) for K, o in M.EULER_ROWS] +
            [(0, K, M.IT_BATCH, o, 2, 0) for K, o in M.PCL_ROWS] + [(0, K, M.IT_BATCH, o, 0, 1) for K, o in M.GROUND_ROWS])


def test_the_table_is_the_matrix(rows, table, tag_table):
    """1: the three row lists of ndt_sweep_exists.hpp are tests/sweep_matrix.py, each row once, and every predicate and wrapper says yes for the
    rows and for nothing else of a box wider than what exists"""
    assert sorted(rows["sweep"]) == sorted(_matrix_sweep_rows()) and len(rows["sweep"]) == 57
    assert sorted(x[0] for x in rows["kd"]) == M.PCA_KD_ROWS and len(rows["kd"]) == 2
    assert sorted(rows["align"]) == sorted(M.ALIGN_ROWS) and len(rows["align"]) == 20
    assert len(M.GROUND_ROWS) == len(set(M.GROUND_ROWS)) == 6
    assert len(rows["sweep"]) + len(rows["kd"]) + len(rows["align"]) == 79
    # Euler for four K, ground for three, PCL the single row, kd for both orders
    assert sorted({K for _, K, _, _, pm, _ in rows["sweep"] if pm == 1}) == [1, 7, 26, 27] and sorted({K for _, K, _, _, _, g in rows["sweep"] if g}) == [1, 7, 26]
    assert [r for r in rows["sweep"] if r[4] == 2] == [(0, 27, 8, 0, 2, 0)] and sorted(rows["kd"]) == [(0,), (1,)]
    # what each translation unit gets: the ORD = 1 rows (28, and the three gated ones), the ORD = 2 rows (16)
    by_ord = lambda o: [r for r in rows["sweep"] if r[3] == o] + [r for r in rows["kd"] if r[0] == o] + [r for r in rows["align"] if r[2] == o]
    assert len([r for r in by_ord(1) if not (len(r) == 6 and r[5])]) == 28 and len([r for r in by_ord(1) if len(r) == 6 and r[5]]) == 3
    assert len(by_ord(2)) == 16 and len(by_ord(0)) + len(by_ord(1)) + len(by_ord(2)) == 79
    # the predicates over the wide boxes: yes for the rows, 0 for every tag the table lacks
    assert tag_table["asked"] == {"tag": 2 * 11 * 5 * 7 * 5 * 2, "align": 2 * 11 * 5 * 2, "ground": 11 * 5}
    assert tag_table["tag"] == set(rows["sweep"]) and tag_table["align"] == set(rows["align"])
    # the wrappers are the table's families: SE(3), Euler, gated, lean
    assert table["sweep"] == {(pca, K, o, it) for pca, K, it, o, pm, g in rows["sweep"] if pm == 0 and not g}
    assert table["euler"] == {(K, o) for pca, K, it, o, pm, g in rows["sweep"] if pm == 1}
    assert tag_table["ground"] == {(K, o) for pca, K, it, o, pm, g in rows["sweep"] if g} == set(M.GROUND_ROWS)
    assert table["lean"] == {(pca, K, o) for pca, K, o, lean in rows["align"] if lean} == {(0, 7, 0), (0, 7, 1)}
    # the column FINE is gone: only the batch item size and the two fine ones occur, and k_sweep's tag derives FINE from IT
    assert {r[2] for r in rows["sweep"]} == {1, 2, M.IT_BATCH} == {1, 2, table["it_batch"]}


def _code(name):
    return _strip_comments(open(os.path.join(CSRC, name)).read())


def test_nobody_else_names_an_instantiation():
    """2: comments aside, a k_sweep< / k_sweep_pca_kd< / k_align_async< tag occurs in lv_slam_amd/csrc in the table header's three tag macros alone
    (the kernels' own definitions name no tag), the tag macros are only ever handed a row's own columns, launch_async_t< is called from the
    align rows' expansion alone, and the lean row is asked for only under lean_exists"""
    sources = sorted(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".h")))
    assert "ndt_sweep_exists.hpp" in sources and not {"ndt_ord1_list.hpp", "ndt_fast_list.hpp", "ndt_ground_list.hpp", "ndt_host_ground.hpp"} & set(sources)
    tag_macros = {"NDT_SWEEP_TAG": ("PCA, K, IT, ORD, PM, GATE", "k_sweep<PCA, K, IT, (IT != SWEEP_IT_BATCH), ORD, PM, GATE>"),
                  "NDT_KD_TAG": ("ORD", "k_sweep_pca_kd<ORD>"), "NDT_ALIGN_TAG": ("PCA, K, ORD, LEAN", "k_align_async<PCA, K, ORD, LEAN>")}
    for f in sources:
        lines = _code(f).splitlines()
        named = [l.strip() for l in lines if re.search(KERNELS + r"\s*<", l)]
        if f == "ndt_sweep_exists.hpp":
            assert sorted(named) == sorted(f"#define {m}({args}) {tag}" for m, (args, tag) in tag_macros.items())
        else:
            assert named == [], (f, named)
        for m, (args, _) in tag_macros.items():      # every use of a tag macro passes the columns of the row being expanded, never a literal
            for used in re.findall(r"\b%s\(([^()]*)\)" % m, "\n".join(lines)):
                assert used == args, (f, m, used)
    # ... and the uses sit in row expansions: `#define <row macro>(<columns>) ...` lines, and launch_async_t's own template tags
    host = _code("ndt_host_sweep.hpp")
    for l in host.splitlines():
        if re.search(r"\bNDT_(SWEEP|KD|ALIGN)_TAG\(", l):
            assert l.startswith("#define NDT_ROW(") or l.strip() == "auto kern = NDT_ALIGN_TAG(PCA, K, ORD, LEAN);", l
    assert not any(re.search(r"\bNDT_(SWEEP|KD|ALIGN)_TAG\(", _code(f)) for f in sources if f not in ("ndt_sweep_exists.hpp", "ndt_host_sweep.hpp"))
    calls = [(f, l.strip()) for f in sources for l in _code(f).splitlines() if "launch_async_t<" in l]
    assert calls == [("ndt_host_sweep.hpp", "#define NDT_ROW(PCA, K, ORD, LEAN) if (same(t, AlignTag{PCA, K, ORD, LEAN})) return launch_async_t<PCA, K, ORD, LEAN>(h, sc, L);")]
    assert re.search(r"#define NDT_ROW\(PCA, K, ORD, LEAN\)[^\n]*\n\s*NDT_ALIGN_ROWS\(NDT_ROW\)\n#undef NDT_ROW", host)
    assert "t.lean = L.lean && lean_exists(t.pca, t.K, t.ord);" in host and len(re.findall(r"\.lean\s*=[^=]", host)) == 1
    # the three translation units expand the table and nothing else: each for its own ORD
    for tu, name, x in (("mi355_ndt.hip", "ELSEWHERE", "extern template"), ("mi355_ndt_ord1.hip", "ORD1", "template"), ("mi355_ndt_fast.hip", "FAST", "template")):
        assert re.search(r"#define NDT_TU %s\n#define NDT_TU_X %s\nNDT_KERNELS_OF_TU\n" % (name, x), _code(tu)), tu
    table_hpp = _code("ndt_sweep_exists.hpp")
    in_tu = {(tu, int(o)): int(v) for tu, o, v in re.findall(r"#define NDT_ROW_IN_TU_([A-Z0-9]+)_(\d) (\d)", table_hpp)}
    assert in_tu == {(tu, o): int(o in own) for tu, own in (("ORD1", (1,)), ("FAST", (2,)), ("ELSEWHERE", (1, 2))) for o in (0, 1, 2)}


def _stubs(path):
    """the host-side launch stubs of the three kernel templates that a file defines, from nm and c++filt: [("k_sweep", (0, 7, 8, 0, 0, 0, 0)), ...]"""
    assert os.path.exists(path), f"{path}: __graft_entry__.build() leaves it"
    syms = subprocess.run(["nm", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    names = subprocess.run(["c++filt"], input=syms, capture_output=True, text=True, check=True).stdout
    val = {"true": 1, "false": 0}
    return [(k, tuple(val[x] if x in val else int(x) for x in (a.strip() for a in args.split(","))))
            for k, args in re.findall(r"\b__device_stub__" + KERNELS[2:] + r"<([^<>]*)>\(", names)]


def test_the_binary_is_the_table(rows):
    """3: the library holds a launch stub for exactly the 79 rows, and each of the three objects build() leaves defines exactly the rows of its
    own ORD: the kernels of the second sum order and of the tolerance arithmetic are compiled beside the first unit, not in it"""
    it8 = M.IT_BATCH
    want = ([("k_sweep", (pca, K, it, int(it != it8), o, pm, g)) for pca, K, it, o, pm, g in rows["sweep"]] + [("k_sweep_pca_kd", r) for r in rows["kd"]] +
            [("k_align_async", r) for r in rows["align"]])
    ord_of = lambda s: s[1][{"k_sweep": 4, "k_sweep_pca_kd": 0, "k_align_async": 2}[s[0]]]
    assert len(want) == len(set(want)) == 79
    lib = _stubs(os.path.join(ROOT, "lv_slam_amd", "libmi355ndt.so"))
    assert sorted(lib) == sorted(want)
    for obj, ords, n in (("mi355_ndt.hip.o", (0,), 32), ("mi355_ndt_ord1.hip.o", (1,), 28 + 3), ("mi355_ndt_fast.hip.o", (2,), 16)):
        got = _stubs(os.path.join(CSRC, obj))
        assert sorted(got) == sorted(s for s in want if ord_of(s) in ords) and len(got) == n, obj
