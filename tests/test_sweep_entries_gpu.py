"""GPU (-m gpu): one derivative sweep (score, g[6], H[6][6]) of the real k_sweep instantiations, checked ENTRY BY ENTRY on tiny scenes, under the
exact and the tolerance arithmetic, through mi355ndt_derivatives_T (an explicit f32 pose: no pose math involved).

The other sweep tests bound the error by a fraction of the largest of the 43 numbers (1e-11 exact, 1e-5 tolerance arithmetic).  The rotation block
of H grows with |r|^2 and the translation block does not, so away from the origin such a bar does not see the translation block or most of the
translation x rotation block at all (tests/test_sweep_entries_cpu.py shows the ratios).  Here every entry has its own scale: the majorant of
tests/ndt_ref.py, the same formulas on absolute values.

  exact arithmetic (both f32 sum orders)   vs the oracle:  |dev - oracle| <= (2 hits + 2 max(7, K)) 2^-53 majorant, K = the cells a search probes
                                           (14 for DIRECT1 / DIRECT7).  Both sides add the SAME f32 terms, in different f64 orders, fewer than
                                           `hits` additions each; ndt_pca's suffix product of weights against the nested product adds at most
                                           one rounding per weight and side: 7 under DIRECT7, up to K under DIRECT26 and the radius search.
                                           vs ref_sweep:   K_EXACT 2^-24 majorant, the bar the oracle itself is held to on the CPU
  tolerance arithmetic                     vs ref_sweep:   K_TOL 2^-24 majorant; the oracle's hit count exactly

Scenes, poses and sizes: tests/ndt_ref.py (4 x 4 x 4 cells; offsets up to (500, -300, 40), where the f32 tail of a leaf's mean is ~3e-5 m; source
sizes across the 64-point tile, the 512-point item and the 2048-point chunk; a pose near the identity and one turned by 2.5 rad).  DIRECT26 and the
radius search also run the "tie" scene, which decides the order rule of ndt_pca + KDTREE.

Which instantiations: tests/sweep_matrix.py, held to the predicates of lv_slam_amd/csrc by tests/test_sweep_entries_cpu.py.  The exact batch
sweeps of DIRECT1 / DIRECT7 and the tolerance batch sweeps run in the first three tests, DIRECT26, KDTREE and k_sweep_pca_kd in
test_direct26_and_kdtree_entry_by_entry, the 24 fine-item sweeps in test_fine_item_sweeps_entry_by_entry."""
import numpy as np
import pytest

import ndt_ref as R
import sweep_matrix as M
from lv_slam_amd import ndt
from oracle import oracle_py as O
from test_sweep_entries_cpu import K_EXACT

pytestmark = pytest.mark.gpu

# Tolerance arithmetic: the largest |dev - ref| / (2^-24 majorant) measured on the MI355X over every case below (single, batch slot, latency mode)
# is K_TOL_MEASURED; the bar is 4 x that, rounded up to a power of two (the f32 accumulation order changes with how hits fall on lanes).
# The operation count allows 64: about a dozen roundings per term, plus at most ~52 f32 additions per accumulator in the largest scene.
# (Against the oracle's exact recipe the same figure is 2.34, 2.75 with the other f32 sum order: fused multiply-adds round less often.)
# What the bar sees: `+ ml` for `- ml` in the mean's head / tail split moves the translation entries at offset (500, -300, 40) by 400-1,700 units,
# a dropped trace term or swapped covariance entries by 1e5 and more; the first of these passes a bar of 1e-5 of the largest entry.
K_TOL_MEASURED = 2.16           # entry g[3] of a one-hit DIRECT1 sweep at offset (500, -300, 40); with several hundred hits it stays below 1
K_TOL = 16
CONFIGS = [(O.VARIANT_OMP, 7), (O.VARIANT_OMP, 1), (O.VARIANT_PCA, 7), (O.VARIANT_PCA, 1)]
IDS = ["omp_direct7", "omp_direct1", "pca_direct7", "pca_direct1"]


MODES = {1: ndt.DIRECT1, 7: ndt.DIRECT7, 26: ndt.DIRECT26, 27: ndt.KDTREE}


def engine(leaf, variant, K, arith, order=0, latency=False):
    eng = ndt.Engine(ndt.default_params(resolution=leaf, neighbor_mode=MODES[K], variant=variant))
    eng.set_option(ndt.OPT_ARITH, arith)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    assert eng.get_option(ndt.OPT_ARITH) == arith and eng.get_option(ndt.OPT_F32_SUM_ORDER) == order
    if latency:
        eng.set_latency_mode(True)
    return eng


def sweeps(variant, K, arith, order=0, latency=False, slot=False, tie=False, served=None):
    """every committed case through the device: yields (case, device row, device hits).  One engine per leaf size, re-targeted scene by scene.
    tie: with the order-rule scene; served(engine, largest source of the batch): asked after every sweep, to assert which kernel ran."""
    engines, aligned = {}, set()
    for sn in list(R.SCENES) + ([R.TIE] if tie else []):
        sc = R.named_scene(sn)
        if sc.leaf not in engines:
            engines[sc.leaf] = engine(sc.leaf, variant, K, arith, order, latency)
        eng = engines[sc.leaf]
        if slot:
            # the scene as pair 0 of a three-slot batch (the hook serves pair 0); the neighbours have other clouds of other sizes, one source
            # longer than a chunk, so pair 0's rows past its own points must come out empty
            other = R.named_scene("far" if sn != "far" else "origin")
            nb_tgt = (other.target[:600], np.concatenate([sc.target, sc.target + np.float32([4 * sc.leaf, 0, 0])]))
            nb_src = (other.pose("near", 700)[0], np.tile((sc if sn != R.TIE else R.named_scene(R.BIG_SCENE)).pose("near", 2049)[0], (2, 1))[:2500])
            eng.batch_reserve(3, max(2 * len(sc.target), 600), 2500)
            eng.batch_set_target(0, sc.target)
            for b in (1, 2):
                eng.batch_set_target(b, nb_tgt[b - 1])
                eng.batch_set_source(b, nb_src[b - 1])
        else:
            eng.set_target(sc.target)
        for case in R.cases(tie):
            if case[0] != sn:
                continue
            src, T, Rj = R.sweep_inputs(*case)
            if slot:
                eng.batch_set_source(0, src)
            else:
                eng.set_source(src)
            if served is not None and sn not in aligned:
                # (mi355ndt_get_partial_rows answers once the bound clouds have been aligned; the hook's own sweep then re-sizes the rows)
                aligned.add(sn)
                eng.batch_align(np.eye(4, dtype=np.float32)) if slot else eng.align(np.eye(4, dtype=np.float32))
            res = R.as_row(eng.derivatives_T(T, Rj))
            if served is not None:
                served(eng, max(len(src), 2500) if slot else len(src))
            yield (case,) + res
    for eng in engines.values():
        eng.close()


def check_exact(variant, K, order, **how):
    worst_o, worst_r, bad = (0.0,), (0.0,), []
    for case, row, hits in sweeps(variant, K, 0, order, **how):
        ref, maj, _, _, orow, ohits = R.reference(*case, variant, K, order)
        bar = (2 * ohits + 2 * max(7, K)) * R.EPS64 * maj
        d = np.abs(row - orow)
        with np.errstate(divide="ignore", invalid="ignore"):
            uo = np.where(d == 0, 0.0, d / bar)
        ur = R.units(row, ref, maj)
        wo, wr = float(uo.max()), float(ur.max())
        worst_o, worst_r = max(worst_o, (wo, int(uo.argmax())) + case), max(worst_r, (wr, int(ur.argmax())) + case)
        if hits != ohits or not np.all(d <= bar) or not np.all(np.abs(row - ref) <= K_EXACT * R.EPS32 * maj):
            bad.append((case, hits, ohits, wo, int(np.argmax(d - bar)), wr))
    how = {k: v for k, v in how.items() if k != "served"}
    print(f"exact variant {variant} K {K} order {order} {how}: |dev - oracle| / bar <= {worst_o[0]:.3f} at entry {worst_o[1:2]} of {worst_o[2:]}; "
          f"|dev - ref| / (2^-24 majorant) <= {worst_r[0]:.3f} at entry {worst_r[1:2]} of {worst_r[2:]}")
    assert not bad, bad[:4]       # (case, hits, oracle hits, |dev - oracle| / bar, worst entry, |dev - ref| in units)


def check_tolerance(variant, K, **how):
    worst, bad = (0.0,), []
    for case, row, hits in sweeps(variant, K, 1, **how):
        ref, maj, _, _, _, ohits = R.reference(*case, variant, K)
        u = R.units(row, ref, maj)
        worst = max(worst, (float(u.max()), int(u.argmax())) + case)
        if hits != ohits or not np.all(np.abs(row - ref) <= K_TOL * R.EPS32 * maj):
            bad.append((case, hits, ohits, float(u.max()), int(u.argmax())))
    how = {k: v for k, v in how.items() if k != "served"}
    print(f"tolerance variant {variant} K {K} {how}: |dev - ref| / (2^-24 majorant) <= {worst[0]:.3f} at entry {worst[1]} of {worst[2:]}")
    assert not bad, bad[:4]       # (case, hits, oracle hits, |dev - ref| in units, worst entry)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("variant,K", CONFIGS, ids=IDS)
def test_exact_arithmetic_entry_by_entry(variant, K, order):
    check_exact(variant, K, order)


@pytest.mark.parametrize("variant,K", CONFIGS, ids=IDS)
def test_tolerance_arithmetic_entry_by_entry(variant, K):
    check_tolerance(variant, K)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("variant,K", CONFIGS, ids=IDS)
def test_as_a_slot_of_a_batch_entry_by_entry(variant, K, arith):
    if arith == 0:
        check_exact(variant, K, 0, slot=True)
    else:
        check_tolerance(variant, K, slot=True)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("variant,K", CONFIGS, ids=IDS)
def test_latency_mode_entry_by_entry(variant, K, arith):
    """mi355ndt_set_latency_mode: the hook sizes its rows in prep_align_ws like an align, so these few-point sweeps run the fine-item kernels"""
    if arith == 0:
        check_exact(variant, K, 0, latency=True)
    else:
        check_tolerance(variant, K, latency=True)


# ---------------------------------------------------------------------------------------- every other instantiation of the k_sweep family
# DIRECT26 and the radius search, both classes, both f32 sum orders: the rows of the matrix with K = 26 / 27, and the literal kernel of
# ndt_pca + KDTREE (k_sweep_pca_kd), for which sweep_exists has no row.
WIDE_ROWS = [r for r in M.EXACT_BATCH if r[1] in (26, 27)] + [(1, 27, o, M.IT_BATCH) for o in M.PCA_KD_ROWS]
SLOT = pytest.mark.parametrize("slot", [False, True], ids=["single", "slot0of3"])


def batch_rows(n):
    """rows per pair of a batch-mode sweep whose largest source has n points (prep_align_ws): four quarters per 2,048-point chunk"""
    return 4 * max(1, -(-n // 2048))


@SLOT
@pytest.mark.parametrize("row", WIDE_ROWS, ids=M.row_id)
def test_direct26_and_kdtree_entry_by_entry(row, slot):
    pca, K, order, it = row

    def served(eng, n):
        assert eng.partial_rows().shape[1] == batch_rows(n)

    check_exact(pca, K, order, slot=slot, tie=True, served=served)


@SLOT
@pytest.mark.parametrize("row", M.FINE, ids=M.row_id)
def test_fine_item_sweeps_entry_by_entry(row, slot, monkeypatch):
    """latency mode at both tile counts (MI355NDT_FINE_TILES, read when the engine is created), both f32 sum orders and the tolerance arithmetic.
    A fine sweep stores one row per block of four items, 256 x tiles points: the row count says that the fine kernels served the call
    (prep_align_ws), and it differs from the batch mode's at every size here."""
    pca, K, order, tiles = row
    monkeypatch.setenv("MI355NDT_FINE_TILES", str(tiles))

    def served(eng, n):
        rows = eng.partial_rows().shape[1]
        assert rows == max(1, -(-n // (256 * tiles))) and rows != batch_rows(n), (rows, n)

    print(f"fine items of {tiles} tile(s): ", end="")
    if order == 2:
        check_tolerance(pca, K, latency=True, slot=slot, served=served)
    else:
        check_exact(pca, K, order, latency=True, slot=slot, served=served)


@pytest.mark.parametrize("order", M.PCA_KD_ROWS)
def test_the_tie_scene_on_the_literal_kernel(order):
    """ndt_pca + KDTREE on the scene whose first point has two leaves at the same f32 squared distance: the device takes the lower leaf index
    first, as the oracle and the reference do, and is far from the sums of the other rule"""
    sc = R.named_scene(R.TIE)
    src, T, Rj = R.sweep_inputs(*R.TIE_CASE)
    ref, maj, _, _, orow, ohits = R.reference(*R.TIE_CASE, O.VARIANT_PCA, 27, order)
    _, leaves, bounds, prm = R.oracle_grid(R.TIE, O.VARIANT_PCA, 27)
    swapped = R.ref_sweep(leaves, bounds, prm, src, T, Rj, 27, tie_last_first=True)[0]
    eng = engine(sc.leaf, O.VARIANT_PCA, 27, 0, order)
    eng.set_target(sc.target)
    eng.set_source(src)
    row, hits = R.as_row(eng.derivatives_T(T, Rj))
    eng.close()
    d = np.abs(row - orow)
    bar = (2 * ohits + 2 * 27) * R.EPS64 * maj
    print(f"tie, order {order}: |dev - oracle| / bar <= {np.max(np.where(d == 0, 0.0, d / bar)):.3f}; |dev - ref| / (2^-24 majorant) <= {R.units(row, ref, maj).max():.3f}; "
          f"|dev - other rule| / (2^-24 majorant) = {R.units(row, swapped, maj).max():.3g}")
    assert hits == ohits == 8 and np.all(d <= bar) and np.all(np.abs(row - ref) <= K_EXACT * R.EPS32 * maj)
    assert R.units(row, swapped, maj).max() > 100 * K_EXACT


# ---------------------------------------------------------------------------------------- computeHessian (k_hessian), calculateScore (k_calc_score)
ALL_SEARCHES = [(v, K) for v in (O.VARIANT_OMP, O.VARIANT_PCA) for K in (1, 7, 26, 27)]


@pytest.mark.parametrize("variant,K", ALL_SEARCHES, ids=[f"{'pca' if v else 'omp'}_{M.NAMES[K]}" for v, K in ALL_SEARCHES])
def test_compute_hessian_and_calculate_score_entry_by_entry(variant, K):
    """mi355ndt_compute_hessian (impl2:622-714) and mi355ndt_calculate_score (impl2:1006-1040) on the tiny scenes, under every search method and
    both classes -- the radius search serves both whatever the method is, and neither reads ndt_pca's weights.  f64 on every side: against the
    oracle and against tests/ndt_ref.py the bar is the f64 one, (2 hits + 2 x 27) 2^-53 majorant, entry by entry (for the score: of the score's own
    majorant); K_EXACT 2^-24 majorant, the bar of the sweeps, holds with it a fortiori."""
    worst = {"H oracle": (0.0,), "H ref": (0.0,), "score oracle": (0.0,), "score ref": (0.0,)}
    bad, engines = [], {}
    for sn in R.SCENES:
        sc = R.named_scene(sn)
        if sc.leaf not in engines:
            engines[sc.leaf] = engine(sc.leaf, variant, K, 0)
        eng = engines[sc.leaf]
        eng.set_target(sc.target)
        for case in R.tangent_cases():
            if case[0] != sn:
                continue
            src, p, T32, _, cloud = R.tangent_case(*case)
            Href, mH, hits, Ho = R.hessian_reference(*case, variant)
            sref, ms, _, so = R.score_reference(*case, variant)
            eng.set_source(src)
            eng.align(T32)                               # (calculateScore reads the Gauss constants the last align left: those of the parameters)
            H = eng.compute_hessian(p).ravel()
            s = eng.calculate_score(cloud)
            bar, sbar = (2 * hits + 54) * R.EPS64 * mH, (2 * hits + 54) * R.EPS64 * ms
            for name, d, b in (("H oracle", np.abs(H - Ho), bar), ("H ref", np.abs(H - Href), bar), ("score oracle", np.abs(s - so), sbar), ("score ref", np.abs(s - sref), sbar)):
                with np.errstate(divide="ignore", invalid="ignore"):
                    u = np.atleast_1d(np.where(d == 0, 0.0, d / b))
                worst[name] = max(worst[name], (float(u.max()), int(u.argmax())) + case)
                if not np.all(d <= b):
                    bad.append((name, case, float(u.max()), int(u.argmax())))
            assert np.all(np.abs(H - Href) <= K_EXACT * R.EPS32 * mH)
    for eng in engines.values():
        eng.close()
    print(f"variant {variant} K {K}: " + "; ".join(f"|dev - {k}| / f64 bar <= {w[0]:.3f} at entry {w[1]} of {w[2:]}" for k, w in worst.items()))
    assert not bad, bad[:4]
