"""GPU (-m gpu): one derivative sweep (score, g[6], H[6][6]) of the real k_sweep instantiations, checked ENTRY BY ENTRY on tiny scenes, under the
exact and the tolerance arithmetic, through mi355ndt_derivatives_T (an explicit f32 pose: no pose math involved).

The other sweep tests bound the error by a fraction of the largest of the 43 numbers (1e-11 exact, 1e-5 tolerance arithmetic).  The rotation block
of H grows with |r|^2 and the translation block does not, so away from the origin such a bar does not see the translation block or most of the
translation x rotation block at all (tests/test_sweep_entries_cpu.py shows the ratios).  Here every entry has its own scale: the majorant of
tests/ndt_ref.py, the same formulas on absolute values.

  exact arithmetic (both f32 sum orders)   vs the oracle:  |dev - oracle| <= (2 hits + 14) 2^-53 majorant.  Both sides add the SAME f32 terms, in
                                           different f64 orders, fewer than `hits` additions each; ndt_pca's suffix product of weights against the
                                           nested product adds at most 7 roundings per side.
                                           vs ref_sweep:   K_EXACT 2^-24 majorant, the bar the oracle itself is held to on the CPU
  tolerance arithmetic                     vs ref_sweep:   K_TOL 2^-24 majorant; the oracle's hit count exactly

Scenes, poses and sizes: tests/ndt_ref.py (4 x 4 x 4 cells; offsets up to (500, -300, 40), where the f32 tail of a leaf's mean is ~3e-5 m; source
sizes across the 64-point tile, the 512-point item and the 2048-point chunk; a pose near the identity and one turned by 2.5 rad)."""
import numpy as np
import pytest

import ndt_ref as R
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


def engine(leaf, variant, K, arith, order=0, latency=False):
    eng = ndt.Engine(ndt.default_params(resolution=leaf, neighbor_mode=ndt.DIRECT7 if K == 7 else ndt.DIRECT1, variant=variant))
    eng.set_option(ndt.OPT_ARITH, arith)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    assert eng.get_option(ndt.OPT_ARITH) == arith and eng.get_option(ndt.OPT_F32_SUM_ORDER) == order
    if latency:
        eng.set_latency_mode(True)
    return eng


def sweeps(variant, K, arith, order=0, latency=False, slot=False):
    """every committed case through the device: yields (case, device row, device hits).  One engine per leaf size, re-targeted scene by scene."""
    engines = {}
    for sn in R.SCENES:
        sc = R.named_scene(sn)
        if sc.leaf not in engines:
            engines[sc.leaf] = engine(sc.leaf, variant, K, arith, order, latency)
        eng = engines[sc.leaf]
        if slot:
            # the scene as pair 0 of a three-slot batch (the hook serves pair 0); the neighbours have other clouds of other sizes, one source
            # longer than a chunk, so pair 0's rows past its own points must come out empty
            other = R.named_scene("far" if sn != "far" else "origin")
            nb_tgt = (other.target[:600], np.concatenate([sc.target, sc.target + np.float32([4 * sc.leaf, 0, 0])]))
            nb_src = (other.pose("near", 700)[0], np.tile(sc.pose("near", 2049)[0], (2, 1))[:2500])
            eng.batch_reserve(3, 2 * len(sc.target), 2500)
            eng.batch_set_target(0, sc.target)
            for b in (1, 2):
                eng.batch_set_target(b, nb_tgt[b - 1])
                eng.batch_set_source(b, nb_src[b - 1])
        else:
            eng.set_target(sc.target)
        for case in R.cases():
            if case[0] != sn:
                continue
            src, T, Rj = R.sweep_inputs(*case)
            if slot:
                eng.batch_set_source(0, src)
            else:
                eng.set_source(src)
            yield (case,) + R.as_row(eng.derivatives_T(T, Rj))
    for eng in engines.values():
        eng.close()


def check_exact(variant, K, order, **how):
    worst_o, worst_r, bad = 0.0, 0.0, []
    for case, row, hits in sweeps(variant, K, 0, order, **how):
        ref, maj, _, _, orow, ohits = R.reference(*case, variant, K, order)
        bar = (2 * ohits + 14) * R.EPS64 * maj
        d = np.abs(row - orow)
        with np.errstate(divide="ignore", invalid="ignore"):
            wo = float(np.max(np.where(d == 0, 0.0, d / bar)))
        wr = float(R.units(row, ref, maj).max())
        worst_o, worst_r = max(worst_o, wo), max(worst_r, wr)
        if hits != ohits or not np.all(d <= bar) or not np.all(np.abs(row - ref) <= K_EXACT * R.EPS32 * maj):
            bad.append((case, hits, ohits, wo, int(np.argmax(d - bar)), wr))
    print(f"exact variant {variant} K {K} order {order} {how}: |dev - oracle| / bar <= {worst_o:.3f}; |dev - ref| / (2^-24 majorant) <= {worst_r:.3f}")
    assert not bad, bad[:4]       # (case, hits, oracle hits, |dev - oracle| / bar, worst entry, |dev - ref| in units)


def check_tolerance(variant, K, **how):
    worst, bad = (0.0,), []
    for case, row, hits in sweeps(variant, K, 1, **how):
        ref, maj, _, _, _, ohits = R.reference(*case, variant, K)
        u = R.units(row, ref, maj)
        worst = max(worst, (float(u.max()), int(u.argmax())) + case)
        if hits != ohits or not np.all(np.abs(row - ref) <= K_TOL * R.EPS32 * maj):
            bad.append((case, hits, ohits, float(u.max()), int(u.argmax())))
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
