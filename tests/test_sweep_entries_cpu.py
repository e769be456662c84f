"""CPU: the float64 reference of one derivative sweep (tests/ndt_ref.py) against the oracle, entry by entry, on the tiny scenes of
tests/test_sweep_entries_gpu.py -- the guard of the reference itself and the anchor of that file's bars.

The oracle evaluates the reference's f32 recipe, ref_sweep the mathematics in f64, so what separates them is the recipe's own rounding: every one of
the 43 numbers (score, g, H) must agree within K_EXACT * 2^-24 * majorant of THAT entry.  The scenes are also shown not to be vacuous, on the
reference alone: partial neighbourhoods, ndt_pca weights of 0 and of >= 100, Hessian entries far below the largest one, the asymmetry of H."""
import numpy as np
import pytest

import ndt_ref as R
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
