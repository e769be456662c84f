"""GPU (-m gpu): the engine's record of what its resident grids hold (lv_slam_amd/csrc/ndt_grid_state.hpp, ensure_grids) walked through every
call that asks for grids, on ONE engine: after each step the result equals, word for word, that of a fresh engine given only what the step
needs, and the number of target builds so far is the one the engine had before the record existed (PARENT_BUILDS).  Then
mi355ndt_batch_set_clouds refused half way through its arguments: nothing has changed.  (The header's rules alone: tests/test_grid_state_cpu.py.)
"""
import numpy as np
import pytest

from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu

KW = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7, variant=ndt.VARIANT_OMP)
KW_KD = dict(KW, neighbor_mode=ndt.KDTREE)
POSE = np.array([0.05, -0.02, 0.01, 0.002, -0.001, 0.01])
# build_launches after each step of walk(), measured with the library of the commit before ndt_grid_state.hpp existed (MI355NDT_LIB pointing at a
# build of it, this module's walk() run once on an MI355X) -- not with the code under test.  Reading that commit gives the same numbers: setInputTarget
# builds (1); calculateScore wants the live flavour (2) and finds it twice (2, 2: computeHessian too); the align is served by it (2); the tolerance
# arithmetic wants its records (3); calculateScore rebuilds live and the align rebuilds the records (4, 5); KDTREE wants centroids (6); DIRECT7 its
# records again (7); the fitness score takes any grid (7); a new target is built once, by setInputTarget (8, 8).
PARENT_BUILDS = [1, 2, 2, 2, 2, 3, 4, 5, 6, 7, 7, 8, 8]


def clouds(seed):
    tgt, src, _ = synth.make_pair(seed, 256, n_beams=32)
    return tgt.numpy(), src.numpy()


def words(r):
    return (r["final"].tobytes(), r["score"], r["iterations"], r["converged"], r["sweeps"], r["hits_last"], r["trans_probability"], r["status"])


def fresh(kw, arith, tgt, src=None):
    e = ndt.Engine(ndt.default_params(**kw))
    e.set_option(ndt.OPT_ARITH, arith)
    e.set_target(tgt)
    if src is not None:
        e.set_source(src)
    return e


def walk(tgt, src, tgt2):
    """[(step, result)] and the build count after each step, of one engine taken through every call that asks for grids"""
    G = synth.default_guess()
    e = ndt.Engine(ndt.default_params(**KW))
    e.profile_enable(True)
    out, builds = [], []

    def step(name, value):
        out.append((name, value))
        builds.append(e.profile_get()["build_launches"])

    e.set_target(tgt); e.set_source(src)
    step("1 align", words(e.align(G)))
    step("2 calculate_score", e.calculate_score(src))
    step("3 calculate_score", e.calculate_score(src))
    step("4 compute_hessian", e.compute_hessian(POSE).tobytes())
    step("5 align", words(e.align(G)))
    e.set_option(ndt.OPT_ARITH, 1)
    step("6 arith 1: align", words(e.align(G)))
    step("7 calculate_score", e.calculate_score(src))
    step("7 align", words(e.align(G)))
    e.set_params(ndt.default_params(**KW_KD))
    step("8 KDTREE: align", words(e.align(G)))
    e.set_params(ndt.default_params(**KW))
    step("9 DIRECT7: align", words(e.align(G)))
    step("10 fitness_score", e.fitness_score())
    e.set_target(tgt2)
    step("11 set_target", None)
    step("11 new target: align", words(e.align(G)))
    return out, builds


def test_walked_engine_matches_fresh_engines_and_the_parents_build_counts():
    tgt, src = clouds(1)
    tgt2 = clouds(2)[0]
    G = synth.default_guess()
    out, builds = walk(tgt, src, tgt2)
    print("build_launches after each step:", builds)
    align0 = words(fresh(KW, 0, tgt, src).align(G))
    align1 = words(fresh(KW, 1, tgt, src).align(G))
    fit = fresh(KW, 1, tgt, src)
    fit.align(G)
    expected = [
        ("1 align", align0),
        ("2 calculate_score", fresh(KW, 0, tgt).calculate_score(src)),
        ("3 calculate_score", fresh(KW, 0, tgt).calculate_score(src)),
        ("4 compute_hessian", fresh(KW, 0, tgt, src).compute_hessian(POSE).tobytes()),
        ("5 align", align0),
        ("6 arith 1: align", align1),
        ("7 calculate_score", fresh(KW, 1, tgt).calculate_score(src)),
        ("7 align", align1),
        ("8 KDTREE: align", words(fresh(KW_KD, 1, tgt, src).align(G))),
        ("9 DIRECT7: align", align1),
        ("10 fitness_score", fit.fitness_score()),
        ("11 set_target", None),
        ("11 new target: align", words(fresh(KW, 1, tgt2, src).align(G))),
    ]
    assert align0[0] != align1[0] or align0[1] != align1[1]                 # (the two arithmetics are told apart by their words)
    for (name, got), (ename, want) in zip(out, expected):
        assert name == ename
        assert got == want, name
    assert builds == PARENT_BUILDS


def test_refused_batch_set_clouds_changes_nothing():
    """9 pairs = two upload groups.  New clouds for pairs 0-7 and a NULL pointer with a count for pair 8: refused (MI355NDT_ERR_BAD_ARG) before any
    group is staged, so the next align still returns the first one's words.  (Refused by the second group's staging alone, the first group's
    rows would hold the new clouds under the old counts and grids.)"""
    a, b = [clouds(s) for s in (1, 2)]
    first = [np.ascontiguousarray(c, np.float32) for c in a]
    second = [np.ascontiguousarray(c, np.float32) for c in b]
    B = 9
    G = synth.default_guess()
    e = ndt.Engine(ndt.default_params(**KW))
    e.batch_reserve(B, max(len(first[0]), len(second[0])), max(len(first[1]), len(second[1])))
    ptrs = lambda c: [c.ctypes.data] * B
    e.batch_set_clouds_raw(0, ptrs(first[0]), [len(first[0])] * B, ptrs(first[1]), [len(first[1])] * B, 12)
    before = [words(r) for r in e.batch_align(G)]
    with pytest.raises(ndt.NDTError) as err:
        e.batch_set_clouds_raw(0, ptrs(second[0])[:8] + [0], [len(second[0])] * 8 + [5], ptrs(second[1]), [len(second[1])] * B, 12)
    assert err.value.code == -2
    assert [words(r) for r in e.batch_align(G)] == before
    # ... and a call that is accepted does change the batch
    e.batch_set_clouds_raw(0, ptrs(second[0]), [len(second[0])] * B, ptrs(second[1]), [len(second[1])] * B, 12)
    after = [words(r) for r in e.batch_align(G)]
    assert after != before and after == [words(fresh(KW, 0, second[0], second[1]).align(G))] * B
