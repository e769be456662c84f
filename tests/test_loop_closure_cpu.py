"""CPU: the loop-closure selection rules of lv_slam_amd/loop_closure.py (LoopDetector::matching / matching_and_bow,
loop_detector.hpp:148-281) on hand-made per-candidate results, the loop guess, and the batched fitness entry point's handle check."""
import ctypes as C

import numpy as np
import pytest

from lv_slam_amd import loop_closure as LC
from lv_slam_amd import ndt

DBL_MAX = 1.7976931348623157e308


def poses(n):
    return [np.eye(4, dtype=np.float32) * (k + 1) for k in range(n)]      # distinguishable stand-ins for final transforms


def test_matching_picks_lowest_converged_and_ties_go_to_the_later_candidate():
    F = poses(5)
    idx, pose, best, aligns = LC.select_matching([True, True, False, True, True], [0.3, 0.2, 0.01, 0.2, 0.4], F, 0.5)
    assert idx == 3 and np.array_equal(pose, F[3])                         # 0.2 twice: the later one replaces the earlier (score > best skips)
    assert best == 0.2 and aligns == 5                                     # the non-converged 0.01 is skipped


def test_matching_threshold_and_no_converged_candidate():
    F = poses(3)
    assert LC.select_matching([True, True, True], [0.7, 0.6, 0.9], F, 0.5) == (None, None, 0.6, 3)
    assert LC.select_matching([False, False], [0.1, 0.2], F, 0.5) == (None, None, DBL_MAX, 2)
    # a converged candidate with nothing in range (DBL_MAX) is taken as best -- and then fails the threshold
    assert LC.select_matching([True], [DBL_MAX], F, 0.5) == (None, None, DBL_MAX, 1)
    idx, pose, best, aligns = LC.select_matching([True], [0.5], F, 0.5)    # best <= thresh: found
    assert (idx, best, aligns) == (0, 0.5, 1) and np.array_equal(pose, F[0])


def test_matching_and_bow_breaks_on_low_bow_score():
    F = poses(5)
    conv = [True] * 5
    scores = [0.9, 0.8, 0.1, 0.7, 0.6]
    bow = [(0.5, 0), (0.3, 1), (0.039, 2), (0.2, 3)]                       # the third entry's BoW score ends the walk: candidate 2 is never aligned
    assert LC.select_matching_and_bow(conv, scores, F, bow, 0.5) == (None, None, 0.8, 2)
    idx, pose, best, aligns = LC.select_matching_and_bow(conv, scores, F, [(0.04, 2)] + bow, 0.5)   # 0.04 itself does not break
    assert (idx, best, aligns) == (2, 0.1, 1) and np.array_equal(pose, F[2])


def test_matching_and_bow_stops_after_threshold_and_counts_aligns():
    F = poses(5)
    conv = [True, False, True, True, True]
    scores = [0.9, 0.05, 0.3, 0.2, 0.1]
    bow = [(0.6, 0), (0.5, 1), (0.4, 2), (0.3, 3), (0.2, 4)]
    # 0: best 0.9; 1: not converged; 2: best 0.3 <= 0.5 -> the walk ends before 3 (whose 0.2 would have been better)
    idx, pose, best, aligns = LC.select_matching_and_bow(conv, scores, F, bow, 0.5)
    assert (idx, best, aligns) == (2, 0.3, 3) and np.array_equal(pose, F[2])
    # a tighter threshold walks all five and finds nothing within it
    assert LC.select_matching_and_bow(conv, scores, F, bow, 0.05) == (None, None, 0.1, 5)
    idx, pose, best, aligns = LC.select_matching_and_bow(conv, scores, F, bow, 0.1)
    assert (idx, best, aligns) == (4, 0.1, 5) and np.array_equal(pose, F[4])
    assert LC.select_matching_and_bow(conv, scores, F, [], 0.5) == (None, None, DBL_MAX, 0)


def test_loop_guess_matches_numpy_restatement():
    rng = np.random.default_rng(3)

    def iso(rng):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = rng.uniform(-200, 200, 3)
        return T

    for _ in range(20):
        N, Cp = iso(rng), iso(rng)
        G = LC.loop_guess(N, Cp)
        want = (np.linalg.inv(N) @ Cp).astype(np.float32)
        want[2, 3] = 0.0
        assert G.dtype == np.float32 and G.shape == (4, 4)
        assert G[2, 3] == 0.0 and np.array_equal(G[3], np.float32([0, 0, 0, 1]))
        assert np.abs(G - want).max() <= 1e-4
    with pytest.raises(ValueError):
        LC.loop_guess(np.eye(3), np.eye(4))


def test_verify_candidates_without_candidates_needs_no_engine():
    assert LC.verify_candidates(None, np.zeros((10, 3), np.float32), [], np.zeros((0, 4, 4), np.float32)) == (None, None, DBL_MAX, 0)


def test_batch_fitness_scores_bad_handle_without_gpu():
    lib = ndt.load_library()
    s = (C.c_double * 4)()
    n = (C.c_longlong * 4)()
    assert lib.mi355ndt_batch_fitness_scores(None, None, 1.0, C.cast(s, C.c_void_p), C.cast(n, C.c_void_p)) == -1
    assert "mi355ndt_batch_fitness_scores" in ndt.SYMBOLS
