"""No GPU: mi355ndt_information_matrix (the weighting half of InformationMatrixCalculator::calc_information_matrix, host arithmetic) against
an independent NumPy statement of the reference's formula, and information.InformationMatrixCalculator's calling pattern with a recording
stand-in engine."""
import ctypes as C

import numpy as np
import pytest

from lv_slam_amd import information, ndt

DBL_MAX = 1.7976931348623157e308
DEFAULTS = dict(use_const_inf_matrix=0, const_stddev_x=0.5, const_stddev_q=0.1, var_gain_a=20.0, min_stddev_x=0.1, max_stddev_x=5.0,
                min_stddev_q=0.05, max_stddev_q=0.2, fitness_score_thresh=0.5)       # information_matrix_calculator.cpp:11-20
SCORES = [0.0, 1e-9, 1e-4, 0.01, 0.1, 0.25, 0.49, 0.4999999, 0.5, 0.5000001, 0.51, 0.75, 1.0, 2.5, 10.0, 1e3, 1e6, 1e300, DBL_MAX]
PARAM_SETS = [{}, dict(fitness_score_thresh=2.5), dict(var_gain_a=1.0, min_stddev_x=0.01, max_stddev_x=50.0, min_stddev_q=0.2, max_stddev_q=0.9),
              dict(var_gain_a=3.7, fitness_score_thresh=0.05)]


def weight(a, max_x, min_y, max_y, x):
    """information_matrix_calculator.hpp:40-44, in f64"""
    with np.errstate(over="ignore"):
        y = (1.0 - np.exp(np.float64(-a) * np.float64(x))) / (1.0 - np.exp(np.float64(-a) * np.float64(max_x)))
    return np.float64(min_y) + (np.float64(max_y) - np.float64(min_y)) * y


def expected_weights(prm, score):
    p = dict(DEFAULTS, **prm)
    wx = weight(p["var_gain_a"], p["fitness_score_thresh"], p["min_stddev_x"] ** 2, p["max_stddev_x"] ** 2, score)
    wq = weight(p["var_gain_a"], p["fitness_score_thresh"], p["min_stddev_q"] ** 2, p["max_stddev_q"] ** 2, score)
    return wx, wq


def test_defaults_are_the_constructors():
    p = ndt.default_inf_params()
    assert {k: getattr(p, k) for k, _ in ndt.InfParams._fields_} == DEFAULTS
    with pytest.raises(TypeError):
        ndt.default_inf_params(no_such_field=1.0)


@pytest.mark.parametrize("prm", PARAM_SETS)
def test_matches_numpy_statement(prm):
    for s in SCORES:
        M = ndt.information_matrix(s, **prm)
        assert M.shape == (6, 6) and M.dtype == np.float64
        off = M.copy()
        np.fill_diagonal(off, 0.0)
        assert (off == 0.0).all(), s                              # off-block and off-diagonal entries: exactly 0
        wx, wq = expected_weights(prm, s)
        for k in range(6):
            w = wx if k < 3 else wq
            d = M[k, k]
            assert d == M[0 if k < 3 else 3, 0 if k < 3 else 3]
            # one f32 ulp of the weight (the float store; leaves room for libm differences in exp)
            assert abs(d - 1.0 / w) <= 2.0 ** -23 * (1.0 / w), (s, k, d, 1.0 / w)
            # ... and the f32 rounding is really there: the entry is 1.0 / (double)(float)x for an f32 x
            x32 = np.float32(1.0 / d)
            assert any(1.0 / np.float64(c) == d for c in (x32, np.nextafter(x32, np.float32(0)), np.nextafter(x32, np.float32(np.inf)))), (s, k, d)


def test_no_clamp_above_the_threshold():
    """A DBL_MAX score (nothing in range) gives a weight strictly above max_var: the reference does not clamp."""
    M = ndt.information_matrix(DBL_MAX)
    assert 1.0 / M[0, 0] > 5.0 ** 2 and 1.0 / M[3, 3] > 0.2 ** 2
    at = ndt.information_matrix(0.5)                              # at the threshold: max_var (to the float's rounding)
    assert abs(1.0 / at[0, 0] - 25.0) <= 25.0 * 2.0 ** -23
    lo = ndt.information_matrix(0.0)                              # a perfect score: min_var
    assert lo[0, 0] == 1.0 / np.float64(np.float32(0.1 ** 2)) and lo[3, 3] == 1.0 / np.float64(np.float32(0.05 ** 2))


def test_constant_branch_divides_by_the_stddev():
    for s in (0.0, 0.3, DBL_MAX):
        M = ndt.information_matrix(s, use_const_inf_matrix=1, const_stddev_x=0.5, const_stddev_q=0.1)
        exp = np.diag([1 / 0.5] * 3 + [1 / 0.1] * 3)
        assert np.array_equal(M, exp)
        assert M[0, 0] != 1 / 0.5 ** 2


def test_null_arguments():
    L = ndt.load_library()
    p = ndt.default_inf_params()
    out = np.zeros(36)
    assert L.mi355ndt_information_matrix(None, 0.1, out.ctypes.data_as(C.c_void_p)) == -2
    assert L.mi355ndt_information_matrix(C.byref(p), 0.1, None) == -2
    L.mi355ndt_inf_params_default(None)                           # ignored
    with pytest.raises(TypeError):
        ndt.information_matrix(0.1, p, var_gain_a=2.0)


class RecordingEngine:
    def __init__(self, scores):
        self.scores, self.calls = scores, []

    def keyframe_fitness_scores(self, ids1, ids2, relposes, max_range=float("inf")):
        self.calls.append((list(ids1), list(ids2), np.asarray(relposes).copy(), max_range))
        n = len(ids1)
        return np.asarray(self.scores[:n], np.float64), np.ones(n, np.int64)


def test_calculator_makes_one_call_for_n_edges():
    scores = [0.01, 0.2, DBL_MAX, 0.7]
    eng = RecordingEngine(scores)
    calc = information.InformationMatrixCalculator(max_range=4.0, fitness_score_thresh=2.5)
    assert calc.params.fitness_score_thresh == 2.5 and calc.params.var_gain_a == 20.0 and not calc.use_const_inf_matrix
    rel = [np.eye(4) * (k + 1) for k in range(4)]
    edges = [(k, k + 1, rel[k]) for k in range(4)]
    out = calc.calc_information_matrices(eng, iter(edges))
    assert len(eng.calls) == 1
    ids1, ids2, P, mr = eng.calls[0]
    assert ids1 == [0, 1, 2, 3] and ids2 == [1, 2, 3, 4] and mr == 4.0 and np.array_equal(P, np.stack(rel))
    assert len(out) == 4
    for m, s in zip(out, scores):
        assert np.array_equal(m, ndt.information_matrix(s, fitness_score_thresh=2.5))
    one = calc.calc_information_matrix(eng, 7, 3, rel[0])
    assert len(eng.calls) == 2 and eng.calls[1][0] == [7] and eng.calls[1][1] == [3]
    assert np.array_equal(one, ndt.information_matrix(scores[0], fitness_score_thresh=2.5))
    assert calc.calc_information_matrices(eng, []) == [] and len(eng.calls) == 2


def test_calculator_constant_mode_makes_no_call():
    eng = RecordingEngine([0.1] * 3)
    calc = information.InformationMatrixCalculator(use_const_inf_matrix=1)
    out = calc.calc_information_matrices(eng, [(0, 1, np.eye(4)), (1, 2, np.eye(4))])
    assert eng.calls == [] and len(out) == 2
    assert all(np.array_equal(m, np.diag([2.0] * 3 + [10.0] * 3)) for m in out)
    assert np.array_equal(calc.calc_information_matrix(eng, 0, 1, np.eye(4)), out[0]) and eng.calls == []
