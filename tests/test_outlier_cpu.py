"""CPU: the restatement mi355ndt_prefilter_outliers is held to (tools/outlier_ref.py) against hand-worked cases and against an independent
formulation (a full sort per row, Python-loop sums), and the parts of the new C ABI that need no device."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("outlier_ref")
NAN = float("nan")


def f32(*rows):
    return np.array(rows, np.float32).reshape(-1, 3)


def line(*xs):
    return f32(*[(x, 0, 0) for x in xs])


def test_five_collinear_points_by_hand():
    # x = 0 1 2 4 8, mean_k = 2: the two nearest others of each point are (1,2) (1,1) (1,2) (2,3) (4,6)
    r = R.statistical(line(0, 1, 2, 4, 8), mean_k=2, stddev_mul=1.0)
    assert r["dist"].tobytes() == np.array([1.5, 1.0, 1.5, 2.5, 5.0], np.float32).tobytes()
    assert (r["n_in"], r["n_valid"]) == (5, 5)
    total, sq = 1.5 + 1.0 + 1.5 + 2.5 + 5.0, 2.25 + 1.0 + 2.25 + 6.25 + 25.0      # 11.5, 36.75: exact in f64
    assert r["mean"] == total / 5
    assert r["stddev"] == math.sqrt((sq - total * total / 5) / 4)
    assert r["threshold"] == total / 5 + 1.0 * math.sqrt((sq - total * total / 5) / 4)    # 2.3 + 1.6047 = 3.9047: only x = 8 is beyond
    assert r["kept"].tolist() == [0, 1, 2, 3]
    # the multiplier moves the threshold, not the distances
    assert R.statistical(line(0, 1, 2, 4, 8), mean_k=2, stddev_mul=2.0)["kept"].tolist() == [0, 1, 2, 3, 4]
    assert R.statistical(line(0, 1, 2, 4, 8), mean_k=2, stddev_mul=-0.5)["kept"].tolist() == [1]     # threshold 1.4976...: 1.5 is beyond


def test_a_cloud_of_mean_k_points_has_nothing_valid():
    r = R.statistical(line(0, 1, 5), mean_k=3)                # nearestKSearch(4) over 3 points comes back short
    assert r["n_valid"] == 0 and not r["dist"].any()
    assert math.isnan(r["threshold"]) and r["kept"].tolist() == [0, 1, 2]
    r = R.statistical(line(0, 1, 5, 100), mean_k=3)           # one more point and every one is valid
    assert r["n_valid"] == 4 and r["dist"].tobytes() == np.array([106 / 3, 104 / 3, 104 / 3, 294 / 3], np.float32).tobytes()


def test_exactly_one_valid_point_gives_a_nan_threshold():
    # (n_valid - 1) = 0: var = 0 / 0.  Through the filter n_valid is 0 or at least mean_k + 1 >= 2, so the rule is checked on the statistics alone
    st = R.statistics(np.array([0.0, 2.5, 0.0], np.float32), 1, 1.0)
    assert st["mean"] == 2.5 and math.isnan(st["stddev"]) and math.isnan(st["threshold"])
    st = R.statistics(np.zeros(3, np.float32), 0, 1.0)
    assert math.isnan(st["mean"]) and math.isnan(st["threshold"])


def test_coincident_points():
    p = f32((0, 0, 0), (0, 0, 0), (0, 0, 0), (3, 0, 0))
    r = R.statistical(p, mean_k=2)
    assert r["dist"].tolist() == [0.0, 0.0, 0.0, 3.0]
    assert (r["mean"], r["stddev"], r["threshold"]) == (0.75, 1.5, 2.25)       # sum 3, sq 9: var = (9 - 9/4) / 3
    assert r["kept"].tolist() == [0, 1, 2]
    assert R.radius(p, 1.0, 2)["kept"].tolist() == [0, 1, 2]                    # coincident points count as neighbours
    assert R.radius(p, 1.0, 3)["kept"].tolist() == []


def test_a_nan_point_is_kept_by_statistical_and_removed_by_radius():
    p = f32((0, 0, 0), (1, 0, 0), (NAN, 0, 0), (2, 0, 0), (50, 0, 0))
    r = R.statistical(p, mean_k=2, stddev_mul=0.5)
    assert r["n_valid"] == 4 and r["dist"].tolist() == [1.5, 1.0, 0.0, 1.5, 48.5]
    assert r["kept"].tolist() == [0, 1, 2, 3]                                   # dist 0 is below any positive threshold
    assert R.radius(p, 1.5, 1)["kept"].tolist() == [0, 1, 3]
    assert R.radius(p, 1.5, 0)["kept"].tolist() == [0, 1, 3, 4]                 # its search finds nothing, not even with nothing asked
    assert R.statistical(p, mean_k=4)["n_valid"] == 0                           # four searchable points < mean_k + 1


def test_radius_comparison_is_strict():
    p = f32((0, 0, 0), (0.5, 0, 0))
    assert np.float32(0.5 * 0.5) == np.float32(0.25)
    assert R.radius(p, 0.5, 1)["kept"].tolist() == []                           # d2 == r2: not counted
    assert R.radius(p, 0.5000001, 1)["kept"].tolist() == [0, 1]
    assert R.radius(p, 0.0, 0)["kept"].tolist() == [0, 1]


def _independent(p, mean_k, stddev_mul, radius, min_neighbors):
    """the same rules by a full sort of every row and Python-loop sums"""
    p = np.asarray(p, np.float32)
    fin = [i for i in range(len(p)) if all(math.isfinite(v) for v in p[i])]
    dist = np.zeros(len(p), np.float32)
    keep_r = np.zeros(len(p), bool)
    r2 = np.float32(radius * radius)
    for i in fin:
        d = p[i] - p[fin]
        d2 = np.sort((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if len(fin) >= mean_k + 1:
            s = 0.0
            for v in d2[1:mean_k + 1]:
                s += float(np.sqrt(np.float32(v)))
            dist[i] = np.float32(s / mean_k)
        keep_r[i] = int((d2 < r2).sum()) - (1 if np.float32(0) < r2 else 0) >= min_neighbors
    total = sq = 0.0
    for v in dist:
        total += float(v)
        sq += float(v) * float(v)
    nv = len(fin) if len(fin) >= mean_k + 1 else 0
    mean = total / nv
    thr = mean + stddev_mul * math.sqrt((sq - total * total / nv) / (nv - 1))
    return dist, mean, thr, [i for i in range(len(p)) if not float(dist[i]) > thr], np.flatnonzero(keep_r).tolist()


def test_restatement_equals_an_independent_formulation():
    rng = np.random.default_rng(7)
    p = np.concatenate([rng.normal(0, 1.0, (440, 3)), rng.uniform(-8, 8, (60, 3))]).astype(np.float32)
    p[17] = p[300]                                            # a duplicate
    p[123, 1] = np.inf                                        # a non-searchable point
    for mean_k, mul, rad, mn in ((20, 1.0, 0.8, 2), (1, 0.0, 0.5, 5), (33, 2.5, 0.3, 1)):
        dist, mean, thr, kept, kept_r = _independent(p, mean_k, mul, rad, mn)
        r = R.statistical(p, mean_k, mul)
        assert r["dist"].tobytes() == dist.tobytes()
        assert np.float64(r["mean"]).tobytes() == np.float64(mean).tobytes()
        assert np.float64(r["threshold"]).tobytes() == np.float64(thr).tobytes()
        assert r["kept"].tolist() == kept and 0 < len(kept) < len(p)
        assert R.radius(p, rad, mn)["kept"].tolist() == kept_r
        out, _ = R.remove_outliers(p, "STATISTICAL", mean_k, mul)
        assert out.tobytes() == p[kept].tobytes()


# ---- the C ABI, without a device ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_library_exports_the_new_symbols(lib):
    for s in ("mi355ndt_outlier_params_default", "mi355ndt_prefilter_outliers"):
        assert hasattr(lib, s) and s in ndt.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mi355_ndt.h")).read()
    for s in ("MI355NDT_OUTLIER_STATISTICAL = 1", "MI355NDT_OUTLIER_RADIUS = 2", "MI355NDT_OPT_OUTLIER_CELL_MM = 10", ":71-78"):
        assert s in hdr                                       # (:71-78: the header says the reference never runs RADIUS)
    assert (ndt.OUTLIER_STATISTICAL, ndt.OUTLIER_RADIUS, ndt.OPT_OUTLIER_CELL_MM) == (1, 2, 10)
    assert callable(ndt.Engine.prefilter_outliers)


def test_params_default_are_the_nodelets(lib):
    p = ndt.OutlierParams(-1, -1, -1.0, -1.0, -1)
    assert lib.mi355ndt_outlier_params_default(C.byref(p)) == 0
    assert (p.method, p.mean_k, p.stddev_mul, p.radius, p.min_neighbors) == (ndt.OUTLIER_STATISTICAL, 20, 1.0, 0.8, 2)   # prefiltering_nodelet.cpp:61-73
    assert lib.mi355ndt_outlier_params_default(None) == -2


def test_struct_layouts_match_header(lib, tmp_path):
    import subprocess
    src = tmp_path / "ol.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "mi355_ndt.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mi355ndt_outlier_params), offsetof(mi355ndt_outlier_params, stddev_mul), offsetof(mi355ndt_outlier_params, min_neighbors),
         sizeof(mi355ndt_outlier_stats), offsetof(mi355ndt_outlier_stats, mean), offsetof(mi355ndt_outlier_stats, threshold));
  return 0;
}''')
    exe = tmp_path / "ol"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(ndt.OutlierParams), ndt.OutlierParams.stddev_mul.offset, ndt.OutlierParams.min_neighbors.offset,
                   C.sizeof(ndt.OutlierStats), ndt.OutlierStats.mean.offset, ndt.OutlierStats.threshold.offset]


def test_argument_errors_without_a_device(lib):
    p = ndt.OutlierParams()
    lib.mi355ndt_outlier_params_default(C.byref(p))
    n = C.c_size_t(99)
    assert lib.mi355ndt_prefilter_outliers(None, C.byref(p), None, None, 0, 12, C.byref(n), None) == -1    # a NULL handle is refused, not dereferenced
    assert n.value == 99
