"""GPU (-m gpu): mi355ndt_prefilter_outliers -- PrefilteringNodelet::outlier_removal over the resident prefilter result -- word for word
against tools/outlier_ref.py: dist[] as bytes, mean / stddev / threshold as bytes, the survivors as bytes and in order, n_out.  No
tolerances, no excluded cases.  Clouds enter through Engine.prefilter with the distance filter off and no down-sampling; that stage drops
non-finite points (as VoxelGrid does), so the restatement is applied to what the prefilter left resident.

Timings: tools/outlier_timing.py, DESIGN.md section 8 (outlier removal)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("outlier_ref")
_REF = {}


def ref(name, cloud, method, **kw):
    """the restatement's answer, computed once per (cloud, parameters) and shared"""
    key = (name, method, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = R.statistical(cloud, **kw) if method == "STATISTICAL" else R.radius(cloud, **kw)
    return _REF[key]


def f64w(x):
    return np.float64(x).tobytes()


def resident(e, cloud):
    """the cloud as the prefilter leaves it resident: distance filter off, no down-sampling"""
    return e.prefilter(cloud, use_distance_filter=False, downsample_resolution=0.0)


def check(e, name, cloud, method="STATISTICAL", **kw):
    """prefilter(cloud) + prefilter_outliers on engine e against the restatement; returns the library's (survivors, stats)"""
    res = resident(e, cloud)
    x = ref(name, res, method, **({"radius": kw["radius"], "min_neighbors": kw["min_neighbors"]} if method == "RADIUS" else kw))
    out, st = e.prefilter_outliers(method=method, return_stats=True, **kw)
    print(f"{name} {method} {kw}: n_in {st['n_in']} n_valid {st['n_valid']} mean {st['mean']!r} stddev {st['stddev']!r} "
          f"threshold {st['threshold']!r} kept {len(out)} | restatement kept {len(x['kept'])} threshold {x['threshold']!r}")
    assert st["dist"].tobytes() == x["dist"].tobytes()
    if method == "STATISTICAL":
        assert (st["n_in"], st["n_valid"]) == (x["n_in"], x["n_valid"])
        assert (f64w(st["mean"]), f64w(st["stddev"]), f64w(st["threshold"])) == (f64w(x["mean"]), f64w(x["stddev"]), f64w(x["threshold"]))
    else:
        assert (st["n_in"], st["n_valid"], st["mean"], st["stddev"], st["threshold"]) == (0, 0, 0.0, 0.0, 0.0)
    assert len(out) == len(x["kept"])
    assert out.tobytes() == res[x["kept"]].tobytes()
    assert e.prefilter_outliers(fetch=False, method="RADIUS", min_neighbors=0) == len(out)     # the resident count follows
    return out, st


def blobs():
    """3,000 points: 2,900 in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.1
    parts = [(g[:m] + rng.uniform(-0.03, 0.03, (m, 3)) + c) for m, c in ((967, (0, 0, 0)), (967, (8, 3, 0)), (966, (-5, 10, 1)))]
    d = rng.normal(size=(100, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 60, (100, 1))
    p = np.concatenate(parts + [far]).astype(np.float32)
    return p[rng.permutation(len(p))]


BLOBS = blobs()


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(**PRM))
    yield e
    e.close()


@pytest.mark.parametrize("n", [1, 20, 21, 257])
def test_small_clouds(eng, n):
    # 1: one workgroup, one lane; mean_k: nothing valid, NaN threshold, all kept; mean_k + 1: every list exactly full; 257: a fifth wave with one live lane
    p = np.random.default_rng(n).normal(0, 0.5, (n, 3)).astype(np.float32)
    out, st = check(eng, f"small{n}", p, mean_k=20, stddev_mul=1.0)
    if n <= 20:
        assert st["n_valid"] == 0 and np.isnan(st["threshold"]) and len(out) == n
    else:
        assert st["n_valid"] == n
    check(eng, f"small{n}", p, "RADIUS", radius=0.5, min_neighbors=5)


@pytest.mark.parametrize("mean_k", [1, 20, 32, 33, 64])
def test_blobs_and_isolated_points(eng, mean_k):
    # both list capacities and their edge; the isolated points' walks cross many empty rings and end by covering the lattice
    out, st = check(eng, "blobs", BLOBS, mean_k=mean_k, stddev_mul=1.0)
    assert st["n_valid"] == 3000 and 2000 < len(out) < 3000


def test_points_on_cell_boundaries_and_duplicates(eng):
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    sheet = np.stack([i.ravel() * 0.5, j.ravel() * 0.5 - 10.0, np.full(1600, 1.5)], 1).astype(np.float32)    # multiples of the 0.5 m cell below
    p = np.concatenate([sheet, sheet[np.random.default_rng(3).choice(1600, 50, replace=False)]])
    eng.set_option(ndt.OPT_OUTLIER_CELL_MM, 500)
    try:
        check(eng, "sheet", p, mean_k=20, stddev_mul=0.5)
        check(eng, "sheet", p, mean_k=4, stddev_mul=1.0)       # ties at the list's edge: four neighbours at the same distance
        check(eng, "sheet", p, "RADIUS", radius=0.5, min_neighbors=1)     # the lattice neighbours sit at d2 == r2 exactly: only duplicates count
        check(eng, "sheet", p, "RADIUS", radius=0.75, min_neighbors=5)
    finally:
        eng.set_option(ndt.OPT_OUTLIER_CELL_MM, 100)


def test_a_stray_point_takes_the_exhaustive_route(eng):
    p = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])
    _, lattice = check(eng, "blobs", BLOBS, mean_k=20, stddev_mul=1.0)
    _, brute = check(eng, "stray", p, mean_k=20, stddev_mul=1.0)
    assert brute["dist"][:3000].tobytes() == lattice["dist"].tobytes()      # the same lists, whichever kernel made them
    check(eng, "stray", p, mean_k=40, stddev_mul=1.0)
    check(eng, "stray", p, "RADIUS", radius=0.5, min_neighbors=5)


def test_nan_points_mixed_in(eng):
    p = BLOBS[:600].copy()
    p[100, 0] = np.nan
    p[433, 2] = np.nan
    assert len(resident(eng, p)) == 598                        # the prefilter stage drops them, as VoxelGrid does
    check(eng, "nan", p, mean_k=20, stddev_mul=1.0)
    out, _ = check(eng, "nan", p, "RADIUS", radius=0.5, min_neighbors=5)
    assert np.isfinite(out).all()


@pytest.mark.parametrize("radius,min_neighbors", [(0.5, 5), (0.8, 2), (0.8, 0), (1e-4, 1), (0.3, 33)])
def test_radius(eng, radius, min_neighbors):
    out, _ = check(eng, "blobs", BLOBS, "RADIUS", radius=radius, min_neighbors=min_neighbors)
    if min_neighbors == 0:
        assert len(out) == 3000
    if radius < 1e-3:
        assert len(out) == 0                                   # smaller than any spacing


def test_cell_size_changes_no_word():
    got = []
    for cell in (50, 100, 1000):
        e = ndt.Engine(ndt.default_params(**PRM))
        e.set_option(ndt.OPT_OUTLIER_CELL_MM, cell)
        assert e.get_option(ndt.OPT_OUTLIER_CELL_MM) == cell
        out, st = check(e, "blobs", BLOBS, mean_k=20, stddev_mul=1.0)
        got.append((out.tobytes(), st["dist"].tobytes(), f64w(st["threshold"])))
        with pytest.raises(ndt.NDTError):
            e.set_option(ndt.OPT_OUTLIER_CELL_MM, 0)
        e.close()
    assert got[0] == got[1] == got[2]


def test_use_prefiltered_installs_the_filtered_cloud(eng):
    tgt, src, _ = synth.make_pair(3, 64, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    G = synth.default_guess()
    eng.set_target(tgt)
    res = resident(eng, src)
    n = eng.prefilter_outliers(fetch=False)
    x = ref("pair3", res, "STATISTICAL", mean_k=20, stddev_mul=1.0)
    assert n == len(x["kept"]) < len(res)
    eng.use_prefiltered(False)
    a = eng.align(G)
    moved = eng.get_aligned()
    other = ndt.Engine(ndt.default_params(**PRM))
    other.set_target(tgt)
    other.set_source(res[x["kept"]])
    b = other.align(G)
    assert np.asarray(a["final"]).tobytes() == np.asarray(b["final"]).tobytes() and a["iterations"] == b["iterations"]
    assert moved.tobytes() == other.get_aligned().tobytes()
    other.close()
    # the chained keyword gives the same cloud
    chained = eng.prefilter(src, use_distance_filter=False, downsample_resolution=0.0, outlier={})
    assert chained.tobytes() == res[x["kept"]].tobytes()
    assert eng.prefilter(src, use_distance_filter=False, downsample_resolution=0.0, outlier=dict(mean_k=20), fetch=False) == n


def test_the_rest_of_the_handle_is_left_as_it_was():
    e = ndt.Engine(ndt.default_params(**PRM))
    tgt, src, _ = synth.make_pair(5, 64, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    G = synth.default_guess()
    e.set_target(tgt)
    e.set_source(src)
    k1, k2 = e.keyframe_add(tgt), e.keyframe_add(src)
    T = np.eye(4)
    before = (e.align(G), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k2], [T], 1.0))      # (the last call builds k1's index)
    check(e, "blobs", BLOBS, mean_k=20, stddev_mul=1.0)
    check(e, "blobs", BLOBS, "RADIUS", radius=0.5, min_neighbors=5)
    after = (e.align(G), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k2], [T], 1.0))
    assert np.asarray(before[0]["final"]).tobytes() == np.asarray(after[0]["final"]).tobytes()
    assert before[0]["iterations"] == after[0]["iterations"] and before[1] == after[1]
    assert before[2][0].tobytes() == after[2][0].tobytes() and np.array_equal(before[2][1], after[2][1])
    assert e.keyframe_get(k1).tobytes() == tgt.astype(np.float32).tobytes()
    e.close()


def test_state_and_argument_errors():
    e = ndt.Engine(ndt.default_params(**PRM))
    with pytest.raises(ndt.NDTError) as err:                   # no prefilter result is resident
        e.prefilter_outliers()
    assert err.value.code == -7
    far = np.full((10, 3), 500.0, np.float32)
    assert e.prefilter(far, downsample_resolution=0.0, fetch=False) == 0      # an empty resident cloud
    out, st = e.prefilter_outliers(return_stats=True)
    assert out.shape == (0, 3) and st["n_in"] == 0
    resident(e, BLOBS[:100])
    for kw in (dict(method="MEDIAN"), dict(method=3), dict(mean_k=0), dict(mean_k=65), dict(min_neighbors=-1), dict(min_neighbors=65),
               dict(radius=float("nan")), dict(radius=-0.5), dict(stddev_mul=float("nan"))):
        with pytest.raises(ndt.NDTError) as err:
            e.prefilter_outliers(**kw)
        assert err.value.code == -2 and str(err.value).count("prefilter_outliers") == 2, kw      # (the call's name and mi355ndt_last_error's text)
    assert e.prefilter_outliers(fetch=False, method="RADIUS", min_neighbors=0) == 100      # refused calls changed nothing
    e.stream_begin(2, 4, 1024, 1024)
    with pytest.raises(ndt.NDTError) as err:
        e.prefilter_outliers()
    assert err.value.code == -7
    e.stream_end()
    assert e.prefilter_outliers(fetch=False, method="RADIUS", min_neighbors=0) == 100
    e.close()
