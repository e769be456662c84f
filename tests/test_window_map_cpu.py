"""CPU: the restatement the GPU tests hold mi355ndt_window_keyframe to (tools/window_map_ref.py) against an independent check that already
exists -- the oracle's VoxelGrid (oracle_py.prefilter without the distance filter) over the window transformed in NumPy f64 -- and, for the
intensity channel, against a dictionary-based recomputation; plus the C-ABI surface of the new entry points without a GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O


def _ref():
    spec = importlib.util.spec_from_file_location("window_map_ref", os.path.join(ROOT, "tools", "window_map_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _ref()


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def concat_f64(scans, rel):
    """The window, written out independently of the tool: scan 0 as it is, scan k by rel[k] in f64 with one rounding at the end."""
    parts = []
    for k, s in enumerate(scans):
        s = np.asarray(s, np.float32)[:, :3]
        if k == 0:
            parts.append(s.copy())
            continue
        T = np.asarray(rel[k], np.float64)
        x, y, z = (s[:, a].astype(np.float64) for a in range(3))
        out = s.copy()
        fin = np.isfinite(s).all(axis=1)
        with np.errstate(invalid="ignore", over="ignore"):
            for a in range(3):
                v = (((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]).astype(np.float32)
                out[fin, a] = v[fin]
        parts.append(out)
    return np.concatenate(parts)


def check(scans, rel, leaf):
    got = R.window_map(scans, rel, leaf)
    assert got.shape[1] == 3
    exp = O.prefilter(concat_f64(scans, rel), use_distance_filter=False, leaf=leaf)
    assert got.shape == exp.shape, (leaf, got.shape, exp.shape)
    assert same_words(got, exp), leaf
    return got


@pytest.fixture(scope="module")
def drive3():
    scans, poses = synth.make_sequence(3, 256)
    scans = [s.numpy().astype(np.float32) for s in scans]
    rel = [np.linalg.inv(poses[0]) @ p for p in poses]
    return scans, rel


def test_one_scan_is_not_moved(drive3):
    scans, _ = drive3
    bogus = [np.full((4, 4), 7.0)]                               # rel_poses[0] is ignored
    got = check(scans[:1], bogus, 0.1)
    assert 100 < len(got) < len(scans[0])


@pytest.mark.parametrize("leaf", [0.1, 0.25])
def test_three_scans_ground_truth_poses(drive3, leaf):
    scans, rel = drive3
    got = check(scans, rel, leaf)
    assert len(got) < sum(len(s) for s in scans)
    # the relative poses matter: identity poses give another cloud
    assert not same_words(got, R.window_map(scans, [np.eye(4)] * 3, leaf))


def test_non_finite_rows_are_dropped(drive3):
    scans, rel = drive3
    rng = np.random.default_rng(21)
    dirty = []
    for s in scans:
        s = s.copy()
        for bad in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(s), 200, replace=False)
            s[rows, rng.integers(0, 3, 200)] = bad
        dirty.append(s)
    got = check(dirty, rel, 0.1)
    assert np.isfinite(got).all()
    assert np.isfinite(check(dirty, rel, 0.0)).all()
    # a point the move pushes out of f32's range is dropped as well
    far = [scans[0][:100], scans[1][:100]]
    T = np.eye(4)
    T[0, 3] = 1e39
    assert len(R.window_map(far, [np.eye(4), T], 0.0)) == 100
    check(far, [np.eye(4), T], 0.1)


def test_empty_scan_in_the_middle(drive3):
    scans, rel = drive3
    empty = np.zeros((0, 3), np.float32)
    a = check([scans[0], empty, scans[1], scans[2]], [rel[0], rel[1], rel[1], rel[2]], 0.1)
    assert same_words(a, R.window_map(scans, rel, 0.1))
    assert R.window_map([empty, empty], [np.eye(4)] * 2, 0.1).shape == (0, 3)


def test_leaf_too_small_returns_the_finite_input(drive3):
    scans, rel = drive3
    s0 = scans[0].copy()
    s0[5] = np.nan
    got = check([s0, scans[1]], rel[:2], 1e-4)
    assert len(got) == len(s0) - 1 + len(scans[1])               # the guard: nothing merged, the non-finite point gone
    assert same_words(got, R.window_map([s0, scans[1]], rel[:2], 0.0))


def test_leaf_zero_is_the_window_in_order(drive3):
    scans, rel = drive3
    got = check(scans, rel, 0.0)
    assert same_words(got, concat_f64(scans, rel))
    assert same_words(got, R.window_points(scans, rel))


def test_transform_rounds_once(drive3):
    scans, rel = drive3
    P = R.transform(scans[1], rel[1])
    T = rel[1]
    differs = 0
    for i in range(0, len(P), 501):
        x, y, z = (float(v) for v in scans[1][i])
        for a in range(3):
            assert P[i, a] == np.float32(((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3])
    # ... which is not the map cloud's transform (pose cast to f32 first, every step rounded to f32)
    M = T.astype(np.float32)
    s = scans[1]
    f32 = ((M[0, 0] * s[:, 0] + M[0, 1] * s[:, 1]) + M[0, 2] * s[:, 2]) + M[0, 3]
    differs = int((f32 != P[:, 0]).sum())
    assert differs > 0


def test_intensity_is_averaged_like_xyz(drive3):
    scans, rel = drive3
    rng = np.random.default_rng(22)
    recs = [np.concatenate([s, rng.uniform(0, 255, (len(s), 1)).astype(np.float32)], axis=1) for s in scans]
    recs[1][::97, 1] = np.nan
    leaf = 0.25
    got = R.window_map(recs, rel, leaf, intensity=True)
    assert got.shape[1] == 4
    assert same_words(got[:, :3], R.window_map(recs, rel, leaf))            # the fourth channel changes nothing about the first three
    # dictionary recomputation: per cell np.float32 running sums in input order
    W = np.concatenate([concat_f64(recs, rel), np.concatenate([r[:, 3:4] for r in recs])], axis=1)
    W = W[np.isfinite(W[:, :3]).all(axis=1)]
    inv = np.float32(1.0) / np.float32(leaf)
    mn = [int(np.floor(W[:, a].min() * inv)) for a in range(3)]
    mx = [int(np.floor(W[:, a].max() * inv)) for a in range(3)]
    cells = {}
    for p in W:
        ijk = [int(np.float32(np.floor(np.float32(p[a] * inv)) - np.float32(mn[a]))) for a in range(3)]
        key = ijk[0] + ijk[1] * (mx[0] - mn[0] + 1) + ijk[2] * (mx[0] - mn[0] + 1) * (mx[1] - mn[1] + 1)
        acc = cells.setdefault(key, [np.zeros(4, np.float32), 0])
        acc[0] = acc[0] + p
        acc[1] += 1
    exp = np.array([cells[k][0] / np.float32(cells[k][1]) for k in sorted(cells)], np.float32)
    assert same_words(got, exp)
    # leaf = 0: the records in order
    assert same_words(R.window_map(recs, rel, 0.0, intensity=True)[:, 3], W[:, 3])


def test_run_lengths_count_the_points(drive3):
    scans, rel = drive3
    rl = R.run_lengths(scans, rel, 0.1)
    assert len(rl) == len(R.window_map(scans, rel, 0.1)) and rl.sum() == sum(len(s) for s in scans)
    still = R.run_lengths([scans[0]] * 5, [np.eye(4)] * 5, 0.1)
    assert still.min() >= 5                                       # a window that stands still: every run holds all copies


# ---- the C-ABI surface, no GPU needed ----------------------------------------------------------------------------------------------
NEW = ["mi355ndt_window_keyframe", "mi355ndt_keyframe_add", "mi355ndt_keyframe_get", "mi355ndt_keyframe_release", "mi355ndt_keyframe_count",
       "mi355ndt_map_cloud_keyframes", "mi355ndt_batch_set_target_keyframe", "mi355ndt_batch_set_source_keyframe"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_new_exports_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "mi355_ndt.h")).read()
    for s in NEW:
        assert s + "(" in hdr, f"{s} not declared in mi355_ndt.h"
        assert hasattr(lib, s) and s in ndt.SYMBOLS
    for m in ("window_keyframe", "keyframe_add", "keyframe_get", "keyframe_release", "keyframe_count", "map_cloud_keyframes",
              "batch_set_target_keyframe", "batch_set_source_keyframe"):
        assert callable(getattr(ndt.Engine, m, None)), m


def test_null_handle_is_refused(lib):
    n, kid = C.c_size_t(7), C.c_int(5)
    assert lib.mi355ndt_window_keyframe(None, 1, None, None, 12, -1, None, 0.1, C.byref(kid), C.byref(n)) == -1     # MI355NDT_ERR_BAD_HANDLE
    assert lib.mi355ndt_keyframe_add(None, None, 0, 12, -1, C.byref(kid)) == -1
    assert lib.mi355ndt_keyframe_get(None, 0, None, 0, 12, -1, C.byref(n)) == -1
    assert lib.mi355ndt_keyframe_release(None, 0) == -1
    assert lib.mi355ndt_keyframe_count(None) == -1
    assert lib.mi355ndt_map_cloud_keyframes(None, 0, None, None, 0.5, None, 0, 12, C.byref(n)) == -1
    assert lib.mi355ndt_batch_set_target_keyframe(None, 0, 0) == -1
    assert lib.mi355ndt_batch_set_source_keyframe(None, 0, 0) == -1
