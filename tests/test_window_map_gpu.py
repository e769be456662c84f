"""GPU (-m gpu): the window map on the device (mi355ndt_window_keyframe, Engine.window_keyframe + keyframe_get) against its CPU restatement
(tools/window_map_ref.py): the same count, x, y, z and intensity equal word for word, in the same order."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


def _ref():
    spec = importlib.util.spec_from_file_location("window_map_ref", os.path.join(ROOT, "tools", "window_map_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _ref()


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(eng, scans, rel, leaf, intensity=False):
    exp = R.window_map(scans, rel, leaf, intensity)
    kid, n = eng.window_keyframe(scans, rel, leaf, intensity)
    got = eng.keyframe_get(kid, intensity)
    print(f"window_keyframe: scans={len(scans)} leaf={leaf} intensity={intensity} points in={sum(len(s) for s in scans)} out gpu={n} ref={len(exp)}")
    assert n == len(exp) == len(got), (n, len(exp), len(got))
    assert same_words(got, exp)
    eng.keyframe_release(kid)
    return got


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def drive():
    """An 8-scan window of a synthetic drive, 65,536 points per scan, with the ground-truth poses relative to the first."""
    scans, poses = synth.make_sequence(8)
    rng = np.random.default_rng(31)
    recs = [np.concatenate([s.numpy().astype(np.float32), rng.uniform(0, 255, (len(s), 1)).astype(np.float32)], axis=1) for s in scans]
    return recs, [np.linalg.inv(poses[0]) @ p for p in poses]


def test_drive_window_matches_restatement(eng, drive):
    recs, rel = drive
    got = check(eng, [r[:, :3] for r in recs], rel, 0.1)
    assert 10000 < len(got) < 8 * 65536
    check(eng, recs, rel, 0.1, intensity=True)                    # 16-byte records, the intensity averaged with the points


def test_one_scan_and_ignored_first_pose(eng, drive):
    recs, rel = drive
    bogus = [np.full((4, 4), 3.0)]
    check(eng, [recs[0][:, :3]], bogus, 0.1)
    check(eng, [recs[0]], bogus, 0.25, intensity=True)


def test_dirty_empty_guard_and_no_downsampling(eng, drive):
    recs, rel = drive
    rng = np.random.default_rng(32)
    dirty = []
    for r in recs[:4]:
        r = r.copy()
        for bad in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(r), 300, replace=False)
            r[rows, rng.integers(0, 3, 300)] = bad
        dirty.append(r)
    empty = np.zeros((0, 4), np.float32)
    scans = [dirty[0], empty, dirty[1], dirty[2], empty, dirty[3]]
    poses = [rel[0], rel[1], rel[1], rel[2], rel[3], rel[3]]
    for intensity in (False, True):
        check(eng, scans, poses, 0.1, intensity)
        check(eng, scans, poses, 0.0, intensity)                  # leaf = 0: the finite points of the window in order
        got = check(eng, scans, poses, 1e-4, intensity)           # "leaf size is too small": the same
        assert len(got) == int(sum(np.isfinite(s[:, :3]).all(axis=1).sum() for s in scans))
    assert "leaf size too small" in (eng.lib.mi355ndt_last_error(eng.h) or b"").decode()
    # an empty first scan, a window of empty scans, a window without a finite point
    check(eng, [empty, dirty[1]], [rel[0], rel[1]], 0.1, True)
    kid, n = eng.window_keyframe([empty, empty], [np.eye(4)] * 2, 0.1)
    assert n == 0 and eng.keyframe_get(kid).shape == (0, 3)
    eng.keyframe_release(kid)
    check(eng, [np.full((1000, 3), np.nan, np.float32)] * 2, [np.eye(4)] * 2, 0.1)
    # a pose that throws a scan out of f32's range
    T = np.eye(4)
    T[1, 3] = -1e39
    check(eng, [recs[0][:5000, :3], recs[1][:5000, :3]], [np.eye(4), T], 0.1)


def test_32_byte_records(eng, drive):
    recs, rel = drive
    wide = []
    for r in recs[:3]:
        w = np.full((len(r), 8), -5.0, np.float32)
        w[:, :4] = r
        wide.append(w)
    exp = R.window_map(recs[:3], rel[:3], 0.1, intensity=True)
    kid, n = eng.window_keyframe(wide, rel[:3], 0.1, intensity=True)
    assert n == len(exp) and same_words(eng.keyframe_get(kid, True), exp)
    assert same_words(eng.keyframe_get(kid), exp[:, :3])
    eng.keyframe_release(kid)
    # the intensity somewhere else in the record: byte offset 20
    for w, r in zip(wide, recs[:3]):
        w[:, 3] = -5.0
        w[:, 5] = r[:, 3]
    K = 3
    ptrs = (C.c_void_p * K)(*[w.ctypes.data for w in wide])
    counts = (C.c_size_t * K)(*[len(w) for w in wide])
    pcm = np.ascontiguousarray(np.transpose(np.asarray(rel[:3], np.float64), (0, 2, 1))).reshape(K, 16)
    kid, n_out = C.c_int(-1), C.c_size_t()
    rc = eng.lib.mi355ndt_window_keyframe(eng.h, K, ptrs, counts, 32, 20, pcm.ctypes.data_as(C.c_void_p), 0.1, C.byref(kid), C.byref(n_out))
    assert rc == 0 and n_out.value == len(exp)
    out = np.full((len(exp), 8), -9.0, np.float32)
    n = C.c_size_t()
    assert eng.lib.mi355ndt_keyframe_get(eng.h, kid.value, out.ctypes.data_as(C.c_void_p), len(exp), 32, 28, C.byref(n)) == 0
    assert same_words(out[:, :3], exp[:, :3]) and same_words(out[:, 7], exp[:, 3]) and (out[:, 3:7] == -9.0).all()
    eng.keyframe_release(kid.value)


def test_window_that_stands_still(eng, drive):
    """20 copies of one scan with noise: voxel runs of 20 points and more (the emit kernel's long-run case)."""
    recs, _ = drive
    rng = np.random.default_rng(33)
    base = recs[0]
    scans = []
    for k in range(20):
        s = base.copy()
        s[:, :3] += rng.normal(0, 0.005, (len(s), 3)).astype(np.float32)
        scans.append(s)
    rel = [np.eye(4)] * 20
    rl = R.run_lengths(scans, rel, 0.1)
    print(f"standing window: voxels={len(rl)} mean run={rl.mean():.1f} max run={rl.max()}")
    assert rl.max() >= 20 and rl.mean() > 5
    check(eng, scans, rel, 0.1, intensity=True)
    # ... and with tiny true motion through the pose table
    rel2 = []
    for k in range(20):
        T = np.eye(4)
        T[0, 3] = 1e-3 * k
        rel2.append(T)
    check(eng, [s[:, :3] for s in scans], rel2, 0.1)


def test_bad_arguments(eng, drive):
    recs, rel = drive
    with pytest.raises(ndt.NDTError) as e:
        eng.window_keyframe([recs[0][:, :3]], [np.eye(4)], float("nan"))
    assert e.value.code == -2
    kid, n = C.c_int(), C.c_size_t()
    assert eng.lib.mi355ndt_window_keyframe(eng.h, 0, None, None, 12, -1, None, 0.1, C.byref(kid), C.byref(n)) == -2
    one = np.ascontiguousarray(recs[0][:100, :3])
    ptrs = (C.c_void_p * 1)(one.ctypes.data)
    counts = (C.c_size_t * 1)(100)
    assert eng.lib.mi355ndt_window_keyframe(eng.h, 1, ptrs, counts, 12, 12, None, 0.1, C.byref(kid), C.byref(n)) == -2     # intensity past the record
    assert eng.lib.mi355ndt_window_keyframe(eng.h, 1, ptrs, counts, 8, -1, None, 0.1, C.byref(kid), C.byref(n)) == -2
    before = eng.keyframe_count()
    check(eng, [one], [np.eye(4)], 0.1)                           # the engine still works, and the failed calls left no keyframe
    assert eng.keyframe_count() == before


# ---- the window as the prefilter chain's one cloud: totals at the 4,096-point sort tile / scan chunk, against the oracle's VoxelGrid over the
# window written out in NumPy f64 (what tests/test_window_map_cpu.py holds the restatement to)
LEAF_TOO_SMALL = "window_keyframe: leaf size too small for the window's extent, voxel indices would overflow; window not down-sampled"


def clustered_records():
    """4,097 records (x, y, z, intensity) in clusters of four within a centimetre -- voxels of several points, also across scans that barely
    move --, three of them not finite"""
    rng = np.random.default_rng(20261021)
    base = np.repeat(rng.uniform([-3.0, -3.0, -0.5], [3.0, 3.0, 0.5], (1025, 3)), 4, axis=0)
    r = np.concatenate([base + rng.normal(0.0, 0.01, base.shape), rng.uniform(0, 255, (len(base), 1))], axis=1).astype(np.float32)[:4097]
    r[7, 0] = np.nan
    r[2100, 2] = np.inf
    r[4090, 1] = -np.inf
    return r


def small_poses(k):
    out = []
    for j in range(k):
        a = 1e-3 * j
        T = np.eye(4)
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = [2e-3 * j, -1e-3 * j, 5e-4 * j]
        out.append(T)
    return out


def check_oracle(eng, recs, rel, leaf):
    """with and without intensity: x, y, z against the oracle, all four channels against the restatement; returns the oracle's cloud"""
    from test_window_map_cpu import concat_f64
    exp = O.prefilter(concat_f64(recs, rel), use_distance_filter=False, leaf=leaf)
    got3 = check(eng, [r[:, :3] for r in recs], rel, leaf)
    got4 = check(eng, recs, rel, leaf, intensity=True)
    assert same_words(got3, exp) and same_words(got4[:, :3], exp)
    return exp


@pytest.mark.parametrize("total", (1, 4096, 4097))
def test_window_totals_at_tile_edges_against_the_oracle(total):
    r = clustered_records()[4097 - total:]                        # (the last record is finite: a window of one point keeps it)
    eng = ndt.Engine()
    assert (eng.lib.mi355ndt_last_error(eng.h) or b"") == b""
    finite = int(np.isfinite(r[:, :3]).all(axis=1).sum())
    splits = [(total,), (total // 2, total - total // 2), (total // 3, total // 3, total - 2 * (total // 3))]
    if total == 4097:
        splits.append((2000, 0, 2097))                            # one scan of the window is empty
    for sizes in splits:
        at = np.cumsum((0,) + sizes)
        recs = [r[at[k]:at[k + 1]] for k in range(len(sizes))]
        rel = small_poses(len(sizes))
        exp = {leaf: check_oracle(eng, recs, rel, leaf) for leaf in (0.1, 0.0, 1e-4)}
        assert len(exp[0.0]) == finite
        if total > 1:                                             # not trivial: points dropped, voxels of several points, the 1e-4 m grid refused
            assert finite < total and len(exp[0.1]) < finite and same_words(exp[1e-4], exp[0.0])
            assert (eng.lib.mi355ndt_last_error(eng.h) or b"").decode() == LEAF_TOO_SMALL
    eng.close()
