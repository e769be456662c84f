"""GPU (-m gpu): the global graph's map cloud on the device (mi355ndt_map_cloud, Engine.map_cloud) against the CPU restatement of
MapCloudGenerator::generate (tools/map_cloud_ref.py): the same number of centres, equal word for word and in the same order."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu


def _ref():
    spec = importlib.util.spec_from_file_location("map_cloud_ref", os.path.join(ROOT, "tools", "map_cloud_ref.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _ref()
PRM = dict(trans_epsilon=0.01, max_iterations=64)


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check(eng, clouds, poses, r):
    exp = R.map_cloud(clouds, poses, r)
    got = eng.map_cloud(clouds, poses, r)
    assert got.shape == exp.shape, (got.shape, exp.shape)
    assert same_words(got, exp)
    return got


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def drive():
    """Every 5th frame of a 40-frame synthetic drive (65,536 points per scan) with its ground-truth poses."""
    scans, poses = synth.make_sequence(40)
    return [scans[k].numpy().astype(np.float32) for k in range(0, 40, 5)], [poses[k] for k in range(0, 40, 5)]


@pytest.mark.parametrize("r", [0.5, 0.05])
def test_drive_keyframes_match_restatement(eng, drive, r):
    clouds, poses = drive
    got = check(eng, clouds, poses, r)
    assert 1000 < len(got) < sum(len(c) for c in clouds)


def test_cloud_uploads_counted(eng, drive):
    clouds, poses = drive
    eng.profile_reset()
    eng.map_cloud(clouds[:3] + [np.zeros((0, 3), np.float32)], poses[:4], 0.5)
    assert eng.profile_get()["cloud_uploads"] == 3                # the non-empty keyframes


def test_non_finite_points_and_empty_keyframes(eng, drive):
    clouds, poses = drive
    rng = np.random.default_rng(11)
    dirty = []
    for c in clouds[:4]:
        c = c.copy()
        for bad in (np.nan, np.inf, -np.inf):
            rows = rng.choice(len(c), 300, replace=False)
            c[rows, rng.integers(0, 3, 300)] = bad
        dirty.append(c)
    empty = np.zeros((0, 3), np.float32)
    ks = [empty, dirty[0], empty, empty, dirty[1], dirty[2], empty, dirty[3], empty]
    ps = [poses[0], poses[0], poses[1], poses[1], poses[1], poses[2], poses[3], poses[3], poses[3]]
    check(eng, ks, ps, 0.5)
    # the first keyframe's first points are not finite: the box starts at a later point
    c0 = dirty[0].copy()
    c0[:100, 1] = np.nan
    check(eng, [c0] + dirty[1:], poses[:4], 0.05)


def test_box_grows_on_all_axes_both_ways(eng):
    rng = np.random.default_rng(12)
    first = np.array([[0.3, -0.2, 0.1]], np.float32)
    blobs = [rng.standard_normal((20000, 3)).astype(np.float32) * 2 + np.float32(s) * np.array(d, np.float32)
             for s in (40, 90, 300) for d in ([1, 1, 1], [-1, -1, -1], [1, -1, 1], [-1, 1, -1])]
    P = np.concatenate([first] + blobs)
    out, box = R.octree_points(P, 0.05, return_box=True)
    assert box.depth >= 14
    assert box.min[0] < -300 and box.max[0] > 300 and box.min[2] < -300 and box.max[2] > 300
    check(eng, [P], [np.eye(4)], 0.05)
    # the same points behind a pose, split over keyframes
    T = np.eye(4)
    T[:3, 3] = [1000.5, -250.25, 7.0]
    parts = np.array_split(P, 7)
    check(eng, parts, [T] * 7, 0.05)


def test_points_on_box_faces_after_growth(eng):
    r = 0.5
    rng = np.random.default_rng(13)
    P = np.concatenate([np.zeros((1, 3), np.float32), rng.uniform(-20, 35, (5000, 3)).astype(np.float32)])
    _, box = R.octree_points(P, r, return_box=True)
    faces = []
    for a in range(3):
        for v in (box.min[a], box.max[a]):
            f = np.float32(v)
            for q in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
                p = np.array([1.0, 2.0, 3.0], np.float32)
                p[a] = q
                faces.append(p)
    # voxel faces inside the box: min + k r, as close as f32 gets, on either side
    for k in (1, 7, 40, 77):
        f = np.float32(box.min[0] + k * r)
        for q in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
            faces.append(np.array([q, 0.5, -0.5], np.float32))
    Q = np.concatenate([P, np.array(faces, np.float32)])
    check(eng, [Q], [np.eye(4)], r)
    check(eng, [Q[:2000], Q[2000:]], [np.eye(4), np.eye(4)], r)


def test_millions_of_points_use_both_sort_stages(eng):
    rng = np.random.default_rng(14)
    P = (rng.standard_normal((3_000_000, 3)) * np.array([60.0, 60.0, 8.0])).astype(np.float32)
    out, box = R.octree_points(P, 0.05, return_box=True)
    assert box.depth >= 11 and 3 * box.depth > 32          # codes wider than the low word
    parts = np.array_split(P, 25)
    check(eng, parts, [np.eye(4)] * 25, 0.05)


def test_error_paths(eng, drive):
    clouds, poses = drive
    assert eng.map_cloud([], [], 0.5) is None
    nan = np.full((1000, 3), np.nan, np.float32)
    assert eng.map_cloud([nan, nan], [np.eye(4), np.eye(4)], 0.5).shape == (0, 3)
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ndt.NDTError) as e:
            eng.map_cloud(clouds[:1], poses[:1], bad)
        assert e.value.code == -2
    # depth limit: 2^21 voxels per axis
    far = np.array([[0, 0, 0], [0.05 * 2 ** 21 * 1.01, 0, 0]], np.float32)
    with pytest.raises(R.MapCloudDepthError):
        R.octree_points(far, 0.05)
    with pytest.raises(ndt.NDTError) as e:
        eng.map_cloud([far], [np.eye(4)], 0.05)
    assert e.value.code == -2 and "2^21" in str(e.value)
    near = np.array([[0, 0, 0], [0.05 * 2 ** 20 * 0.99, 0, 0]], np.float32)
    check(eng, [near], [np.eye(4)], 0.05)
    # the engine still works after the errors
    check(eng, clouds[:2], poses[:2], 0.5)


def test_raw_call_capacity_and_strides(eng, drive):
    clouds, poses = drive
    exp = R.map_cloud(clouds[:2], poses[:2], 0.5)
    m = len(exp)
    # PointXYZI-like records (16 bytes) in, 16-byte records out
    recs = [np.concatenate([c, np.full((len(c), 1), 7.0, np.float32)], axis=1) for c in clouds[:2]]
    ptrs = (C.c_void_p * 2)(*[x.ctypes.data for x in recs])
    counts = (C.c_size_t * 2)(*[len(x) for x in recs])
    pcm = np.ascontiguousarray(np.transpose(np.asarray(poses[:2], np.float64), (0, 2, 1))).reshape(2, 16)
    n_out = C.c_size_t()
    small = np.full((m - 1, 4), -9.0, np.float32)
    rc = eng.lib.mi355ndt_map_cloud(eng.h, 2, ptrs, counts, 16, pcm.ctypes.data_as(C.c_void_p), 0.5, small.ctypes.data_as(C.c_void_p), m - 1, 16,
                                    C.byref(n_out))
    assert rc == -2 and n_out.value == m
    assert (small == -9.0).all()                             # nothing written
    big = np.full((m + 5, 4), -9.0, np.float32)
    rc = eng.lib.mi355ndt_map_cloud(eng.h, 2, ptrs, counts, 16, pcm.ctypes.data_as(C.c_void_p), 0.5, big.ctypes.data_as(C.c_void_p), m + 5, 16,
                                    C.byref(n_out))
    assert rc == 0 and n_out.value == m
    assert same_words(big[:m, :3], exp)
    assert (big[:m, 3] == -9.0).all() and (big[m:] == -9.0).all()
    assert eng.map_cloud(clouds[:2], poses[:2], 0.5, fetch=False) == m


def test_refused_in_stream_mode():
    e = ndt.Engine(ndt.default_params(**PRM))
    e.stream_begin(2, 4, 4096, 4096)
    try:
        P = np.random.default_rng(1).standard_normal((100, 3)).astype(np.float32)
        with pytest.raises(ndt.NDTError) as ex:
            e.map_cloud([P], [np.eye(4)], 0.5)
        assert ex.value.code == -7
    finally:
        e.stream_end()
    assert e.map_cloud([P], [np.eye(4)], 0.5).shape[0] > 0
    e.close()


def _batch(pairs):
    e = ndt.Engine(ndt.default_params(**PRM))
    e.batch_reserve(len(pairs), max(len(t) for t, _ in pairs), max(len(s) for _, s in pairs))
    for k, (t, s) in enumerate(pairs):
        e.batch_set_target(k, t)
        e.batch_set_source(k, s)
    return e


def _res_words(res):
    return [(r["final"].tobytes(), r["score"], r["iterations"], r["converged"], r["trans_probability"]) for r in res]


def test_no_side_effects_on_batch_and_prefilter(drive):
    clouds, poses = drive
    pairs = []
    for k in range(4):
        t, s, _ = synth.make_pair(200 + k, 256)
        pairs.append((t.numpy(), s.numpy()))
    G = [synth.default_guess()] * 4

    def run(with_map):
        e = _batch(pairs)
        a1 = _res_words(e.batch_align(G))
        if with_map:
            e.map_cloud(clouds, poses, 0.05)
        a2 = _res_words(e.batch_align(G))
        f = e.batch_fitness_scores(1.0)
        if with_map:
            e.map_cloud(clouds[:3], poses[:3], 0.5)
        f2 = e.batch_fitness_scores()
        e.close()
        return a1, a2, [x.tobytes() for x in f], [x.tobytes() for x in f2]

    assert run(True) == run(False)

    raw = clouds[0][:20000]

    def run_pf(with_map):
        e = ndt.Engine(ndt.default_params(**PRM))
        pf = e.prefilter(raw, 0.5, 100.0, 0.2)
        if with_map:
            e.map_cloud(clouds[:2], poses[:2], 0.5)
        e.use_prefiltered(as_target=True)
        e.set_source(pairs[0][1])
        r1 = e.align(synth.default_guess())
        if with_map:
            e.map_cloud(clouds[2:4], poses[2:4], 0.05)
        r2 = e.fitness_score()
        e.close()
        return pf.tobytes(), _res_words([r1]), r2

    assert run_pf(True) == run_pf(False)
