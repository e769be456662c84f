"""CPU: tools/knn_ref.py, the brute-force restatement the keyframe search surface (mi355ndt_keyframe_knn / _radius_search) is held to --
checked itself: against scipy's kd-tree in f64 where f32 and f64 squared distances coincide, and rule by rule (ties, the two inclusion
rules, the fill values, non-finite points on either side)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from tools import knn_ref as R

INF = np.float32(np.inf)


def clustered_grid_cloud(rng, n_clusters, per_cluster, n_queries):
    """Points and queries on a grid of 2^-10 m inside +-64 m.  Coordinates there have 17 significant bits, so a squared distance is exact
    in f32 only between points less than 2 m apart on every axis (three squares below 2^22 grid units each, their sum below 2^24): the
    points come in clusters 2 m wide and every query sits inside one, so that its nearest neighbours are that close.  The test checks
    that the distances it compares do coincide; across clusters they need not."""
    centres = rng.integers(-60 * 1024, 60 * 1024 + 1, (n_clusters, 3))
    p = (centres[:, None, :] + rng.integers(-1024, 1025, (n_clusters, per_cluster, 3))).reshape(-1, 3)
    q = centres[rng.integers(0, n_clusters, n_queries)] + rng.integers(-512, 513, (n_queries, 3))
    p, q = (p.astype(np.float64) / 1024.0).astype(np.float32), (q.astype(np.float64) / 1024.0).astype(np.float32)
    assert np.abs(p).max() <= 64.0 and np.abs(q).max() <= 64.0
    assert (p.astype(np.float64) * 1024.0 == np.round(p.astype(np.float64) * 1024.0)).all()
    return p, q


def d2_f64(p, q, ids):
    d = q.astype(np.float64)[:, None, :] - p.astype(np.float64)[ids]
    return (d * d).sum(axis=2)


@pytest.mark.parametrize("k", [1, 5, 20])
def test_equals_the_kd_tree_in_f64_where_the_distances_are_exact(k):
    rng = np.random.default_rng(100 + k)
    p, q = clustered_grid_cloud(rng, 64, 64, 300)
    nq = len(q)
    ids, d2, cnt = R.knn(p, q, k)
    assert (cnt == k).all()
    assert (d2_f64(p, q, ids) == d2.astype(np.float64)).all(), "f32 and f64 squared distances must coincide for the neighbours compared"
    dd, ii = cKDTree(p.astype(np.float64)).query(q.astype(np.float64), k)
    ii = ii.reshape(nq, k)
    # a random cloud without ties: no two of a query's k + 1 nearest at one distance (f64, exact)
    near = np.sort(((q.astype(np.float64)[:, None, :] - p.astype(np.float64)[None, :, :]) ** 2).sum(axis=2), axis=1)[:, :k + 1]
    untied = (np.diff(near, axis=1) > 0).all(axis=1)
    assert untied.sum() >= nq - nq // 20, "the draw is to be (almost) free of ties"
    assert (ii[untied] == ids[untied]).all()
    # ... and with ties the same distances, whatever the order among equals
    assert (np.sort(d2_f64(p, q, ii), axis=1) == d2.astype(np.float64)).all()


def test_equal_distances_come_out_in_id_order():
    rng = np.random.default_rng(3)
    base = rng.uniform(-5, 5, (100, 3)).astype(np.float32)
    p = np.concatenate([base, base])                       # point i and point i + 100 coincide
    ids, d2, cnt = R.knn(p, base[:10], 4)
    assert (ids[:, 0] == np.arange(10)).all() and (ids[:, 1] == np.arange(10) + 100).all()
    assert (d2[:, :2] == 0).all() and (ids[:, 2] + 100 == ids[:, 3]).all() and (d2[:, 2] == d2[:, 3]).all()
    # an integer lattice queried at a cell centre: eight corners at the same distance, in id order
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    ids, d2, cnt = R.knn(g, np.array([[1.5, 1.5, 1.5]], np.float32), 8)
    assert (d2 == np.float32(0.75)).all() and (np.diff(ids[0]) > 0).all() and cnt[0] == 8


def test_max_range_is_inclusive_and_radius_is_strict():
    p = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 5]], np.float32)
    q = np.zeros((1, 3), np.float32)
    ids, d2, cnt = R.knn(p, q, 4, max_range=3.0)
    assert cnt[0] == 2 and list(ids[0]) == [0, 1, -1, -1] and list(d2[0]) == [0.0, 9.0, INF, INF]
    ids, d2, cnt = R.radius_search(p, q, 3.0, 4)
    assert cnt[0] == 1 and list(ids[0]) == [0, -1, -1, -1] and list(d2[0]) == [0.0, INF, INF, INF]
    ids, d2, cnt = R.radius_search(p, q, 0.0, 2)                       # radius 0: nothing, not even a coincident point
    assert cnt[0] == 0 and (ids == -1).all() and (d2 == INF).all()
    ids, d2, cnt = R.radius_search(p, q, 4.5, 2)                       # the count takes in every point within, the list max_nn of them
    assert cnt[0] == 3 and list(ids[0]) == [0, 1] and list(d2[0]) == [0.0, 9.0]


def test_unused_slots_and_short_clouds():
    p = np.array([[1, 0, 0], [2, 0, 0]], np.float32)
    ids, d2, cnt = R.knn(p, np.zeros((3, 3), np.float32), 5)
    assert (cnt == 2).all() and (ids[:, 2:] == -1).all() and (d2[:, 2:] == INF).all() and (ids[:, :2] == [0, 1]).all()
    ids, d2, cnt = R.knn(np.zeros((0, 3), np.float32), np.zeros((3, 3), np.float32), 2)
    assert (cnt == 0).all() and (ids == -1).all() and (d2 == INF).all()
    ids, d2, cnt = R.knn(p, np.zeros((0, 3), np.float32), 2)
    assert ids.shape == (0, 2) and d2.shape == (0, 2) and cnt.shape == (0,)


def test_non_finite_points_on_either_side():
    nan, inf = np.float32(np.nan), INF
    p = np.array([[0, 0, 0], [nan, 0, 0], [1, 0, 0], [0, inf, 0], [2, 0, 0]], np.float32)
    q = np.array([[0.1, 0, 0], [nan, 0, 0], [0, -inf, 0], [5, 0, 0]], np.float32)
    ids, d2, cnt = R.knn(p, q, 5)
    assert list(cnt) == [3, 0, 0, 3]
    assert list(ids[0]) == [0, 2, 4, -1, -1] and list(ids[3]) == [4, 2, 0, -1, -1]      # ids are positions in the cloud, gaps and all
    assert (ids[1:3] == -1).all() and (d2[1:3] == INF).all()
    # a query made non-finite by the move finds nothing either
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 3e38
    ids, d2, cnt = R.knn(p, np.array([[3e38, 0, 0], [0, 0, 0]], np.float32), 2, T=T)
    assert list(cnt) == [0, 2] and (ids[0] == -1).all()
    ids, d2, cnt = R.radius_search(p, q, 10.0, 2)
    assert list(cnt) == [3, 0, 0, 3]


def test_the_move_rounds_every_operation_on_its_own():
    rng = np.random.default_rng(11)
    T = np.eye(4, dtype=np.float32)
    c, s = np.float32(np.cos(0.3)), np.float32(np.sin(0.3))
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [0.1, -0.2, 0.3]
    q = rng.uniform(-50, 50, (200, 3)).astype(np.float32)
    moved, live = R.move(q, T)
    assert live.all()
    for i in range(0, 200, 17):
        x, y, z = q[i]
        for a in range(3):
            want = np.float32(np.float32(np.float32(np.float32(T[a, 0] * x) + np.float32(T[a, 1] * y)) + np.float32(T[a, 2] * z)) + T[a, 3])
            assert moved[i, a] == want
