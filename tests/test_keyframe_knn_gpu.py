"""GPU (-m gpu): mi355ndt_keyframe_knn / _knn_ids / _radius_search -- exact k-nearest and radius search over resident keyframes.  Every
word is compared with tools/knn_ref.py, the brute-force restatement: ids and counts as integers, d2 as bit patterns; and with the surfaces
that run the same search internally (ICP's correspondences, the keyframe fitness scores' index)."""
import numpy as np
import pytest

from lv_slam_amd import ndt, search
from tools import knn_ref as R

pytestmark = pytest.mark.gpu
ORDERS = (ndt.KNN_ORDER_INPUT, ndt.KNN_ORDER_CELL)
INF = np.float32(np.inf)


def cloud(n, seed, half=8.0):
    """n points of a few surfaces' worth of structure inside +-half m: walls and a floor, jittered"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-half, half, (n, 3)).astype(np.float32)
    wall = rng.integers(0, 3, n)
    p[np.arange(n), wall] = (np.round(p[np.arange(n), wall] / 4.0) * 4.0 + rng.normal(0, 0.02, n)).astype(np.float32)
    return p


def pose(seed, shift=0.3):
    rng = np.random.default_rng(seed)
    yaw = rng.normal(0, 0.05)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = rng.normal(0, shift, 3)
    return T


def same(got, want):
    return all(np.asarray(g).dtype == w.dtype and np.asarray(g).shape == w.shape and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(got, want))


def describe(got, want):
    bad = [(name, int((np.asarray(g) != w).sum())) for name, g, w in zip(("ids", "d2", "counts"), got, want)]
    return f"words that differ: {bad}"


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine()
    yield e
    e.close()


class Store:
    """keyframes of one engine by (size, seed): uploaded once, shared by the tests"""

    def __init__(self, e):
        self.e, self.kf = e, {}

    def get(self, n, seed=0):
        if (n, seed) not in self.kf:
            c = cloud(n, 100 + seed)
            self.kf[(n, seed)] = (self.e.keyframe_add(c), c)
        return self.kf[(n, seed)]


@pytest.fixture(scope="module")
def store(eng):
    return Store(eng)


def check_knn(e, kid, c, q, k, max_range=float("inf"), T=None):
    want = R.knn(c, q, k, max_range, T)
    out = None
    for order in ORDERS:
        got = e.keyframe_knn(kid, q, k, max_range, T, order)
        assert same(got, want), f"order {order}: " + describe(got, want)
        out = got
    assert same(e.keyframe_knn(kid, q, k, max_range, T), want)          # the engine's choice
    return out


def check_radius(e, kid, c, q, radius, max_nn, T=None):
    want = R.radius_search(c, q, radius, max_nn, T)
    for order in ORDERS:
        got = e.keyframe_radius_search(kid, q, radius, max_nn, T, order)
        assert same(got, want), f"order {order}: " + describe(got, want)
    return want


# ---- wave and list edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tgt", [1, 4, 257, 4096])
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 4096])
def test_query_counts_and_cloud_sizes(eng, store, n_tgt, nq):
    kid, c = store.get(n_tgt)
    q = cloud(nq, 7 * nq + n_tgt) + np.float32(0.05)
    ids, d2, cnt = check_knn(eng, kid, c, q, 5)
    assert (cnt == min(5, n_tgt)).all()


@pytest.mark.parametrize("k", [1, 5, 8, 9, 20, 32, 33, 64])
def test_every_side_of_every_list_capacity(eng, store, k):
    for n_tgt in (257, 4096):
        kid, c = store.get(n_tgt)
        check_knn(eng, kid, c, cloud(200, k) + np.float32(0.03), k)
    kid, c = store.get(4)                                             # fewer points than k (but for k = 1)
    ids, d2, cnt = check_knn(eng, kid, c, cloud(70, k), k)
    assert (cnt == min(k, 4)).all() and (ids[:, min(k, 4):] == -1).all() and (d2[:, min(k, 4):] == INF).all()


# ---- queries ----------------------------------------------------------------------------------------------------------
def test_queries_outside_the_lattice_far_away_and_moved(eng, store):
    kid, c = store.get(4096)
    rng = np.random.default_rng(5)
    outside = rng.uniform(-30, 30, (300, 3)).astype(np.float32)       # most of them outside the cloud's +-8 m box
    far = (rng.uniform(-1, 1, (65, 3)) * 1e6).astype(np.float32)
    far[0] = [1e6, 1e6, 1e6]
    mixed = np.concatenate([outside[:100], far[:10], cloud(100, 9)])
    for q in (outside, far, mixed):
        for T in (None, pose(1), pose(2, 5.0)):
            check_knn(eng, kid, c, q, 5, T=T)
            check_knn(eng, kid, c, q, 20, T=T)


def test_queries_from_a_keyframe_equal_queries_from_the_host(eng, store):
    kid, c = store.get(4096)
    qid, q = store.get(257, seed=3)
    T = pose(4)
    want = R.knn(c, q, 9, T=T.astype(np.float32))
    for order in ORDERS:
        got = eng.keyframe_knn_ids([kid], [qid], [T], 9, query_order=order)
        assert same(got, want), describe(got, want)
        assert same(eng.keyframe_knn(kid, q, 9, T=T.astype(np.float32), query_order=order), want)


# ---- ranges -----------------------------------------------------------------------------------------------------------
def test_max_range_cuts_lists_short_or_empties_them(eng, store):
    kid, c = store.get(4096)
    q = cloud(300, 21) + np.float32(0.04)
    full = R.knn(c, q, 20)
    r_mid = float(np.sqrt(np.median(full[1][:, 10].astype(np.float64))))
    ids, d2, cnt = check_knn(eng, kid, c, q, 20, max_range=r_mid)
    assert 0 < (cnt < 20).sum() and (cnt > 0).any()
    # a distance exactly on the limit is kept: the limit is the square root of an entry that has an exact one
    c2 = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32)
    k2 = eng.keyframe_add(c2)
    ids, d2, cnt = check_knn(eng, k2, c2, np.zeros((1, 3), np.float32), 3, max_range=3.0)
    assert cnt[0] == 2 and list(ids[0]) == [0, 1, -1]
    eng.keyframe_release(k2)
    r_none = float(np.sqrt(full[1][:, 0].astype(np.float64).min())) * 0.5
    ids, d2, cnt = check_knn(eng, kid, c, q, 20, max_range=r_none)
    assert (cnt == 0).all() and (ids == -1).all() and (d2 == INF).all()
    check_knn(eng, kid, c, q, 5, max_range=0.0)


# ---- ties -------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_id(eng):
    base = cloud(1000, 31)
    dup = np.concatenate([base, base])[np.random.default_rng(1).permutation(2000)]
    kid = eng.keyframe_add(dup)
    for k in (1, 2, 5, 8):
        check_knn(eng, kid, dup, base[:300], k)
        check_knn(eng, kid, dup, cloud(100, 32), k)
    eng.keyframe_release(kid)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    g = g[np.random.default_rng(2).permutation(len(g))]
    kid = eng.keyframe_add(g)
    centres = (np.stack(np.meshgrid(np.arange(11), np.arange(11), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3) + 0.5).astype(np.float32)
    for k in (1, 8, 9, 32):
        ids, d2, cnt = check_knn(eng, kid, g, centres, k)
    assert (d2[:, :8] == np.float32(0.75)).all() and (np.diff(ids[:, :8], axis=1) > 0).all()
    eng.keyframe_release(kid)


# ---- non-finite points ------------------------------------------------------------------------------------------------
def test_non_finite_queries_and_non_finite_searched_points(eng, store):
    kid, c = store.get(4096)
    q = cloud(200, 41)
    q[3, 0] = np.nan
    q[64, 1] = np.inf
    q[65, 2] = -np.inf
    q[199] = np.nan
    ids, d2, cnt = check_knn(eng, kid, c, q, 5, T=pose(6))
    assert (cnt[[3, 64, 65, 199]] == 0).all() and (cnt[[0, 1, 2, 66]] == 5).all()
    check_radius(eng, kid, c, q, 1.0, 8)
    holes = cloud(1000, 42)
    holes[::7, 0] = np.nan
    holes[5::11, 2] = np.inf
    k2 = eng.keyframe_add(holes)
    ids, d2, cnt = check_knn(eng, k2, holes, cloud(300, 43), 9)
    assert np.isfinite(holes[ids.ravel()]).all()
    check_radius(eng, k2, holes, cloud(300, 43), 1.5, 16)
    eng.keyframe_release(k2)
    # a query the move makes non-finite
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 3e38
    big = np.array([[3e38, 0, 0], [0, 0, 0]], np.float32)
    ids, d2, cnt = check_knn(eng, kid, c, big, 3, T=T)
    assert cnt[0] == 0


# ---- no lattice, nothing to search --------------------------------------------------------------------------------------
def test_a_stray_point_leaves_no_lattice_and_the_words_stay(eng):
    c = cloud(700, 51)
    c[123] = [1e12, 0, 0]
    kid = eng.keyframe_add(c)
    q = np.concatenate([cloud(130, 52), np.array([[9e11, 0, 0]], np.float32)])
    for k in (1, 5, 33):
        check_knn(eng, kid, c, q, k)
    check_knn(eng, kid, c, q, 5, max_range=0.5, T=pose(7))
    check_radius(eng, kid, c, q, 1.0, 8)
    eng.keyframe_release(kid)


def test_nothing_to_search(eng):
    q = cloud(70, 61)
    for c in (np.full((100, 3), np.nan, np.float32), np.zeros((0, 3), np.float32)):
        kid = eng.keyframe_add(c)
        ids, d2, cnt = check_knn(eng, kid, c, q, 5)
        assert (cnt == 0).all() and (ids == -1).all() and (d2 == INF).all()
        want = check_radius(eng, kid, c, q, 10.0, 4)
        assert (want[2] == 0).all()
        eng.keyframe_release(kid)


# ---- invariance ---------------------------------------------------------------------------------------------------------
def test_no_word_depends_on_the_cell_size(eng, store):
    _, c = store.get(4096)
    q = np.concatenate([cloud(300, 71), np.random.default_rng(3).uniform(-30, 30, (100, 3)).astype(np.float32)])
    want_k, want_r = R.knn(c, q, 20, 2.0), R.radius_search(c, q, 0.7, 8)
    for cell in (50, 400):
        e = ndt.Engine()
        e.set_option(ndt.OPT_KF_FITNESS_CELL_MM, cell)
        kid = e.keyframe_add(c)
        for order in ORDERS:
            assert same(e.keyframe_knn(kid, q, 20, 2.0, query_order=order), want_k), (cell, order)
            assert same(e.keyframe_radius_search(kid, q, 0.7, 8, query_order=order), want_r), (cell, order)
        e.close()


# ---- the item entry ---------------------------------------------------------------------------------------------------
def test_items_equal_one_item_calls(eng, store):
    a, _ = store.get(4096)
    b, _ = store.get(257)
    stray = cloud(300, 81)
    stray[7] = [1e12, 0, 0]
    s = eng.keyframe_add(stray)                                       # an item without a lattice rides the same call
    q1, _ = store.get(4096, seed=5)
    q2, _ = store.get(257, seed=3)
    q3, _ = store.get(1)
    searched, queries = [a, b, a, s, b], [q2, q1, q3, q2, b]
    poses = [pose(10 + i) for i in range(5)]
    sizes = [eng.keyframe_get(x, fetch=False) for x in queries]
    for order in ORDERS:
        before = eng.profile_get()
        ids, d2, cnt = eng.keyframe_knn_ids(searched, queries, poses, 9, 3.0, order)
        after = eng.profile_get()
        assert after["cloud_uploads"] == before["cloud_uploads"] and after["cloud_upload_bytes"] == before["cloud_upload_bytes"]
        assert ids.shape == (sum(sizes), 9)
        at = 0
        for i in range(5):
            one = eng.keyframe_knn_ids([searched[i]], [queries[i]], [poses[i]], 9, 3.0, order)
            sl = slice(at, at + sizes[i])
            assert same((ids[sl], d2[sl], cnt[sl]), one), (order, i)
            want = R.knn(eng.keyframe_get(searched[i]), eng.keyframe_get(queries[i]), 9, 3.0, poses[i].astype(np.float32))
            assert same(one, want), (order, i, describe(one, want))
            at += sizes[i]
    # a wrong total: refused, nothing written
    p = ndt.KnnParams(9, 3.0, 0)
    import ctypes as C
    n = sum(sizes)
    oi, od, oc = np.full((n + 1, 9), 77, np.int32), np.full((n + 1, 9), 7.0, np.float32), np.full(n + 1, 7, np.int32)
    si, qi = np.asarray(searched, np.int32), np.asarray(queries, np.int32)
    pcm = np.ascontiguousarray(np.transpose(np.asarray(poses), (0, 2, 1))).reshape(5, 16)
    for total in (n + 1, n - 1):
        rc = eng.lib.mi355ndt_keyframe_knn_ids(eng.h, 5, si.ctypes.data_as(C.c_void_p), qi.ctypes.data_as(C.c_void_p), pcm.ctypes.data_as(C.c_void_p),
                                               C.byref(p), total, oi.ctypes.data_as(C.c_void_p), od.ctypes.data_as(C.c_void_p), oc.ctypes.data_as(C.c_void_p))
        assert rc == -2 and b"total_queries" in eng.lib.mi355ndt_last_error(eng.h)
        assert (oi == 77).all() and (od == 7.0).all() and (oc == 7).all()
    eng.keyframe_release(s)


# ---- radius -----------------------------------------------------------------------------------------------------------
def test_radius_search(eng, store):
    kid, c = store.get(4096)
    q = cloud(300, 91) + np.float32(0.02)
    ids, d2, cnt = check_radius(eng, kid, c, q, 1.5, 8)               # counts above max_nn, the lists hold the nearest max_nn
    assert (cnt > 8).any()
    full = cnt > 8
    assert (ids[full] == R.knn(c, q, 8)[0][full]).all()
    for max_nn in (1, 9, 33, 64):
        check_radius(eng, kid, c, q, 0.8, max_nn)
    ids, d2, cnt = check_radius(eng, kid, c, q, 1e3, 64)              # the whole cloud
    assert (cnt == 4096).all()
    check_radius(eng, kid, c, q, float("inf"), 4)
    check_radius(eng, kid, c, q, 0.6, 8, T=pose(12))
    base = cloud(500, 92)
    dup = np.concatenate([base, base])
    k2 = eng.keyframe_add(dup)
    ids, d2, cnt = check_radius(eng, k2, dup, base[:100], 0.0, 4)     # strict: radius 0 finds nothing, coincident points included
    assert (cnt == 0).all() and (ids == -1).all()
    # a distance exactly on the radius is not within
    c3 = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32)
    k3 = eng.keyframe_add(c3)
    ids, d2, cnt = check_radius(eng, k3, c3, np.zeros((1, 3), np.float32), 3.0, 3)
    assert cnt[0] == 1 and list(ids[0]) == [0, -1, -1]
    eng.keyframe_release(k2)
    eng.keyframe_release(k3)


# ---- the surfaces that run the same search ----------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [None, 0.2])
def test_k1_equals_icp_correspondences(eng, store, thr):
    kid, tgt = store.get(4096)
    sid, src = store.get(4096, seed=5)
    G = pose(13).astype(np.float32)
    eng.icp_set_params(ndt.default_icp_params(**({} if thr is None else dict(corr_dist_threshold=thr))))
    eng.icp_set_target(None, kid)
    eng.icp_set_source(None, sid)
    idx, d2i, sums, m = eng.icp_correspondences(G)
    mr = float(ndt.default_icp_params().corr_dist_threshold) if thr is None else thr
    ids, d2, cnt = eng.keyframe_knn(kid, src, 1, mr, G)
    matched = cnt == 1
    assert matched.sum() == m and (thr is None or 0 < m < len(src))
    assert (idx == ids[:, 0]).all()                                   # unmatched: -1 on both surfaces
    assert d2i[matched].tobytes() == d2[matched, 0].tobytes()
    assert (d2i[~matched] == 0).all() and (d2[~matched, 0] == INF).all()


def test_the_index_is_shared_with_the_fitness_scores_both_ways():
    c, s = cloud(4096, 111), cloud(2000, 112)
    T, q = pose(14), cloud(300, 113)
    want = R.knn(c, q, 5)
    # fitness first, then the search
    e = ndt.Engine()
    a, b = e.keyframe_add(c), e.keyframe_add(s)
    sc1 = e.keyframe_fitness_scores([a], [b], [T], 1.0)
    assert same(e.keyframe_knn(a, q, 5), want)
    sc2 = e.keyframe_fitness_scores([a], [b], [T], 1.0)
    e.close()
    # the search first, then the fitness scores
    e = ndt.Engine()
    a, b = e.keyframe_add(c), e.keyframe_add(s)
    assert same(e.keyframe_knn(a, q, 5), want)
    sc3 = e.keyframe_fitness_scores([a], [b], [T], 1.0)
    assert same(e.keyframe_knn(a, q, 5), want)
    e.close()
    for x in (sc2, sc3):
        assert x[0].tobytes() == sc1[0].tobytes() and x[1].tobytes() == sc1[1].tobytes()


# ---- state and arguments ------------------------------------------------------------------------------------------------
def test_refused_calls(eng, store):
    kid, c = store.get(257)
    q = cloud(10, 121)
    want = R.knn(c, q, 5)
    gone = eng.keyframe_add(c[:10])
    eng.keyframe_release(gone)
    bad = [lambda: eng.keyframe_knn(kid, q, 0), lambda: eng.keyframe_knn(kid, q, 65), lambda: eng.keyframe_knn(kid, q, 5, -1.0),
           lambda: eng.keyframe_knn(kid, q, 5, float("nan")), lambda: eng.keyframe_knn(gone, q, 5), lambda: eng.keyframe_knn(10 ** 6, q, 5),
           lambda: eng.keyframe_knn(kid, q, 5, query_order=3),
           lambda: eng.keyframe_radius_search(kid, q, -1.0, 4), lambda: eng.keyframe_radius_search(kid, q, float("nan"), 4),
           lambda: eng.keyframe_radius_search(kid, q, 1.0, 0), lambda: eng.keyframe_radius_search(kid, q, 1.0, 65),
           lambda: eng.keyframe_radius_search(gone, q, 1.0, 4),
           lambda: eng.keyframe_knn_ids([kid], [gone], [np.eye(4)], 5, total_queries=10), lambda: eng.keyframe_knn_ids([10 ** 6], [kid], [np.eye(4)], 5, total_queries=257),
           lambda: eng.keyframe_knn_ids([kid], [kid], [np.eye(4)], 65)]
    for f in bad:
        with pytest.raises(ndt.NDTError) as ex:
            f()
        assert ex.value.code == -2 and str(ex.value).strip() != "", f
    with pytest.raises(ndt.NDTError) as ex:
        eng.keyframe_knn(gone, q, 5)
    assert "released" in str(ex.value)
    with pytest.raises(ndt.NDTError) as ex:
        eng.keyframe_knn(10 ** 6, q, 5)
    assert "never given out" in str(ex.value)
    import ctypes as C
    p = ndt.KnnParams(5, float("inf"), 0)
    out = np.zeros(64, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert eng.lib.mi355ndt_keyframe_knn(eng.h, kid, vp(q), 10, 8, None, C.byref(p), vp(out), vp(out), vp(out)) == -2      # stride < 12
    assert eng.lib.mi355ndt_keyframe_knn(eng.h, kid, vp(q), 10, 12, None, C.byref(p), None, vp(out), vp(out)) == -2       # a null output
    assert eng.lib.mi355ndt_keyframe_radius_search(eng.h, kid, vp(q), 10, 12, None, 1.0, 4, 0, vp(out), vp(out), None) == -2
    assert eng.lib.mi355ndt_last_error(eng.h) != b""
    # n = 0 and no items: fine, nothing written
    ids, d2, cnt = eng.keyframe_knn(kid, np.zeros((0, 3), np.float32), 5)
    assert ids.shape == (0, 5) and cnt.shape == (0,)
    ids, d2, cnt = eng.keyframe_knn_ids([], [], np.zeros((0, 4, 4)), 5)
    assert ids.shape == (0, 5)
    assert same(eng.keyframe_knn(kid, q, 5), want)                    # ... and the surface works as before


def test_refused_in_stream_mode_and_the_stream_is_left_alone():
    from lv_slam_amd import synth
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    c = cloud(1000, 131)
    q = cloud(70, 132)
    kid = e.keyframe_add(c)
    want = R.knn(c, q, 5)
    tgt, src, _ = synth.make_pair(1, 128, n_beams=32)
    tgt, src = np.ascontiguousarray(tgt.numpy(), np.float32), np.ascontiguousarray(src.numpy(), np.float32)
    G = np.ascontiguousarray(synth.default_guess().T).ravel()

    def one_batch(poke):
        """a streamed batch of one pair, `poke` called between its submit and its collect: the pair's result"""
        e.stream_begin(2, 4, 4096, 4096)
        try:
            bid = e.stream_submit_host_raw([tgt.ctypes.data], [len(tgt)], [src.ctypes.data], [len(src)], 12, G)
            poke()
            return e.stream_collect(bid, 1)[0]
        finally:
            e.stream_end()

    def refused():
        for f in (lambda: e.keyframe_knn(kid, q, 5), lambda: e.keyframe_radius_search(kid, q, 1.0, 4),
                  lambda: e.keyframe_knn_ids([kid], [kid], [np.eye(4)], 5, total_queries=1000)):
            with pytest.raises(ndt.NDTError) as ex:
                f()
            assert ex.value.code == -7 and "stream" in str(ex.value)

    plain, poked = one_batch(lambda: None), one_batch(refused)
    assert poked["final"].tobytes() == plain["final"].tobytes() and poked["iterations"] == plain["iterations"] and poked["score"] == plain["score"]
    assert e.keyframe_count() == 1
    assert same(e.keyframe_knn(kid, q, 5), want)
    e.close()


# ---- the Python mirror --------------------------------------------------------------------------------------------------
def test_kdtree_mirror_owns_what_it_uploads_and_borrows_what_it_is_given(eng, store):
    kid, c = store.get(257)
    q = cloud(70, 141)
    n0 = eng.keyframe_count()
    tree = search.KdTreeFLANN(engine=eng)
    tree.setInputCloud(c)
    assert eng.keyframe_count() == n0 + 1
    ids, d2 = tree.nearestKSearch(q, 5)
    want = R.knn(c, q, 5)
    assert same((ids, d2), want[:2])
    assert same(tree.radiusSearch(q, 1.0, 8), R.radius_search(c, q, 1.0, 8))
    ids1, _ = tree.nearestKSearch(q[0], 1)                            # one point
    assert ids1.shape == (1, 1) and ids1[0, 0] == want[0][0, 0]
    tree.setInputCloud(keyframe=kid)                                  # the owned keyframe goes, the borrowed one is used
    assert eng.keyframe_count() == n0
    assert same(tree.nearestKSearch(q, 5), want[:2])
    tree.close()
    assert eng.keyframe_count() == n0                                 # a borrowed id is not released
    assert same(eng.keyframe_knn(kid, q, 5), want)
    tree = search.KdTreeFLANN(engine=eng)
    tree.setInputCloud(c)
    tree.close()
    assert eng.keyframe_count() == n0                                 # an owned one is
