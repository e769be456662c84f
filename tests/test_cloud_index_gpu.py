"""GPU (-m gpu): a resident keyframe owns ONE spatial index (CloudIndex), built by whichever of mi355ndt_keyframe_fitness_scores and the GICP
surface searches it first and found by the other.  Every comparison here is of bytes: the scores, inlier counts, covariances, idx, M, m and
final poses do not depend on which surface built the index, on the cell it was built with, on a release of another keyframe or on an outlier
call in between, and they equal what host clouds give (a one-pair engine's fitness_score(T=...), gicp_set_target(cloud)).

Four keyframes, the smallest shapes at which sharing can go wrong: 65 points (one live lane in a second wave, k = 20 still served), 257 (a
second 256-tile with one point), 600 blob points with three non-finite rows, 300 blob points and one at 1e12 m (no lattice: both surfaces
take the exhaustive path)."""
import numpy as np
import pytest

from lv_slam_amd import ndt

pytestmark = pytest.mark.gpu


def blobs():
    """the outlier test's cloud: 2,900 points in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.1
    parts = [(g[:m] + rng.uniform(-0.03, 0.03, (m, 3)) + c) for m, c in ((967, (0, 0, 0)), (967, (8, 3, 0)), (966, (-5, 10, 1)))]
    d = rng.normal(size=(100, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 60, (100, 1))
    p = np.concatenate(parts + [far]).astype(np.float32)
    return p[rng.permutation(len(p))]


def clouds():
    b = blobs()
    nan = b[:600].copy()
    nan[100, 0] = np.nan
    nan[433, 2] = np.nan
    nan[599, 1] = np.inf
    return {"n65": np.random.default_rng(65).normal(0, 0.5, (65, 3)).astype(np.float32),
            "n257": np.random.default_rng(257).normal(0, 0.5, (257, 3)).astype(np.float32),
            "nan600": nan,
            "stray": np.concatenate([b[:300], np.array([[1e12, 0, 0]], np.float32)])}, b


CLOUDS, BLOBS = clouds()
NAMES = list(CLOUDS)


def pose(tx, ty, tz, yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    T[:3, 3] = [tx, ty, tz]
    return T


# (searched, moved, relative pose): every keyframe searched, both paths on both sides, a self edge, one keyframe searched twice
EDGES = [("n257", "n65", pose(0.05, -0.02, 0.01, 0.01)), ("nan600", "n257", pose(0.1, 0.05, 0.0, -0.02)), ("n257", "nan600", pose(-0.1, 0.0, 0.02, 0.0)),
         ("stray", "n65", pose(0.0, 0.1, 0.0, 0.03)), ("n65", "stray", pose(0.02, 0.0, 0.0, 0.0)), ("n257", "n257", pose(0.01, 0.01, 0.0, 0.005)),
         ("stray", "stray", np.eye(4))]
MAX_RANGE = 1.0
GUESS = pose(0.03, -0.02, 0.01, 0.01).astype(np.float32)


def engine():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    e.gicp_set_params(ndt.default_gicp_params(k_correspondences=20, max_iterations=20))
    return e


def add_all(e):
    return {name: e.keyframe_add(CLOUDS[name]) for name in NAMES}


def scores_by_id(e, ids, edges=EDGES):
    s, n = e.keyframe_fitness_scores([ids[a] for a, _, _ in edges], [ids[b] for _, b, _ in edges], [T for _, _, T in edges], MAX_RANGE)
    return {"scores": s.tobytes(), "inliers": n.astype(np.int64).tobytes()}


def gicp_results(e, set_side, names=NAMES, pair=True):
    """covariances of each cloud, then correspondences and align of 257 -> 600; set_side(role, name) puts a cloud on a side"""
    out = {}
    for name in names:
        set_side(ndt.GICP_TARGET, name)
        out["cov_" + name] = e.gicp_covariances(ndt.GICP_TARGET).tobytes()
    if pair:
        set_side(ndt.GICP_TARGET, "nan600")
        set_side(ndt.GICP_SOURCE, "n257")
        idx, M, m = e.gicp_correspondences(GUESS)
        r = e.gicp_align(GUESS)
        assert m >= 4 and r["iterations"] >= 1                   # (the pair is one the optimiser works on)
        out.update(idx=idx.tobytes(), M=M.tobytes(), m=m, final=r["final"].tobytes(), converged=r["converged"], iterations=r["iterations"],
                   n_matched=r["n_matched"], aligned=e.gicp_get_aligned().tobytes())
    return out


def gicp_by_id(e, ids, **kw):
    def set_side(role, name):
        (e.gicp_set_target if role == ndt.GICP_TARGET else e.gicp_set_source)(keyframe=ids[name])
    return gicp_results(e, set_side, **kw)


def fitness_then_gicp(between=None):
    """engine A: the fitness surface builds every index, the GICP surface finds them; between(e): called between the two"""
    e = engine()
    ids = add_all(e)
    got = scores_by_id(e, ids)
    if between:
        between(e)
    got.update(gicp_by_id(e, ids))
    return e, ids, got


_A = {}


def result_a():
    """engine A's bytes, computed once and shared (never changed)"""
    if not _A:
        e, _, got = fitness_then_gicp()
        e.close()
        _A.update(got)
    return _A


def test_the_order_of_the_two_surfaces_does_not_matter():
    a = result_a()
    e = engine()                                                # engine B: GICP builds every index, the fitness surface finds them
    ids = add_all(e)
    b = gicp_by_id(e, ids)
    b.update(scores_by_id(e, ids))
    e.close()
    e = engine()                                                # engine C: host clouds, and a one-pair engine for the scores
    c = gicp_results(e, lambda role, name: (e.gicp_set_target if role == ndt.GICP_TARGET else e.gicp_set_source)(CLOUDS[name]))
    s, n = [], []
    for searched, moved, T in EDGES:
        e.set_target(CLOUDS[searched])
        e.set_source(CLOUDS[moved])
        score, inl = e.fitness_score(MAX_RANGE, T=T)
        s.append(score)
        n.append(inl)
    e.close()
    c.update(scores=np.array(s, np.float64).tobytes(), inliers=np.array(n, np.int64).tobytes())
    assert np.frombuffer(a["inliers"], np.int64).min() >= 1     # (every edge scores something)
    assert a.keys() == b.keys() == c.keys()
    for key in a:
        assert a[key] == b[key], f"fitness first against GICP first: {key}"
        assert a[key] == c[key], f"keyframes by id against host clouds: {key}"


def test_the_cell_option_between_the_two_uses_changes_no_word():
    e, _, got = fitness_then_gicp(lambda e: e.set_option(ndt.OPT_KF_FITNESS_CELL_MM, 400))
    assert e.get_option(ndt.OPT_KF_FITNESS_CELL_MM) == 400
    e.close()
    assert got == result_a()


def test_release_of_one_keyframe_leaves_the_others_and_a_new_one_gives_the_same_bytes():
    a = result_a()
    e, ids, _ = fitness_then_gicp()
    e.keyframe_release(ids["n257"])
    with pytest.raises(ndt.NDTError) as err:
        scores_by_id(e, ids)
    assert err.value.code == -2
    with pytest.raises(ndt.NDTError) as err:
        e.gicp_set_target(keyframe=ids["n257"])
    assert err.value.code == -2
    with pytest.raises(ndt.NDTError) as err:                    # (the source of the last align)
        e.gicp_align(GUESS)
    assert err.value.code == -2
    keep = [i for i, (s, m, _) in enumerate(EDGES) if "n257" not in (s, m)]
    others = scores_by_id(e, ids, [EDGES[i] for i in keep])
    assert others["scores"] == np.frombuffer(a["scores"], np.float64)[keep].tobytes()
    assert others["inliers"] == np.frombuffer(a["inliers"], np.int64)[keep].tobytes()
    rest = [name for name in NAMES if name != "n257"]
    cov = gicp_by_id(e, ids, names=rest, pair=False)
    assert all(cov["cov_" + name] == a["cov_" + name] for name in rest)
    ids["n257"] = e.keyframe_add(CLOUDS["n257"])                # the same points under a new id
    again = scores_by_id(e, ids)
    again.update(gicp_by_id(e, ids))
    e.close()
    assert again == a


def outliers(e):
    e.prefilter(BLOBS, use_distance_filter=False, downsample_resolution=0.0, fetch=False)
    return e.prefilter_outliers(return_stats=True)


def test_an_outlier_call_in_between_disturbs_nothing():
    seen = []
    e, _, got = fitness_then_gicp(lambda e: seen.append(outliers(e)))
    e.close()
    assert got == result_a()
    e = engine()
    out, stats = outliers(e)
    e.close()
    assert 0 < len(out) < len(BLOBS) and seen[0][0].tobytes() == out.tobytes()
    assert seen[0][1]["dist"].tobytes() == stats["dist"].tobytes()
    assert {k: v for k, v in seen[0][1].items() if k != "dist"} == {k: v for k, v in stats.items() if k != "dist"}
