"""GPU (-m gpu): the GICP batch (mi355ndt_gicp_batch_*: every candidate of a loop check aligned in one lockstep batch) against the single-pair
surface on the same engine, run first.  Every comparison is tobytes() equality -- final, converged, iterations, inner_status, n_matched,
delta, the aligned cloud -- except test 5, which holds two slots to tools/gicp_ref.py with the bars of tests/test_gicp_gpu.py
(test_align_against_the_restatement): converged flag and outer iterations equal, pose within 1e-4 m / 1e-5 rad.
Shapes are those of tests/test_gicp_gpu.py: synth.make_pair(0, n_azimuth=64) (4,096 points) and its blobs cloud.  No excluded points, no
skipped cases.  Timings: tools/gicp_timing.py --batch, DESIGN.md section 8."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import gicp, loop_closure, ndt, synth

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("gicp_ref")
G0 = synth.default_guess()
I4 = np.eye(4, dtype=np.float32)
FACTORY = {k: R.FACTORY[k] for k in R.DEFAULTS}
KEYS = ("converged", "iterations", "inner_status", "n_matched")


def blobs():
    """the cloud of tests/test_gicp_gpu.py: 2,900 points in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.1
    parts = [(g[:m] + rng.uniform(-0.03, 0.03, (m, 3)) + c) for m, c in ((967, (0, 0, 0)), (967, (8, 3, 0)), (966, (-5, 10, 1)))]
    d = rng.normal(size=(100, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 60, (100, 1))
    p = np.concatenate(parts + [far]).astype(np.float32)
    return p[rng.permutation(len(p))]


BLOBS = blobs()


def set_params(e, **kw):
    e.gicp_set_params(ndt.default_gicp_params(**kw))


def single(e, guess, cloud=None, keyframe=None):
    """the single-pair surface: (the align's record, the aligned cloud)"""
    e.gicp_set_source(cloud, keyframe)
    r = e.gicp_align(guess)
    return r, e.gicp_get_aligned()


def batch(e, sources, guesses):
    """one batch align of `sources` (arrays, or ints = keyframe ids): ([record], [aligned cloud], rounds, requests)"""
    e.gicp_batch_reserve(len(sources))
    for k, s in enumerate(sources):
        if isinstance(s, (int, np.integer)):
            e.gicp_batch_set_source(k, keyframe=int(s))
        else:
            e.gicp_batch_set_source(k, s)
    res = e.gicp_batch_align(np.stack(guesses))
    rounds, req = e.gicp_batch_stats()
    return res, [e.gicp_batch_get_aligned(k) for k in range(len(sources))], rounds, req


def assert_same(got, want, what):
    (rb, ab), (rs, as_) = got, want
    print(f"{what}: batch {[rb[k] for k in KEYS]} delta {rb['delta']!r} | single {[rs[k] for k in KEYS]} delta {rs['delta']!r}")
    assert rb["final"].tobytes() == rs["final"].tobytes(), what
    assert [rb[k] for k in KEYS] == [rs[k] for k in KEYS], what
    assert np.float64(rb["delta"]).tobytes() == np.float64(rs["delta"]).tobytes(), what
    assert ab.shape == as_.shape and ab.tobytes() == as_.tobytes(), what


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(eng):
    """test 1's seven candidates against pair 0's target, factory parameters: the single-pair results first, then ONE batch align"""
    tgt, src, _ = synth.make_pair(0, n_azimuth=64)
    tgt, src = tgt.numpy(), src.numpy()
    set_params(eng, **FACTORY)
    eng.gicp_set_target(tgt)
    eng.gicp_set_source(src)
    idx, _, m = eng.gicp_correspondences(G0)
    hit, miss = np.flatnonzero(idx >= 0), np.flatnonzero(idx < 0)
    assert m == 4058 and len(miss) == 38

    def cut(n_points):                                       # matched points first, as test_correspondences_pair0 cuts them
        return src[np.sort(np.concatenate([hit[:n_points - len(miss)], miss]))]
    D = np.eye(4)
    D[:3, :3] = synth.rot_zyx(0.004, -0.003, 0.005)
    D[:3, 3] = [0.05, -0.03, 0.02]
    moved = R.move_f32(D.astype(np.float32), src)
    G1 = (G0.astype(np.float64) @ np.linalg.inv(D)).astype(np.float32)
    G1[3] = [0, 0, 0, 1]
    sources = [src, moved, src[::2], cut(255), cut(256), cut(257), cut(3 + len(miss))]
    assert [len(s) for s in sources[3:]] == [255, 256, 257, 41]
    guesses = [G0, G1, G0, G0, G0, G0, G0]
    singles = [single(eng, g, s) for s, g in zip(sources, guesses)]
    res, aligned, rounds, req = batch(eng, sources, guesses)
    return dict(tgt=tgt, sources=sources, guesses=guesses, singles=singles, res=res, aligned=aligned, rounds=rounds, req=req)


# ---- 1, 2: the batch against the single-pair surface -------------------------------------------------------------------
def test_mixed_batch_equals_the_single_pair_surface(mixed):
    S = mixed["singles"]
    for k in range(7):
        assert_same((mixed["res"][k], mixed["aligned"][k]), S[k], f"slot {k}")
    rounds, req = mixed["rounds"], mixed["req"]
    print("rounds", rounds, "requests", list(req), "sum", int(req.sum()))
    # the three-match slot ends after round 1 while the others go on -- known from the single-pair results, so the batch ran rounds with
    # part of its slots
    assert (S[6][0]["iterations"], S[6][0]["converged"], S[6][0]["n_matched"], S[6][0]["inner_status"]) == (0, False, 3, -2)
    assert all(S[k][0]["iterations"] >= 1 for k in range(6))
    assert req[6] == 1 and all(req[k] > 1 for k in range(6))
    assert rounds == req.max() and req.sum() > rounds


def test_batch_of_one_equals_the_single_call(eng, mixed):
    set_params(eng, **FACTORY)
    eng.gicp_set_target(mixed["tgt"])
    res, aligned, rounds, req = batch(eng, mixed["sources"][:1], mixed["guesses"][:1])
    assert_same((res[0], aligned[0]), mixed["singles"][0], "K = 1")
    assert rounds == req[0] > 1


# ---- 3: host clouds and keyframes -----------------------------------------------------------------------------------
def test_host_cloud_and_keyframe_slots_give_equal_bytes(eng, mixed):
    set_params(eng, **FACTORY)
    src = mixed["sources"][0]
    eng.gicp_set_target(mixed["tgt"])
    ks = eng.keyframe_add(src)
    eng.gicp_set_source(keyframe=ks)
    cov_before = eng.gicp_covariances(ndt.GICP_SOURCE)
    G2 = mixed["guesses"][1]
    by_id = [single(eng, G0, keyframe=ks), single(eng, G2, keyframe=ks)]
    res, aligned, _, _ = batch(eng, [src, ks, ks], [G0, G0, G2])
    assert_same((res[0], aligned[0]), mixed["singles"][0], "host cloud")
    assert_same((res[1], aligned[1]), (res[0], aligned[0]), "keyframe against host cloud")
    assert_same((res[1], aligned[1]), by_id[0], "keyframe, first guess")
    assert_same((res[2], aligned[2]), by_id[1], "the same keyframe, second guess")
    assert res[2]["final"].tobytes() != res[1]["final"].tobytes()
    eng.gicp_set_source(keyframe=ks)
    assert eng.gicp_covariances(ndt.GICP_SOURCE).tobytes() == cov_before.tobytes()
    assert eng.keyframe_get(ks).tobytes() == src.tobytes()
    # a keyframe the GICP surface has not seen yet: the batch builds its index and covariances, the single call finds them
    k2 = eng.keyframe_add(mixed["sources"][2])
    res, aligned, _, _ = batch(eng, [k2], [G0])
    assert_same((res[0], aligned[0]), mixed["singles"][2], "fresh keyframe")
    assert_same(single(eng, G0, keyframe=k2), mixed["singles"][2], "... and the single call after it")
    eng.keyframe_release(ks)
    eng.keyframe_release(k2)


# ---- 4: the exhaustive path, two slots in one grid ----------------------------------------------------------------------
def test_exhaustive_target_two_slots(eng):
    tgt = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])      # no lattice: fit_tiles with its workgroup barriers
    a = BLOBS[:400].copy() + np.float32(0.01)
    a[7, 0] = np.nan
    b = BLOBS[:300].copy()
    set_params(eng, **dict(FACTORY, corr_dist_threshold=0.5))
    eng.gicp_set_target(tgt)
    singles = [single(eng, I4, a), single(eng, I4, b)]
    res, aligned, rounds, req = batch(eng, [a, b], [I4, I4])
    for k in range(2):
        assert_same((res[k], aligned[k]), singles[k], f"exhaustive slot {k}")
    assert res[0]["n_matched"] >= 300 and rounds == req.max()


# ---- 5: against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_slots_against_the_restatement(eng, mixed, k):
    tgt, src = mixed["tgt"], mixed["sources"][k]
    set_params(eng, **FACTORY)
    eng.gicp_set_target(tgt)
    eng.gicp_set_source(src)
    ct, cs = eng.gicp_covariances(ndt.GICP_TARGET), eng.gicp_covariances(ndt.GICP_SOURCE)
    want = R.align(src, tgt, G0, FACTORY, cov_src=cs, cov_tgt=ct)
    got = mixed["res"][k]
    dt, dr = se3_err(want["final"], got["final"])
    print(f"slot {k}: batch converged {got['converged']} iterations {got['iterations']} | restatement {want['converged']} {want['iterations']} "
          f"| pose difference {dt:.3e} m {dr:.3e} rad")
    assert all(abs(d - 1.0) >= 1e-3 for d in want["deltas"])
    assert (got["converged"], got["iterations"]) == (want["converged"], want["iterations"])
    assert dt <= 1e-4 and dr <= 1e-5
    assert mixed["aligned"][k].tobytes() == R.move_f32(got["final"], src).tobytes()


# ---- 6: what the batch leaves as it was -----------------------------------------------------------------------------------
def test_single_pair_surface_and_ndt_are_left_as_they_were(mixed):
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    tgt, src, _ = synth.make_pair(5, 64, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    e.set_target(tgt)
    e.set_source(src)
    k1 = e.keyframe_add(tgt)
    ndt_before = (e.align(G0), e.get_aligned(), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k1], [np.eye(4)], 1.0))
    gt, gs = mixed["tgt"], mixed["sources"][0]
    set_params(e, **FACTORY)
    e.gicp_set_target(gt)
    r1, a1 = single(e, G0, gs)
    x = [0.03, -0.02, 0.01, 0.004, -0.006, 0.008]
    f1, g1 = e.gicp_cost(x, G0)                                  # over the correspondences the align left resident
    res, _, rounds, _ = batch(e, [gs[::2], mixed["sources"][1], k1], [G0, mixed["guesses"][1], G0])
    assert rounds > 1 and res[0]["iterations"] >= 1
    f2, g2 = e.gicp_cost(x, G0)                                  # the resident correspondences still serve
    assert (np.float64(f2).tobytes(), g2.tobytes()) == (np.float64(f1).tobytes(), g1.tobytes())
    assert e.gicp_get_aligned().tobytes() == a1.tobytes()        # the last final transformation and the source are the single call's
    assert_same(single(e, G0, gs), (r1, a1), "single pair after the batch")
    ndt_after = (e.align(G0), e.get_aligned(), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k1], [np.eye(4)], 1.0))
    assert np.asarray(ndt_before[0]["final"]).tobytes() == np.asarray(ndt_after[0]["final"]).tobytes()
    assert (ndt_before[0]["iterations"], ndt_before[0]["score"], ndt_before[0]["trans_probability"]) == \
        (ndt_after[0]["iterations"], ndt_after[0]["score"], ndt_after[0]["trans_probability"])
    assert ndt_before[1].tobytes() == ndt_after[1].tobytes() and ndt_before[2] == ndt_after[2]
    assert ndt_before[3][0].tobytes() == ndt_after[3][0].tobytes() and np.array_equal(ndt_before[3][1], ndt_after[3][1])
    assert e.keyframe_get(k1).tobytes() == tgt.tobytes()
    e.close()


# ---- 7: errors --------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(ndt.NDTError) as err:
        call()
    return err.value.code, str(err.value)


def test_state_and_argument_errors():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    set_params(e, **FACTORY)
    p = BLOBS[:200]
    two = np.stack([I4, I4])
    assert code_of(lambda: e.gicp_batch_stats())[0] == -7                       # nothing reserved
    assert code_of(lambda: e.gicp_batch_align(np.zeros((0, 4, 4), np.float32)))[0] == -7
    for n in (0, 65, -1):
        c, text = code_of(lambda: e.gicp_batch_reserve(n))
        assert c == -2 and "1..64" in text
    e.gicp_batch_reserve(64)
    e.gicp_batch_reserve(2)                                                      # drops the 64
    assert code_of(lambda: e.gicp_batch_set_source(2, p))[0] == -2               # slots out of range
    assert code_of(lambda: e.gicp_batch_set_source(-1, p))[0] == -2
    assert code_of(lambda: e._chk(e.lib.mi355ndt_gicp_batch_get_aligned(e.h, 2, two.ctypes.data, 12), "gicp_batch_get_aligned"))[0] == -2
    e.gicp_batch_set_source(0, p)
    e.gicp_batch_set_source(1, p[::2])
    c, text = code_of(lambda: e.gicp_batch_align(two))                           # no target
    assert c == -7 and "no target" in text
    e.gicp_set_target(BLOBS)
    e.gicp_batch_reserve(2)
    e.gicp_batch_set_source(0, p)
    c, text = code_of(lambda: e.gicp_batch_align(two))                           # slot 1 unset
    assert c == -7 and "slot 1 is unset" in text
    assert code_of(lambda: e.gicp_batch_get_aligned(0))[0] == -7                 # no batch align has run
    e.gicp_batch_set_source(1, p[:19])                                           # 19 points at k = 20
    c, text = code_of(lambda: e.gicp_batch_align(two))
    assert c == -2 and "slot 1" in text and "k_correspondences (20) exceeds" in text
    e.gicp_batch_set_source(1, p[::2])
    res = e.gicp_batch_align(two)                                                # ... and the next batch align on the same handle succeeds
    ra = single(e, I4, p)
    assert_same((res[0], e.gicp_batch_get_aligned(0)), ra, "after the refused calls")
    assert code_of(lambda: e.gicp_batch_set_source(1, keyframe=7))[0] == -2      # never given out
    kid = e.keyframe_add(p[::2])
    e.gicp_batch_set_source(1, keyframe=kid)
    e.keyframe_release(kid)                                                      # released between set_source_keyframe and batch_align
    c, text = code_of(lambda: e.gicp_batch_align(two))
    assert c == -2 and "released" in text
    assert code_of(lambda: e.gicp_batch_set_source(1, keyframe=kid))[0] == -2
    e.gicp_batch_set_source(1, p[::2])
    e.stream_begin(2, 4, 1024, 1024)
    for call in (lambda: e.gicp_batch_reserve(2), lambda: e.gicp_batch_set_source(0, p), lambda: e.gicp_batch_set_source(0, keyframe=0),
                 lambda: e.gicp_batch_align(two), lambda: e.gicp_batch_get_aligned(0), lambda: e.gicp_batch_stats()):
        assert code_of(call)[0] == -7
    e.stream_end()
    res2 = e.gicp_batch_align(two)                                               # the refused calls changed nothing
    assert res2[0]["final"].tobytes() == res[0]["final"].tobytes() and res2[1]["final"].tobytes() == res[1]["final"].tobytes()
    e.close()


# ---- 8: loop-closure verification ---------------------------------------------------------------------------------------------
def test_verify_candidates_gicp_equals_the_sequential_loop(eng, mixed):
    tgt = mixed["tgt"]
    cands = [mixed["sources"][0], None, mixed["sources"][2]]
    guesses = np.stack([G0, mixed["guesses"][1], G0])
    kid = eng.keyframe_add(mixed["sources"][1])
    cands[1] = kid                                               # ids and arrays mixed
    reg = gicp.GeneralizedIterativeClosestPoint.from_factory(engine=eng)
    kt = eng.keyframe_add(tgt)
    converged, scores, finals = [], [], []
    for c, g in zip(cands, guesses):                             # the reference's loop: align, getFitnessScore, one candidate after the other
        reg.setInputTarget(tgt)
        if isinstance(c, int):
            reg.setInputSource(keyframe=c)
            kc, own = c, False
        else:
            reg.setInputSource(c)
            kc, own = eng.keyframe_add(c), True
        reg.align(g)
        sc, _ = eng.keyframe_fitness_scores([kt], [kc], [reg.getFinalTransformation()], 4.0)
        converged.append(reg.hasConverged()); scores.append(float(sc[0])); finals.append(reg.getFinalTransformation().copy())
        if own:
            eng.keyframe_release(kc)
    n_kf = eng.keyframe_count()
    print("converged", converged, "scores", scores)
    thresh = max(scores) + 1.0                                   # (every converged candidate is within it: the rule's tie and order decide)
    bow = [(0.9, 2), (0.5, 0), (0.01, 1)]                        # the walk ends before candidate 1
    for b, th in ((None, thresh), (None, min(scores) / 2), (bow, min(scores) / 2), (bow, thresh)):
        want = loop_closure.select_matching(converged, scores, finals, th) if b is None else \
            loop_closure.select_matching_and_bow(converged, scores, finals, b, th)
        got = loop_closure.verify_candidates_gicp(eng, kt if b is None else tgt, cands, guesses, 4.0, th, bow=b)
        print("bow" if b else "all", "thresh", th, "->", got[0], got[2], got[3])
        assert (got[0], got[2], got[3]) == (want[0], want[2], want[3])
        assert (got[1] is None and want[1] is None) or got[1].tobytes() == want[1].tobytes()
        assert eng.keyframe_count() == n_kf                      # the call's own keyframes are released
    assert any(converged)
    eng.keyframe_release(kid)
    eng.keyframe_release(kt)
