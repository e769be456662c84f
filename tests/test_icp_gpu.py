"""GPU (-m gpu): the ICP surface (mi355ndt_icp_*: pcl::IterativeClosestPoint, registration_method = ICP) against tools/icp_ref.py.

  one step         idx and m exactly, d2 word for word, each of the 16 sums within 1e-11 of the sum of its absolute terms (the bar of the
                   GICP cost sums: the same tree).
  the fused move   two iterations through the align path, the working cloud word for word.
  align            pairs 0-3, from the identity and from default_guess(), four parameter sets (32 cases): converged, state and iterations
                   equal, pose within 1e-4 m / 1e-5 rad; and on the restatement alone the deciding quantity of the last two iterations
                   (tr2 against the epsilon, or the MSE difference against 1e-12) at least 1 % away from its threshold.  All 32 cases
                   have that margin (the smallest: 6.9 % -- pair 2, identity, epsilon 1e-6 with corr_dist_threshold 1.0): none was replaced.
The aligns' restatement screens its nearest-point candidates with a kd-tree (tools/icp_ref.py _nearest_screened: provably the exhaustive
answer; tests/test_icp_cpu.py compares the two); the steps use the exhaustive search unless said otherwise.
No excluded points, no skipped cases.  Timings: tools/icp_timing.py, DESIGN.md section 8."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import icp, ndt, synth

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("icp_ref")
G0 = synth.default_guess()
I4 = np.eye(4, dtype=np.float32)
SETS = {"factory": R.FACTORY, "eps1e-6": dict(R.FACTORY, transformation_epsilon=1e-6),
        "eps1e-6_corr1": dict(R.FACTORY, transformation_epsilon=1e-6, corr_dist_threshold=1.0), "max3": dict(R.DEFAULTS, max_iterations=3)}
_PAIR = {}


def pair(p):
    if p not in _PAIR:
        tgt, src, dT = synth.make_pair(p, n_azimuth=64)
        _PAIR[p] = (tgt.numpy(), src.numpy(), dT)
    return _PAIR[p]


def blobs():
    """2,900 points in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away (the GICP tests' cloud)"""
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
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    yield e
    e.close()


def set_params(e, **kw):
    kw.pop("use_reciprocal_correspondences", None)
    e.icp_set_params(ndt.default_icp_params(**kw))


def check_step(e, src, tgt, guess, T=None, thr=None, exhaustive=True):
    set_params(e, **({} if thr is None else dict(corr_dist_threshold=thr)))
    e.icp_set_target(tgt)
    e.icp_set_source(src)
    idx, d2, sums, m = e.icp_correspondences(guess, T)
    want = R.one_step(src, tgt, guess, T, R.DEFAULTS["corr_dist_threshold"] if thr is None else thr, exhaustive=exhaustive)
    print(f"n {len(src)} threshold {thr}: matched {m} (restatement {want['m']})")
    assert m == want["m"] and np.array_equal(idx, want["idx"])
    assert d2.tobytes() == want["d2"].tobytes()
    for k in range(16):
        print(f"  sum[{k}]: engine {sums[k]!r} restatement {want['sums'][k]!r} |diff| {abs(sums[k] - want['sums'][k]):.3e} bar {1e-11 * want['abs_sums'][k]:.3e}")
    assert all(abs(sums[k] - want["sums"][k]) <= 1e-11 * want["abs_sums"][k] for k in range(16))
    idx2, d22, sums2, m2 = e.icp_correspondences(guess, T)       # two calls, equal bytes
    assert (idx2.tobytes(), d22.tobytes(), sums2.tobytes(), m2) == (idx.tobytes(), d2.tobytes(), sums.tobytes(), m)
    return idx, d2, sums, m


# ---- one step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096])
def test_step_source_sizes_on_the_lattice(eng, n):
    tgt, src, _ = pair(0)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = synth.rot_zyx(0.004, -0.003, 0.002).astype(np.float32)
    T[:3, 3] = [0.05, -0.02, 0.01]
    _, _, _, m = check_step(eng, src[:n], tgt, G0, T)
    assert m == n                                               # the default distance: every finite point matches


def test_step_slot_wrap(eng):
    # 65,537 + 300 points: 258 chunks, so the chunks' slots c % 256 wrap
    tgt, src, _ = pair(0)
    rng = np.random.default_rng(3)
    big = (np.tile(src, (17, 1))[:65837] + rng.normal(0, 0.05, (65837, 3))).astype(np.float32)
    _, _, _, m = check_step(eng, big, tgt, G0, exhaustive=False)
    assert m == 65837


def test_step_exhaustive_target_and_non_finite_source(eng):
    tgt = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])     # no lattice: the exhaustive path
    clean = BLOBS[:400].copy() + np.float32(0.01)
    idx0, d20, _, m0 = check_step(eng, clean, tgt, I4, thr=0.5)
    src = clean.copy()
    src[7, 0] = np.nan
    src[200, 2] = np.inf
    src[399, 1] = -np.inf
    idx, d2, _, m = check_step(eng, src, tgt, I4, thr=0.5)
    bad = np.array([7, 200, 399])
    keep = np.setdiff1d(np.arange(400), bad)
    assert (idx[bad] == -1).all() and m0 >= 300 and m == m0 - int((idx0[bad] >= 0).sum())
    assert np.array_equal(idx[keep], idx0[keep]) and d2[keep].tobytes() == d20[keep].tobytes()      # the others are unchanged
    # the same source against the lattice
    idx1, _, _, _ = check_step(eng, src, BLOBS, I4, thr=0.5)
    assert np.array_equal(idx1, idx)


def test_step_distance_threshold_leaves_points_unmatched(eng):
    tgt, src, _ = pair(0)
    idx, d2, _, m = check_step(eng, src, tgt, I4, thr=1.0)       # the identity leaves the clouds about a metre apart
    assert 0 < m < len(src)
    assert (d2[idx >= 0].astype(np.float64) <= 1.0).all() and not d2[idx < 0].any()


def test_step_tie_goes_to_the_lower_id(eng):
    far = np.array([[8, 8, 0], [-8, 8, 1], [8, -8, 2], [-8, -8, 3], [0, 9, 0]], np.float32)
    src = np.array([[0, 0, 0], [0.25, 0, 0], [-0.25, 0, 0]], np.float32)
    for a, b in ((1.0, -1.0), (-1.0, 1.0)):
        tgt = np.concatenate([np.array([[a, 0.5, 0], [b, 0.5, 0]], np.float32), far])      # mirrored about the first source point, exact in f32
        idx, d2, _, m = check_step(eng, src, tgt, I4)
        assert m == 3 and idx[0] == 0 and d2[0] == np.float32(1.25)
        assert idx[1] == (0 if a > 0 else 1) and idx[2] == (1 if a > 0 else 0)
        idx, _, _, _ = check_step(eng, src, np.concatenate([tgt, np.array([[1e12, 0, 0]], np.float32)]), I4)   # ... and on the exhaustive path
        assert idx[0] == 0


# ---- the fused move ---------------------------------------------------------------------------------------------------
def test_fused_move_two_iterations(eng):
    tgt, src, _ = pair(1)
    eng.icp_set_target(tgt)
    eng.icp_set_source(src)
    set_params(eng, max_iterations=1)
    T1 = eng.icp_align(I4)["final"]                             # final = T1 * I: T1's own words
    _, _, sums, m = eng.icp_correspondences(I4, T1)
    T2 = R.estimate(sums, m)
    set_params(eng, max_iterations=2)
    r = eng.icp_align(I4)
    assert r["iterations"] == 2 and r["state"] == R.ITERATIONS and r["converged"]
    assert r["final"].tobytes() == R.mul4_f32(T2, T1).tobytes()  # T2 is the engine's second transformation
    want = R.align(src, tgt, I4, dict(R.DEFAULTS, max_iterations=2), transformations=[T1, T2])
    got = eng.icp_get_aligned()
    assert got.tobytes() == want["aligned"].tobytes()
    assert got.tobytes() == R.move_f32(T2, R.move_f32(T1, R.move_f32(I4, src))).tobytes()
    assert eng.icp_get_aligned().tobytes() == got.tobytes()      # a second read moves nothing


# ---- aligns -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("gname", ["identity", "default_guess"])
@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_align_against_the_restatement(eng, p, gname, name):
    tgt, src, dT = pair(p)
    G = I4 if gname == "identity" else G0
    prm = SETS[name]
    want = R.align(src, tgt, G, prm, exhaustive=False)
    margin = R.margin(want, prm)
    set_params(eng, **prm)
    eng.icp_set_target(tgt)
    eng.icp_set_source(src)
    got = eng.icp_align(G)
    dt, dr = se3_err(want["final"], got["final"])
    print(f"pair {p} {gname} {name}: engine converged {got['converged']} {ndt.ICP_STATES[got['state']]} iterations {got['iterations']} matches {got['matches']} "
          f"mse {got['mse']!r} | restatement {want['converged']} {R.STATE_NAMES[want['state']]} {want['iterations']} {want['matches']} {want['mse']!r} "
          f"| margin {margin:.3e} | pose difference {dt:.3e} m {dr:.3e} rad | error against the true motion {se3_err(dT, got['final'])}")
    assert margin >= 0.01
    assert (got["converged"], got["state"], got["iterations"]) == (want["converged"], want["state"], want["iterations"])
    assert dt <= 1e-4 and dr <= 1e-5
    assert got["matches"] == want["matches"]


# ---- keyframes --------------------------------------------------------------------------------------------------------
def test_align_by_keyframe_ids_gives_the_same_bytes_and_release_refuses(eng):
    tgt, src, _ = pair(2)
    reg = icp.IterativeClosestPoint.from_factory(transformation_epsilon=1e-6, engine=eng)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    a = reg.align(G0)
    fa, ra, sa = reg.getFinalTransformation().copy(), dict(reg.result), reg.getFitnessScore(1.0)
    assert ra["iterations"] > 3
    kt, ks = eng.keyframe_add(tgt), eng.keyframe_add(src)
    reg.setInputTarget(keyframe=kt)
    reg.setInputSource(keyframe=ks)
    b = reg.align(G0)
    rb = reg.result
    assert (rb["converged"], rb["iterations"], rb["state"], rb["matches"], rb["mse"]) == (ra["converged"], ra["iterations"], ra["state"], ra["matches"], ra["mse"])
    assert reg.getFinalTransformation().tobytes() == fa.tobytes() and a.tobytes() == b.tobytes()
    assert reg.getFitnessScore(1.0) == sa
    assert eng.keyframe_get(ks).tobytes() == src.tobytes() and eng.keyframe_get(kt).tobytes() == tgt.tobytes()   # the rows are as they were
    eng.keyframe_release(kt)
    with pytest.raises(ndt.NDTError) as err:
        eng.icp_align(G0)
    assert err.value.code == -2 and "released" in str(err.value)
    with pytest.raises(ndt.NDTError) as err:
        eng.icp_set_target(keyframe=kt)
    assert err.value.code == -2
    eng.keyframe_release(ks)
    with pytest.raises(ndt.NDTError) as err:
        eng.icp_set_source(keyframe=ks)
    assert err.value.code == -2


# ---- the other surfaces -------------------------------------------------------------------------------------------------
def test_gicp_and_ndt_on_the_same_handle_are_left_as_they_were():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    tgt, src, _ = synth.make_pair(5, 64, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    e.set_target(tgt)
    e.set_source(src)
    k1 = e.keyframe_add(tgt)
    e.gicp_set_params(ndt.default_gicp_params(transformation_epsilon=0.01, max_iterations=64))
    e.gicp_set_target(keyframe=k1)
    e.gicp_set_source(src)

    def surfaces():
        g = e.gicp_align(G0)
        return (e.align(G0), e.get_aligned(), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k1], [np.eye(4)], 1.0), g, e.gicp_get_aligned(),
                e.gicp_covariances(ndt.GICP_TARGET))
    before = surfaces()
    gt, gs, _ = pair(1)
    set_params(e, **SETS["eps1e-6"])
    e.icp_set_target(gt)
    e.icp_set_source(gs)
    assert e.icp_align(G0)["iterations"] >= 2
    e.icp_set_target(keyframe=k1)                               # ... and over the keyframe whose index the others search
    e.icp_set_source(src)
    assert e.icp_align(G0)["iterations"] >= 1
    after = surfaces()
    assert np.asarray(before[0]["final"]).tobytes() == np.asarray(after[0]["final"]).tobytes()
    assert (before[0]["iterations"], before[0]["score"], before[0]["trans_probability"]) == (after[0]["iterations"], after[0]["score"], after[0]["trans_probability"])
    assert before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
    assert before[3][0].tobytes() == after[3][0].tobytes() and np.array_equal(before[3][1], after[3][1])
    assert before[4]["final"].tobytes() == after[4]["final"].tobytes() and (before[4]["iterations"], before[4]["delta"]) == (after[4]["iterations"], after[4]["delta"])
    assert before[5].tobytes() == after[5].tobytes() and before[6].tobytes() == after[6].tobytes()
    assert e.keyframe_get(k1).tobytes() == tgt.tobytes()
    e.close()


def test_state_and_argument_errors():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    for call in (lambda: e.icp_align(G0), lambda: e.icp_correspondences(G0)):
        with pytest.raises(ndt.NDTError) as err:                # no target is set
            call()
        assert err.value.code == -7 and "no target" in str(err.value)
    p = BLOBS[:100]
    e.icp_set_target(p)
    with pytest.raises(ndt.NDTError) as err:                    # no source is set
        e.icp_align(G0)
    assert err.value.code == -7 and "no source" in str(err.value)
    e.icp_set_source(p)
    with pytest.raises(ndt.NDTError) as err:
        e.icp_get_aligned()
    assert err.value.code == -7
    for kw in (dict(transformation_epsilon=-1.0), dict(transformation_epsilon=float("nan")), dict(corr_dist_threshold=-0.5),
               dict(euclidean_fitness_epsilon=float("nan")), dict(max_iterations=-1), dict(min_number_correspondences=-1)):
        with pytest.raises(ndt.NDTError) as err:
            e.icp_set_params(ndt.default_icp_params(**kw))
        assert err.value.code == -2 and str(err.value).count("icp_set_params") == 2, kw
    with pytest.raises(ndt.NDTError) as err:
        e.icp_set_params(ndt.default_icp_params(use_reciprocal_correspondences=1))
    assert err.value.code == -2 and "use_reciprocal_correspondences is not served" in str(err.value)
    with pytest.raises(ndt.NDTError):
        icp.IterativeClosestPoint.from_factory(use_reciprocal_correspondences=True, engine=e)
    with pytest.raises(ndt.NDTError) as err:
        e.icp_set_target(keyframe=3)                            # never given out
    assert err.value.code == -2
    for empty in (lambda: e.icp_set_source(np.zeros((0, 3), np.float32)), lambda: e.icp_set_target(np.zeros((0, 3), np.float32))):
        empty()
        with pytest.raises(ndt.NDTError) as err:
            e.icp_align(I4)
        assert err.value.code == -2 and "empty" in str(err.value)
        e.icp_set_target(p)
        e.icp_set_source(p)
    e.stream_begin(2, 4, 1024, 1024)
    for call in (lambda: e.icp_align(G0), lambda: e.icp_set_target(p), lambda: e.icp_set_source(p), lambda: e.icp_correspondences(G0),
                 lambda: set_params(e), lambda: e.icp_get_aligned(), lambda: e.icp_set_target(keyframe=0)):
        with pytest.raises(ndt.NDTError) as err:
            call()
        assert err.value.code == -7
    e.stream_end()
    idx, d2, _, m = e.icp_correspondences(I4)                   # the refused calls changed nothing
    assert m == 100 and np.array_equal(idx, np.arange(100)) and not d2.any()
    r = e.icp_align(I4)                                         # the cloud on itself
    assert r["converged"] and r["iterations"] >= 1 and r["matches"] == 100 and r["mse"] == 0.0
    dt, dr = se3_err(I4, r["final"])
    assert dt <= 1e-6 and dr <= 1e-6
    e.close()
