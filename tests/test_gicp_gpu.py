"""GPU (-m gpu): the GICP surface (mi355ndt_gicp_*: pclomp::GeneralizedIterativeClosestPoint, registration_method = GICP_OMP) against
tools/gicp_ref.py.

  covariances      absolute 1e-9 per entry.  Entries are at most 1; the two Jacobi runs (the same algorithm on the same f64 input) are backward
                   stable to about 50 ulp; the smallest relative gap between a neighbourhood's two smallest eigenvalues, asserted below for
                   every cloud compared (>= 1e-5; 3.7e-4 on pair 0), bounds the eigenvector error by 50 * 1.1e-16 / gap <= 5.5e-10 (1.5e-11 on
                   pair 0).
  correspondences  the restatement is fed the engine's covariances: idx and m exactly, M word for word.
  cost             with the engine's idx and M: f and each gradient term within 1e-11 of the sum of the absolute terms (the sweep bar).
  align            factory parameters, pairs 0-3: converged flag and outer iterations equal, pose within 1e-4 m / 1e-5 rad.
No excluded points, no skipped cases.  Timings: tools/gicp_timing.py, DESIGN.md section 8."""
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import gicp, ndt, synth

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
_REF, _PAIR = {}, {}


def pair(p):
    if p not in _PAIR:
        tgt, src, dT = synth.make_pair(p, n_azimuth=64)
        _PAIR[p] = (tgt.numpy(), src.numpy(), dT)
    return _PAIR[p]


def ref_cov(name, cloud, k, eps=1e-3):
    """the restatement's covariances and eigenvalue gap, computed once per (cloud, k, eps) and shared"""
    key = (name, k, eps)
    if key not in _REF:
        cov, ev = R.covariances(cloud, k, eps, return_eigenvalues=True)
        fin = np.isfinite(np.asarray(cloud, np.float32)).all(axis=1)
        with np.errstate(all="ignore"):
            gap = float(((ev[fin, 1] - ev[fin, 0]) / ev[fin, 2]).min()) if k > 3 else math.inf
        _REF[key] = (cov, gap)
    return _REF[key]


def blobs():
    """the outlier test's cloud: 2,900 points in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away"""
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
    e.gicp_set_params(ndt.default_gicp_params(**kw))


def check_cov(e, name, cloud, k, eps=1e-3, gap_floor=1e-5):
    set_params(e, k_correspondences=k, gicp_epsilon=eps)
    e.gicp_set_target(cloud)
    got = e.gicp_covariances(ndt.GICP_TARGET).reshape(-1, 9)
    want, gap = ref_cov(name, cloud, k, eps)
    err = float(np.abs(got - want).max())
    print(f"{name} n {len(cloud)} k {k}: max |cov - restatement| {err:.3e}, smallest eigenvalue gap {gap:.3e}")
    assert gap >= gap_floor
    assert np.abs(got).max() <= 1.0 + 1e-12
    assert err <= 1e-9
    e.gicp_set_target(cloud)                                    # a second run from scratch: the same bytes
    assert e.gicp_covariances(ndt.GICP_TARGET).tobytes() == got.reshape(-1, 3, 3).tobytes()
    return got


# ---- covariances --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [20, 65, 257])
def test_covariances_small_clouds(eng, n):
    # 20 = k: every list exactly full; 65: a second wave with one live lane; 257: a fifth wave with one
    p = np.random.default_rng(n).normal(0, 0.5, (n, 3)).astype(np.float32)
    check_cov(eng, f"small{n}", p, 20)


def test_covariances_k_above_the_searchable_points_is_refused(eng):
    p = np.random.default_rng(19).normal(0, 0.5, (19, 3)).astype(np.float32)
    set_params(eng, k_correspondences=20)
    eng.gicp_set_target(p)
    with pytest.raises(ndt.NDTError) as err:
        eng.gicp_covariances(ndt.GICP_TARGET)
    assert err.value.code == -2 and "k_correspondences (20) exceeds" in str(err.value)
    q = np.concatenate([p, np.full((5, 3), np.nan, np.float32)])        # 24 points, 19 of them searchable
    eng.gicp_set_target(q)
    with pytest.raises(ndt.NDTError) as err:
        eng.gicp_covariances(ndt.GICP_TARGET)
    assert err.value.code == -2
    for k in (0, 65):
        with pytest.raises(ndt.NDTError) as err:
            set_params(eng, k_correspondences=k)
        assert err.value.code == -2 and "1..64" in str(err.value)


def test_covariances_pair0_target(eng):
    check_cov(eng, "pair0_target", pair(0)[0], 20)


def test_covariances_k_of_one(eng):
    p = (np.random.default_rng(5).integers(-64, 64, (300, 3)) / 8.0).astype(np.float32)     # squares exact in f32: a zero matrix each
    got = check_cov(eng, "dyadic", p, 1)
    assert np.array_equal(got, np.broadcast_to(np.diag([1.0, 1.0, 1e-3]).ravel(), got.shape))


@pytest.mark.parametrize("k", [20, 64])
def test_covariances_blobs_lattice_and_exhaustive(eng, k):
    lattice = check_cov(eng, "blobs", BLOBS, k)
    stray = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])      # no lattice: the exhaustive path
    # (no floor on this cloud's gap: the stray point's own neighbourhood spans 1e12 m, its f64 sums cancel and its two small eigenvalues are
    # rounding residue; the point is compared like every other, and the 3,000 others are the cloud above, whose gap is asserted)
    brute = check_cov(eng, "stray", stray, k, gap_floor=0.0)
    # the stray point is in nobody's neighbourhood: the same lists, whichever path made them
    assert brute[:3000].tobytes() == lattice.tobytes()


def test_covariances_nan_rows(eng):
    p = BLOBS[:600].copy()
    p[100, 0] = np.nan
    p[433, 2] = np.nan
    p[599, 1] = np.inf
    got = check_cov(eng, "nan", p, 20)
    assert not got[[100, 433, 599]].any() and got[0].any()


def test_covariances_epsilon_and_k_key_the_cache(eng):
    p = BLOBS[:500]
    a = check_cov(eng, "b500", p, 20, 1e-3)
    set_params(eng, k_correspondences=20, gicp_epsilon=0.25)           # the cloud stays: the covariances follow the parameters
    b = eng.gicp_covariances(ndt.GICP_TARGET).reshape(-1, 9)
    assert np.abs(b - ref_cov("b500", p, 20, 0.25)[0]).max() <= 1e-9 and np.abs(a - b).max() > 0.1


# ---- correspondences ----------------------------------------------------------------------------------------------
def engine_match(e, src, tgt, guess, T, thr, k=20):
    set_params(e, k_correspondences=k, corr_dist_threshold=thr)
    e.gicp_set_target(tgt)
    e.gicp_set_source(src)
    ct = e.gicp_covariances(ndt.GICP_TARGET)
    cs = e.gicp_covariances(ndt.GICP_SOURCE)
    idx, M, m = e.gicp_correspondences(guess, T)
    return idx, M, m, cs, ct


def check_match(e, src, tgt, guess, T, thr):
    idx, M, m, cs, ct = engine_match(e, src, tgt, guess, T, thr)
    ridx, rM, rm = R.correspondences(src, tgt, cs, ct, guess, T if T is not None else I4, thr)
    print(f"threshold {thr}: matched {m} of {len(src)} (restatement {rm})")
    assert m == rm and np.array_equal(idx, ridx)
    assert M.reshape(-1, 9).tobytes() == rM.tobytes()
    return idx, M, m


def test_correspondences_pair0(eng):
    tgt, src, _ = pair(0)
    idx, M, m = check_match(eng, src, tgt, G0, None, 5.0)
    assert m == 4058 and (idx < 0).sum() == 38                 # some points unmatched
    T = R.apply_state(I4, [0.05, -0.02, 0.01, 0.002, -0.003, 0.004])
    G = G0.copy()
    G[:3, :3] = synth.rot_zyx(0.01, 0.0, -0.005).astype(np.float32)
    check_match(eng, src, tgt, G, T, 5.0)                      # a rotation in both: R = the f64 product's block
    _, _, m = check_match(eng, src, tgt, G0, None, 1e-3)
    assert m == 0                                              # none matched
    # a source cut to leave three matches, then four (the optimiser needs four)
    hit, miss = np.flatnonzero(idx >= 0), np.flatnonzero(idx < 0)
    for want in (3, 4):
        cut = src[np.sort(np.concatenate([hit[:want], miss]))]
        _, _, m = check_match(eng, cut, tgt, G0, None, 5.0)
        assert m == want
        set_params(eng, **dict(FACTORY, corr_dist_threshold=5.0))
        r = eng.gicp_align(G0)
        assert (r["iterations"] == 0 and not r["converged"] and r["inner_status"] == -2) if want == 3 else r["iterations"] >= 1
        assert r["n_matched"] >= want if want == 4 else r["n_matched"] == 3


def test_correspondences_exhaustive_target_and_non_finite_source(eng):
    tgt = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])
    src = BLOBS[:400].copy() + np.float32(0.01)
    src[7, 0] = np.nan
    src[200, 2] = np.inf
    idx, _, m = check_match(eng, src, tgt, I4, None, 0.5)
    assert idx[7] == -1 and idx[200] == -1 and m >= 300


# ---- cost ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m_want", [1, 4, 257, 4058])
def test_cost_sums(eng, m_want):
    tgt, src, _ = pair(0)
    full, _, _ = R.correspondences(src, tgt, np.zeros((len(src), 9)), np.zeros((len(tgt), 9)), G0, I4, 5.0) if "full" not in _REF else _REF["full"]
    _REF["full"] = (full, None, None)
    hit, miss = np.flatnonzero(full >= 0), np.flatnonzero(full < 0)
    cut = src if m_want == len(hit) else src[np.sort(np.concatenate([hit[:m_want], miss]))]
    idx, M, m, _, _ = engine_match(eng, cut, tgt, G0, None, 5.0)
    assert m == m_want
    base = G0.copy()
    base[:3, :3] = synth.rot_zyx(0.01, -0.004, 0.002).astype(np.float32)
    for x, b in (([0.0] * 6, G0), ([0.03, -0.02, 0.01, 0.004, -0.006, 0.008], base)):
        f, g = eng.gicp_cost(x, b)
        sums, abss, rm = R.cost_sums(cut, tgt, idx, M, x, b)
        rf, rg = R.cost_from_sums(sums, rm, x)
        w = 2.0 / rm
        # the bound of each output: 1e-11 of the absolute terms that enter it, through the same scaling
        tol = [1e-11 * abss[0] / rm] + [1e-11 * abss[1 + k] * w for k in range(3)]
        for a in (3, 4, 5):
            unit = [0.0] * 6
            R.r_derivative(x, np.ones((3, 3)), unit)                  # (only to size the array)
            D = [0.0] * 6
            tol_a = 0.0
            for i in range(3):
                for j in range(3):
                    E = np.zeros((3, 3))
                    E[i][j] = 1.0
                    R.r_derivative(x, E, D)                           # D[a] = dR_a(j, i)
                    tol_a += abs(D[a]) * abss[4 + 3 * i + j] * w
            tol.append(1e-11 * tol_a)
        got, want = [f] + list(g), [rf] + list(rg)
        for k in range(7):
            print(f"m {m} x {'0' if not any(x) else 'x1'} out[{k}]: engine {got[k]!r} restatement {want[k]!r} |diff| {abs(got[k] - want[k]):.3e} bar {tol[k]:.3e}")
        assert rm == m and all(abs(got[k] - want[k]) <= tol[k] for k in range(7))
        f2, g2 = eng.gicp_cost(x, b)
        assert (np.float64(f2).tobytes(), g2.tobytes()) == (np.float64(f).tobytes(), g.tobytes())       # two calls, equal bytes


# ---- align --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0, 1, 2, 3])
def test_align_against_the_restatement(eng, p):
    tgt, src, dT = pair(p)
    set_params(eng, **FACTORY)
    eng.gicp_set_target(tgt)
    eng.gicp_set_source(src)
    ct, cs = eng.gicp_covariances(ndt.GICP_TARGET), eng.gicp_covariances(ndt.GICP_SOURCE)
    if p == 0:                                                  # (pair 0 with the restatement's own covariances, the others with the engine's, held to 1e-9 above)
        ct, cs = ref_cov("pair0_target", tgt, 20)[0], ref_cov("pair0_source", src, 20)[0]
    want = R.align(src, tgt, G0, FACTORY, cov_src=cs, cov_tgt=ct)
    got = eng.gicp_align(G0)
    dt, dr = se3_err(want["final"], got["final"])
    print(f"pair {p}: engine converged {got['converged']} iterations {got['iterations']} inner {got['inner_status']} matched {got['n_matched']} "
          f"delta {got['delta']!r} | restatement {want['converged']} {want['iterations']} {want['inner_status']} {want['n_matched']} {want['delta']!r} "
          f"| pose difference {dt:.3e} m {dr:.3e} rad | error against the true motion {se3_err(dT, got['final'])}")
    assert all(abs(d - 1.0) >= 1e-3 for d in want["deltas"])
    assert (got["converged"], got["iterations"]) == (want["converged"], want["iterations"])
    assert dt <= 1e-4 and dr <= 1e-5
    moved = eng.gicp_get_aligned()
    assert moved.tobytes() == R.move_f32(got["final"], src).tobytes()


def test_align_by_keyframe_ids_gives_the_same_bytes_and_release_refuses(eng):
    tgt, src, _ = pair(2)
    reg = gicp.GeneralizedIterativeClosestPoint.from_factory(engine=eng)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    a = reg.align(G0)
    fa, ra = reg.getFinalTransformation().copy(), dict(reg.result)
    cov_host = eng.gicp_covariances(ndt.GICP_TARGET)
    kt, ks = eng.keyframe_add(tgt), eng.keyframe_add(src)
    reg.setInputTarget(keyframe=kt)
    reg.setInputSource(keyframe=ks)
    b = reg.align(G0)
    assert reg.hasConverged() == ra["converged"] and reg.result["iterations"] == ra["iterations"] and reg.result["delta"] == ra["delta"]
    assert reg.getFinalTransformation().tobytes() == fa.tobytes() and a.tobytes() == b.tobytes()
    assert eng.gicp_covariances(ndt.GICP_TARGET).tobytes() == cov_host.tobytes()
    # the keyframe keeps its covariances: another source against the same target keyframe, then back
    reg.setInputSource(src[::2])
    reg.align(G0)
    reg.setInputSource(keyframe=ks)
    assert reg.align(G0).tobytes() == a.tobytes()
    eng.keyframe_release(kt)
    with pytest.raises(ndt.NDTError) as err:
        eng.gicp_align(G0)
    assert err.value.code == -2 and "released" in str(err.value)
    with pytest.raises(ndt.NDTError) as err:
        eng.gicp_set_target(keyframe=kt)
    assert err.value.code == -2
    assert eng.keyframe_get(ks).tobytes() == src.tobytes()      # the other keyframe's rows are as they were
    eng.keyframe_release(ks)


def test_ndt_align_on_the_same_handle_is_left_as_it_was():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    tgt, src, _ = synth.make_pair(5, 64, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    e.set_target(tgt)
    e.set_source(src)
    k1 = e.keyframe_add(tgt)
    before = (e.align(G0), e.get_aligned(), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k1], [np.eye(4)], 1.0))
    gt, gs, _ = pair(1)
    set_params(e, **FACTORY)
    e.gicp_set_target(gt)
    e.gicp_set_source(gs)
    r = e.gicp_align(G0)
    assert r["iterations"] >= 1
    e.gicp_set_target(keyframe=k1)                              # ... and over a keyframe that has a fitness index already
    e.gicp_covariances(ndt.GICP_TARGET, fetch=False)
    after = (e.align(G0), e.get_aligned(), e.fitness_score(1.0), e.keyframe_fitness_scores([k1], [k1], [np.eye(4)], 1.0))
    assert np.asarray(before[0]["final"]).tobytes() == np.asarray(after[0]["final"]).tobytes()
    assert (before[0]["iterations"], before[0]["score"], before[0]["trans_probability"]) == (after[0]["iterations"], after[0]["score"], after[0]["trans_probability"])
    assert before[1].tobytes() == after[1].tobytes() and before[2] == after[2]
    assert before[3][0].tobytes() == after[3][0].tobytes() and np.array_equal(before[3][1], after[3][1])
    assert e.keyframe_get(k1).tobytes() == tgt.tobytes()
    e.close()


def test_state_and_argument_errors():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    for call in (lambda: e.gicp_align(G0), lambda: e.gicp_correspondences(G0)):
        with pytest.raises(ndt.NDTError) as err:                # no cloud is set
            call()
        assert err.value.code == -7
    with pytest.raises(ndt.NDTError) as err:
        e.gicp_covariances(ndt.GICP_SOURCE)
    assert err.value.code == -7
    p = BLOBS[:100]
    e.gicp_set_target(p)
    e.gicp_set_source(p)
    with pytest.raises(ndt.NDTError) as err:                    # no correspondences are resident
        e.gicp_cost([0.0] * 6, I4)
    assert err.value.code == -7
    with pytest.raises(ndt.NDTError) as err:
        e.gicp_get_aligned()
    assert err.value.code == -7
    for kw in (dict(gicp_epsilon=float("nan")), dict(rotation_epsilon=-1.0), dict(corr_dist_threshold=float("nan")), dict(max_iterations=-1),
               dict(max_inner_iterations=-1), dict(k_correspondences=65)):
        with pytest.raises(ndt.NDTError) as err:
            set_params(e, **kw)
        assert err.value.code == -2 and str(err.value).count("gicp_set_params") == 2, kw
    with pytest.raises(ndt.NDTError) as err:
        e.gicp_set_target(keyframe=3)                           # never given out
    assert err.value.code == -2
    with pytest.raises(ndt.NDTError):
        e._chk(e.lib.mi355ndt_gicp_covariances(e.h, 2, None, 0), "gicp_covariances")
    e.stream_begin(2, 4, 1024, 1024)
    for call in (lambda: e.gicp_align(G0), lambda: e.gicp_set_target(p), lambda: e.gicp_covariances(ndt.GICP_TARGET), lambda: e.gicp_correspondences(G0),
                 lambda: e.gicp_cost([0.0] * 6, I4), lambda: set_params(e), lambda: e.gicp_get_aligned()):
        with pytest.raises(ndt.NDTError) as err:
            call()
        assert err.value.code == -7
    e.stream_end()
    idx, _, m = e.gicp_correspondences(I4)                      # the refused calls changed nothing
    assert m == 100 and np.array_equal(idx, np.arange(100))
    e.close()
