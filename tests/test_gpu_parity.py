"""GPU (-m gpu): the HIP path through the C-ABI vs the oracle and vs the committed golden fixtures.

Bars: voxel grid -- cell indices / counts / pca weights bit-exact, mean and f32 icov bit-exact
(same op order, IEEE f64 div/sqrt on both sides); sweep (score, g, H) -- rtol 1e-11 of the
largest entry (only the f64 summation ORDER differs); align -- identical iteration count and
SE(3) within the north-star tolerance trans < 1e-4 m, rot < 1e-5 rad."""
import os
import numpy as np
import pytest

from conftest import se3_err
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

CASES = ["omp_direct7_r1", "omp_direct1_r1", "omp_direct26_r2", "pca_direct7_r1", "pca_direct1_r05", "omp_kdtree_r1", "pca_kdtree_r1"]
FIELDS = ["resolution", "step_size", "outlier_ratio", "trans_epsilon", "max_iterations", "neighbor_mode", "variant",
          "min_points_per_voxel", "min_covar_eigvalue_mult"]


def both_params(**kw):
    return ndt.default_params(**kw), O.default_params(**kw)


def golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    pv = z["params"]
    kw = dict(resolution=float(pv[0]), step_size=float(pv[1]), outlier_ratio=float(pv[2]), trans_epsilon=float(pv[3]),
              max_iterations=int(pv[4]), neighbor_mode=int(pv[5]), variant=int(pv[6]), min_points_per_voxel=int(pv[7]),
              min_covar_eigvalue_mult=float(pv[8]))
    return z, kw


def check_voxels(eng, grid, exact=True):
    mn, mx, dv, nv = eng.get_grid()
    omn, omx, odv = grid.bounds()
    assert np.array_equal(mn, omn) and np.array_equal(mx, omx) and np.array_equal(dv, odv)
    lv = grid.leaves()
    # searchable = every leaf that reached min_points (eigen failures keep their slot with n = -1)
    minp = grid.prm.min_points_per_voxel
    sel = lv[(lv["n"] >= minp) | (lv["n"] == -1)]
    assert nv == len(sel)
    v = eng.get_voxels()
    assert np.array_equal(v["idx"], sel["idx"])
    assert np.array_equal(v["n"], sel["n"])
    live = sel["n"] >= minp
    if exact:
        assert np.array_equal(v["mean"], sel["mean"])
        assert np.array_equal(v["icov"][live], sel["icov"][live].astype(np.float32))
    else:
        assert np.allclose(v["mean"], sel["mean"], rtol=1e-14, atol=0)
        assert np.allclose(v["icov"][live], sel["icov"][live].astype(np.float32), rtol=1e-6)
    if grid.prm.variant == O.VARIANT_PCA:
        assert np.array_equal(v["weight"][live], sel["weight"][live])
    return len(sel)


def check_sweep(a, b, rtol=1e-11):
    s1, g1, H1, h1 = a
    s2, g2, H2, h2 = b
    assert h1 == h2
    scale = max(1.0, abs(s2), np.abs(g2).max(), np.abs(H2).max())
    assert abs(s1 - s2) <= rtol * scale
    assert np.abs(g1 - g2).max() <= rtol * scale
    assert np.abs(H1 - H2).max() <= rtol * scale


@pytest.mark.parametrize("name", CASES)
def test_golden_voxels_sweep_align(golden_dir, name):
    z, kw = golden(golden_dir, name)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    grid = O.Grid(z["target"], op)
    eng.set_target(z["target"])
    check_voxels(eng, grid)
    # sweeps at the fixture poses: vs oracle (tight) and vs the independent NumPy restatement (fixture)
    eng.set_source(z["src_sweep"])
    for p, T, sc, gr, H, hits in zip(z["sweep_p"], z["sweep_T"], z["sweep_score"], z["sweep_g"], z["sweep_H"], z["sweep_hits"]):
        got = eng.derivatives_T(T, T[:3, :3])
        check_sweep(got, O.derivatives(grid, z["src_sweep"], T, T[:3, :3]))
        check_sweep(got, (float(sc), gr, H, int(hits)), rtol=1e-8)
        got_p = eng.derivatives(p)
        check_sweep(got_p, O.derivatives_at(grid, z["src_sweep"], p), rtol=1e-9)
    # align
    eng.set_source(z["src_align"])
    r = eng.align(z["guess"])
    ro = O.align(grid, z["src_align"], z["guess"])
    assert r["iterations"] == ro["iterations"] == int(z["align_iterations"])
    assert r["converged"] == ro["converged"] and r["sweeps"] == ro["sweeps"]
    for ref in (ro["final"], z["align_final"]):
        dt, dr = se3_err(ref, r["final"])
        assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert abs(r["score"] - ro["score"]) <= 1e-9 * max(1.0, abs(ro["score"]))
    assert r["hits_last"] == ro["hits_last"]
    assert abs(r["trans_probability"] - ro["trans_probability"]) <= 1e-9 * max(1.0, abs(ro["trans_probability"]))
    # output cloud = source moved by the final pose (f32, PCL scalar form)
    out = eng.get_aligned()
    F = r["final"]
    s = z["src_align"].astype(np.float32)
    exp = np.stack([((F[a, 0] * s[:, 0] + F[a, 1] * s[:, 1]) + F[a, 2] * s[:, 2]) + F[a, 3] for a in range(3)], axis=1)
    assert np.array_equal(out, exp.astype(np.float32))


@pytest.mark.parametrize("mode,variant,res", [(ndt.DIRECT7, 0, 1.0), (ndt.DIRECT1, 1, 1.0), (ndt.DIRECT7, 1, 0.5), (ndt.KDTREE, 0, 1.0), (ndt.KDTREE, 1, 1.0)])
def test_full_size_pair_vs_oracle(mode, variant, res):
    """BASELINE config 2 (65,536-pt pair, HIP path, SE(3) checked against the CPU restatement) + the nodelet's
    pca/DIRECT1 setting + config 5's 0.5 m pca grid."""
    tgt, src, dT = synth.make_pair(0, 1024)
    tgt, src = tgt.numpy(), src.numpy()
    kw = dict(resolution=res, trans_epsilon=0.01, max_iterations=64, neighbor_mode=mode, variant=variant)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    nv = check_voxels(eng, grid)
    assert nv > 500
    eng.set_source(src)
    G = synth.default_guess()
    p0 = O.se3_log(G.astype(np.float64))
    check_sweep(eng.derivatives(p0), O.derivatives_at(grid, src, p0))
    r = eng.align(G)
    ro = O.align(grid, src, G)
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    # and the registration is physically right: recovered motion ~ true motion (scene-noise level)
    # (not for ndt_pca + KDTREE: the distance-ordered compounding of up to 27 integer weights lets a handful of points decide the
    #  step, and the reference algorithm itself -- oracle and HIP alike -- lands metres away from the true motion)
    if not (mode == ndt.KDTREE and variant == 1):
        dt, dr = se3_err(dT, r["final"])
        assert dt < 0.1 and dr < 0.01, (dt, dr)
    # the same pair with the other evaluation order of the three-term f32 sums (MI355NDT_OPT_F32_SUM_ORDER = 1) against the oracle's
    # matching variant: the engine a maintainer selects if a real build of the reference shows Eigen 3.3's SSE pairing
    if not (mode == ndt.KDTREE and variant == 1):
        try:
            O.lib().ora_set_variant(1, 256)
            eng.set_option(ndt.OPT_F32_SUM_ORDER, 1)
            check_sweep(eng.derivatives(p0), O.derivatives_at(grid, src, p0))
            r1, ro1 = eng.align(G), O.align(grid, src, G)
            assert r1["iterations"] == ro1["iterations"] and r1["converged"] == ro1["converged"]
            dt, dr = se3_err(ro1["final"], r1["final"])
            assert dt < 1e-4 and dr < 1e-5, (dt, dr)
        finally:
            O.lib().ora_set_variant(0, 256)
    eng.close()


def test_window_map_target_vs_oracle():
    """`align` against a multi-scan "window map" (loop_detector.hpp:219, global_graph_nodelet.cpp:212-242):
    target = 8 consecutive scans merged in the first scan's frame (524,288 pts, >> one scan), source = the next scan."""
    scans, poses = synth.make_sequence(9, 1024)
    P0i = np.linalg.inv(poses[0])
    parts = []
    for k in range(8):
        M = (P0i @ poses[k]).astype(np.float32)
        parts.append((scans[k].numpy() @ M[:3, :3].T + M[:3, 3]).astype(np.float32))
    tgt = np.ascontiguousarray(np.concatenate(parts, axis=0))
    src = scans[8].numpy()
    true = P0i @ poses[8]
    kw = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    assert check_voxels(eng, grid) > 2000
    eng.set_source(src)
    G = true.copy()
    G[0, 3] += 0.4                                   # a loop-closure style guess: close, not exact
    G = G.astype(np.float32)
    p0 = O.se3_log(G.astype(np.float64))
    check_sweep(eng.derivatives(p0), O.derivatives_at(grid, src, p0))
    r, ro = eng.align(G), O.align(grid, src, G)
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    dt, dr = se3_err(true, r["final"])
    assert dt < 0.1 and dr < 0.01, (dt, dr)
    (fs, n_in), (fo, n_o) = eng.fitness_score(2.0), O.fitness_score(tgt, src, r["final"], 2.0)    # loop_detector.hpp:249-262
    assert n_in == n_o and abs(fs - fo) <= 1e-12 * max(1.0, abs(fo))


MT_CASES = ["omp_direct7_mt", "pca_direct1_mt"]


@pytest.mark.parametrize("name", MT_CASES)
def test_golden_compute_hessian(golden_dir, name):
    """computeHessian / updateHessian (impl2:622-714) through the parity hook, vs the NumPy fixture and the oracle."""
    z, kw = golden(golden_dir, name)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    eng.set_target(z["target"])
    eng.set_source(z["src_align"])
    H = eng.compute_hessian(z["hess_p"])
    Ho = O.compute_hessian(O.Grid(z["target"], op), z["src_align"], z["hess_p"])
    scale = np.abs(Ho).max()
    assert np.abs(H - Ho).max() <= 1e-11 * scale
    assert np.abs(H - z["hess_H"]).max() <= 1e-10 * scale


@pytest.mark.parametrize("name", MT_CASES)
@pytest.mark.parametrize("tag", ["far", "near", "over"])
def test_golden_align_live_more_thuente(golden_dir, name, tag):
    """step_size <= eps/2 (impl2:888): More-Thuente loop + computeHessian live; fixtures cover Wolfe-at-first-trial (no loop),
    loop at the second step only, and loop at the first step (its computeHessian result feeds the next Newton solve)."""
    z, kw = golden(golden_dir, name)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    eng.set_target(z["target"])
    eng.set_source(z["src_align"])
    G = z["guess_" + tag]
    r = eng.align(G)
    ro = O.align(O.Grid(z["target"], op), z["src_align"], G)
    assert r["iterations"] == ro["iterations"] == int(z[tag + "_iterations"])
    assert r["converged"] == ro["converged"] == bool(z[tag + "_converged"])
    assert r["sweeps"] == ro["sweeps"] == 1 + len(z[tag + "_mt_its"]) + int(z[tag + "_mt_its"].sum())
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    dt, dr = se3_err(z[tag + "_final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert abs(r["score"] - ro["score"]) <= 1e-9 * abs(ro["score"])


def test_full_size_live_more_thuente_vs_oracle():
    """65,536-pt pair with step_size <= eps/2: batch of 3 guesses (far / converged / a hair off) == oracle, and switching the
    same engine back to the shipped step size gives the ordinary result again (grid rebuilt without the f64 extras or with,
    same voxels)."""
    tgt, src, _ = synth.make_pair(1, 1024)
    tgt, src = tgt.numpy(), src.numpy()
    base = dict(trans_epsilon=0.01, max_iterations=64)
    gp, op = both_params(**base)
    eng = ndt.Engine(gp)
    eng.set_target(tgt)
    eng.set_source(src)
    r0 = eng.align(synth.default_guess())
    near = r0["final"].copy()
    over = near.copy()
    over[0, 3] -= np.float32(0.002)
    gl, ol = both_params(step_size=0.004, **base)
    eng.set_params(gl)
    grid = O.Grid(tgt, ol)
    loops = 0
    for G in (synth.default_guess(), near, over):
        r, ro = eng.align(G), O.align(grid, src, G)
        assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"] and r["sweeps"] == ro["sweeps"]
        dt, dr = se3_err(ro["final"], r["final"])
        assert dt < 1e-4 and dr < 1e-5, (dt, dr)
        loops += ro["mt_loops"]
    assert loops > 0                                   # the loop (and computeHessian) really ran
    eng.set_params(gp)
    r1 = eng.align(synth.default_guess())
    assert r1["iterations"] == r0["iterations"] and np.array_equal(r1["final"], r0["final"])


def test_full_size_sweep_properties():
    """Size-independent properties of the derivative sweep at the full 65,536-pt size (no oracle involved):
    additivity over a split of the source cloud, invariance under a permutation of the source points, and hit conservation."""
    tgt, src, _ = synth.make_pair(5, 1024)
    tgt, src = tgt.numpy(), src.numpy()
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    eng.set_target(tgt)
    p = O.se3_log(synth.default_guess().astype(np.float64)) + np.array([0.02, -0.01, 0.0, 0.002, -0.001, 0.004])
    eng.set_source(src)
    s_all, g_all, H_all, h_all = eng.derivatives(p)
    cut = 40000                                            # not a multiple of the 2048-pt reduction chunk
    eng.set_source(src[:cut])
    s_a, g_a, H_a, h_a = eng.derivatives(p)
    eng.set_source(src[cut:])
    s_b, g_b, H_b, h_b = eng.derivatives(p)
    assert h_a + h_b == h_all
    scale = np.abs(H_all).max()
    assert abs((s_a + s_b) - s_all) <= 1e-11 * abs(s_all)
    assert np.abs((g_a + g_b) - g_all).max() <= 1e-11 * max(1.0, np.abs(g_all).max())
    assert np.abs((H_a + H_b) - H_all).max() <= 1e-11 * scale
    perm = np.random.default_rng(3).permutation(len(src))
    eng.set_source(np.ascontiguousarray(src[perm]))
    s_p, g_p, H_p, h_p = eng.derivatives(p)
    assert h_p == h_all
    assert abs(s_p - s_all) <= 1e-11 * abs(s_all) and np.abs(H_p - H_all).max() <= 1e-11 * scale
    # the target's leaves do not depend on the order of the target points beyond f64 summation rounding
    eng2 = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    eng2.set_target(np.ascontiguousarray(tgt[np.random.default_rng(4).permutation(len(tgt))]))
    v1, v2 = eng.get_voxels(0), eng2.get_voxels(0)
    assert np.array_equal(v1["idx"], v2["idx"]) and np.array_equal(v1["n"], v2["n"])
    assert np.abs(v1["mean"] - v2["mean"]).max() <= 1e-12 * 128


def test_two_engines_from_two_threads():
    """Distinct handles are independent: two engines driven concurrently from two host threads give the
    same bits as the same work done one after the other."""
    import threading
    jobs = []
    for k in range(2):
        t, s_, _ = synth.make_pair(40 + k, 256, n_beams=32)
        jobs.append((t.numpy(), s_.numpy()))
    G = synth.default_guess()
    ref = []
    for t, s_ in jobs:
        e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
        e.set_target(t); e.set_source(s_)
        ref.append(e.align(G))
    out = [None, None]

    def work(k):
        e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
        for _ in range(5):                        # overlap for real: several build + align rounds per thread
            e.set_target(jobs[k][0]); e.set_source(jobs[k][1])
            out[k] = e.align(G)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    for k in range(2):
        assert np.array_equal(out[k]["final"], ref[k]["final"]) and out[k]["iterations"] == ref[k]["iterations"]
        assert out[k]["score"] == ref[k]["score"]


@pytest.mark.parametrize("variant", [0, 1])
def test_degenerate_geometry_vs_oracle(variant):
    """The leaf pass on inputs that stress its guards (voxel_grid_covariance_omp_impl.hpp:337-364): voxels of identical points
    (covariance = the Identity seed's (n-1)/n^2 * I only), exactly planar and collinear voxels (eigenvalue inflation), coordinates
    around 500 m (f32 cell arithmetic far from the origin), NaN / inf points in both clouds.  Voxels bit-exact, sweeps and the
    alignment equal to the oracle's.  (At 5 km the f32 point arithmetic of the reference quantises moved points to 0.5 mm, the
    Newton iteration oscillates until max_iterations in oracle and HIP alike, and poses agree only to ~1e-4 m at the data:
    tools/far_origin.py.)"""
    rng = np.random.default_rng(17 + variant)
    base, _, _ = synth.make_pair(50, 128, n_beams=32)
    base = base.numpy()
    off = np.float32([500.0, -300.0, 40.0])
    parts = [base + off]
    parts.append(np.repeat(np.float32([[510.25, -290.5, 41.5]]), 12, axis=0))                       # 12 identical points
    pl = rng.uniform(0, 1, (40, 3)).astype(np.float32); pl[:, 2] = 0.5                                # planar voxel
    parts.append(pl + np.float32([520.0, -310.0, 42.0]))
    ln = np.zeros((20, 3), np.float32); ln[:, 0] = np.linspace(0.05, 0.95, 20)                        # collinear voxel
    parts.append(ln + np.float32([530.0, -320.0, 43.25]))
    tgt = np.concatenate(parts).astype(np.float32)
    tgt[::97] = np.nan
    tgt[5::211, 1] = np.inf
    src = (base[::3] + off + np.float32([0.3, -0.2, 0.05])).astype(np.float32)
    src[::53] = np.nan
    kw = dict(trans_epsilon=0.01, max_iterations=64, variant=variant, neighbor_mode=ndt.DIRECT7)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    check_voxels(eng, grid)
    # (the Identity seed of cov_ -- voxel_grid_covariance_omp.h:101 -- adds (n-1)/n^2 to the diagonal, so even the voxel of
    #  identical points passes the eigenvalue test: its covariance is (n-1)/n^2 * I)
    lv = grid.leaves()
    assert (lv["n"] >= 6).sum() > 100
    eng.set_source(src)
    p = np.array([0.05, -0.02, 0.01, 0.003, -0.002, 0.006])
    check_sweep(eng.derivatives(p), O.derivatives_at(grid, src, p))
    G = np.eye(4, dtype=np.float32)
    r, ro = eng.align(G), O.align(grid, src, G)
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)


def test_non_default_parameters_vs_oracle():
    """Every tunable away from its constructor default at once: resolution, step size, outlier ratio, epsilon, iteration cap,
    min_points_per_voxel (voxel_grid_covariance_omp.h:204) and the eigenvalue inflation factor (:205)."""
    tgt, src, _ = synth.make_pair(60, 256, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    kw = dict(resolution=1.5, step_size=0.05, outlier_ratio=0.3, trans_epsilon=0.02, max_iterations=12, neighbor_mode=ndt.DIRECT7,
              min_points_per_voxel=3, min_covar_eigvalue_mult=0.1)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    check_voxels(eng, grid)
    eng.set_source(src)
    G = synth.default_guess()
    p0 = O.se3_log(G.astype(np.float64))
    check_sweep(eng.derivatives(p0), O.derivatives_at(grid, src, p0))
    r, ro = eng.align(G), O.align(grid, src, G)
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"] and r["sweeps"] == ro["sweeps"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert abs(r["trans_probability"] - ro["trans_probability"]) <= 1e-9 * max(1.0, abs(ro["trans_probability"]))


@pytest.mark.parametrize("min_points,resolution", [(1, 0.4), (2, 0.5), (12, 1.0)])
def test_voxel_grids_at_other_min_points(min_points, resolution):
    """The build records a leaf's run start where it marks its cell (k_mark: per-wave slices of LS_SLICE / min_points + 2 entries, strung
    together by voxel id in k_rank): with min_points 1 and small cells every occupied cell is a leaf and a slice of 256 sorted
    positions holds far more than 64 of them; the grids stay bit-exact (voxel_grid_covariance_omp.h:204, impl:297), in a single build
    and in a ragged batch."""
    clouds = [synth.make_pair(k, 256, n_beams=32)[0].numpy() for k in (11, 12, 13)]
    clouds[1] = clouds[1][:5000]
    clouds[2] = clouds[2][:777]
    kw = dict(resolution=resolution, neighbor_mode=ndt.DIRECT7, min_points_per_voxel=min_points)
    gp, op = both_params(**kw)
    eng = ndt.Engine(gp)
    for c in clouds:
        eng.set_target(c)
        check_voxels(eng, O.Grid(c, op))
    eng.batch_reserve(len(clouds), max(len(c) for c in clouds), 64)
    for b, c in enumerate(clouds):
        eng.batch_set_target(b, c)
        eng.batch_set_source(b, clouds[0][:64])
    eng.batch_build_targets()
    for b, c in enumerate(clouds):
        lv = O.Grid(c, op).leaves()
        sel = lv[(lv["n"] >= min_points) | (lv["n"] == -1)]
        v = eng.get_voxels(b)
        assert np.array_equal(v["idx"], sel["idx"]) and np.array_equal(v["n"], sel["n"])
        assert np.array_equal(v["mean"], sel["mean"])
        live = sel["n"] >= min_points
        assert np.array_equal(v["icov"][live], sel["icov"][live].astype(np.float32))


def test_identity_alignment_property():
    """identical clouds + identity guess => nothing to do: |delta| -> 0 within the 3-sweep minimum."""
    tgt, _, _ = synth.make_pair(2, 256)
    tgt = tgt.numpy()
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    eng.set_target(tgt)
    eng.set_source(tgt)
    r = eng.align(np.eye(4, dtype=np.float32))
    assert r["converged"] and r["iterations"] <= 3
    dt, dr = se3_err(np.eye(4), r["final"])
    assert dt < 0.02 and dr < 0.002       # steps are clamped to >= eps/2 = 0.005 each


def test_edge_cases():
    prm = ndt.default_params(trans_epsilon=0.01, max_iterations=64)
    eng = ndt.Engine(prm)
    rng = np.random.default_rng(3)
    tgt = rng.uniform(-5, 5, (3000, 3)).astype(np.float32)
    # align before any input: state error, not a crash
    with pytest.raises(ndt.NDTError) as e:
        eng.align(np.eye(4, dtype=np.float32))
    assert e.value.code == -7
    eng.set_target(tgt)
    # zero hits: source far from every voxel -> delta == 0 -> converged, 0 iterations, final == guess (impl2:147-152)
    src = (rng.uniform(-1, 1, (100, 3)) + 500).astype(np.float32)
    eng.set_source(src)
    G = np.eye(4, dtype=np.float32)
    G[0, 3] = 0.25
    r = eng.align(G)
    assert r["converged"] and r["iterations"] == 0 and r["sweeps"] == 1 and np.array_equal(r["final"], G) and r["hits_last"] == 0
    # non-finite points are skipped on both sides (the !is_dense branches)
    tgt2 = tgt.copy()
    tgt2[::7] = np.nan
    src2 = rng.uniform(-4, 4, (777, 3)).astype(np.float32)
    src2[::5, 1] = np.inf
    op = O.default_params(trans_epsilon=0.01, max_iterations=64)
    grid = O.Grid(tgt2, op)
    eng.set_target(tgt2)
    check_voxels(eng, grid)
    eng.set_source(src2)
    p = np.array([0.1, -0.05, 0.02, 0.01, 0.02, -0.03])
    check_sweep(eng.derivatives(p), O.derivatives_at(grid, src2, p))
    # ragged sizes: 1-point source, source not a multiple of the 1024-pt chunk
    for n in (1, 1023, 1025):
        s = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
        eng.set_source(s)
        check_sweep(eng.derivatives(p), O.derivatives_at(grid, s, p))
    # stride: PointXYZI-style 32-byte records
    rec = np.zeros((len(tgt), 8), np.float32)
    rec[:, :3] = tgt
    rec[:, 4] = 77.0
    eng.set_target(rec)
    check_voxels(eng, O.Grid(tgt, op))


def _align_with(prm, tgt, src, G):
    e = ndt.Engine(prm)
    e.set_target(tgt)
    e.set_source(src)
    return e.align(G)


def test_set_resolution_revoxelises_only_when_a_source_is_set():
    """setResolution (ndt_omp.h:126-136): `if (resolution_ != resolution) { resolution_ = resolution; if (input_) init(); }`.  With a source
    set the target is re-voxelised at once; WITHOUT one the grid keeps its 1 m leaves until the next setInputTarget while the next align
    already takes its Gauss constants from the new value (impl2:93-100) -- the oracle reproduces that state with a grid built at 1 m and
    align parameters at 2 m."""
    tgt, src, _ = synth.make_pair(4, 256, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    G = synth.default_guess()
    # (a) source first: re-init
    reg = ndt.NormalDistributionsTransform()
    reg.setTransformationEpsilon(0.01)
    reg.setMaximumIterations(64)
    reg.setInputSource(src)
    reg.setInputTarget(tgt)
    n1 = reg.engine.get_grid()[3]
    reg.setResolution(2.0)
    n2 = reg.engine.get_grid()[3]
    assert n1 != n2 and len(reg.getTargetCells()) == n2            # ndt_pca.h:129-133 accessor
    check_voxels(reg.engine, O.Grid(tgt, O.default_params(resolution=2.0)))
    out = reg.align(G)
    ro = O.align(O.Grid(tgt, O.default_params(resolution=2.0, trans_epsilon=0.01, max_iterations=64)), src, G)
    assert reg.getFinalNumIteration() == ro["iterations"] and reg.hasConverged() == ro["converged"]
    dt, dr = se3_err(ro["final"], reg.getFinalTransformation())
    assert dt < 1e-4 and dr < 1e-5
    assert out.shape == src.shape
    assert abs(reg.getTransformationProbability() - ro["trans_probability"]) < 1e-9
    # (b) no source yet: the grid stays as it is ...
    reg = ndt.NormalDistributionsTransform()
    reg.setTransformationEpsilon(0.01)
    reg.setMaximumIterations(64)
    reg.setInputTarget(tgt)
    v1 = reg.engine.get_voxels(0)
    reg.setResolution(2.0)
    assert reg.getResolution() == 2.0
    v2 = reg.engine.get_voxels(0)
    assert len(v1) == n1 and np.array_equal(v1["idx"], v2["idx"]) and np.array_equal(v1["icov"], v2["icov"])
    check_voxels(reg.engine, O.Grid(tgt, O.default_params(resolution=1.0)))
    # ... and the align that follows runs on 1 m leaves with the constants of 2 m
    reg.setInputSource(src)
    reg.align(G)
    g1 = O.Grid(tgt, O.default_params(resolution=1.0))
    g1.prm = O.default_params(resolution=2.0, trans_epsilon=0.01, max_iterations=64)
    ro = O.align(g1, src, G)
    assert reg.getFinalNumIteration() == ro["iterations"] and reg.hasConverged() == ro["converged"]
    dt, dr = se3_err(ro["final"], reg.getFinalTransformation())
    assert dt < 1e-4 and dr < 1e-5
    assert abs(reg.getTransformationProbability() - ro["trans_probability"]) < 1e-9
    ro_plain = O.align(O.Grid(tgt, O.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64)), src, G)
    assert ro_plain["score"] != ro["score"]                        # (the state really differs from both plain configurations)
    # the next setInputTarget voxelises at 2 m
    reg.setInputTarget(tgt)
    assert reg.engine.get_grid()[3] == n2


def test_switch_to_kdtree_after_target():
    """setNeighborhoodSearchMethod(KDTREE) after setInputTarget (ndt_omp.h:162-164 just stores the enum; the reference's grid
    always owns its kd-tree): the engine has to produce the leaf centroids it skipped for the DIRECT build."""
    tgt, src, _ = synth.make_pair(6, 256, n_beams=32)
    tgt, src = tgt.numpy(), src.numpy()
    reg = ndt.NormalDistributionsTransform()
    reg.setTransformationEpsilon(0.01)
    reg.setMaximumIterations(64)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.align(synth.default_guess())
    it7 = reg.getFinalNumIteration()
    reg.setNeighborhoodSearchMethod(ndt.KDTREE)
    reg.align(synth.default_guess())
    ro = O.align(O.Grid(tgt, O.default_params(trans_epsilon=0.01, max_iterations=64, neighbor_mode=O.KDTREE)), src, synth.default_guess())
    assert reg.getFinalNumIteration() == ro["iterations"] and reg.hasConverged() == ro["converged"]
    dt, dr = se3_err(ro["final"], reg.getFinalTransformation())
    assert dt < 1e-4 and dr < 1e-5
    reg.setNeighborhoodSearchMethod(ndt.DIRECT7)             # and back: same answer as before the detour
    reg.align(synth.default_guess())
    assert reg.getFinalNumIteration() == it7


def test_batch_matches_single_and_oracle():
    """configs 3/4 in miniature: a batch of independent pairs == the same pairs run one at a time (bit-identical),
    and == the oracle to tolerance; ragged cloud sizes inside one batch."""
    prm_kw = dict(trans_epsilon=0.01, max_iterations=64)
    pairs = []
    for k in range(5):
        t, s, dT = synth.make_pair(10 + k, 128 if k % 2 else 192, n_beams=32)
        pairs.append((t.numpy(), s.numpy()[: len(s) - 37 * k], dT))
    G = synth.default_guess()
    eng = ndt.Engine(ndt.default_params(**prm_kw))
    eng.batch_reserve(len(pairs), max(len(p[0]) for p in pairs), max(len(p[1]) for p in pairs))
    for k, (t, s, _) in enumerate(pairs):
        eng.batch_set_target(k, t)
        eng.batch_set_source(k, s)
    eng.batch_build_targets()
    res = eng.batch_align(np.broadcast_to(G, (len(pairs), 4, 4)))
    single = ndt.Engine(ndt.default_params(**prm_kw))
    for k, (t, s, _) in enumerate(pairs):
        single.set_target(t)
        single.set_source(s)
        r1 = single.align(G)
        assert np.array_equal(res[k]["final"], r1["final"])           # bit-identical: fixed reduction tree
        assert res[k]["score"] == r1["score"] and res[k]["iterations"] == r1["iterations"]
        ro = O.align(O.Grid(t, O.default_params(**prm_kw)), s, G)
        assert res[k]["iterations"] == ro["iterations"] and res[k]["converged"] == ro["converged"]
        dt, dr = se3_err(ro["final"], res[k]["final"])
        assert dt < 1e-4 and dr < 1e-5
    # run-to-run determinism
    res2 = eng.batch_align(np.broadcast_to(G, (len(pairs), 4, 4)))
    for a, b in zip(res, res2):
        assert np.array_equal(a["final"], b["final"]) and a["score"] == b["score"]


def test_many_pairs_with_one_very_large_grid():
    """Many pairs AND one very large grid (25 cell bits next to 9 bits' worth of pairs).  The sort key is the cell index alone and no
    pass leaves a target's segment, so the batch's widest grid only sets the digit plan (three 10-bit passes here instead of two
    10-bit ones) for every segment.  Same voxels as the oracle, same alignment as a single-pair engine."""
    rng = np.random.default_rng(11)
    t0, s0, _ = synth.make_pair(30, 64, n_beams=32)
    t0, s0 = t0.numpy(), s0.numpy()
    big = np.concatenate([t0, rng.uniform(-128, 128, (3000, 3)).astype(np.float32) * np.float32([1.0, 1.0, 0.9])])   # ~256^3 cells
    B = 260                                                    # 9 pair bits + 25 cell bits
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    eng.batch_reserve(B, len(big), len(s0))
    for k in range(B):
        eng.batch_set_target(k, big if k == 0 else t0)
        eng.batch_set_source(k, s0)
    eng.batch_build_targets()
    mn, mx, dv, nvox = eng.get_grid(0)
    assert int(dv[0]) * int(dv[1]) * int(dv[2]) > (1 << 23)   # really the wide case
    op = O.default_params(trans_epsilon=0.01, max_iterations=64)
    g0 = O.Grid(big, op)
    lv = g0.valid_leaves()
    v = eng.get_voxels(0)
    assert len(v) == len(lv) and np.array_equal(v["idx"], lv["idx"]) and np.array_equal(v["mean"], lv["mean"])
    G = synth.default_guess()
    res = eng.batch_align(np.broadcast_to(G, (B, 4, 4)))
    single = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    single.set_target(t0)
    single.set_source(s0)
    r1 = single.align(G)
    for k in (1, 2, B - 1):
        assert np.array_equal(res[k]["final"], r1["final"]) and res[k]["iterations"] == r1["iterations"]
    ro = O.align(g0, s0, G)
    assert res[0]["iterations"] == ro["iterations"]
    dt, dr = se3_err(ro["final"], res[0]["final"])
    assert dt < 1e-4 and dr < 1e-5


def test_device_resident_batch_zero_copy():
    import torch
    dev = torch.device("cuda:0")
    B, naz = 4, 256
    T = torch.zeros(B, 3, naz * 64, device=dev)
    S = torch.zeros(B, 3, naz * 64, device=dev)
    host = []
    for k in range(B):
        t, s, dT = synth.make_pair(20 + k, naz, device=dev)
        T[k] = t.T
        S[k] = s.T
        host.append((t.cpu().numpy(), s.cpu().numpy()))
    torch.cuda.synchronize()
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    n = naz * 64
    eng.batch_bind_device(T.data_ptr(), [n] * B, n, S.data_ptr(), [n] * B, n)
    eng.batch_build_targets()
    G = synth.default_guess()
    res = eng.batch_align(G)
    for k in range(B):
        ro = O.align(O.Grid(host[k][0], O.default_params(trans_epsilon=0.01, max_iterations=64)), host[k][1], G)
        assert res[k]["iterations"] == ro["iterations"]
        dt, dr = se3_err(ro["final"], res[k]["final"])
        assert dt < 1e-4 and dr < 1e-5


def test_sparse_hits_and_many_chunks():
    """Regimes that stress the sweep's queue/staging logic: (a) a big source whose points mostly miss the target
    (queue fills slowly, entries outlive a tile), (b) sources spanning many 2048-point chunks and several
    per-XCD item queues, (c) DIRECT26 (four probe groups per tile) at a non-trivial size."""
    rng = np.random.default_rng(11)
    tgt = (rng.normal(0, 1.0, (20000, 3)) * np.array([6, 6, 1.5])).astype(np.float32)
    # (a) sparse: source spread over a 10x larger volume
    src = (rng.uniform(-1, 1, (30011, 3)) * np.array([60, 60, 15])).astype(np.float32)
    for mode in (ndt.DIRECT7, ndt.DIRECT1, ndt.DIRECT26):
        gp, op = both_params(trans_epsilon=0.01, max_iterations=64, neighbor_mode=mode)
        eng = ndt.Engine(gp)
        grid = O.Grid(tgt, op)
        eng.set_target(tgt)
        check_voxels(eng, grid)
        eng.set_source(src)
        for p in (np.zeros(6), np.array([0.3, -0.2, 0.1, 0.02, -0.01, 0.03])):
            check_sweep(eng.derivatives(p), O.derivatives_at(grid, src, p))
    # (b)+(c) dense, 17 chunks, DIRECT26, ndt_pca weights
    src2 = (tgt[rng.integers(0, len(tgt), 33333)] + rng.normal(0, 0.05, (33333, 3))).astype(np.float32)
    gp, op = both_params(trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT26, variant=1)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    eng.set_source(src2)
    p = np.array([0.05, 0.02, -0.03, 0.004, 0.002, -0.006])
    check_sweep(eng.derivatives(p), O.derivatives_at(grid, src2, p), rtol=1e-10)
    G = np.eye(4, dtype=np.float32)
    G[0, 3] = 0.2
    r, ro = eng.align(G), O.align(grid, src2, G)
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)


def test_non_power_of_two_leaf():
    """resolution 0.7 m: the sweep must take the true f32 division path for the cell index (impl:379-381)."""
    tgt, src, _ = synth.make_pair(6, 256)
    tgt, src = tgt.numpy(), src.numpy()
    gp, op = both_params(resolution=0.7, trans_epsilon=0.01, max_iterations=64)
    eng = ndt.Engine(gp)
    grid = O.Grid(tgt, op)
    eng.set_target(tgt)
    check_voxels(eng, grid)
    eng.set_source(src)
    G = synth.default_guess()
    p0 = O.se3_log(G.astype(np.float64))
    check_sweep(eng.derivatives(p0), O.derivatives_at(grid, src, p0))
    r, ro = eng.align(G), O.align(grid, src, G)
    assert r["iterations"] == ro["iterations"]
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5


def test_size_independent_properties_full_size():
    """BASELINE sizes (65,536 and 131,072 points): properties that need no oracle run.
    (1) additivity: the sweep over a cloud equals the sum of the sweeps over its two halves (per-point terms);
    (2) permutation invariance of the source order (only the f64 summation order changes);
    (3) the hit count is the integer sum of the halves; (4) run-to-run determinism, bit for bit."""
    for naz, variant, mode in ((1024, 0, ndt.DIRECT7), (2048, 1, ndt.DIRECT7)):
        tgt, src, _ = synth.make_pair(31, naz)
        tgt, src = tgt.numpy(), src.numpy()
        eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64, neighbor_mode=mode, variant=variant,
                                            resolution=1.0 if variant == 0 else 0.5))
        eng.set_target(tgt)
        p = O.se3_log(synth.default_guess().astype(np.float64))
        eng.set_source(src)
        whole = eng.derivatives(p)
        again = eng.derivatives(p)
        assert whole[0] == again[0] and np.array_equal(whole[2], again[2])            # (4)
        half = len(src) // 2 + 333
        eng.set_source(src[:half])
        a = eng.derivatives(p)
        eng.set_source(src[half:])
        b = eng.derivatives(p)
        assert a[3] + b[3] == whole[3]                                                  # (3)
        scale = np.abs(whole[2]).max()
        assert abs((a[0] + b[0]) - whole[0]) <= 1e-11 * max(1.0, abs(whole[0]))         # (1)
        assert np.abs((a[1] + b[1]) - whole[1]).max() <= 1e-11 * scale
        assert np.abs((a[2] + b[2]) - whole[2]).max() <= 1e-11 * scale
        perm = np.random.default_rng(5).permutation(len(src))
        eng.set_source(src[perm])
        c = eng.derivatives(p)
        assert c[3] == whole[3] and np.abs(c[2] - whole[2]).max() <= 1e-11 * scale      # (2)


def test_empty_clouds_are_refused():
    eng = ndt.Engine(ndt.default_params())
    eng.set_target(np.zeros((0, 3), np.float32))
    eng.set_source(np.zeros((10, 3), np.float32))
    with pytest.raises(ndt.NDTError) as e:
        eng.align(np.eye(4, dtype=np.float32))
    assert e.value.code == -7
    reg = ndt.NormalDistributionsTransform()
    assert reg.align().shape == (0, 3) and not reg.hasConverged()      # no target/source yet: PCL prints an error and returns


def test_fitness_score_loop_closure_surface():
    """getFitnessScore(max_range) of the loop-closure caller (loop_detector.hpp:249-262)."""
    tgt, src, dT = synth.make_pair(40, 256)
    tgt, src = tgt.numpy(), src.numpy()
    reg = ndt.NormalDistributionsTransform()
    reg.setTransformationEpsilon(0.01)
    reg.setMaximumIterations(64)
    assert reg.getFitnessScore() == 1.7976931348623157e308           # nothing set yet
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    # before any align the final transformation is the identity
    s0, n0 = reg.engine.fitness_score(25.0)
    e0, m0 = O.fitness_score(tgt, src, np.eye(4, dtype=np.float32), 25.0)
    assert n0 == m0 and abs(s0 - e0) <= 1e-12 * max(1.0, e0)
    reg.align(synth.default_guess())
    F = reg.getFinalTransformation()
    for mr in (0.04, 1.0, 25.0, float("inf")):
        got, n = reg.engine.fitness_score(mr)
        exp, m = O.fitness_score(tgt, src, F, mr)
        assert n == m, (mr, n, m)
        assert abs(got - exp) <= 1e-12 * max(1.0, exp), (mr, got, exp)
    assert reg.getFitnessScore(25.0) < s0                              # the registration improved the fit
    # explicit transform, source far outside the target grid, nothing in range
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 5000.0
    assert reg.engine.fitness_score(4.0, far) == (1.7976931348623157e308, 0)
    got, n = reg.engine.fitness_score(float("inf"), far)
    exp, m = O.fitness_score(tgt, src, far, float("inf"))
    assert n == m == len(src) and abs(got - exp) <= 1e-12 * exp


def test_prefilter_next_row_n2():
    """PrefilteringNodelet distance_filter + VoxelGrid 0.1 m downsample on the device, then straight
    into setInputSource / setInputTarget without a host round trip."""
    scan, _, _ = synth.make_pair(50, 1024)
    raw = scan.numpy().copy()
    raw[::501] = np.nan
    raw[7] = [0.2, 0.1, 0.0]
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    for near, far, leaf in ((0.5, 100.0, 0.1), (0.5, 100.0, 0.0), (1.0, 40.0, 0.25), (0.5, 100.0, 1e-4)):
        got = eng.prefilter(raw, near, far, leaf)
        exp = O.prefilter(raw, near, far, leaf)
        assert got.shape == exp.shape, (leaf, got.shape, exp.shape)
        assert np.array_equal(got, exp), leaf                     # same f32 sums in the same (input) order
    # 32-byte PointXYZI-style records in, no distance filter
    rec = np.zeros((len(raw), 8), np.float32)
    rec[:, :3] = raw
    assert np.array_equal(eng.prefilter(rec, use_distance_filter=False, downsample_resolution=0.2),
                          O.prefilter(raw, leaf=0.2, use_distance_filter=False))
    assert eng.prefilter(np.zeros((0, 3), np.float32)).shape == (0, 3)
    # device-to-device hand-off: prefiltered key frame as target, prefiltered next scan as source == the host route
    tgt, src, _ = synth.make_pair(51, 1024)
    tgt, src = tgt.numpy(), src.numpy()
    ft, fs = O.prefilter(tgt), O.prefilter(src)
    eng.prefilter(tgt, fetch=False)
    eng.use_prefiltered(as_target=True)
    eng.prefilter(src, fetch=False)
    eng.use_prefiltered(as_target=False)
    G = synth.default_guess()
    r = eng.align(G)
    e2 = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    e2.set_target(ft)
    e2.set_source(fs)
    r2 = e2.align(G)
    assert r["iterations"] == r2["iterations"] and np.array_equal(r["final"], r2["final"]) and r["score"] == r2["score"]
    assert eng.get_aligned().shape == fs.shape


def test_caller_stream_and_engine_cell_cap():
    import torch
    tgt, src, _ = synth.make_pair(60, 256)
    tgt, src = tgt.numpy(), src.numpy()
    G = synth.default_guess()
    e1 = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    e1.set_target(tgt); e1.set_source(src)
    r1 = e1.align(G)
    # the same work on a caller-owned HIP stream (torch's), then back on the engine's own stream
    st = torch.cuda.Stream()
    e2 = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    e2.set_stream(st.cuda_stream)
    e2.set_target(tgt); e2.set_source(src)
    r2 = e2.align(G)
    e2.set_stream(None)
    r3 = e2.align(G)
    assert np.array_equal(r1["final"], r2["final"]) and np.array_equal(r1["final"], r3["final"]) and r1["score"] == r2["score"] == r3["score"]
    # a grid beyond the engine's 2^25-cell cap is reported per pair (status -4) and behaves like an empty target
    e3 = ndt.Engine(ndt.default_params(resolution=0.02, trans_epsilon=0.01, max_iterations=64))
    e3.set_target(tgt)
    with pytest.raises(ndt.NDTError) as ex:
        e3.get_grid()
    assert ex.value.code == -4
    e3.set_source(src)
    r = e3.align(G)
    assert r["status"] == -4 and r["hits_last"] == 0 and r["iterations"] == 0 and np.array_equal(r["final"], G)


def test_repeated_uploads_into_one_slot_land_in_call_order():
    """Uploads are asynchronous on copy streams.  Two uploads into the SAME rows with no build / align between them -- setInputSource(A)
    then setInputSource(B), or a pair slot of a batch set twice -- must leave the second cloud there, with the second count (the
    copy stream is chosen by destination, so they are ordered).  Also: before any align() the incremental transforms are Identity
    (pcl::Registration::align resets them), and the pose-record packer refuses a batch that was never aligned."""
    tgt, src, _ = synth.make_pair(12, 512)
    tgt, src = tgt.numpy(), src.numpy()
    decoy = (src[::3] + np.float32([40.0, -25.0, 3.0])).astype(np.float32)          # a shorter cloud somewhere else entirely
    G = synth.default_guess()
    ref = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    ref.set_target(tgt)
    a, b = ref.get_incremental()
    assert np.array_equal(a, np.eye(4, dtype=np.float32)) and np.array_equal(b, np.eye(4, dtype=np.float32))
    ref.set_source(src)
    want = ref.align(G)
    for rep in range(8):                                   # the race, if there is one, needs a few tries
        e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
        e.set_target(tgt)
        for _ in range(3):
            e.set_source(decoy)
            e.set_source(src)
        got = e.align(G)
        assert np.array_equal(got["final"], want["final"]) and got["iterations"] == want["iterations"] and got["score"] == want["score"]
        e.close()
    # the same through the batch calls, several slots, each set twice (first with the decoy)
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    eng.batch_reserve(5, len(tgt), len(src))
    with pytest.raises(ndt.NDTError):
        import torch
        buf = torch.empty(5, 24, dtype=torch.int32, device="cuda")
        eng.batch_pose_records(0, 1, buf.data_ptr(), 5)    # nothing aligned yet
    for k in range(5):
        eng.batch_set_target(k, decoy)
        eng.batch_set_source(k, decoy)
    for k in range(5):
        eng.batch_set_target(k, tgt)
        eng.batch_set_source(k, src)
    res = eng.batch_align(np.broadcast_to(G, (5, 4, 4)))
    for r in res:
        assert np.array_equal(r["final"], want["final"]) and r["iterations"] == want["iterations"]
    eng.synchronize()


def test_compounded_pca_weights_keep_the_newton_solve_finite():
    """ndt_pca multiplies its integer weight (scale * |mean|, voxel_grid_covariance_pca.h:222-226) once more for every neighbour a
    point hits (ndt_pca_impl2.hpp:294-296): 1.5 km from the origin with DIRECT26 the Hessian's entries pass 1e80, and the few
    points with the most neighbours dominate it (H is numerically rank-deficient whatever the source).  Eigen 3.3's JacobiSVD
    divides by the largest coefficient first; a Jacobi SVD that does not overflows in its squared column norms and skips its
    rotations (found by tools/fuzz_parity.py; the solve itself: tests/test_solve6_gpu.py).  Short runs: these runs are chaotic
    (BASELINE.md 5), parity is only meaningful before the chaos amplifies the last bit."""
    rng = np.random.default_rng(23)
    centres = rng.uniform(-6, 6, (60, 3))
    tgt = (centres[rng.integers(0, 60, 9000)] + rng.normal(0, 0.45, (9000, 3)) + [1500.0, -900.0, 30.0]).astype(np.float32)
    G = np.eye(4, dtype=np.float32)
    G[:3, 3] = [0.05, -0.03, 0.02]
    full = (tgt[::9] + rng.normal(0, 0.01, (1000, 3))).astype(np.float32)
    for cap in (0, 2):
        kw = dict(variant=1, neighbor_mode=ndt.DIRECT26, resolution=1.0, trans_epsilon=0.01, max_iterations=cap, min_points_per_voxel=3)
        gp, op = both_params(**kw)
        eng = ndt.Engine(gp)
        grid = O.Grid(tgt, op)
        eng.set_target(tgt)
        check_voxels(eng, grid)
        for src, big in ((full, 1e80), (full[[10, 500]], 1e40)):
            eng.set_source(src)
            p0 = O.se3_log(G.astype(np.float64))
            s, g, H, hits = eng.derivatives(p0)
            assert hits > 0 and np.abs(np.asarray(H)).max() > big, (hits, np.abs(np.asarray(H)).max())
            check_sweep((s, g, H, hits), O.derivatives_at(grid, src, p0))
            r, ro = eng.align(G), O.align(grid, src, G)
            assert r["iterations"] == ro["iterations"] == cap + 2 and r["converged"] == ro["converged"]
            assert np.isfinite(r["final"]).all()
            dt, dr = se3_err(ro["final"], r["final"])
            assert dt < 1e-4 and dr < 1e-5, (cap, len(src), dt, dr)
            mt, mr = se3_err(G, r["final"])
            assert mt + mr > 1e-3, (mt, mr)                      # real steps were taken (each at least eps / 2 long, impl2:890-892)
        eng.close()


def test_leaf_too_small_guards_beyond_the_int64_range():
    """The "leaf size is too small" guards (voxel_grid_covariance_omp_impl.hpp:75-84, pcl::VoxelGrid::applyFilter) where the
    reference's own int64 product overflows: a 1e-4 m prefilter leaf over a 240 m cloud (1.5e19 cells) leaves the cloud as it is,
    in input order; a target with a stray point at 1e30 has no grid (per-pair status MI355NDT_ERR_GRID) and aligns like an empty one."""
    rng = np.random.default_rng(9)
    pts = rng.uniform(-120, 120, (4000, 3)).astype(np.float32)
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    for gate in (False, True):
        got, exp = eng.prefilter(pts, 0.5, 100.0, 1e-4, gate), O.prefilter(pts, 0.5, 100.0, 1e-4, gate)
        assert np.array_equal(got, exp)
    assert np.array_equal(eng.prefilter(pts, 0.5, 100.0, 1e-4, False), pts)
    # a source point 1e7 / 1e12 m outside the target's grid is still matched to its nearest target point (and counted when
    # max_range allows it): the ring walk must reach the grid from any distance
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    e.set_target(pts)
    far_src = pts[:300].copy()
    far_src[5] = [1e7, -1e7, 1e7]
    far_src[9] = [-1e12, 1e12, 1e12]
    far_src[11] = [1e30, 0.0, 0.0]                       # squared distance overflows f32: inf <= max_range is false, as in PCL
    e.set_source(far_src)
    for mr in (1.0, 1e16, float("inf")):
        got, n = e.fitness_score(mr, np.eye(4, dtype=np.float32))
        exp, m = O.fitness_score(pts, far_src, np.eye(4, dtype=np.float32), mr)
        assert n == m and abs(got - exp) <= 1e-12 * max(1.0, exp), (mr, got, exp, n, m)
    assert n == 299
    e.close()
    stray = pts.copy()
    stray[7] = [1e30, 0.0, 0.0]
    for target, prm in ((stray, ndt.default_params(trans_epsilon=0.01, max_iterations=64)), (pts, ndt.default_params(resolution=1e-4, trans_epsilon=0.01, max_iterations=64))):
        e = ndt.Engine(prm)
        e.set_target(target)
        with pytest.raises(ndt.NDTError) as ex:
            e.get_grid()
        assert ex.value.code == -4
        e.set_source(pts[:500])
        G = np.eye(4, dtype=np.float32)
        r = e.align(G)
        assert r["status"] == -4 and r["hits_last"] == 0 and r["iterations"] == 0 and np.array_equal(r["final"], G)
        # getFitnessScore searches the target CLOUD (pcl::Registration's kd-tree), grid or no grid
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = [0.3, -0.2, 0.1]
        for mr in (0.5, 25.0, float("inf")):
            got, n = e.fitness_score(mr, T)
            exp, m = O.fitness_score(target, pts[:500], T, mr)
            assert n == m and n > 0 and abs(got - exp) <= 1e-12 * max(1.0, exp), (mr, got, exp, n, m)
        e.close()


def test_calculate_score_golden_and_gauss_members(golden_dir):
    """mi355ndt_calculate_score (calculateScore, ndt_omp_impl2.hpp:1006-1040) on the fixture clouds: before any align the members hold
    the CONSTRUCTOR's Gauss constants (resolution 1.0 whatever setResolution said, impl2:70-76), after an align those of its parameters."""
    z = np.load(os.path.join(golden_dir, "calc_score.npz"))
    for tag in ("omp", "pca"):
        fx, kw = golden(golden_dir, str(z[f"{tag}_fixture"]))
        p, po = both_params(**kw)
        grid = O.Grid(fx["target"], po)
        eng = ndt.Engine(p)
        eng.set_target(fx["target"])
        cloud = z[f"{tag}_cloud"]
        got = eng.calculate_score(cloud)
        want = float(z[f"{tag}_score_ctor"])
        assert abs(got - want) <= 1e-9 * abs(want)                                    # NumPy restatement (eigh icov): 1e-9
        assert abs(got - O.calculate_score(grid, cloud, z[f"{tag}_gauss_ctor"])) <= 1e-12 * abs(want)   # oracle: f64 summation order only
        eng.set_source(fx["src_align"])
        eng.align(fx["guess"])                                                        # computeTransformation sets gauss_d*_ (impl2:93-100)
        got = eng.calculate_score(cloud)
        want = float(z[f"{tag}_score_align"])
        assert abs(got - want) <= 1e-9 * abs(want)
        assert abs(got - O.calculate_score(grid, cloud)) <= 1e-12 * abs(want)
        assert eng.calculate_score(cloud + np.float32(1e4)) == 0.0                    # nothing within one resolution of any centroid
        assert np.isnan(eng.calculate_score(np.zeros((0, 3), np.float32)))
        # the registration still works afterwards (calculateScore builds the f64 inverse covariances on demand)
        r, ro = eng.align(fx["guess"]), O.align(grid, fx["src_align"], fx["guess"])
        assert r["iterations"] == ro["iterations"] and se3_err(r["final"], ro["final"])[0] < 1e-4
        eng.close()


@pytest.mark.parametrize("variant,mode,res", [(0, ndt.DIRECT7, 1.0), (1, ndt.DIRECT1, 1.0)])
def test_calculate_score_full_size_vs_oracle(variant, mode, res):
    """65,536-point clouds, both classes, through the class mirror: calculateScore of the aligned output cloud within 1e-12 relative."""
    tgt, src, _ = synth.make_pair(7, 1024)
    tgt, src = tgt.numpy(), src.numpy()
    kw = dict(resolution=res, trans_epsilon=0.01, max_iterations=64, neighbor_mode=mode, variant=variant)
    _, po = both_params(**kw)
    reg = ndt.NormalDistributionsTransform(variant=variant)
    reg.setResolution(res); reg.setTransformationEpsilon(0.01); reg.setMaximumIterations(64); reg.setNeighborhoodSearchMethod(mode)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    out = reg.align(synth.default_guess())
    got = reg.calculateScore(out)
    grid = O.Grid(tgt, po)
    want = O.calculate_score(grid, out)
    assert want != 0 and abs(got - want) <= 1e-12 * abs(want), (got, want)
    raw = reg.calculateScore(src)
    assert abs(raw - O.calculate_score(grid, src)) <= 1e-12 * abs(want) and raw < got   # the aligned cloud is the more likely one
    reg.engine.close()


def test_convert_transform_matches_oracle_bit_for_bit(golden_dir):
    z = np.load(os.path.join(golden_dir, "calc_score.npz"))
    for x, M in zip(z["ct_x"], z["ct_M"]):
        got = ndt.NormalDistributionsTransform.convertTransform(x)
        assert np.array_equal(got, O.convert_transform(x)) and np.abs(got.astype(np.float64) - M).max() < 1e-6
    with pytest.raises(ValueError):
        ndt.NormalDistributionsTransform.convertTransform(np.zeros(5))


@pytest.mark.parametrize("variant,mode", [(0, ndt.DIRECT7), (1, ndt.DIRECT1), (0, ndt.KDTREE)])
def test_f32_sum_order_option_vs_oracle_variant(variant, mode):
    """MI355NDT_OPT_F32_SUM_ORDER = 1 evaluates the three-term f32 sums of impl2:581, 594-613 as (t0 + t2) + t1 -- the lane pairing of
    Eigen 3.3's SSE predux<Packet4f> -- exactly as the oracle does under ORA_VAR_SUM3_02_1: sweeps to 1e-11, align to the same iteration
    count and inside the SE(3) tolerance, for the single registration, the batch path and the latency mode; order 0 is the default."""
    tgt, src, _ = synth.make_pair(9, 512)
    tgt, src = tgt.numpy(), src.numpy()
    kw = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=mode, variant=variant)
    p, po = both_params(**kw)
    grid = O.Grid(tgt, po)
    G = synth.default_guess()
    eng = ndt.Engine(p)
    assert eng.get_option(ndt.OPT_F32_SUM_ORDER) == 0
    eng.set_target(tgt); eng.set_source(src)
    pt = np.array([1.0, 0.02, -0.01, 0.003, -0.002, 0.01])
    base = eng.derivatives(pt)
    try:
        O.lib().ora_set_variant(1, 256)                                               # ORA_VAR_SUM3_02_1
        eng.set_option(ndt.OPT_F32_SUM_ORDER, 1)
        assert eng.get_option(ndt.OPT_F32_SUM_ORDER) == 1
        alt = eng.derivatives(pt)
        check_sweep(alt, O.derivatives_at(grid, src, pt))
        assert alt[3] == base[3] and (alt[0] != base[0] or not np.array_equal(alt[2], base[2]))   # same hits, other last bits
        ro = O.align(grid, src, G)
        for lat in (False, True):
            eng.set_latency_mode(lat)
            r = eng.align(G)
            assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
            dt, dr = se3_err(r["final"], ro["final"])
            assert dt < 1e-4 and dr < 1e-5
    finally:
        O.lib().ora_set_variant(0, 256)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, 0)
    eng.set_latency_mode(False)
    check_sweep(eng.derivatives(pt), base, rtol=0.0)                                  # back to the canonical order: same bits as before
    with pytest.raises(ndt.NDTError):
        eng.set_option(ndt.OPT_F32_SUM_ORDER, 2)
    with pytest.raises(ndt.NDTError):
        eng.set_option(99, 0)
    eng.close()
