"""GPU (-m gpu): sweeps, the computeHessian pass and aligns at poses turned by up to pi, against the oracle.

Every other parity test starts from synth.default_guess() (identity rotation) and sweeps at tangents of at most ~0.01 rad, so the pose code of the Newton
control -- p = log(guess) through the trace <= 0 branch of the matrix -> quaternion conversion, the re-basing log(exp(dp) exp(p)) with w near or below 0,
float(exp(p)) feeding a rotation that is nowhere near the identity to the sweep -- met the real kernels only next to R = I.  Here the SAME geometry is
presented turned: for a rotation Q the source is Q^-1 src (formed in f64, rounded to f32) and the pose is default_guess() Q, so the hit count stays that of
the unrotated pair (asserted on the oracle alone, within 1 %: the tests are not vacuous) while R, Rj and the tangent are large.
(ndt_omp_impl2.hpp:102-129, 163-166, 894-900; tests/test_se3_gpu.py checks the same math function by function.)

Not asserted: pose parity over aligns that do not settle.  From guesses turned by about 2 rad or more the reference's iteration often runs into
max_iterations + 2 (docs/experiments.md 10k); such trajectories amplify last-bit differences between two math libraries."""
import functools
import numpy as np
import pytest

from conftest import se3_err
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O
from test_gpu_parity import check_sweep, both_params

pytestmark = pytest.mark.gpu

ROTATIONS = {                                        # name: (axis, angle [rad])
    "yaw_1.5": ((0, 0, 1), 1.5),
    "yaw_-2.0": ((0, 0, 1), -2.0),
    "skew123_2.5": ((1, 2, 3), 2.5),
    "yaw_pi-1e-3": ((0, 0, 1), np.pi - 1e-3),
    "pi_about_x": ((1, 0, 0), np.pi),
    "skew_3.1": ((1, -1, 0.2), 3.1),
}
# guesses beyond 120 degrees (trace <= 0) plus the two other half turns: every sub-branch of the matrix -> quaternion conversion
FIRST_STEP_ROTATIONS = dict({k: ROTATIONS[k] for k in ("skew123_2.5", "yaw_pi-1e-3", "pi_about_x", "skew_3.1")},
                            pi_about_y=((0, 1, 0), np.pi), pi_about_z=((0, 0, 1), np.pi))
SWEEP_CONFIGS = {
    "omp_direct7": dict(resolution=1.0, neighbor_mode=ndt.DIRECT7, variant=0),
    "pca_direct1": dict(resolution=1.0, neighbor_mode=ndt.DIRECT1, variant=1),
    "omp_kdtree": dict(resolution=1.0, neighbor_mode=ndt.KDTREE, variant=0),
    "omp_direct26_r2": dict(resolution=2.0, neighbor_mode=ndt.DIRECT26, variant=0),
}
# (pair, axis, angle): aligns the oracle settles in at most 10 iterations, none of them next to a convergence decision (checked below, on the oracle)
SETTLING = [(1, (0, 0, 1), 1.5), (2, (1, 0, 0), 1.1), (3, (0, 1, 0), 1.5), (4, (1, 2, 3), 1.1), (5, (0, 0, 1), -1.3), (6, (1, 0, 0), 1.5), (7, (0, 1, 0), -1.3),
            (8, (1, 2, 3), 1.5)]
BASE = dict(trans_epsilon=0.01, max_iterations=64)


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


@functools.lru_cache(maxsize=None)
def pair(k):
    tgt, src, _ = synth.make_pair(k, 256, n_beams=32)              # 8,192 points: the size of smoke()
    tgt, src = tgt.numpy(), src.numpy()
    tgt.setflags(write=False); src.setflags(write=False)
    return tgt, src


@functools.lru_cache(maxsize=None)
def turned(k, axis, angle):
    """(Q^-1 src as f32, default_guess() Q as f64 4x4)"""
    R = rotation(axis, angle)
    Q = np.eye(4)
    Q[:3, :3] = R
    s = (pair(k)[1].astype(np.float64) @ R).astype(np.float32)     # rows: (R^T x)^T = x^T R
    G64 = synth.default_guess().astype(np.float64) @ Q
    s.setflags(write=False); G64.setflags(write=False)
    return s, G64


def assert_same_geometry(grid, k, s, p):
    """on the oracle alone: the turned source at the turned pose meets the leaves the plain source meets at the plain guess (within 1 %)"""
    h0 = O.derivatives_at(grid, pair(k)[1], O.se3_log(synth.default_guess().astype(np.float64)))[3]
    h = O.derivatives_at(grid, s, p)[3]
    assert h0 > 2000 and abs(h - h0) <= 0.01 * h0, (h, h0)


def words(r):
    return (r["final"].tobytes(), np.float64(r["score"]).tobytes(), r["iterations"], r["converged"], r["sweeps"], r["hits_last"], np.float64(r["trans_probability"]).tobytes())


@pytest.mark.parametrize("cfg", list(SWEEP_CONFIGS))
def test_one_sweep_at_turned_poses(cfg):
    """T1: computeDerivatives at p = log(default_guess() Q): 1e-11 of the largest entry, equal hit counts"""
    gp, op = both_params(**BASE, **SWEEP_CONFIGS[cfg])
    tgt, _ = pair(1)
    eng = ndt.Engine(gp)
    eng.set_target(tgt)
    grid = O.Grid(tgt, op)
    for name, (axis, angle) in ROTATIONS.items():
        s, G64 = turned(1, axis, angle)
        p = O.se3_log(G64)
        assert_same_geometry(grid, 1, s, p)
        eng.set_source(s)
        check_sweep(eng.derivatives(p), O.derivatives_at(grid, s, p))
    eng.close()


@pytest.mark.parametrize("cfg", ["omp_direct7", "pca_direct1"])
def test_one_sweep_at_turned_poses_tolerance_arithmetic(cfg):
    """T1 under MI355NDT_OPT_ARITH = 1: the bar of tests/test_tolerance_mode.py (1e-5 of the largest entry of each of score, g, H; the oracle's hits exactly)"""
    gp, op = both_params(**BASE, **SWEEP_CONFIGS[cfg])
    tgt, _ = pair(1)
    eng = ndt.Engine(gp)
    eng.set_option(ndt.OPT_ARITH, 1)
    assert eng.get_option(ndt.OPT_ARITH) == 1
    eng.set_target(tgt)
    grid = O.Grid(tgt, op)
    for name, (axis, angle) in ROTATIONS.items():
        s, G64 = turned(1, axis, angle)
        p = O.se3_log(G64)
        assert_same_geometry(grid, 1, s, p)
        eng.set_source(s)
        sc, g, H, hits = eng.derivatives(p)
        so, go, Ho, ho = O.derivatives_at(grid, s, p)
        assert hits == ho, name
        assert abs(sc - so) <= 1e-5 * abs(so), name
        assert np.max(np.abs(np.asarray(g) - go)) <= 1e-5 * np.max(np.abs(go)), name
        assert np.max(np.abs(np.asarray(H).reshape(6, 6) - np.asarray(Ho).reshape(6, 6))) <= 1e-5 * np.max(np.abs(Ho)), name
    eng.close()


@pytest.mark.parametrize("cfg", ["omp_direct7", "pca_direct1"])
def test_compute_hessian_at_turned_poses(cfg):
    """T2: computeHessian / updateHessian (impl2:622-714) through the parity hook, the golden Hessian test's bar"""
    gp, op = both_params(**BASE, **SWEEP_CONFIGS[cfg])
    tgt, _ = pair(1)
    eng = ndt.Engine(gp)
    eng.set_target(tgt)
    grid = O.Grid(tgt, op)
    for name, (axis, angle) in ROTATIONS.items():
        s, G64 = turned(1, axis, angle)
        p = O.se3_log(G64)
        assert_same_geometry(grid, 1, s, p)
        eng.set_source(s)
        H = eng.compute_hessian(p)
        Ho = O.compute_hessian(grid, s, p)
        scale = np.abs(Ho).max()
        assert scale > 0 and np.abs(H - Ho).max() <= 1e-11 * scale, (name, np.abs(H - Ho).max() / scale)
    eng.close()


@functools.lru_cache(maxsize=1)
def settling_set():
    """T3's pairs with their oracle results; on the oracle alone: <= 10 iterations, converged, and no step length within 1e-6 (relative) of trans_epsilon --
    the same aligns with trans_epsilon (1 -+ 1e-6) take the same number of iterations, so no convergence decision of the run is a knife-edge one"""
    out = []
    for k, axis, angle in SETTLING:
        tgt, _ = pair(k)
        s, G64 = turned(k, axis, angle)
        G = G64.astype(np.float32)
        op = O.default_params(**BASE)
        grid = O.Grid(tgt, op)
        assert_same_geometry(grid, k, s, O.se3_log(G64))
        ro = O.align(grid, s, G)
        assert ro["converged"] and ro["iterations"] <= 10, (k, ro["iterations"])
        for f in (1 - 1e-6, 1 + 1e-6):
            of = O.default_params(trans_epsilon=BASE["trans_epsilon"] * f, max_iterations=BASE["max_iterations"])
            assert O.align(O.Grid(tgt, of), s, G)["iterations"] == ro["iterations"], (k, f)
        out.append((tgt, s, G, ro))
    assert len({ro["iterations"] for *_, ro in out}) >= 3
    return out


def check_align(r, ro, what):
    assert r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"], (what, r["iterations"], ro["iterations"])
    assert r["sweeps"] == ro["sweeps"] and r["hits_last"] == ro["hits_last"], (what, r["sweeps"], ro["sweeps"], r["hits_last"], ro["hits_last"])
    dt, dr = se3_err(ro["final"], r["final"])
    assert dt < 1e-4 and dr < 1e-5, (what, dt, dr)


def test_aligns_from_turned_guesses_on_every_route():
    """T3: rotations up to 1.5 rad about z, x, y and a skew axis, each pair with its own turned guess: a single registration, a batch on the round-based
    align and a batch on the one-launch align give the oracle's iterations / converged / sweeps / hits_last, its pose to tolerance, and one another's words"""
    S = settling_set()
    B = len(S)
    gp = ndt.default_params(**BASE)
    single = ndt.Engine(gp)
    w_single = []
    for k, (tgt, s, G, ro) in enumerate(S):
        single.set_target(tgt)
        single.set_source(s)
        r = single.align(G)
        check_align(r, ro, ("single", k))
        w_single.append(words(r))
    single.close()
    guesses = np.stack([G for _, _, G, _ in S])
    for label, a_opt in (("rounds", 0), ("one_launch", 2)):
        eng = ndt.Engine(gp)
        eng.set_option(ndt.OPT_ASYNC_ALIGN, a_opt)
        eng.batch_reserve(B, max(len(x[0]) for x in S), max(len(x[1]) for x in S))
        for k, (tgt, s, _, _) in enumerate(S):
            eng.batch_set_target(k, tgt)
            eng.batch_set_source(k, s)
        eng.batch_build_targets()
        eng.profile_enable(True); eng.profile_reset()
        res = eng.batch_align(guesses)
        pr = eng.profile_get()
        eng.profile_enable(False)
        assert (pr["update_launches"] == 0) == (label == "one_launch"), pr          # the option really selects the route
        for k, (r, (_, _, _, ro)) in enumerate(zip(res, S)):
            check_align(r, ro, (label, k))
            assert words(r) == w_single[k], (label, k)
        eng.close()


@pytest.mark.parametrize("name", list(FIRST_STEP_ROTATIONS))
def test_first_steps_from_guesses_beyond_120_degrees(name):
    """T4: max_iterations = 0 -- the reference then takes exactly 2 iterations and 3 sweeps (the test of impl2:175-179 comes after the step): init_pair_state on a
    guess whose quaternion comes from the trace <= 0 branch, two Newton steps re-based by newton_rebase from such a pose, the sweeps at float(exp(p))."""
    axis, angle = FIRST_STEP_ROTATIONS[name]
    kw = dict(trans_epsilon=0.01, max_iterations=0)
    gp, op = both_params(**kw)
    tgt, _ = pair(1)
    s, G64 = turned(1, axis, angle)
    G = G64.astype(np.float32)
    assert np.trace(G[:3, :3].astype(np.float64)) <= 0
    grid = O.Grid(tgt, op)
    assert_same_geometry(grid, 1, s, O.se3_log(G64))
    ro = O.align(grid, s, G)
    assert ro["iterations"] == 2 and ro["sweeps"] == 3
    # three routes to the re-basing step: the round-based update kernel (newton_update exchanges the two exponentials itself), and newton_rebase
    # under the sweep of the latency mode and inside the one-launch align
    got = {}
    for route in ("rounds", "latency", "one_launch"):
        eng = ndt.Engine(gp)
        if route == "one_launch":
            eng.set_option(ndt.OPT_ASYNC_ALIGN, 2)
            eng.batch_reserve(1, len(tgt), len(s))
            eng.batch_set_target(0, tgt)
            eng.batch_set_source(0, s)
            eng.batch_build_targets()
            eng.profile_enable(True); eng.profile_reset()
            r = eng.batch_align(G[None])[0]
            assert eng.profile_get()["update_launches"] == 0
        else:
            eng.set_latency_mode(route == "latency")
            eng.set_target(tgt)
            eng.set_source(s)
            r = eng.align(G)
        check_align(r, ro, (name, route))
        inc, prev = eng.get_incremental(0)
        for g, want in ((inc, ro["transformation"]), (prev, ro["previous_transformation"])):
            assert np.abs(g.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max()), (name, route, g, want)   # one f32 ulp
        assert np.abs(inc - np.eye(4)).max() > 1e-4 and not np.array_equal(inc, prev)       # (two real, different steps)
        got[route] = (words(r), inc.tobytes(), prev.tobytes())
        eng.close()
    assert got["rounds"] == got["latency"] == got["one_launch"]


def test_first_step_rotations_enter_every_quaternion_branch():
    """(CPU-side bookkeeping of T4: which sub-branch of the matrix -> quaternion conversion each f32 guess takes)"""
    seen = set()
    for axis, angle in FIRST_STEP_ROTATIONS.values():
        m = turned(1, axis, angle)[1].astype(np.float32).astype(np.float64)[:3, :3]
        assert np.trace(m) <= 0
        i = 1 if m[1, 1] > m[0, 0] else 0
        i = 2 if m[2, 2] > m[i, i] else i
        seen.add(i)
    assert seen == {0, 1, 2}
