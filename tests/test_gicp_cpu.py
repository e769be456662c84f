"""CPU: the GICP surface's host pieces (pclomp::GeneralizedIterativeClosestPoint, registration_method = GICP_OMP).

  * the optimiser, lv_slam_amd/csrc/gicp_bfgs.hpp, compiled into a stand-alone program (tests/cpp/gicp_bfgs_main.cpp) with
    -fsanitize=address,undefined -ffp-contract=off, against tools/gicp_ref.py's BFGS word for word: every iterate, f, gradient norm, exit
    code and the number of evaluations of the functor;
  * the restatement alone: closed forms of the covariances, the gradient against central differences, the outer loop's exits and its
    composition of the final transformation, the motion it recovers on synth.make_pair(p, n_azimuth=64), p = 0..3;
  * the C-ABI without a GPU: defaults, struct layouts, NULL arguments.  (MI355NDT_ERR_STATE needs a handle, hence a GPU: tests/test_gicp_gpu.py.)
"""
import ctypes as C
import importlib.util
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import ndt, synth


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("gicp_ref")
G0 = synth.default_guess()
PAIRS = (0, 1, 2, 3)
_PAIR = {}


def pair(p):
    """(target, source, true motion, target covariances, source covariances, their eigenvalues) of make_pair(p, 64): computed once"""
    if p not in _PAIR:
        tgt, src, dT = synth.make_pair(p, n_azimuth=64)
        tgt, src = tgt.numpy(), src.numpy()
        ct, evt = R.covariances(tgt, 20, 1e-3, return_eigenvalues=True)
        cs, evs = R.covariances(src, 20, 1e-3, return_eigenvalues=True)
        _PAIR[p] = (tgt, src, dT, ct, cs, evt, evs)
    return _PAIR[p]


# ---- the optimiser ----------------------------------------------------------------------------------------------
W = [1.0, 2.5, 0.5, 4.0, 1.5, 3.0]
CEN = [0.5, -1.25, 2.0, 0.125, -0.75, 1.5]


class Poly:
    """the 6-D function of tests/cpp/gicp_bfgs_main.cpp, statement for statement (+ - * / only)"""

    def __init__(self):
        self.evaluations = 0

    def fdf(self, x):
        self.evaluations += 1
        t = [x[i] - CEN[i] for i in range(6)]
        f, g = 0.0, [0.0] * 6
        for i in range(6):
            f = f + W[i] * (t[i] * t[i])
            g[i] = 2.0 * W[i] * t[i]
        u = t[0] * t[1] + t[2] * t[3]
        f = f + 0.25 * (u * u)
        g[0] = g[0] + 0.5 * u * t[1]
        g[1] = g[1] + 0.5 * u * t[0]
        g[2] = g[2] + 0.5 * u * t[3]
        g[3] = g[3] + 0.5 * u * t[2]
        d = 1.0 + t[5] * t[5]
        q = (t[4] * t[4]) / d
        f = f + q
        g[4] = g[4] + 2.0 * t[4] / d
        g[5] = g[5] - 2.0 * t[5] * q / d
        return f, g

    def f(self, x):
        return self.fdf(x)[0]

    def df(self, x):
        return self.fdf(x)[1]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gicp_bfgs") / "gicp_bfgs_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-ffp-contract=off", "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "gicp_bfgs_main.cpp"), "-o", exe])
    return exe


def word(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def python_run(start, max_inner):
    fn = Poly()
    x = [float(v) for v in start]
    lines = []

    def trace(inner, result, x, b):
        lines.append(" ".join([str(inner), str(result)] + [word(v) for v in x] + [word(b.f), word(R.norm(b.gradient))]))
    result, inner = R.minimize(R.BFGS(fn), x, 1e-2, max_inner, trace)
    lines.append(f"end {result} {inner} {fn.evaluations} {1 if R.accepted(result, inner, max_inner) else 0}")
    return lines, result, inner


BFGS_CASES = {
    "start_a": ([3.0, -2.0, 1.0, 2.0, -3.0, 0.5], 50),
    "start_b": ([-1.0, 4.0, -2.0, 1.5, 2.0, -1.0], 50),
    "zero_gradient": (CEN, 20),                   # NoProgress before any step
    "cut_by_max_inner": ([3.0, -2.0, 1.0, 2.0, -3.0, 0.5], 2),
}


@pytest.mark.parametrize("name", list(BFGS_CASES))
def test_optimiser_program_equals_python_word_for_word(program, name):
    start, max_inner = BFGS_CASES[name]
    out = subprocess.run([program, str(max_inner)] + [repr(float(v)) for v in start], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stderr      # a sanitizer report ends the program with a message
    lines, result, inner = python_run(start, max_inner)
    print(name, "->", lines[-1])
    assert out.stdout.splitlines() == lines
    if name == "zero_gradient":
        assert (result, inner) == (R.NO_PROGRESS, 1) and lines[0].split()[2:8] == [word(v) for v in CEN]
    elif name == "cut_by_max_inner":
        assert (result, inner) == (R.RUNNING, 2) and R.accepted(result, inner, max_inner)
    else:
        assert result == R.SUCCESS and 2 < inner < max_inner
        x = [struct.unpack("<d", bytes.fromhex(w)[::-1])[0] for w in lines[-2].split()[2:8]]
        assert max(abs(x[i] - CEN[i]) for i in range(6)) < 1e-2     # the minimum is at CEN (every term is a square that vanishes there)


# ---- the restatement alone ----------------------------------------------------------------------------------------
def test_planar_patch_gives_identity_minus_the_normal():
    """points on the plane z = x + 2 y at multiples of 1/8: every coordinate, product and sum is exact, so cov = I - (1 - eps) n n' to f64
    rounding"""
    i, j = np.meshgrid(np.arange(9), np.arange(9), indexing="ij")
    p = np.stack([i.ravel() / 8.0, j.ravel() / 8.0, (i.ravel() + 2 * j.ravel()) / 8.0], 1).astype(np.float32)
    n = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    for eps in (1e-3, 0.25):
        cov = R.covariances(p, 20, eps).reshape(-1, 3, 3)
        want = np.eye(3) - (1.0 - eps) * np.outer(n, n)
        err = np.abs(cov - want).max()
        print("planar patch, eps", eps, "max error", err)
        assert err < 1e-9


def test_k_of_one_gives_diag_1_1_eps():
    p = (np.random.default_rng(5).integers(-64, 64, (40, 3)) / 8.0).astype(np.float32)     # squares exact in f32: a zero matrix each
    cov = R.covariances(p, 1, 1e-3).reshape(-1, 3, 3)
    assert np.array_equal(cov, np.broadcast_to(np.diag([1.0, 1.0, 1e-3]), cov.shape))


def test_non_finite_rows_and_argument_errors():
    p = np.random.default_rng(6).normal(0, 1, (30, 3)).astype(np.float32)
    p[4, 1] = np.nan
    p[17, 0] = np.inf
    cov = R.covariances(p, 20, 1e-3)
    assert not cov[4].any() and not cov[17].any() and np.isfinite(cov).all() and cov[0].any()
    clean = R.covariances(np.delete(p, [4, 17], axis=0), 20, 1e-3)
    assert np.array_equal(np.delete(cov, [4, 17], axis=0), clean)      # non-finite points are in no neighbourhood
    for k in (0, 65, 29):
        with pytest.raises(ValueError):
            R.covariances(p, k, 1e-3)


def test_properties_of_the_pairs_the_tests_use():
    """what the comparisons of this file and of tests/test_gicp_gpu.py lean on, asserted of every pair they use: no tie at the 20th
    neighbour, no exact 1-NN tie under the default guess, well separated small eigenvalues"""
    for p in PAIRS:
        tgt, src, _, ct, cs, evt, evs = pair(p)
        for cloud, ev in ((tgt, evt), (src, evs)):
            _, d2, _ = R.knn(cloud, 21)
            assert (d2[:, 19] < d2[:, 20]).all()
            gap = ((ev[:, 1] - ev[:, 0]) / ev[:, 2]).min()
            assert gap > 1e-4, (p, gap)
        q = R.move_f32(G0, src)
        two = np.stack([np.partition(R.d2_rows(tgt, q[r:r + 512]), 1, axis=1)[:, :2] for r in range(0, len(q), 512)])
        two = two.reshape(-1, 2)
        assert (two[:, 0] < two[:, 1]).all()
        idx, _, m = R.correspondences(src, tgt, cs, ct, G0, np.eye(4, dtype=np.float32), 5.0)
        print("pair", p, "matched", m, "of", len(src))
        assert 4 <= m < len(src)
    assert R.correspondences(*pair(0)[1::-1], pair(0)[4], pair(0)[3], G0, np.eye(4, dtype=np.float32), 5.0)[2] == 4058


def test_gradient_agrees_with_central_differences():
    """g against (f(x + h e) - f(x - h e)) / 2h of the restatement's own f, at a state away from zero, base = a pure rotation.

    The base has no translation on purpose: the reference forms the rotation gradient from (B p) (x) temp with the WHOLE base transformation
    (:323, :369), translation included, where the derivative of applyState(B, x) p takes the base's rotation only; with a translation in the
    base the reference's g[3..5] is off by 2/m sum temp' dR t_B and no difference quotient agrees with it.

    Bar, per component: N / h + 2 |D(h) - D(2h)| / 3.
      N  bounds what the f32 rounding of pp puts into one value of f.  pp is three f32 products and three f32 additions of terms bounded by
         |p|_1 + |t|_inf, from entries of Tx that are themselves f32 roundings (u = 2^-24 each): |delta pp| <= 8 u (|p|_1 + |t|_inf) =: d_i.
         f = 1/m sum res' M res moves by at most 1/m sum (2 |M res|_1 d_i + |M|_1 d_i^2).  Two values enter D(h): 2 N / 2h.
      D(h) - D(2h) is three times the h^2 term of the quotient's truncation error (Richardson); twice that estimate is allowed.
    h = 2^-6 for the translations (f is quadratic in them: no truncation) and 2^-12 for the angles (|p| up to 60 m makes f''' large)."""
    tgt, src, _, ct, cs, _, _ = pair(0)
    base = np.eye(4, dtype=np.float32)
    base[:3, :3] = synth.rot_zyx(0.02, -0.01, 0.015).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 1.0
    idx, M, m = R.correspondences(src, tgt, cs, ct, base, T, 5.0)
    x = [0.9, 0.02, -0.01, 0.002, -0.003, 0.004]
    f, g = R.cost(src, tgt, idx, M, x, base)
    # N
    mt = np.flatnonzero(idx >= 0)
    Tx = R.apply_state(base, x)
    p = src[mt].astype(np.float64)
    res = (R.move_f32(Tx, src[mt]) - tgt[idx[mt]]).astype(np.float64)
    Mm = M.reshape(-1, 3, 3)[mt]
    d = 8 * 2.0 ** -24 * (np.abs(p).sum(axis=1) + np.abs(Tx[:3, 3]).max())
    N = float((2 * np.abs(np.einsum("nij,nj->ni", Mm, res)).sum(axis=1) * d + np.abs(Mm).sum(axis=(1, 2)) * d * d).sum() / m)

    def quotient(i, h):
        xp, xm = list(x), list(x)
        xp[i] += h
        xm[i] -= h
        return (R.cost(src, tgt, idx, M, xp, base)[0] - R.cost(src, tgt, idx, M, xm, base)[0]) / (2 * h)
    for i in range(6):
        h = 2.0 ** -6 if i < 3 else 2.0 ** -12
        d1, d2 = quotient(i, h), quotient(i, 2 * h)
        bar = N / h + 2 * abs(d1 - d2) / 3
        print(f"g[{i}] = {g[i]!r}  quotient {d1!r}  difference {abs(g[i] - d1):.3e}  bar {bar:.3e} (N {N:.3e}, h {h})")
        assert abs(g[i] - d1) <= bar
        assert bar < 0.01 * max(abs(v) for v in (g[:3] if i < 3 else g[3:]))      # the bar means something: 1 % of the block's largest term
    assert m > 3000 and f > 0


def test_final_transformation_is_composed_as_the_reference_does():
    """final = [R_t R_g | t_t + t_g] (:508-511): the translations are added, the guess's is NOT rotated by R_t"""
    prev = np.eye(4, dtype=np.float32)
    prev[:3, :3] = synth.rot_zyx(0.3, 0.1, -0.2).astype(np.float32)
    prev[:3, 3] = [0.5, -0.25, 0.125]
    guess = np.eye(4, dtype=np.float32)
    guess[:3, :3] = synth.rot_zyx(-0.1, 0.2, 0.05).astype(np.float32)
    guess[:3, 3] = [1.0, 2.0, -3.0]
    F = R.compose_final(prev, guess)
    assert np.array_equal(F[:3, 3], prev[:3, 3] + guess[:3, 3])
    assert np.allclose(F[:3, :3], prev[:3, :3].astype(np.float64) @ guess[:3, :3].astype(np.float64), atol=3e-7)
    assert np.abs(F[:3, 3] - (prev.astype(np.float64) @ guess.astype(np.float64))[:3, 3]).max() > 0.1     # not the 4x4 product
    assert np.array_equal(F[3], [0, 0, 0, 1])
    # applyState(base = guess, x) is the same composition: the cost and the result agree about what x means
    x = [0.5, -0.25, 0.125, 0.0, 0.0, 0.0]
    assert np.array_equal(R.apply_state(guess, x)[:3, 3], guess[:3, 3] + np.array(x[:3], np.float32))


def test_fewer_than_four_matches_end_the_loop_unconverged():
    rng = np.random.default_rng(9)
    tgt = rng.normal(0, 1, (40, 3)).astype(np.float32)
    src = np.concatenate([tgt[:3] + np.float32(0.01), rng.normal(0, 1, (27, 3)).astype(np.float32) + np.float32(500.0)])
    G = np.eye(4, dtype=np.float32)
    G[1, 3] = 0.001
    r = R.align(src, tgt, G, dict(R.FACTORY, corr_dist_threshold=1.0))
    assert (r["converged"], r["iterations"], r["n_matched"], r["inner_status"]) == (False, 0, 3, R.NOT_STARTED)
    assert np.array_equal(r["final"], G)                           # previous_transformation_ = identity, composed with the guess
    src[3] = tgt[3] + np.float32(0.01)                             # a fourth match: the optimiser runs
    r = R.align(src, tgt, G, dict(R.FACTORY, corr_dist_threshold=1.0))
    assert r["iterations"] >= 1 and r["n_matched"] >= 4 and r["inner_status"] != R.NOT_STARTED


# recorded with this file's restatement (translation [m], rotation [rad]) against make_pair's true motion, factory parameters
RECORDED = {0: (0.1914, 0.006417), 1: (0.2268, 0.02156), 2: (0.0834, 0.004001), 3: (0.1678, 0.008934)}


@pytest.mark.parametrize("p", PAIRS)
def test_align_recovers_the_true_motion(p):
    """align with the factory's parameters on make_pair(p, n_azimuth=64) from default_guess().  Recorded errors against the true motion:
    pair 0: 0.1914 m, 6.417e-3 rad; pair 1: 0.2268 m, 2.156e-2 rad; pair 2: 0.0834 m, 4.001e-3 rad; pair 3: 0.1678 m, 8.934e-3 rad (4,096
    points per cloud; the rotation gradient's base-translation term, INTEGRATION.md section 4, ends every inner run with NoProgress).  The
    bar is twice the recorded value.  Every outer delta lies at least 1e-3 away from 1, so the number of outer iterations does not hang on
    a rounding."""
    tgt, src, dT, ct, cs, _, _ = pair(p)
    r = R.align(src, tgt, G0, R.FACTORY, cov_src=cs, cov_tgt=ct)
    dt, dr = se3_err(dT, r["final"])
    print(f"pair {p}: converged {r['converged']} iterations {r['iterations']} inner {r['inner_status']} matched {r['n_matched']} "
          f"deltas {r['deltas']} error {dt:.4e} m {dr:.4e} rad")
    assert r["converged"] and 1 <= r["iterations"] < 64
    assert all(abs(d - 1.0) >= 1e-3 for d in r["deltas"])
    assert dt <= 2 * RECORDED[p][0] and dr <= 2 * RECORDED[p][1]
    g_dt, g_dr = se3_err(dT, G0)
    assert dt < g_dt or g_dt < 2 * RECORDED[p][0]                 # (closer than the guess, unless the guess was that close already)
    assert np.array_equal(r["aligned"], R.move_f32(r["final"], src))


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_gicp_defaults_are_the_constructors(lib):
    p = ndt.default_gicp_params()
    assert (p.k_correspondences, p.gicp_epsilon, p.rotation_epsilon, p.transformation_epsilon, p.max_iterations, p.max_inner_iterations,
            p.corr_dist_threshold) == (20, 1e-3, 2e-3, 5e-4, 200, 20, 5.0)                       # gicp_omp.h:110-120
    assert {k: getattr(p, k) for k in R.DEFAULTS} == R.DEFAULTS
    assert lib.mi355ndt_gicp_params_default(None) == -2
    with pytest.raises(TypeError):
        ndt.default_gicp_params(no_such_field=1)


def test_gicp_struct_layouts_match_header(lib, tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "mi355_ndt.h"
int main(void) {
  printf("%zu %zu %zu %zu ", sizeof(mi355ndt_gicp_params), offsetof(mi355ndt_gicp_params, gicp_epsilon), offsetof(mi355ndt_gicp_params, max_iterations),
         offsetof(mi355ndt_gicp_params, corr_dist_threshold));
  printf("%zu %zu %zu %zu %d %d\\n", sizeof(mi355ndt_gicp_result), offsetof(mi355ndt_gicp_result, converged), offsetof(mi355ndt_gicp_result, n_matched),
         offsetof(mi355ndt_gicp_result, delta), MI355NDT_GICP_TARGET, MI355NDT_GICP_SOURCE);
  return 0;
}''')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(ndt.GicpParams), ndt.GicpParams.gicp_epsilon.offset, ndt.GicpParams.max_iterations.offset,
                   ndt.GicpParams.corr_dist_threshold.offset, C.sizeof(ndt.GicpResult), ndt.GicpResult.converged.offset,
                   ndt.GicpResult.n_matched.offset, ndt.GicpResult.delta.offset, ndt.GICP_TARGET, ndt.GICP_SOURCE]


def test_gicp_null_handle_is_refused_not_dereferenced(lib):
    p = ndt.default_gicp_params()
    buf = (C.c_double * 16)()
    assert lib.mi355ndt_gicp_set_params(None, C.byref(p)) == -1
    assert lib.mi355ndt_gicp_set_target(None, buf, 1, 12) == -1 and lib.mi355ndt_gicp_set_source(None, buf, 1, 12) == -1
    assert lib.mi355ndt_gicp_set_target_keyframe(None, 0) == -1 and lib.mi355ndt_gicp_set_source_keyframe(None, 0) == -1
    assert lib.mi355ndt_gicp_covariances(None, 0, None, 0) == -1
    assert lib.mi355ndt_gicp_correspondences(None, None, None, None, None, None) == -1
    assert lib.mi355ndt_gicp_cost(None, None, None, None, None) == -1
    assert lib.mi355ndt_gicp_align(None, None, None) == -1
    assert lib.mi355ndt_gicp_get_aligned(None, None, 12) == -1


def test_mirror_has_the_reference_method_names(lib):
    from lv_slam_amd import gicp
    for n in ("setCorrespondenceRandomness", "setMaximumOptimizerIterations", "setRotationEpsilon", "setTransformationEpsilon",
              "setMaximumIterations", "setMaxCorrespondenceDistance", "setInputTarget", "setInputSource", "align", "getFinalTransformation",
              "hasConverged"):
        assert callable(getattr(gicp.GeneralizedIterativeClosestPoint, n, None)), n
    if lib.mi355ndt_device_count() <= 0:
        with pytest.raises(ndt.NDTError) as e:                        # no CPU fallback
            gicp.GeneralizedIterativeClosestPoint()
        assert e.value.code == -5
