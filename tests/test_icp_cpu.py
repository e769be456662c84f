"""CPU: the restatement of pcl::IterativeClosestPoint (tools/icp_ref.py) against constructed truth -- a known rigid motion, the reflection
branch of the rigid estimate, every exit of the loop, the 3x3 Jacobi SVD against numpy -- and the pieces of the Python layer that need no
GPU.  The engine is held to the restatement in tests/test_icp_gpu.py."""
import importlib.util
import math
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import synth


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("icp_ref")
I4 = np.eye(4, dtype=np.float32)
_PAIR = {}


def pair0():
    if 0 not in _PAIR:
        tgt, src, _ = synth.make_pair(0, n_azimuth=64)
        _PAIR[0] = (tgt.numpy(), src.numpy())
    return _PAIR[0]


def test_factory_and_defaults():
    assert R.DEFAULTS == dict(transformation_epsilon=0.0, max_iterations=10, euclidean_fitness_epsilon=-1.7976931348623157e308,
                              corr_dist_threshold=math.sqrt(1.7976931348623157e308), min_number_correspondences=3, use_reciprocal_correspondences=0)
    assert {k: v for k, v in R.FACTORY.items() if R.DEFAULTS[k] != v} == dict(transformation_epsilon=0.01, max_iterations=64)   # registrations.cpp:21-29
    with pytest.raises(ValueError):
        R.align(np.zeros((4, 3)), np.zeros((4, 3)), I4, dict(use_reciprocal_correspondences=1))


def test_known_rigid_motion_is_found_in_one_estimate():
    # a jittered unit lattice and its copy under a motion small against the spacing: every nearest neighbour is the true partner
    rng = np.random.default_rng(1)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 3) - 2.5
    src = (g + rng.uniform(-0.1, 0.1, g.shape)).astype(np.float32)
    M = np.eye(4)
    M[:3, :3] = synth.rot_zyx(0.01, -0.006, 0.004)
    M[:3, 3] = [0.15, -0.1, 0.05]          # 0.19 m: against a spacing of 1 m +- 0.1 m, and past the factory's sqrt(0.01) m in one step
    tgt = (src.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
    step = R.one_step(src, tgt, I4)
    assert step["m"] == len(src) and np.array_equal(step["idx"], np.arange(len(src)))
    T = R.estimate(step["sums"], step["m"])
    dt, dr = se3_err(M, T)
    print(f"first estimate against the motion: {dt:.3e} m {dr:.3e} rad")
    assert dt <= 1e-6 and dr <= 1e-7
    res = R.align(src, tgt, I4, R.FACTORY)
    assert (res["converged"], res["state"], res["iterations"]) == (True, R.TRANSFORM, 2)
    assert res["trace"][0]["state"] == R.NOT_CONVERGED and res["trace"][0]["T"].tobytes() == T.tobytes()
    assert res["aligned"].tobytes() == R.move_f32(res["trace"][1]["T"], R.move_f32(T, R.move_f32(I4, src))).tobytes()   # cumulative f32 moves
    assert res["final"].tobytes() == R.mul4_f32(res["trace"][1]["T"], R.mul4_f32(T, I4)).tobytes()


def test_reflection_branch_gives_a_rotation():
    # a planar cloud (Sigma's last singular value is zero) and its copy, on odd trials mirrored IN the plane before it is turned: the best
    # orthogonal map is then a reflection, det U * det V < 0, and the estimate must be the rotation that turns the plane over instead
    rng = np.random.default_rng(2)
    hits = 0
    for trial in range(40):
        p = np.concatenate([rng.uniform(-2, 2, (50, 2)), np.zeros((50, 1))], axis=1)
        Rz = synth.rot_zyx(rng.uniform(-0.3, 0.3), 0.0, 0.0)
        mirror = np.diag([1.0, -1.0, 1.0]) if trial % 2 else np.eye(3)
        q = p @ mirror @ Rz.T
        cp, cq = p.mean(axis=0), q.mean(axis=0)
        Sg = ((q - cq).T @ (p - cp)) / len(p)
        U, S, V = R.jacobi_svd3(Sg)
        assert S[2] <= 1e-15 * S[0]
        neg = R.det3(U) * R.det3(V) < 0.0
        assert neg == bool(trial % 2)
        hits += int(neg)
        Rm, _ = R.rigid_from_sigma(Sg, list(cp), list(cq))
        Rm = np.array(Rm)
        assert abs(np.linalg.det(Rm) - 1.0) <= 1e-12 and np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12
        want = Rz @ (np.diag([1.0, -1.0, -1.0]) if trial % 2 else np.eye(3))      # (mirrored: half a turn about the plane's x axis)
        assert np.abs(Rm - want).max() <= 1e-12
        assert np.abs(p @ Rm.T - q).max() <= 1e-12                               # ... which still maps the cloud onto its copy
    # ... and a matrix built so: U = I, V = diag(1, 1, -1) up to the SVD's own sign choices
    Rm, _ = R.rigid_from_sigma(np.diag([3.0, 2.0, 0.0]) @ np.diag([1.0, 1.0, -1.0]), [0.0] * 3, [0.0] * 3)
    assert abs(np.linalg.det(np.array(Rm)) - 1.0) <= 1e-12
    Rm, _ = R.rigid_from_sigma(-np.diag([3.0, 2.0, 1.0]), [0.0] * 3, [0.0] * 3)   # a full-rank reflection: det U det V = -1
    U, _, V = R.jacobi_svd3(-np.diag([3.0, 2.0, 1.0]))
    assert R.det3(U) * R.det3(V) < 0.0 and abs(np.linalg.det(np.array(Rm)) - 1.0) <= 1e-12
    print("trials with det U det V < 0:", hits)
    assert hits == 20


def test_every_exit():
    tgt, src = pair0()
    G0 = synth.default_guess()
    r = R.align(src, tgt, I4, dict(R.DEFAULTS, max_iterations=3), exhaustive=False)
    assert (r["converged"], r["state"], r["iterations"]) == (True, R.ITERATIONS, 3)
    r = R.align(src, tgt, G0, R.FACTORY, exhaustive=False)
    assert (r["converged"], r["state"], r["iterations"]) == (True, R.TRANSFORM, 1)      # the squared-translation slip: one step under 0.1 m ends it
    r = R.align(src, tgt, I4, R.FACTORY, exhaustive=False)
    assert (r["converged"], r["state"], r["iterations"]) == (True, R.TRANSFORM, 2)
    r = R.align(src, tgt, I4, dict(R.FACTORY, euclidean_fitness_epsilon=1e-3), exhaustive=False)
    assert r["converged"] and r["state"] in (R.REL_MSE, R.TRANSFORM)
    r = R.align(src, tgt, I4, dict(R.DEFAULTS, max_iterations=64, euclidean_fitness_epsilon=1e-3), exhaustive=False)
    assert (r["converged"], r["state"]) == (True, R.REL_MSE) and 1 < r["iterations"] < 64
    last = r["trace"][-1]
    assert abs(last["mse"] - last["prev_mse"]) / last["prev_mse"] < 1e-3
    r = R.align(src, tgt, G0, dict(R.FACTORY, corr_dist_threshold=1e-6), exhaustive=False)
    assert (r["converged"], r["state"], r["iterations"], r["matches"]) == (False, R.NO_CORRESPONDENCES, 0, 0)
    assert r["aligned"].tobytes() == R.move_f32(G0, src).tobytes() and r["final"].tobytes() == G0.tobytes()
    # the constructor's epsilon 0 on a pair small enough that the correspondences stop changing: the MSE stops changing
    r = R.align(src[::16], tgt[::16], G0, dict(R.DEFAULTS, max_iterations=64))
    print("ABS_MSE case:", R.STATE_NAMES[r["state"]], r["iterations"])
    assert (r["converged"], r["state"]) == (True, R.ABS_MSE) and r["iterations"] < 64
    last = r["trace"][-1]
    assert abs(last["mse"] - last["prev_mse"]) < 1e-12


def test_jacobi_svd_against_numpy():
    rng = np.random.default_rng(0)
    worst = 0.0
    for i in range(600):
        A = rng.normal(size=(3, 3)) * 10.0 ** rng.integers(-8, 9)
        if i % 3 == 1:
            A = np.outer(rng.normal(size=3), rng.normal(size=3))                                    # rank 1
        if i % 3 == 2:
            A = np.outer(rng.normal(size=3), rng.normal(size=3)) + np.outer(rng.normal(size=3), rng.normal(size=3))   # rank 2
        U, S, V = (np.array(x) for x in R.jacobi_svd3(A))
        sv = np.linalg.svd(A, compute_uv=False)
        assert S[0] >= S[1] >= S[2] >= 0.0
        worst = max(worst, np.abs(S - sv).max() / sv[0], np.abs(U @ np.diag(S) @ V.T - A).max() / sv[0],
                    np.abs(U.T @ U - np.eye(3)).max(), np.abs(V.T @ V - np.eye(3)).max())
    print(f"worst relative difference: {worst:.3e}")
    assert worst <= 1e-13
    U, S, V = R.jacobi_svd3(np.zeros((3, 3)))                                                      # Eigen's convention for a zero matrix
    assert U == [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]] and V == U and S == [0.0, 0.0, 0.0]
    U, S, V = R.jacobi_svd3(np.diag([1.0, 5.0, 3.0]))
    assert S == [5.0, 3.0, 1.0]


def test_screened_search_is_the_exhaustive_search():
    pytest.importorskip("scipy")
    tgt, src = pair0()
    tgt = tgt.copy()
    tgt[5] = np.nan                                                                                # a row the tree must not hold
    ties = np.concatenate([tgt, tgt[:50]])                                                         # duplicates: ties to the lower id
    for t, G, thr in ((tgt, synth.default_guess(), R.DEFAULTS["corr_dist_threshold"]), (tgt, I4, 1.0), (ties, synth.default_guess(), 2.0)):
        a = R.one_step(src, t, G, None, thr)
        b = R.one_step(src, t, G, None, thr, exhaustive=False)
        assert a["m"] == b["m"] and np.array_equal(a["idx"], b["idx"]) and a["d2"].tobytes() == b["d2"].tobytes()
        assert a["sums"].tobytes() == b["sums"].tobytes()
    assert (a["idx"][a["idx"] >= 0] < len(tgt)).all()


def test_tree_sum_is_the_fixed_tree():
    rng = np.random.default_rng(4)
    v = rng.normal(size=(700, 2)) * 10.0 ** rng.integers(-6, 7, (700, 2))
    chunks = []
    for c0 in range(0, 700, 256):                                                                  # the tree, spelled out for three chunks
        a = np.zeros((256, 2))
        a[:len(v[c0:c0 + 256])] = v[c0:c0 + 256]
        waves = []
        for w in range(4):
            lane = a[64 * w:64 * w + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                lane = np.array([lane[i] + lane[i ^ o] for i in range(64)])
            waves.append(lane[0])
        chunks.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    slots = np.zeros((256, 2))
    for c, part in enumerate(chunks):
        slots[c % 256] = slots[c % 256] + part
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        for t in range(o):
            slots[t] = slots[t] + slots[t + o]
    assert R.tree_sum(v).tobytes() == slots[0].tobytes()
    assert abs(R.tree_sum(v) - v.sum(axis=0)).max() <= 1e-11 * np.abs(v).sum(axis=0).max()


def test_host_pieces_of_the_engine():
    # the engine's own jacobi_svd3, estimate, criteria and icp_outer (C++, host only) over a CPU evaluator: tests/hip/icp_host_check.hip
    import subprocess

    import __graft_entry__ as g
    exe = g.build_icp_host_check() if os.path.exists(g.HIPCC) else os.path.join(g.ROOT, "tests", "hip", "icp_host_check")   # (else: prebuilt)
    if not os.path.exists(exe):
        pytest.skip("no hipcc and no prebuilt tests/hip/icp_host_check")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "icp_host_check: ok" in out.stdout


def test_verify_candidates_icp_drives_one_batch_and_one_score_call():
    from lv_slam_amd import loop_closure

    class Fake:
        def __init__(self):
            self.calls, self.next = [], 10

        def keyframe_add(self, c):
            self.next += 1
            return self.next

        def keyframe_release(self, i):
            self.calls.append(("release", i))

        def icp_set_target(self, cloud=None, keyframe=None):
            self.calls.append(("target", keyframe))

        def icp_batch_reserve(self, n):
            self.calls.append(("reserve", n))

        def icp_batch_set_source(self, k, cloud=None, keyframe=None):
            self.calls.append(("source", k, keyframe))

        def icp_batch_align(self, G):
            self.calls.append(("align", len(G)))
            return [dict(converged=k != 1, final=np.eye(4, dtype=np.float32) * (k + 1)) for k in range(len(G))]

        def keyframe_fitness_scores(self, a, b, T, r):
            self.calls.append(("scores", list(a), list(b)))
            return np.array([0.9, 0.1, 0.3][: len(a)]), None

    e = Fake()
    G = np.stack([I4] * 3)
    got = loop_closure.verify_candidates_icp(e, 5, [np.zeros((4, 3), np.float32), 7, 8], G, 1.0, 0.5)
    assert got[0] == 2 and got[2] == 0.3 and got[3] == 3 and got[1].tobytes() == (np.eye(4, dtype=np.float32) * 3).tobytes()
    kinds = [c[0] for c in e.calls]
    assert kinds.count("align") == 1 and kinds.count("scores") == 1 and kinds.count("reserve") == 1
    assert ("target", 5) in e.calls and ("source", 0, 11) in e.calls and ("source", 1, 7) in e.calls and ("release", 11) in e.calls
    assert ("scores", [5, 5, 5], [11, 7, 8]) in e.calls
