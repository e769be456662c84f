"""CPU: tools/ndt_pcl_ref.py, the restatement of pcl::NormalDistributionsTransform that MI355NDT_OPT_NDT_CLASS = 1 is held to, checked against
itself and against the f32 Euler restatement; the committed fixture against the tool; select_registration_method branch by branch; the header's
option constant against the binding; the class-taking functions of ndt_grid_state.hpp."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, registrations


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


P = _load("ndt_pcl_ref")
E, mg = P.E, P.mg
SWEEP_BAR = 1e-11                                                    # test_gpu_parity.check_sweep's rtol: what the device is held to


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_pcl.npz"))


@pytest.fixture(scope="module")
def scene():
    return P.cells_of(4, 1.0), E.subsample(E.clouds(4)[1], 200), mg.gauss_constants(0.55, 1.0)


FD_POSES = {"general": [1.0, 0.02, -0.01, 0.1, 0.2, 0.3], "snapped": [1.0, 0.0, 0.0, 0.15, 5e-5, -0.2], "pitch_1.2": [1.0, 0.0, 0.0, -0.3, 1.2, 0.4]}


@pytest.mark.parametrize("name", list(FD_POSES))
def test_gradient_is_the_derivative_of_the_score(scene, name):
    """the analytic gradient against central differences of the restatement's own score over FIXED (point, leaf) pairs (exact_move: the moved
    point in f64, a smooth function; hood_pose: the pairs of the centre pose).  Bounds as in tests/test_ndt_euler_cpu.py: h = 1e-6 leaves ~1e-10
    truncation and ~1e-8 rounding relative to a gradient of order 1e2, so 1e-7; inside the snap the tables are off by 5e-5: 5e-4."""
    cells, s, (d1, d2, _) = scene
    p = np.array(FD_POSES[name], np.float64)
    s = (s.astype(np.float64) @ E.rot64(p)).astype(np.float32)           # the moved cloud is the plain pair's: hundreds of hits
    score, g, _, hits = P.sweep_pcl(cells, s, p, d1, d2, exact_move=True)
    h = 1e-6
    fd = np.array([(P.sweep_pcl(cells, s, p + h * e, d1, d2, exact_move=True, hood_pose=p)[0] - P.sweep_pcl(cells, s, p - h * e, d1, d2, exact_move=True, hood_pose=p)[0]) / (2 * h)
                   for e in np.eye(6)])
    err = np.abs(g - fd).max() / np.abs(g).max()
    print(name, "score", score, "hits", hits, "max |g|", np.abs(g).max(), "relative error", err)
    assert hits > 150 and np.abs(g).max() > 1.0
    assert err < (5e-4 if name == "snapped" else 1e-7)
    if name == "snapped":
        assert err > 1e-7                                             # the snap is really taken
    # and the sweep as the class runs it (the f32 moved point widened) is that function to the f32 rounding of a coordinate
    got = P.sweep_pcl(cells, s, p, d1, d2)
    assert got[3] == hits and np.abs(got[1] - g).max() / np.abs(g).max() < 1e-4


def test_hessian_is_the_derivative_of_the_gradient(scene):
    """... and the Hessian against central differences of the gradient, same bound -- but for entry (4, 4): row d1 of h_ang ends in +sy where the
    second derivative has -sy (tests/test_ndt_euler_cpu.py); the table is restated as it stands, and this test says so"""
    cells, s, (d1, d2, _) = scene
    p = np.array(FD_POSES["general"], np.float64)
    s = (s[:60].astype(np.float64) @ E.rot64(p)).astype(np.float32)
    _, _, H, hits = P.sweep_pcl(cells, s, p, d1, d2, exact_move=True)
    h = 1e-6
    fd = np.array([(P.sweep_pcl(cells, s, p + h * e, d1, d2, exact_move=True, hood_pose=p)[1] - P.sweep_pcl(cells, s, p - h * e, d1, d2, exact_move=True, hood_pose=p)[1]) / (2 * h)
                   for e in np.eye(6)])
    err = np.abs(H - fd) / np.abs(H).max()
    d1_entry = err[4, 4]
    err[4, 4] = 0.0
    print("hits", hits, "max error", err.max(), "entry (4, 4)", d1_entry)
    assert hits > 50 and err.max() < 1e-7
    assert d1_entry > 1e-5


def test_the_vectorised_search_is_radius_search(scene):
    """all_pairs finds, for every point, the leaves make_golden.radius_search returns"""
    cells, s, _ = scene
    xt = P.move_cloud(E.convert_transform_f32([1.0, 0, 0, 0, 0, 0]), s[:40])
    pi, li = P.all_pairs(cells, xt, 1.0)
    cand = [L for _, L in sorted(cells.grid["leaves"].items()) if L.n_pushed >= cells.grid["min_points"]]
    total = 0
    for i in range(len(xt)):
        want = {id(L) for L in mg.radius_search(cells.grid, xt[i], 1.0)}
        assert {id(cand[k]) for k in li[pi == i]} == want
        total += len(want)
    assert total > len(xt) // 2                                     # not vacuous: on average more than every second point meets a leaf


def test_f64_class_is_not_the_f32_model_with_kdtree(fx):
    """for every sweep case of the fixture the f64 restatement and the f32 one (sweep_euler, KDTREE, same pose) differ by more than 100 x the
    sweep bar and by less than 1e-4 of the largest entry: a device that merely ran model 1 with KDTREE fails the GPU tests, and the two are the
    same mathematics"""
    keys = [f"shape/{n}" for n in P.SHAPE_SIZES] + [f"pose/{name}" for name in P.pose_cases()]
    assert len(keys) == 10
    for k in keys:
        k32 = k.replace("/", "_f32/", 1)
        a = [np.asarray(fx[f"{k}/{f}"], np.float64) for f in ("score", "g", "H")]
        b = [np.asarray(fx[f"{k32}/{f}"], np.float64) for f in ("score", "g", "H")]
        assert int(fx[k + "/hits"]) == int(fx[k32 + "/hits"]) > 0
        largest = max(np.abs(x).max() for x in a)
        scale = max(1.0, largest)                                     # check_sweep's scale
        d = max(np.abs(x - y).max() for x, y in zip(a, b))
        print(k, "hits", int(fx[k + "/hits"]), "difference / scale", d / scale)
        assert d > 100 * SWEEP_BAR * scale and d < 1e-4 * largest


def test_fixture_is_what_the_tool_writes(fx):
    """one sweep case and one align case regenerated and compared with the committed fixture word for word; and what the GPU tests rely on"""
    out = {}
    E._pack_sweep(out, "shape/65", P.shape_case(65))
    E._pack_sweep(out, "shape/1", P.shape_case(1))
    E._pack_align(out, "align/4", P.align_case(4))
    for k, v in out.items():
        assert np.asarray(v).tobytes() == fx[k].tobytes(), k
    assert int(fx["shape/1/hits"]) >= 1
    assert all(int(fx[f"pose/{name}/hits"]) > 1000 for name in P.pose_cases())
    assert len(P.ALIGNS) >= 7 and sum(a[1] is None and a[3] == 1.0 for a in P.ALIGNS) >= 4
    assert any(a[1] == (1, 0, 0) and a[2] == -0.3 for a in P.ALIGNS) and any(a[1] == (0, 0, 1) and a[2] == 1.3 for a in P.ALIGNS)
    for i, a in enumerate(P.ALIGNS):
        steps = fx[f"align/{i}/steps"]
        assert len(steps) == int(fx[f"align/{i}/iterations"]) and (np.abs(steps - 0.01) > 0.05 * 0.01).all()
        if a[3] == P.FACTORY_RES:
            assert a[3] == 0.5 and int(fx[f"align/{i}/points_with_hits"]) > 0.75 * a[4]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ndt_pcl.npz")) < 1 << 20


# ----------------------------------------------------------------------------- the factory
def test_factory_plan_every_branch_every_default():
    plan = registrations.plan_registration
    p = plan({})                                                     # registration_method defaults to NDT_OMP
    assert p.kind == "NDT_OMP" and p.settings == dict(transformation_epsilon=0.01, maximum_iterations=64, ndt_resolution=0.5, ndt_num_threads=0,
                                                      ndt_nn_search_method="DIRECT7", neighbor_mode=ndt.DIRECT7) and p.warnings == []
    p = plan({"registration_method": "ICP"})
    assert p.kind == "ICP" and p.settings == dict(transformation_epsilon=0.01, maximum_iterations=64, use_reciprocal_correspondences=False)
    for name, kind in (("GICP", "GICP"), ("GICP_OMP", "GICP_OMP"), ("FAST_GICP_OMP", "GICP_OMP")):
        p = plan({"registration_method": name})
        assert p.kind == kind and p.settings == dict(transformation_epsilon=0.01, maximum_iterations=64, use_reciprocal_correspondences=False,
                                                     gicp_correspondence_randomness=20, gicp_max_optimizer_iterations=20)
    # PCL's class: "NDT", and every name that holds neither ICP (as a whole) nor GICP nor OMP -- with the warning when it holds no "NDT"
    for name, warned in (("NDT", False), ("ndt", True), ("FOO", True), ("icp", True)):
        p = plan({"registration_method": name})
        assert p.kind == "NDT" and p.settings == dict(transformation_epsilon=0.01, maximum_iterations=64, ndt_resolution=0.5), name
        assert (p.warnings == [f"warning: unknown registration type({name})", "       : use NDT"]) == warned and bool(p.warnings) == warned
    p = plan({"registration_method": "FOO_OMP"})                     # unknown with OMP: warned, pclomp's class
    assert p.kind == "NDT_OMP" and len(p.warnings) == 2
    for search, mode in (("DIRECT1", ndt.DIRECT1), ("KDTREE", ndt.KDTREE), ("DIRECT7", ndt.DIRECT7), ("DIRECT26", ndt.DIRECT7), ("kdtree", ndt.DIRECT7)):
        p = plan({"registration_method": "NDT_OMP", "ndt_nn_search_method": search, "ndt_num_threads": 4, "ndt_resolution": 1.5})
        assert p.kind == "NDT_OMP" and p.settings["neighbor_mode"] == mode and p.settings["ndt_num_threads"] == 4 and p.settings["ndt_resolution"] == 1.5
    p = plan({"registration_method": "NDT", "transformation_epsilon": 0.02, "maximum_iterations": 30, "ndt_resolution": 2.0})
    assert p.settings == dict(transformation_epsilon=0.02, maximum_iterations=30, ndt_resolution=2.0)


class _FakeNDT:
    """records what the factory does to the object it builds (no device here)"""

    def __init__(self, **kw):
        self.kw, self.calls = kw, []
        for name in ("setTransformationEpsilon", "setMaximumIterations", "setResolution") + (() if kw.get("ndt_class") == "pcl" else ("setNeighborhoodSearchMethod", "setNumThreads")):
            setattr(self, name, lambda v, name=name: self.calls.append((name, v)))


class _FakeReg:
    made = []

    @classmethod
    def from_factory(cls, *a, **kw):
        cls.made.append((cls.__name__, a, kw))
        return cls()


def test_factory_builds_what_the_plan_names(monkeypatch, capsys):
    monkeypatch.setattr(registrations.ndt, "NormalDistributionsTransform", _FakeNDT)
    monkeypatch.setattr(registrations.icp, "IterativeClosestPoint", type("ICP", (_FakeReg,), {}))
    monkeypatch.setattr(registrations.gicp, "GeneralizedIterativeClosestPoint", type("GICPOMP", (_FakeReg,), {}))
    for name in ("NDT", "ndt", "FOO"):                               # all three: PCL's class at resolution 0.5, no search method, no thread count
        reg = registrations.select_registration_method({"registration_method": name})
        assert reg.kw == {"ndt_class": "pcl"}
        assert reg.calls == [("setTransformationEpsilon", 0.01), ("setMaximumIterations", 64), ("setResolution", 0.5)]
        out = capsys.readouterr()
        assert out.out == "registration: NDT 0.5\n"
        assert out.err == ("" if name == "NDT" else f"warning: unknown registration type({name})\n       : use NDT\n")
    for search, mode in (("DIRECT1", ndt.DIRECT1), ("KDTREE", ndt.KDTREE), ("anything", ndt.DIRECT7)):
        reg = registrations.select_registration_method({"registration_method": "NDT_OMP", "ndt_nn_search_method": search, "ndt_num_threads": 3}, engine="E")
        assert reg.kw == {"engine": "E"}
        assert reg.calls == [("setNumThreads", 3), ("setTransformationEpsilon", 0.01), ("setMaximumIterations", 64), ("setResolution", 0.5),
                             ("setNeighborhoodSearchMethod", mode)]
    reg = registrations.select_registration_method({})               # the default: NDT_OMP, DIRECT7, no thread count set
    assert reg.calls[0] == ("setTransformationEpsilon", 0.01) and reg.calls[-1] == ("setNeighborhoodSearchMethod", ndt.DIRECT7)
    _FakeReg.made.clear()
    registrations.select_registration_method({"registration_method": "ICP"})
    registrations.select_registration_method({"registration_method": "GICP_OMP", "gicp_correspondence_randomness": 10}, engine="E")
    assert _FakeReg.made == [("ICP", (0.01, 64, False), {}), ("GICPOMP", (0.01, 64, 10, 20), {"engine": "E"})]
    with pytest.raises(NotImplementedError, match="GICP"):
        registrations.select_registration_method({"registration_method": "GICP"})


def test_header_option_matches_binding(tmp_path):
    """MI355NDT_OPT_NDT_CLASS as the header spells it is what the python binding passes"""
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include "mi355_ndt.h"\nint main(void) { printf("%d %d\\n", MI355NDT_OPT_NDT_CLASS, MI355NDT_OPT_POSE_MODEL); return 0; }\n')
    exe = tmp_path / "opt"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"13", b"12"] and ndt.OPT_NDT_CLASS == 13 and ndt.OPT_POSE_MODEL == 12
    assert ndt.NDT_CLASSES == {"omp": 0, "pcl": 1}


def test_grid_state_takes_the_class(tmp_path):
    """the class-taking functions of ndt_grid_state.hpp (a stand-alone host program under the address and undefined-behaviour sanitizers): class 1
    needs centroids and f64 inverse covariances whatever neighbor_mode says -- DIRECT1 included -- and nothing else; class 0 answers as before"""
    exe = str(tmp_path / "grid_class_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_class_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    extras = {tuple(int(v) for v in l[1:7]): tuple(int(v) for v in l[7:11]) for l in lines if l[0] == "extras"}
    assert len(extras) == 128
    assert all(v == (1, 1, 0, 0) for k, v in extras.items() if k[0] == 1)
    assert extras[(1, ndt.DIRECT1, 0, 0, 0, 0)] == (1, 1, 0, 0) and extras[(0, ndt.DIRECT1, 0, 0, 0, 0)] == (0, 0, 0, 0)
    assert [l for l in lines if l[0] == "same"] == [["same", "0"]]
    model = {(int(l[1]), int(l[2])): tuple(int(v) for v in l[3:7]) for l in lines if l[0] == "model"}
    # (model, arith as seen with OPT_ARITH = 1, may leave the rounds, search run for DIRECT1)
    assert model == {(0, 0): (0, 1, 1, ndt.DIRECT1), (0, 1): (1, 0, 0, ndt.DIRECT1), (1, 0): (1, 0, 0, ndt.KDTREE), (1, 1): (1, 0, 0, ndt.KDTREE)}
    refuses = {tuple(int(v) for v in l[1:5]): int(l[5]) for l in lines if l[0] == "refuses"}
    for (cls, pm, variant, mt), r in refuses.items():
        assert r == int((cls == 1 or pm == 1) and (variant == 1 or mt == 1)), (cls, pm, variant, mt)
    assert [l[1] for l in lines if l[0] == "rebuild"] == ["0", "1"]  # class 0 / DIRECT7 grids do not serve class 1; class 1's serve class 0
