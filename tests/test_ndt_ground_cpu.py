"""CPU: tools/ndt_ground_ref.py, the restatement of pclomp_ground::NormalDistributionsTransformGround that MI355NDT_OPT_GROUND_CLASS is held to,
checked against make_golden's ndt_omp sweep; the committed fixture's scene conditions and one of its cases against the tool; the header's option
constant against the binding; the ground-class-taking functions of ndt_grid_state.hpp and ground_sweep_exists as tables."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("ndt_ground_ref")
mg = G.mg


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_ground.npz"))


@pytest.mark.parametrize("mode", [G.DIRECT1, G.DIRECT7])
def test_class_all_is_twice_ndt_omp(mode):
    """1: flag_class 0 gates nothing and masks nothing: g and H are 2 * make_golden.sweep's to 1e-15 of the largest entry (the reference
    doubles hit by hit inside a point's sums, not at the end: with one hit per point -- DIRECT1 -- the two are the same bits), the score and
    the hit count are equal"""
    tgt, src = G.clouds(2)
    grid = mg.build_grid(tgt, 1.0)
    d1, d2, _ = mg.gauss_constants(0.55, 1.0)
    _, T = G.sweep_pose()
    s = G.subsample(src, 200)
    score, g, H, hits, used = G.sweep_ground(grid, s, T, T, d1, d2, mode, (0,))[0]
    s0, g0, H0, hits0 = mg.sweep(grid, s, T, T, d1, d2, mode)
    scale = max(np.abs(g0).max(), np.abs(H0).max())
    eg, eH = np.abs(g - 2 * g0).max() / (2 * scale), np.abs(H - 2 * H0).max() / (2 * scale)
    print(f"mode {mode}: hits {hits}, points added {used}, |g - 2 g0| {eg:.3e}, |H - 2 H0| {eH:.3e} of the largest entry")
    assert hits == hits0 > 100 and used == len(s)
    assert score == s0
    assert eg <= 1e-15 and eH <= 1e-15
    if mode == G.DIRECT1:
        assert (g == 2 * g0).all() and (H == 2 * H0).all()


def test_masks_and_gates_of_the_restatement():
    """the hand-made floor-next-to-wall scene: the last neighbour decides, a dead leaf and a point outside the grid add nothing"""
    _, src = G.floor_wall_scene()
    grid = G.floor_wall_grid()
    assert list(G.leaf_codes(grid)) == [1, 2, 3, 0, 2]                # cell order: floor, beside, ramp, dead, above
    T = mg.se3_exp(G.IDENTITY_P).astype(np.float32)
    codes = G.deciding_codes(grid, src, T, G.DIRECT7)
    assert [tuple(c) for c in codes] == [(1, 2), (1, 2), (2, 1), (2, 1), (2, 1), (2, 1), (3, 3), (0, 0), (0, 0), (0, 0), (0, 0)]
    r = G.hand_sweeps(G.DIRECT7)
    # points added: class 1 = last code 1 (four) + the four without neighbours (angle2xy stays 0: < 10); class 2 = last code 2 (two)
    assert (r[1][4], r[2][4], r[0][4]) == (8, 2, 11)
    assert (r[1][3], r[2][3], r[0][3]) == (8, 6, 15)
    for f, held in ((1, [0, 1, 5]), (2, [2, 3, 4])):
        g, H = r[f][1], r[f][2]
        assert (g[held] == 0).all() and (H[held, :] == 0).all() and (H[:, held] == 0).all()
        free = [a for a in range(6) if a not in held]
        assert np.abs(g[free]).min() > 0 and np.linalg.matrix_rank(H) == 3
    d1 = G.hand_sweeps(G.DIRECT1)
    assert (d1[1][4], d1[2][4], d1[0][4]) == (6, 4, 11) and d1[0][3] == 7


def test_three_leaf_scene_codes():
    tgt, want = G.three_leaf_scene()
    grid = mg.build_grid(tgt, 1.0)
    assert list(G.leaf_codes(grid)) == want == [1, 2, 3]              # (the cell with five points is no record)
    G.assert_scene(grid, "three leaves")


def test_fixture_scenes_satisfy_the_conditions(fx):
    """2a: every valid leaf of every fixture scene lies at least 0.5 degrees from both thresholds and has (ev1 - ev0) / ev2 >= 1e-6 -- recomputed
    here, and equal to what the tool stored"""
    assert G.MIN_ANGLE_MARGIN == 0.5 and G.MIN_EIGEN_GAP == 1e-6
    scenes = G.fixture_scenes()
    assert (1, 10.0) in scenes and (2, 1.0) in scenes
    for pair, res in scenes:
        tgt, _ = G.clouds(pair)
        grid = mg.build_grid(tgt, res)
        m10, m80, gap = G.scene_conditions(grid)
        print(f"pair {pair} resolution {res}: {m10:.3f} and {m80:.3f} degrees from the thresholds, eigenvalue gap {gap:.3e}")
        assert m10 >= 0.5 and m80 >= 0.5 and gap >= 1e-6
        assert np.allclose(fx[f"scene/{pair}/{res}"], [m10, m80, gap], rtol=1e-9, atol=0)
        codes = G.leaf_codes(grid)
        assert (codes == fx[f"codes/{pair}/{res}"]).all() and set(codes) >= {1, 2, 3}


def test_fixture_aligns_keep_clear_of_decisions(fx):
    """2b: every step length at least 5 % from trans_epsilon; the nodelet's configuration is there; one case ends after ONE iteration with a
    step below epsilon, where ndt_omp's rule (`nr_iterations_ &&`) would go on; classes 1 and 2 solve at rank 3, class 3 at rank 6"""
    assert G.ALIGNS[0] == (1, 10.0, G.DIRECT1, 1) and G.PRM["trans_epsilon"] == 0.01 and G.PRM["max_iterations"] == 64
    assert {(m, f) for _, _, m, f in G.ALIGNS} == {(m, f) for m in (G.DIRECT1, G.DIRECT7) for f in (0, 1, 2)}
    ones = 0
    for i, (pair, res, mode, flag) in enumerate(G.ALIGNS):
        steps, ranks = fx[f"align/{i}/steps"], fx[f"align/{i}/ranks"]
        assert G.steps_clear(steps) and len(steps) == int(fx[f"align/{i}/iterations"]) >= 1 and int(fx[f"align/{i}/converged"]) == 1
        assert (ranks == (6 if flag == 0 else 3)).all()
        if len(steps) == 1:
            assert steps[0] < 0.01
            ones += 1
    assert ones >= 1 and int(fx["align/1/iterations"]) == 1
    for name in G.LAST_SCENES:
        assert int(fx[f"last/{name}/differing"]) >= G.MIN_DIFFERING == 20


def test_fixture_regenerates(fx):
    """2c: one sweep case and one align case of the committed fixture, from the tool"""
    r = G.shape_case(65)
    for f, opt in G.OPTION_OF_FLAG.items():
        assert float(fx[f"shape/65/{opt}/score"]) == r[f][0] and (fx[f"shape/65/{opt}/g"] == r[f][1]).all() and (fx[f"shape/65/{opt}/H"] == r[f][2]).all()
        assert int(fx[f"shape/65/{opt}/hits"]) == r[f][3]
    a = G.align_case(1)
    assert a["iterations"] == int(fx["align/1/iterations"]) == 1 and (a["final"] == fx["align/1/final"]).all() and a["sweeps"] == int(fx["align/1/sweeps"])
    assert os.path.getsize(G.FIXTURE) <= os.path.getsize(os.path.join(os.path.dirname(G.FIXTURE), "ndt_euler.npz"))


def test_header_option_matches_binding(tmp_path):
    """3: MI355NDT_OPT_GROUND_CLASS as the header spells it is what the python binding passes"""
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include "mi355_ndt.h"\nint main(void) { printf("%d %d\\n", MI355NDT_OPT_GROUND_CLASS, MI355NDT_BUILD_LEAF_CLASS); return 0; }\n')
    exe = tmp_path / "opt"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"15", b"18"] and ndt.OPT_GROUND_CLASS == 15 and ndt.GROUND_BUILD_BUFFERS == {"leaf_class": (18, np.dtype("u1"))}
    assert ndt.GROUND_CLASSES == {None: 0, "horizontal": 1, "vertical": 2, "all": 3} and ndt.GROUND_FLAG_CLASS == G.OPTION_OF_FLAG


def test_grid_state_takes_the_ground_class(tmp_path):
    """4: the ground-class-taking overloads of ndt_grid_state.hpp and ground_sweep_exists (a stand-alone host program under the address and
    undefined-behaviour sanitizers)"""
    exe = str(tmp_path / "ground_state_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "ground_state_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr
    lines = [l.split() for l in run.stdout.splitlines()]
    rows = lambda tag: [[int(v) for v in l[1:]] for l in lines if l[0] == tag]
    assert {v: ok for v, ok in rows("valid")} == {-1: 0, 0: 1, 1: 1, 2: 1, 3: 1, 4: 0, 5: 0}
    assert {g: ok for g, ok in rows("gated")} == {0: 0, 1: 1, 2: 1, 3: 0}
    assert rows("same") == [[0]]                                     # ground class 0: the answers (and messages) of the functions without it
    extras = {tuple(r[:6]): tuple(r[6:]) for r in rows("extras")}
    assert len(extras) == 4 * 64
    for (g, search, variant, mt, arith, live), x in extras.items():
        base = extras[(0, search, variant, mt, 0 if g else arith, live)]
        assert x == base[:4] + (int(g in (1, 2)),), (g, search, variant, mt, arith, live)      # the exact arithmetic's extras + the class codes
    assert extras[(0, ndt.DIRECT7, 0, 0, 1, 0)] == (0, 0, 0, 1, 0) and extras[(1, ndt.DIRECT7, 0, 0, 1, 0)] == (0, 0, 0, 0, 1)
    model = {tuple(r[:3]): tuple(r[3:]) for r in rows("model")}
    for (g, cls, pm), (arith, leaves) in model.items():
        assert (arith, leaves) == ((0, 0) if g else model[(0, cls, pm)])
    assert model[(0, 0, 0)] == (1, 1)
    refuses = {tuple(r[:6]): r[6] for r in rows("refuses")}
    assert len(refuses) == 4 * 2 * 2 * 4 * 2 * 2
    for (g, cls, pm, search, variant, mt), r in refuses.items():
        if g == 0:
            want = int((cls == 1 or pm == 1) and (variant == 1 or mt == 1))
        else:
            want = int(cls == 1 or pm == 1 or variant == 1 or mt == 1 or search == ndt.KDTREE)
        assert r == want, (g, cls, pm, search, variant, mt)
    # grids built for class 0 lack the codes class 1 needs; class 1's serve class 0; class 3 needs nothing more than class 0; 1 and 2 share
    assert [r[0] for r in rows("rebuild")] == [0, 1, 1, 1, 1]
    sweep = {(K, o) for K, o, ok in rows("sweep") if ok}
    assert sweep == {(K, o) for K in (1, 7, 26) for o in (0, 1)} and len(rows("sweep")) == 29 * 5
