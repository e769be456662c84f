"""CPU: tools/ndt_euler_ref.py, the restatement of the Euler-angle NDT (include/ndt_omp/ndt_omp_impl.hpp) that MI355NDT_OPT_POSE_MODEL = 1 is
held to, checked against itself; the committed fixture against the tool; the header's option constant against the binding."""
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


E = _load("ndt_euler_ref")
mg = E.mg


@pytest.fixture(scope="module")
def scene():
    tgt, src = E.clouds(4)
    return mg.build_grid(tgt, 1.0), E.subsample(src, 200), mg.gauss_constants(0.55, 1.0)


# poses at which the turned-back source meets the target: general angles; one angle inside the 10e-5 snap of impl.hpp:292-325; large pitch
FD_POSES = {"general": [1.0, 0.02, -0.01, 0.1, 0.2, 0.3], "snapped": [1.0, 0.0, 0.0, 0.15, 5e-5, -0.2], "pitch_1.2": [1.0, 0.0, 0.0, -0.3, 1.2, 0.4]}


@pytest.mark.parametrize("name", list(FD_POSES))
def test_gradient_is_the_derivative_of_the_score(scene, name):
    """the analytic gradient of the restatement (plain f64 mode: the same J from j_ang, no f32 rounding) against central differences of its
    own score.  Bounds: a central difference with h = 1e-6 of a smooth function with derivatives of order 1e2 carries ~1e-10 h^2 truncation
    and ~1e-16 * |score| / h = 1e-8 rounding, relative to a gradient of order 1e2: 1e-7 is two orders above that.  Inside the snap the tables
    take sin = 0, cos = 1 for an angle of 5e-5, an error of 5e-5 in the entries of j_ang, so the gradient is off by that relative amount
    times a few terms: 5e-4."""
    grid, s, (d1, d2, _) = scene
    p = np.array(FD_POSES[name], np.float64)
    s = (s.astype(np.float64) @ E.rot64(p)).astype(np.float32)           # the moved cloud is the plain pair's: hundreds of hits
    score, g, _ = E.sweep_euler_f64(grid, s, p, d1, d2, E.DIRECT7)
    h = 1e-6
    fd = np.array([(E.sweep_euler_f64(grid, s, p + h * e, d1, d2, E.DIRECT7, hood_pose=p)[0] - E.sweep_euler_f64(grid, s, p - h * e, d1, d2, E.DIRECT7, hood_pose=p)[0]) / (2 * h)
                   for e in np.eye(6)])
    err = np.abs(g - fd).max() / np.abs(g).max()
    print(name, "score", score, "max |g|", np.abs(g).max(), "relative error", err)
    assert np.abs(g).max() > 1.0
    assert err < (5e-4 if name == "snapped" else 1e-7)
    if name == "snapped":
        assert err > 1e-7                                             # the snap is really taken: the tables are not those of the exact pose
    # and the f32 evaluation is the f64 one to f32 rounding (a few hundred terms of relative error 1e-7 each)
    r32 = E.sweep_euler(grid, s, p, d1, d2, E.DIRECT7, T32=None)
    assert r32[3] > 150
    assert np.abs(r32[1] - g).max() / np.abs(g).max() < (5e-4 if name == "snapped" else 1e-5)


def test_hessian_is_the_derivative_of_the_gradient(scene):
    """... and the Hessian (h_ang: the second tables) against central differences of the gradient, same bound -- but for entry (4, 4): row d1 of
    h_ang ends in +sy (impl.hpp:359, 381) where the second derivative of Rx Ry Rz by the pitch has -sy.  The reference's table is restated as it
    stands, so that one entry is NOT the derivative of the gradient, and this test says so."""
    grid, s, (d1, d2, _) = scene
    p = np.array(FD_POSES["general"], np.float64)
    s = (s[:60].astype(np.float64) @ E.rot64(p)).astype(np.float32)
    _, _, H = E.sweep_euler_f64(grid, s, p, d1, d2, E.DIRECT7, hessian=True)
    h = 1e-6
    fd = np.array([(E.sweep_euler_f64(grid, s, p + h * e, d1, d2, E.DIRECT7, hood_pose=p)[1] - E.sweep_euler_f64(grid, s, p - h * e, d1, d2, E.DIRECT7, hood_pose=p)[1]) / (2 * h)
                   for e in np.eye(6)])
    err = np.abs(H - fd) / np.abs(H).max()
    d1_entry = err[4, 4]
    err[4, 4] = 0.0
    assert err.max() < 1e-7
    assert d1_entry > 1e-5


def test_euler_round_trip():
    """convert_transform(euler_angles_012(R)) reproduces R to f32 rounding, negative roll (the chart near roll = pi) included; the f32
    composition agrees with make_golden's f64 one to f32 rounding"""
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.uniform(-3.1, 3.1, (300, 3)), [[-0.3, 0, 0], [-1e-3, 0.2, 0.1], [-3.0, 1.0, -2.0], [0.3, 0, 0], [0, 0, 0]]])
    flipped = 0
    for a in xs:
        x = np.concatenate([rng.normal(0, 2, 3), a])
        M = E.convert_transform_f32(x)
        assert np.abs(M - mg.convert_transform(x)).max() <= 4 * 2.0 ** -24          # a few roundings of entries of size <= 1
        e = E.euler_angles_012(M)
        back = E.convert_transform_f32(np.concatenate([x[:3], e.astype(np.float64)]))
        assert np.abs(back - M).max() <= 8 * 2.0 ** -24, (a, e)
        if -np.pi < a[0] < 0 and abs(a[1]) < 1.5:
            # Eigen's rule: atan2(m12, m22) > 0 moves the first angle by -pi.  The roll that comes back lies in [0, pi]
            assert e[0] >= 0 and abs(abs(e[0] - a[0]) - np.pi) < 1e-5, (a, e)
            flipped += 1
    assert flipped > 50
    e = E.euler_angles_012(E.convert_transform_f32([0, 0, 0, -0.3, 0, 0]))           # a guess with roll -0.3 starts at roll pi - 0.3, pitch and yaw +-pi
    assert abs(e[0] - (np.pi - 0.3)) < 1e-6 and abs(abs(e[1]) - np.pi) < 1e-6 and abs(abs(e[2]) - np.pi) < 1e-6


def test_fixture_is_what_the_tool_writes(golden_dir):
    """one case of each kind regenerated and compared with the committed fixture word for word"""
    z = np.load(os.path.join(golden_dir, "ndt_euler.npz"))
    out = {}
    E._pack_sweep(out, "shape/65", E.shape_case(65))
    E._pack_sweep(out, "shape/1", E.shape_case(1))
    for k, v in out.items():
        assert np.asarray(v).tobytes() == z[k].tobytes(), k
    assert int(z["shape/1/hits"]) == 1
    # what the GPU tests rely on: every pose case meets more than 1000 leaves, every align keeps clear of a convergence decision
    keys = [k for k in z.files if k.startswith("pose/") and k.endswith("/hits")]
    assert len(keys) == 3 * 5 * 2 and all(int(z[k]) > 1000 for k in keys)
    for i in range(len(E.ALIGNS)):
        steps = z[f"align/{i}/steps"]
        assert len(steps) == int(z[f"align/{i}/iterations"]) and (np.abs(steps - 0.01) > 0.05 * 0.01).all()


def test_header_option_matches_binding(tmp_path):
    """MI355NDT_OPT_POSE_MODEL as the header spells it is what the python binding passes"""
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include "mi355_ndt.h"\nint main(void) { printf("%d\\n", MI355NDT_OPT_POSE_MODEL); return 0; }\n')
    exe = tmp_path / "opt"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == ndt.OPT_POSE_MODEL == 12
    assert ndt.POSE_MODELS == {"se3": 0, "euler": 1}
