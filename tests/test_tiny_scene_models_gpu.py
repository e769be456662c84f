"""GPU (-m gpu): the two newest sweeps -- the Euler-angle pose model (MI355NDT_OPT_POSE_MODEL = 1: k_sweep<false, K, 8, false, ORD, 1>, four
searches, two f32 sum orders) and PCL's f64 class (MI355NDT_OPT_NDT_CLASS = 1: k_sweep<false, 27, 8, false, 0, 2>) -- on the tiny scenes of
tests/ndt_ref.py, where tests/test_ndt_euler_gpu.py and tests/test_ndt_pcl_gpu.py run them on synthetic scans near the origin: a 4 x 4 x 4-cell
grid (all but eight cells touch a face), source rows outside the grid and a NaN row, 37 m ("mid") and 580 m ("far") from the origin, 1, 64, 65 and
513 points, a yaw of 0.02 rad and (roll, pitch, yaw) = (0.12, 0.15, 0.2) about the block's centre, through mi355ndt_derivatives(p).

Bars: those tests' own -- test_gpu_parity.check_sweep at 1e-11 of the largest of the 43 numbers, equal hit counts -- against the restatements
(tools/ndt_euler_ref.sweep_euler, tools/ndt_pcl_ref.sweep_pcl) as tests/golden/ndt_tiny_models.npz holds them (tests/golden/make_tiny_models.py
writes it, tests/test_tiny_scene_models_cpu.py regenerates cases).  The worst ratio to that bar is printed for the score and g, and for the
translation, the mixed and the rotation blocks of H apart."""
import importlib.util
import os

import numpy as np
import pytest

import sweep_matrix as M
from conftest import ROOT
from lv_slam_amd import ndt
from test_gpu_parity import check_sweep

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_tiny_models", os.path.join(ROOT, "tests", "golden", "make_tiny_models.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)
MODES = {1: ("direct1", ndt.DIRECT1), 7: ("direct7", ndt.DIRECT7), 26: ("direct26", ndt.DIRECT26), 27: ("kdtree", ndt.KDTREE)}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_tiny_models.npz"))


def fixture_sweep(fx, key):
    return float(fx[key + "/score"]), fx[key + "/g"], fx[key + "/H"], int(fx[key + "/hits"])


def run(eng, fx, key_of, label):
    """every (scene, pose, size) through eng.derivatives(p) against the fixture; prints the worst ratios to check_sweep's bar, block by block"""
    worst = {}
    for sn in T.SCENES:
        sc = T.R.named_scene(sn)
        eng.set_target(sc.target)
        for n in T.SIZES:
            eng.set_source(T.source(sn, n))
            for pn in T.ANGLES:
                got = eng.derivatives(T.pose_vector(sn, pn))
                ref = fixture_sweep(fx, key_of(sn, pn, n))
                scale = 1e-11 * max(1.0, abs(ref[0]), np.abs(ref[1]).max(), np.abs(ref[2]).max())
                dH = np.abs(got[2] - ref[2]) / scale
                for block, v in (("score", abs(got[0] - ref[0]) / scale), ("g", np.abs(got[1] - ref[1]).max() / scale), ("H trans", dH[:3, :3].max()),
                                 ("H mixed", max(dH[:3, 3:].max(), dH[3:, :3].max())), ("H rot", dH[3:, 3:].max())):
                    worst[block] = max(worst.get(block, (0.0,)), (float(v), sn, pn, n))
                assert got[3] == ref[3], (label, sn, pn, n, got[3], ref[3])
                check_sweep(got, ref)
    print(f"{label}: worst |dev - restatement| / (1e-11 largest entry): " + "; ".join(f"{b} {w[0]:.3g} {w[1:]}" for b, w in worst.items()))


@pytest.mark.parametrize("K,order", M.EULER_ROWS, ids=[f"{MODES[K][0]}_ord{o}" for K, o in M.EULER_ROWS])
def test_euler_model_on_the_tiny_scenes(fx, K, order):
    name, mode = MODES[K]
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64, resolution=1.0, neighbor_mode=mode))
    eng.set_option(ndt.OPT_POSE_MODEL, 1)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    run(eng, fx, lambda sn, pn, n: T.euler_key(sn, pn, n, name, order), f"euler {name} order {order}")
    eng.close()


@pytest.mark.parametrize("K,order", M.PCL_ROWS, ids=["pcl"])
def test_pcl_class_on_the_tiny_scenes(fx, K, order):
    assert (K, order) == (27, 0)                                     # the one kernel: the radius search, no f32 sum to order
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64, resolution=1.0))
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    run(eng, fx, T.pcl_key, "pcl")
    eng.close()
