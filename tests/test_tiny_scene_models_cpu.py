"""CPU: tests/golden/ndt_tiny_models.npz is what tests/golden/make_tiny_models.py writes -- the Euler-angle model and PCL's f64 class on the tiny
scenes of tests/ndt_ref.py -- and its cases are the ones tests/test_tiny_scene_models_gpu.py needs: hits everywhere, fewer than a full
neighbourhood somewhere, rows that meet nothing, a rotation block of H that dwarfs the translation block."""
import importlib.util
import os

import numpy as np

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("make_tiny_models", os.path.join(ROOT, "tests", "golden", "make_tiny_models.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


def test_fixture_is_what_the_tool_writes(golden_dir):
    """one small case of each model regenerated and compared with the committed fixture word for word"""
    z = np.load(os.path.join(golden_dir, "ndt_tiny_models.npz"))
    out = {}
    T.E._pack_sweep(out, T.euler_key("far", "rpy", 65, "direct7", 1), T.euler_case("far", "rpy", 65, "direct7", 1))
    T.E._pack_sweep(out, T.euler_key("mid", "yaw", 1, "kdtree", 0), T.euler_case("mid", "yaw", 1, "kdtree", 0))
    T.E._pack_sweep(out, T.pcl_key("far", "rpy", 513), T.pcl_case("far", "rpy", 513))
    T.E._pack_sweep(out, T.pcl_key("mid", "yaw", 64), T.pcl_case("mid", "yaw", 64))
    for k, v in out.items():
        assert np.asarray(v).tobytes() == z[k].tobytes(), k
    cases = [(s, p, n) for s in T.SCENES for p in T.ANGLES for n in T.SIZES]
    assert len(z.files) == 4 * (len(cases) * len(T.SEARCHES) * 2 + len(cases))


def test_the_cases_are_not_vacuous(golden_dir):
    z = np.load(os.path.join(golden_dir, "ndt_tiny_models.npz"))
    for s in T.SCENES:
        for p in T.ANGLES:
            for n in T.SIZES:
                hits = {m: int(z[T.euler_key(s, p, n, m, 0) + "/hits"]) for m in T.SEARCHES}
                assert all(int(z[T.euler_key(s, p, n, m, 1) + "/hits"]) == h for m, h in hits.items())     # the sum order moves no hit
                pcl = int(z[T.pcl_key(s, p, n) + "/hits"])
                # every case meets a leaf; DIRECT7 and the radius search stay inside the 3 x 3 x 3 block; PCL's class is the radius search
                block = hits["direct26"] + hits["direct1"]
                assert 1 <= hits["direct1"] <= hits["direct7"] <= block and 1 <= hits["kdtree"] <= block and pcl == hits["kdtree"], (s, p, n, hits, pcl)
                finite = n - (1 if n >= 8 else 0)
                if n >= 8:
                    # three rows outside the grid and a NaN row; grid-face cells: fewer than the full neighbourhood on average
                    assert hits["direct1"] <= n - 4 and hits["direct7"] < 7 * finite and hits["direct26"] < 26 * finite
                # the two f32 sum orders are different evaluations
                if n > 1:
                    assert float(z[T.euler_key(s, p, n, "direct7", 0) + "/score"]) != float(z[T.euler_key(s, p, n, "direct7", 1) + "/score"])
            # away from the origin the rotation block of H dwarfs the translation block: a bar of 1e-11 of the largest entry says little about the latter
            H = np.abs(z[T.pcl_key(s, p, 513) + "/H"])
            assert H[:3, :3].max() < 1e-2 * H[3:, 3:].max(), (s, p)
