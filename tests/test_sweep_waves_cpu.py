"""CPU: lv_slam_amd/csrc/ndt_sweep_waves.hpp -- MI355NDT_OPT_SWEEP_WAVES as the engine's host side decides it -- compiled into a stand-alone program
(tests/cpp/sweep_waves_main.cpp) with -fsanitize=address,undefined and compared with the rules written out here: the option takes 0, 2 and 3
and is refused while a stream is open; only the exact ndt_omp / DIRECT7 launch has a three-wave body; the automatic choice takes it where the
estimated records of a target stay under a quarter of an XCD's L2 shared by the three pairs in flight.  (mi355ndt_set_option needs a handle,
hence a GPU: tests/test_sweep_waves_gpu.py asks the engine the same questions.)"""
import os
import subprocess

import pytest

from conftest import ROOT
from lv_slam_amd import ndt

HEADER = os.path.join(ROOT, "lv_slam_amd", "csrc", "ndt_sweep_waves.hpp")
OK, BAD_ARG, STATE = 0, -2, -7


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep_waves") / "sweep_waves_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "sweep_waves_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr             # a sanitizer report writes to stderr and changes the status
    t = {}
    for l in run.stdout.splitlines():
        w = l.split()
        t.setdefault(w[0], []).append([float(x) if "." in x or "e" in x else int(x) for x in w[1:]])
    return t


def test_option_values_and_the_stream(tables):
    got = {(s, v): rc for s, v, rc in tables["option"]}
    assert len(got) == 16
    for v in range(-2, 6):
        assert got[(0, v)] == (OK if v in (0, 2, 3) else BAD_ARG), v       # out of range: refused
        assert got[(1, v)] == STATE, v                                     # a stream is open: refused, whatever the value
    assert ndt.OPT_SWEEP_WAVES == 14 and ndt.ERR[STATE] and ndt.ERR[BAD_ARG]


def test_only_exact_omp_direct7_has_a_three_wave_body(tables):
    got = {(p, k, o): e for p, k, o, e in tables["exists"]}
    assert len(got) == 24
    for (p, k, o), e in got.items():
        assert e == int(p == 0 and k == 7 and o in (0, 1)), (p, k, o)      # not ndt_pca, not DIRECT1 / DIRECT26 / KDTREE, not the tolerance arithmetic


def test_threshold_and_estimate(tables):
    (l2, pairs, thresh, ppm2, rec), = tables["const"]
    # a quarter of an XCD's 4 MB L2 for the records of the three pairs in flight at three waves per SIMD
    assert (l2, pairs, rec) == (4 << 20, 3, 64) and thresh == l2 // 4 // pairs == 349525 and ppm2 == 32
    for res, mp, n, b in tables["bytes"]:
        leaves = min(n / (ppm2 * res * res), n / mp)
        assert b == int(leaves * rec), (res, mp, n, b)
    by = {(res, mp, n): b for res, mp, n, b in tables["bytes"]}
    assert by[(1, 6, 65536)] == 131072 and by[(0.5, 6, 131072)] == 1 << 20  # configs 3 and 5


def test_the_choice(tables):
    (_, _, thresh, ppm2, rec), = tables["const"]
    rows = tables["choice"]
    assert len(rows) == 3 * 2 * 4 * 3 * 4 * 5
    for opt, variant, mode, ord_, res, n, waves in rows:
        body = variant == ndt.VARIANT_OMP and mode == ndt.DIRECT7 and ord_ in (0, 1)
        fits = int(min(n / (ppm2 * res * res), n / 6) * rec) <= thresh
        want = 3 if body and (opt == 3 or (opt == 0 and fits)) else 2
        assert waves == want, (opt, variant, mode, ord_, res, n, waves)
    pick = {tuple(r[:6]): r[6] for r in rows}
    assert pick[(0, 0, ndt.DIRECT7, 0, 1, 65536)] == 3                      # config 3: three waves
    assert pick[(0, 0, ndt.DIRECT7, 0, 0.5, 131072)] == 2                   # config 5's grids: two
    assert pick[(0, 0, ndt.DIRECT7, 1, 1, 4096)] == 3 and pick[(0, 0, ndt.DIRECT7, 2, 1, 4096)] == 2


def test_header_has_nothing_of_hip():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "__global__" not in text and "hipStream" not in text and "__device__" not in text
