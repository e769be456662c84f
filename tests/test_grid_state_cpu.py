"""CPU: lv_slam_amd/csrc/ndt_grid_state.hpp -- what a configuration needs of the resident target grids (grid_extras) and whether the grids a
build left serve a need (grids_serve) -- compiled into a stand-alone program (tests/cpp/grid_state_main.cpp) with -fsanitize=address,undefined
and compared, over all 4 searches x 2 variants x {dead, live More-Thuente} x MI355NDT_OPT_ARITH {0, 1} x live {false, true}, with the rules
written out here as the build stated them before the header existed (what it made was decided inside the kernel chain: centroids for KDTREE or
a live More-Thuente loop, f64 inverse covariances for the live loop, kd weights for ndt_pca + KDTREE, the tolerance arithmetic's records for
MI355NDT_OPT_ARITH = 1 with DIRECT1 / DIRECT7 and the dead loop).  (The engine that uses the header: tests/test_grid_state_gpu.py.)
"""
import itertools
import os
import subprocess

import pytest

from conftest import ROOT
from lv_slam_amd import ndt

HEADER = os.path.join(ROOT, "lv_slam_amd", "csrc", "ndt_grid_state.hpp")
CONFIGS = list(itertools.product((ndt.KDTREE, ndt.DIRECT26, ndt.DIRECT7, ndt.DIRECT1), (ndt.VARIANT_OMP, ndt.VARIANT_PCA), (0, 1), (0, 1)))


def expected_extras(search, variant, mt, arith, live):
    mt_live = bool(mt or live)
    return (int(search == ndt.KDTREE or mt_live),                                       # cent
            int(mt_live),                                                               # icov64
            int(search == ndt.KDTREE and variant == ndt.VARIANT_PCA),                   # kdw
            int(arith == 1 and search in (ndt.DIRECT1, ndt.DIRECT7) and not mt_live))   # recs_fast


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grid_state") / "grid_state_main")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "grid_state_main.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stderr == "", run.stderr             # a sanitizer report writes to stderr and changes the status
    lines = [l.split() for l in run.stdout.splitlines()]
    extras = {tuple(int(v) for v in l[1:6]): tuple(int(v) for v in l[6:10]) for l in lines if l[0] == "extras"}
    serve = {(int(l[1]), int(l[2])): int(l[3]) for l in lines if l[0] == "serve"}
    invalid = [int(l[1]) for l in lines if l[0] == "invalid"]
    return extras, serve, invalid


def test_the_enumeration_is_the_headers():
    assert (ndt.KDTREE, ndt.DIRECT26, ndt.DIRECT7, ndt.DIRECT1) == (0, 1, 2, 3) and (ndt.VARIANT_OMP, ndt.VARIANT_PCA) == (0, 1)
    assert len(CONFIGS) == 32 and [((s * 2 + v) * 2 + m) * 2 + a for s, v, m, a in CONFIGS] == list(range(32))


def test_grid_extras_of_every_configuration(tables):
    extras = tables[0]
    assert len(extras) == 64
    for (s, v, m, a), live in itertools.product(CONFIGS, (0, 1)):
        assert extras[(s, v, m, a, live)] == expected_extras(s, v, m, a, live), (s, v, m, a, live)
    # the live flavour never holds the tolerance arithmetic's records, and is the configuration's own where its More-Thuente loop is live
    assert all(extras[c + (1,)][3] == 0 and extras[c + (1,)][:2] == (1, 1) for c in CONFIGS)
    assert all(extras[c + (0,)] == extras[c + (1,)] for c in CONFIGS if c[2] == 1)


def test_grids_serve_of_every_pair(tables):
    _, serve, invalid = tables
    assert len(serve) == 32 * 32
    for (ia, ca), (ib, cb) in itertools.product(enumerate(CONFIGS), repeat=2):
        made, need = expected_extras(*ca, 0), expected_extras(*cb, 0)
        assert serve[(ia, ib)] == int(all(m or not n for m, n in zip(made, need))), (ca, cb)
    assert all(serve[(i, i)] == 1 for i in range(32))                       # a build for c serves c
    assert invalid == [0]                                                   # grids over a cloud that is gone serve nothing, whatever they hold


def test_header_has_nothing_of_hip():
    text = open(HEADER).read()
    assert "#include <hip" not in text and "__global__" not in text and "hipStream" not in text and "__device__" not in text
    assert [l for l in text.splitlines() if l.startswith("#include")] == ['#include "mi355_ndt.h"']
