"""CPU: the host pieces of the GICP batch (mi355ndt_gicp_batch_*: every candidate of a loop check aligned in one lockstep batch).

  * the rendezvous, lv_slam_amd/csrc/gicp_lockstep.hpp, under the optimiser, lv_slam_amd/csrc/gicp_bfgs.hpp, compiled into a stand-alone
    program (tests/cpp/gicp_lockstep_main.cpp) with -fsanitize=thread -pthread -ffp-contract=off: 1, 2, 5 and 64 starts minimised one after
    the other and in lockstep agree word for word (x, f, status, inner iterations, evaluations per slot), rounds == max_k requests[k], and a
    run whose serve callback fails in round 3 returns with every worker ended.  A ThreadSanitizer report fails the test;
  * the C-ABI without a GPU: the new symbols, NULL handles, MI355NDT_GICP_BATCH_MAX.  (What needs a handle: tests/test_gicp_batch_gpu.py.)
"""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
from lv_slam_amd import ndt

KS = (1, 2, 5, 64)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gicp_lockstep") / "gicp_lockstep_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=thread", "-pthread",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "gicp_lockstep_main.cpp"), "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_lockstep_program_agrees_with_the_sequential_runs(run):
    print(run.stdout[-2000:])
    assert run.returncode == 0 and run.stderr == "", run.stderr           # a ThreadSanitizer report writes to stderr and changes the status
    lines = [l.split() for l in run.stdout.splitlines()]
    assert not any("differs" in l for l in lines)
    for K in KS:
        slots = [l for l in lines if l[0] == str(K) and l[1] != "rounds"]
        rounds = [int(l[2]) for l in lines if l[0] == str(K) and l[1] == "rounds"]
        assert len(slots) == K and len(rounds) == 1
        requests = [int(l[4]) for l in slots]
        assert rounds[0] == max(requests)
        if K > 1:
            assert sum(requests) > rounds[0] and len(set(requests)) > 1     # the slots end in different rounds
        if K >= 5:
            assert slots[2][2:5] == ["1", "1", "1"]                         # zero_gradient: NoProgress before its first step, one evaluation
    assert lines[-1][:4] == ["failure", "in", "round", "3:"] and lines[-1][-4:] == ["0", "after", "3", "rounds"]


def test_lockstep_header_has_nothing_of_hip():
    text = open(os.path.join(ROOT, "lv_slam_amd", "csrc", "gicp_lockstep.hpp")).read()
    assert "#include <hip" not in text and "__global__" not in text and "hipStream" not in text


# ---- the C-ABI without a GPU --------------------------------------------------------------------------------------
BATCH_SYMBOLS = ("mi355ndt_gicp_batch_reserve", "mi355ndt_gicp_batch_set_source", "mi355ndt_gicp_batch_set_source_keyframe",
                 "mi355ndt_gicp_batch_align", "mi355ndt_gicp_batch_get_aligned", "mi355ndt_gicp_batch_stats")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_batch_symbols_exist(lib):
    for name in BATCH_SYMBOLS:
        assert name in ndt.SYMBOLS and callable(getattr(lib, name)), name
    for name in ("gicp_batch_reserve", "gicp_batch_set_source", "gicp_batch_align", "gicp_batch_get_aligned", "gicp_batch_stats"):
        assert callable(getattr(ndt.Engine, name, None)), name
    from lv_slam_amd import loop_closure
    assert callable(loop_closure.verify_candidates_gicp)


def test_batch_null_handle_is_refused_not_dereferenced(lib):
    buf = (C.c_double * 16)()
    n = C.c_int(0)
    assert lib.mi355ndt_gicp_batch_reserve(None, 1) == -1
    assert lib.mi355ndt_gicp_batch_reserve(None, 65) == -1
    assert lib.mi355ndt_gicp_batch_set_source(None, 0, buf, 1, 12) == -1
    assert lib.mi355ndt_gicp_batch_set_source_keyframe(None, 0, 0) == -1
    assert lib.mi355ndt_gicp_batch_align(None, None, None) == -1
    assert lib.mi355ndt_gicp_batch_get_aligned(None, 0, None, 12) == -1
    assert lib.mi355ndt_gicp_batch_stats(None, C.byref(n), None) == -1


def test_batch_max_in_the_header_is_the_mirrors(lib, tmp_path):
    """MI355NDT_GICP_BATCH_MAX is 64 in the header and in the mirror; the engine refuses 0 and 65 slots (tests/test_gicp_batch_gpu.py), and
    the mirror refuses guesses of another shape before the library sees them"""
    src = tmp_path / "mx.c"
    src.write_text('#include <stdio.h>\n#include "mi355_ndt.h"\nint main(void) { printf("%d %zu\\n", MI355NDT_GICP_BATCH_MAX, sizeof(mi355ndt_gicp_result)); return 0; }\n')
    exe = tmp_path / "mx"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [64, C.sizeof(ndt.GicpResult)] and ndt.GICP_BATCH_MAX == 64
    if lib.mi355ndt_device_count() <= 0:
        with pytest.raises(ndt.NDTError) as e:                            # no CPU fallback
            ndt.Engine()
        assert e.value.code == -5
