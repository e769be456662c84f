"""mi355ndt::NormalDistributionsTransformGround of include/mi355_ndt_pcl.hpp -- the object scan_matching_odom_nodelet.cpp:329 declares as
ground_s2k -- built against tests/pcl_stub (there is no PCL in this image).

CPU: the class compiles warning-free as C++14 (-Wall -Werror) and links against libmi355ndt.so.
GPU: driven through the nodelet's set-up sequence (:121-126, with a resolution at which the synthetic pair is a fixture scene) it returns what
the python class returns for one align."""
import os
import subprocess

import numpy as np
import pytest


def build_adaptor():
    import __graft_entry__ as entry
    entry.build()
    return entry.build_adaptor_ground_test()


def test_ground_adaptor_compiles_and_links_against_pcl_stub():
    exe = build_adaptor()
    assert os.path.exists(exe)
    und = subprocess.check_output(["nm", "-u", exe], text=True)
    for sym in ["mi355ndt_create", "mi355ndt_set_option", "mi355ndt_get_option", "mi355ndt_set_target", "mi355ndt_set_source", "mi355ndt_align", "mi355ndt_get_incremental"]:
        assert sym in und, sym


@pytest.mark.gpu
def test_ground_adaptor_end_to_end(tmp_path):
    from lv_slam_amd import ndt, synth
    exe = build_adaptor()
    tgt, src, _ = synth.make_pair(1, 256, n_beams=32)
    tgt, src = tgt.numpy().astype(np.float32), src.numpy().astype(np.float32)[::16]
    tgt.tofile(tmp_path / "t.f32")
    src.tofile(tmp_path / "s.f32")
    res = 10.0                                                       # the nodelet's ground_s2k resolution
    out = subprocess.check_output([exe, str(tmp_path / "t.f32"), str(tmp_path / "s.f32"), str(len(tgt)), str(len(src)), str(res)], text=True, timeout=300).split()
    F = np.array(out[:16], np.float32).reshape(4, 4).T
    L = np.array(out[16:32], np.float32).reshape(4, 4).T
    iters, conv, tp, cls, bad = int(out[32]), int(out[33]), float(out[34]), int(out[35]), int(out[36])
    assert cls == 1 and bad == -2                                    # constructed with flag_class 1; 7 is no class: MI355NDT_ERR_BAD_ARG
    reg = ndt.NormalDistributionsTransformGround()
    reg.setNumThreads(4)
    reg.setTransformationEpsilon(0.01)
    reg.setMaximumIterations(64)
    reg.setResolution(res)
    reg.setNeighborhoodSearchMethod(ndt.DIRECT1)
    reg.setInputTarget(tgt)
    reg.setInputSource(src)
    reg.align(synth.default_guess())
    print(f"ground adaptor: iterations {iters} / {reg.getFinalNumIteration()}, converged {conv}")
    assert np.array_equal(F, reg.getFinalTransformation()) and iters == reg.getFinalNumIteration() >= 1 and conv == int(reg.hasConverged()) == 1
    assert tp == reg.getTransformationProbability() and np.array_equal(L, reg.getLastIncrementalTransformation())
    # and it is the ground class that ran: the plain class ends elsewhere
    plain = ndt.NormalDistributionsTransform()
    plain.setTransformationEpsilon(0.01); plain.setMaximumIterations(64); plain.setResolution(res); plain.setNeighborhoodSearchMethod(ndt.DIRECT1)
    plain.setInputTarget(tgt); plain.setInputSource(src)
    plain.align(synth.default_guess())
    assert not np.array_equal(F, plain.getFinalTransformation())
    reg.engine.close(); plain.engine.close()
