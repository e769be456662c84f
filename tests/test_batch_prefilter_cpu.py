"""CPU: the parts of the batch prefilter surface that need no GPU -- mi355ndt_prefilter_params_default, and the Python wrappers' own argument
checks, which refuse before the library is called."""
import ctypes as C

import numpy as np
import pytest

from lv_slam_amd import ndt


def test_prefilter_params_default():
    L = ndt.load_library()
    p = ndt.PrefilterParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert L.mi355ndt_prefilter_params_default(C.byref(p)) == ndt.OK
    assert p.use_distance_filter == 1 and p.distance_near == 1.0 and p.distance_far == 100.0          # prefiltering_nodelet.cpp:83-85
    assert p.downsample_resolution == np.float32(0.1) and p.use_transform == 0
    assert list(p.transform_colmajor) == list(np.eye(4, dtype=np.float32).ravel())
    assert L.mi355ndt_prefilter_params_default(None) == -2
    assert ndt.OPT_PREFILTER_GROUP == 11


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called the library ({name}) before refusing its arguments")


def _engine_without_gpu():
    eng = object.__new__(ndt.Engine)            # no mi355ndt_create: the checks below must not reach the library
    eng.lib, eng.h = _NoLibrary(), None
    return eng


def test_wrappers_refuse_before_calling_the_library():
    eng = _engine_without_gpu()
    a = np.zeros((10, 3), np.float32)
    with pytest.raises(ValueError):
        eng.batch_prefilter([a, a], [a])                                   # one source per target
    with pytest.raises(ValueError):
        eng.batch_prefilter(None, None)
    for bad in (np.eye(3), np.zeros(16), np.zeros((4, 4, 1))):
        with pytest.raises(ValueError):
            eng.batch_prefilter([a], None, transform=bad)
        with pytest.raises(ValueError):
            eng.sequence_run_raw([a, a], [0.0, 0.1], transform=bad)
    with pytest.raises(ValueError):
        eng.sequence_run_raw([a, a], [0.0])                                # one stamp per frame
    with pytest.raises(ValueError):
        eng.batch_prefilter([np.zeros((10, 2), np.float32)], None)         # not a cloud
