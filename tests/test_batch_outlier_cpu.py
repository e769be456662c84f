"""CPU: the parts of the batch outlier surface that need no GPU -- mi355ndt_outlier_params_default is what it was, the new symbols are
exported, and the Python wrappers refuse bad arguments before the library is called."""
import ctypes as C

import numpy as np
import pytest

from lv_slam_amd import ndt


def test_outlier_params_default_is_unchanged():
    L = ndt.load_library()
    p = ndt.OutlierParams()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert L.mi355ndt_outlier_params_default(C.byref(p)) == ndt.OK
    assert (p.method, p.mean_k, p.stddev_mul, p.radius, p.min_neighbors) == (ndt.OUTLIER_STATISTICAL, 20, 1.0, 0.8, 2)   # prefiltering_nodelet.cpp:63-64, 72-73
    assert L.mi355ndt_outlier_params_default(None) == -2
    assert C.sizeof(ndt.OutlierParams) == 32 and C.sizeof(ndt.OutlierStats) == 40 and C.sizeof(ndt.PrefilterParams) == 96   # the layouts stay


def test_new_symbols_are_exported():
    L = ndt.load_library()
    for name in ("mi355ndt_batch_remove_outliers", "mi355ndt_sequence_run_raw_outliers"):
        assert name in ndt.SYMBOLS
        assert getattr(L, name) is not None
    assert L.mi355ndt_batch_remove_outliers(None, 0, 1, 3, None, None, None, None, None) == -1              # MI355NDT_ERR_BAD_HANDLE
    assert L.mi355ndt_sequence_run_raw_outliers(None, 0, None, None, 12, None, None, None, None, None, None, None, None, None) == -1


def test_the_keywords_become_the_struct():
    p = ndt._outlier_dict({})
    assert (p.method, p.mean_k, p.stddev_mul, p.radius, p.min_neighbors) == (ndt.OUTLIER_STATISTICAL, 20, 1.0, 0.8, 2)
    p = ndt._outlier_dict(dict(method="radius", radius=0.5, min_neighbors=5))
    assert (p.method, p.mean_k, p.stddev_mul, p.radius, p.min_neighbors) == (ndt.OUTLIER_RADIUS, 20, 1.0, 0.5, 5)
    assert ndt._outlier_dict(dict(method="no such method")).method == 0                                     # the library refuses it with its own message


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
    for bad in (dict(mean_kk=20), dict(fetch=False), dict(return_stats=True), dict(mean_k=20, sides=3), [], "STATISTICAL", 20):
        with pytest.raises(ValueError):
            eng.batch_prefilter([a], [a], outlier=bad)
        with pytest.raises(ValueError):
            eng.sequence_run_raw([a, a], [0.0, 0.1], outlier=bad)
    with pytest.raises(ValueError):
        eng.batch_remove_outliers(targets=False, sources=False)
    with pytest.raises(ValueError):
        eng.batch_remove_outliers(0, 2, False, False, method="RADIUS")
    with pytest.raises(ValueError):
        eng.sequence_run_raw([a, a], [0.0], outlier={})                    # one stamp per frame
    with pytest.raises(ValueError):
        eng.batch_prefilter([a, a], [a], outlier={})                       # one source per target
