"""CPU: the [N,4] restatement the GPU tests hold the prefilter's intensity channel to (tools/prefilter_xyzi_ref.py) against a dictionary-based
recomputation and, on its first three columns, against tools/prefilter_options_ref.py; the C ABI of mi355ndt_prefilter_params_ex2 and of
the resident-scan entry points without a device; WindowKeyframer over resident scan ids against a fake engine.  Every comparison of floats
is word for word."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import keyframes as KF
from lv_slam_amd import ndt


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(name, m)
    spec.loader.exec_module(m)
    return m


PR = _load("prefilter_options_ref")
X = _load("prefilter_xyzi_ref")
BAD_HANDLE, BAD_ARG = -1, -2


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def cloud():
    """2,000 points on a 0.1 m lattice, 1..5 per cell, more than 512 cells; intensities i * 0.37f and some of large magnitude and both
    signs, so the order of an f32 sum shows; a few non-finite coordinates and intensities"""
    rng = np.random.default_rng(5)
    cells = rng.integers(-40, 40, (700, 3))
    rows = np.concatenate([np.repeat(cells[k:k + 1], rng.integers(1, 6), axis=0) for k in range(len(cells))])[:2000]
    rows = rows[rng.permutation(len(rows))]
    p = ((rows + 0.5) * 0.1 + rng.uniform(-0.03, 0.03, rows.shape)).astype(np.float32)
    inten = (np.arange(len(p), dtype=np.float32) * np.float32(0.37)).astype(np.float32)
    inten[::13] *= np.float32(1e7)
    inten[5::17] *= np.float32(-3e6)
    P = np.concatenate([p, inten[:, None]], axis=1)
    P[3::211, 0] = np.nan
    P[7::307, 2] = np.inf
    P[11::97, 3] = np.nan
    P[19::101, 3] = np.inf
    return P


MOVE = np.array([[0.96, -0.28, 0.0, 0.3], [0.28, 0.96, 0.0, -0.2], [0.0, 0.0, 1.0, 0.05], [0, 0, 0, 1]], np.float32)
CASES = [dict(), dict(leaf=0.25), dict(leaf=0.0), dict(use_distance_filter=False), dict(transform=MOVE), dict(leaf=1e-7),
         dict(downsample_method="APPROX_VOXELGRID"), dict(downsample_method="APPROX_VOXELGRID", transform=MOVE, use_distance_filter=False)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_first_three_columns_are_the_xyz_restatement(cloud, case):
    prm = CASES[case]
    got = X.prefilter(cloud, prm)
    assert got.shape[1] == 4 and got.dtype == np.float32
    assert same_words(got[:, :3], PR.prefilter(cloud[:, :3], prm)), prm


def _dictionary(P, prm):
    """The chain recomputed point by point: a dict of running np.float32 sums per cell (VOXELGRID: ascending cell index, VoxelGrid's own
    index arithmetic; APPROX: the 512-entry table written out independently of the tool)."""
    q = dict(X.DEFAULTS, **prm)
    P = np.array(P, np.float32)
    if q["transform"] is not None:
        P[:, :3] = PR.move(P[:, :3], q["transform"])
    fin = np.isfinite(P[:, :3]).all(axis=1)
    if q["use_distance_filter"]:
        with np.errstate(all="ignore"):
            d = np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2]).astype(np.float64)
        fin &= (d > q["distance_near"]) & (d < q["distance_far"])
    P = P[fin]
    inv = np.float32(1.0) / np.float32(q["leaf"])
    out = []
    with np.errstate(all="ignore"):
        if q["downsample_method"] == "APPROX_VOXELGRID":
            table = {}
            for p in P:
                c = tuple(int(np.floor(np.float32(p[a] * inv))) for a in range(3))
                h = (c[0] * 7171 + c[1] * 3079 + c[2] * 4231) & 511
                if h in table and table[h][0] != c:
                    out.append((len(out), table[h][1] / np.float32(table[h][2])))
                    del table[h]
                e = table.setdefault(h, [c, np.zeros(4, np.float32), 0])
                e[1] = e[1] + p
                e[2] += 1
            for h in sorted(table):
                out.append((len(out), table[h][1] / np.float32(table[h][2])))
            return np.array([v for _, v in out], np.float32).reshape(-1, 4)
        mn = [int(np.floor(np.float32(P[:, a].min() * inv))) for a in range(3)]
        mx = [int(np.floor(np.float32(P[:, a].max() * inv))) for a in range(3)]
        d0, d1 = mx[0] - mn[0] + 1, mx[1] - mn[1] + 1
        cells = {}
        for p in P:
            ijk = [int(np.float32(np.floor(np.float32(p[a] * inv)) - np.float32(mn[a]))) for a in range(3)]
            e = cells.setdefault(ijk[0] + ijk[1] * d0 + ijk[2] * d0 * d1, [np.zeros(4, np.float32), 0])
            e[0] = e[0] + p
            e[1] += 1
        return np.array([cells[k][0] / np.float32(cells[k][1]) for k in sorted(cells)], np.float32).reshape(-1, 4)


@pytest.mark.parametrize("case", [0, 1, 3, 4, 6, 7])
def test_against_a_dictionary_recomputation(cloud, case):
    got, exp = X.prefilter(cloud, CASES[case]), _dictionary(cloud, CASES[case])
    assert len(got) > 100 and same_words(got, exp), CASES[case]
    # the intensities are not a function of the cell alone: the order of the sum shows
    assert len(np.unique(got[np.isfinite(got[:, 3]), 3])) > 50


def test_no_downsampling_keeps_the_points_own_intensity(cloud):
    for prm in (dict(leaf=0.0), dict(leaf=1e-7), dict(leaf=1e-10, downsample_method="APPROX_VOXELGRID")):   # (each too small by its method's rule)
        got = X.prefilter(cloud, prm)
        keep = X.gate_mask(cloud[:, :3], 0.5, 100.0)
        assert same_words(got, cloud[keep]), prm
    assert not np.isfinite(X.prefilter(cloud, leaf=0.0)[:, 3]).all()        # a kept point's non-finite intensity is kept


@pytest.mark.parametrize("method", ["VOXELGRID", "APPROX_VOXELGRID"])
@pytest.mark.parametrize("leaf", [0.1, 0.0])
def test_calibration_zeroes_every_intensity(cloud, method, leaf):
    got = X.prefilter(cloud, angle_calibration=True, downsample_method=method, leaf=leaf)
    assert len(got) > 100
    assert np.array_equal(got[:, 3].view(np.uint32), np.zeros(len(got), np.uint32))     # +0.0f: the sign bit too
    assert same_words(got[:, :3], PR.prefilter(cloud[:, :3], angle_calibration=True, downsample_method=method, leaf=leaf))


def test_outlier_stage_keeps_the_survivors_intensity(cloud):
    base = X.prefilter(cloud, leaf=0.25)
    base = base[:600]
    got, r = X.remove_outliers(base, method="STATISTICAL", mean_k=4, stddev_mul=1.0)
    assert 0 < len(got) < len(base) and same_words(got, base[r["kept"]])
    full = X.prefilter(cloud[:1500], leaf=0.25, outlier=dict(method="RADIUS", radius_m=0.3, min_neighbors=2))
    assert full.shape[1] == 4 and 0 < len(full) < len(X.prefilter(cloud[:1500], leaf=0.25))
    with pytest.raises(ValueError):
        X.prefilter(cloud[:, :3])


# ---- the C ABI, without a device -----------------------------------------------------------------------------------------------------
NEW = ["mi355ndt_prefilter_params_ex2_default", "mi355ndt_batch_get_cloud_i", "mi355ndt_keyframe_from_prefiltered", "mi355ndt_keyframe_from_slot",
       "mi355ndt_window_keyframe_ids"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_struct_layout_matches_header(tmp_path):
    src = tmp_path / "pf2.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "mi355_ndt.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u\\n", sizeof(mi355ndt_prefilter_params), sizeof(mi355ndt_prefilter_params_ex),
         offsetof(mi355ndt_prefilter_params_ex, downsample_method), offsetof(mi355ndt_prefilter_params_ex, use_angle_calibration),
         offsetof(mi355ndt_prefilter_params_ex, angle_calibration_rad), sizeof(mi355ndt_prefilter_params_ex2),
         offsetof(mi355ndt_prefilter_params_ex2, ex), offsetof(mi355ndt_prefilter_params_ex2, intensity_offset_bytes),
         offsetof(mi355ndt_prefilter_params_ex2, reserved), (unsigned)MI355NDT_PREFILTER_EXTENDED2);
  return 0;
}''')
    exe = tmp_path / "pf2"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    E, E2 = ndt.PrefilterParamsEx, ndt.PrefilterParamsEx2
    assert got[:5] == [96, 112, 96, 100, 104]                                  # what they were
    assert got[5:9] == [C.sizeof(E2), E2.ex.offset, E2.intensity_offset_bytes.offset, E2.reserved.offset] == [120, 0, 112, 116]
    assert got[9] == ndt.PREFILTER_EXTENDED2 == 0x50467833
    assert C.sizeof(E) == 112


def test_new_exports_are_declared_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "mi355_ndt.h")).read()
    for s in NEW:
        assert s + "(" in hdr, f"{s} not declared in mi355_ndt.h"
        assert hasattr(lib, s) and s in ndt.SYMBOLS
    for m in ("keyframe_from_prefiltered", "keyframe_from_slot", "window_keyframe_ids"):
        assert callable(getattr(ndt.Engine, m, None)), m


def test_ex2_default(lib):
    p = ndt.PrefilterParamsEx2()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert lib.mi355ndt_prefilter_params_ex2_default(C.byref(p)) == ndt.OK
    assert (p.intensity_offset_bytes, p.reserved, p.ex.base.extended) == (-1, 0, ndt.PREFILTER_EXTENDED2)
    q = ndt.PrefilterParamsEx()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))
    assert lib.mi355ndt_prefilter_params_ex_default(C.byref(q)) == ndt.OK
    q.base.extended = ndt.PREFILTER_EXTENDED2
    assert bytes(p.ex) == bytes(q)                                             # ex's fields are what _ex_default gives
    assert lib.mi355ndt_prefilter_params_ex2_default(None) == BAD_ARG
    # the wrapper's struct: column 3 of the records
    w = ndt._prefilter_params(0.5, 100.0, 0.1, True, None, "APPROX_VOXELGRID", True, intensity=True)
    assert isinstance(w, ndt.PrefilterParamsEx2) and (w.intensity_offset_bytes, w.reserved) == (12, 0)
    assert (w.ex.downsample_method, w.ex.use_angle_calibration, w.ex.base.extended) == (1, 1, ndt.PREFILTER_EXTENDED2)
    x = ndt._prefilter_params(0.5, 100.0, 0.1, True, None)
    assert isinstance(x, ndt.PrefilterParamsEx) and x.base.extended == ndt.PREFILTER_EXTENDED
    for prm in (w, x):                                                          # what the C calls are given: the head of either struct
        assert C.addressof(ndt._base_ref(prm)._obj) == C.addressof(prm)


def test_null_handle_and_null_arguments_are_refused(lib):
    n, kid = C.c_size_t(7), C.c_int(5)
    assert lib.mi355ndt_batch_get_cloud_i(None, 0, 1, None, 0, 16, 12, C.byref(n)) == BAD_HANDLE
    assert lib.mi355ndt_keyframe_from_prefiltered(None, C.byref(kid)) == BAD_HANDLE
    assert lib.mi355ndt_keyframe_from_slot(None, 0, 1, C.byref(kid)) == BAD_HANDLE
    ids = (C.c_int * 1)(0)
    assert lib.mi355ndt_window_keyframe_ids(None, 1, ids, None, 0.1, 0, C.byref(kid), C.byref(n)) == BAD_HANDLE
    assert (n.value, kid.value) == (7, 5)
    x2 = ndt.PrefilterParamsEx2()
    lib.mi355ndt_prefilter_params_ex2_default(C.byref(x2))
    assert lib.mi355ndt_prefilter_p(None, None, 0, 16, C.byref(x2.ex.base), None, 0, 16, C.byref(n)) == BAD_HANDLE


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called the library ({name}) before refusing its arguments")


def test_wrappers_refuse_xyz_records_with_intensity():
    eng = object.__new__(ndt.Engine)
    eng.lib, eng.h = _NoLibrary(), None
    a = np.zeros((10, 3), np.float32)
    for call in (lambda: eng.prefilter_p(a, intensity=True), lambda: eng.prefilter(a, intensity=True), lambda: eng.batch_prefilter([a], None, intensity=True),
                 lambda: eng.sequence_run_raw([a, a], [0.0, 0.1], intensity=True), lambda: eng.window_keyframe_ids([], [])):
        with pytest.raises(ValueError):
            call()


# ---- WindowKeyframer over resident scan ids ------------------------------------------------------------------------------------------
def pose(x):
    P = np.eye(4)
    P[0, 3] = x
    return P


class FakeEngine:
    def __init__(self):
        self.calls, self.released = [], []

    def window_keyframe(self, scans, rel_poses, leaf=0.1, intensity=False):
        self.calls.append(("arrays", list(scans), [np.array(r) for r in rel_poses], leaf, intensity))
        return 1000 + len(self.calls), 1

    def window_keyframe_ids(self, ids, rel_poses, leaf=0.1, intensity=False):
        assert not self.released or not set(ids) & set(self.released)          # no scan is released before its window has closed
        self.calls.append(("ids", list(ids), [np.array(r) for r in rel_poses], leaf, intensity))
        return 1000 + len(self.calls), 1

    def keyframe_release(self, kid):
        assert self.calls and kid in self.calls[-1][1]
        self.released.append(kid)


XS = [0.0, 0.5, 1.5, 2.5, 3.0, 4.4, 4.6, 7.0]                                  # keyframes at 0.0, 2.5, 4.6, 7.0


def test_window_keyframer_over_ids_has_the_same_policy():
    a, b = FakeEngine(), FakeEngine()
    wa = KF.WindowKeyframer(a, 2.0, 0.5, leaf=0.2, intensity=True)
    wb = KF.WindowKeyframer(b, 2.0, 0.5, leaf=0.2, intensity=True)
    outs = []
    for k, x in enumerate(XS):
        ra = wa.push(pose(x), np.full((k + 1, 4), float(k), np.float32), seq=k)
        rb = wb.push(pose(x), 40 + k, seq=k)
        outs.append((ra, rb))
        assert (ra is None) == (rb is None)
        if ra is not None:
            assert (ra.seq, ra.n_scans, ra.accum_distance) == (rb.seq, rb.n_scans, rb.accum_distance) and np.array_equal(ra.odom, rb.odom)
    assert [k for k, (r, _) in enumerate(outs) if r is not None] == [3, 6, 7]
    assert [c[0] for c in a.calls] == ["arrays"] * 3 and [c[0] for c in b.calls] == ["ids"] * 3
    assert [c[1] for c in b.calls] == [[40, 41, 42], [43, 44, 45], [46]]
    for ca, cb in zip(a.calls, b.calls):
        assert [int(s[0, 0]) + 40 for s in ca[1]] == cb[1] and ca[3:] == cb[3:] == (0.2, True)
        assert all(np.array_equal(x, y) for x, y in zip(ca[2], cb[2]))
    assert b.released == [40, 41, 42, 43, 44, 45, 46] and a.released == []      # released after their window closed, the open window's kept
    last = wb.flush()
    assert last is not None and b.calls[-1][1] == [47] and b.released[-1] == 47


def test_an_id_twice_in_a_window_is_released_once():
    e = FakeEngine()
    w = KF.WindowKeyframer(e, 2.0, 0.5)
    w.push(pose(0.0), 5)
    w.push(pose(0.1), 5)
    w.push(pose(0.2), np.int32(6))
    w.flush()
    assert e.calls[0][1] == [5, 5, 6] and e.released == [5, 6]


def test_a_mixed_window_raises():
    e = FakeEngine()
    w = KF.WindowKeyframer(e, 2.0, 0.5)
    w.push(pose(0.0), 5)
    with pytest.raises(ValueError):
        w.push(pose(0.1), np.zeros((3, 3), np.float32))
    w2 = KF.WindowKeyframer(e, 2.0, 0.5)
    w2.push(pose(0.0), np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        w2.push(pose(0.1), 7)
    assert e.calls == []
    w2.push(pose(5.0), 7)                                                       # a new window may be of the other kind
    assert e.calls[-1][0] == "arrays"
