"""CPU: the restatement the prefilter's APPROX_VOXELGRID and vertical-angle calibration are held to (tools/prefilter_options_ref.py) against
hand-worked cases, an independent formulation and mpmath, and the parts of the new C ABI and of the wrappers that need no device."""
import ctypes as C
import importlib.util
import math
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


R = _load("prefilter_options_ref")
LEAF = 0.25


def at(cell, jitter=(0.0, 0.0, 0.0)):
    """a point in `cell` of the 0.25 m lattice: the cell's centre plus a jitter below 0.05, so no product sits on a cell edge"""
    return (np.asarray(cell, np.float64) + 0.5) * LEAF + np.asarray(jitter, np.float64)


# ---- the approximate voxel grid -------------------------------------------------------------------------
def test_multipliers_mod_512():
    assert [m % 512 for m in R.MULTIPLIERS] == [3, 7, 135] and R.HISTSIZE == 512


def test_a_hand_worked_collision_sequence():
    A = np.array([40, 8, 2])
    B, Cc = A + (7, -3, 0), A + (0, 0, 512)                    # 7 * 3 - 3 * 7 = 0 and 512 * 135 = 0 (mod 512): one bucket
    a1, b1, a2, a3, c1 = at(A, (0.01, 0, 0)), at(B), at(A, (-0.03, 0.02, 0)), at(A, (0.04, 0.04, -0.04)), at(Cc)
    pts = np.array([a1, b1, a2, a3, c1], np.float32)
    f, _ = R.cells(pts, LEAF)
    assert f.astype(int).tolist() == [A.tolist(), B.tolist(), A.tolist(), A.tolist(), Cc.tolist()]
    # A B A A C: the runs A | B | A A | C -- B flushes A, the second A flushes B, C flushes the pair, the final flush emits C
    out = R.approx_voxel_grid(pts, LEAF)
    want = np.array([pts[0], pts[1], (pts[2] + pts[3]) / np.float32(2), pts[4]], np.float32)
    assert out.tobytes() == want.tobytes()
    # the same cells without a collision in between: one centroid per cell, in table order
    apart = np.array([a1, a2, a3, at(A + (1, 0, 0))], np.float32)
    out = R.approx_voxel_grid(apart, LEAF)
    assert out.tobytes() == np.array([((apart[0] + apart[1]) + apart[2]) / np.float32(3), apart[3]], np.float32).tobytes()


def test_final_flush_is_in_table_order():
    A = np.array([40, 8, 2])
    cells = [A + (2, 0, 0), A + (0, 0, 0), A + (1, 0, 0)]      # buckets h + 6, h, h + 3
    pts = np.array([at(c) for c in cells], np.float32)
    h = [(int(c[0]) * 7171 + int(c[1]) * 3079 + int(c[2]) * 4231) & 511 for c in cells]
    assert len(set(h)) == 3
    assert R.approx_voxel_grid(pts, LEAF).tobytes() == pts[np.argsort(h)].tobytes()


def test_empty_single_and_non_finite():
    assert R.approx_voxel_grid(np.zeros((0, 3), np.float32), LEAF).shape == (0, 3)
    one = np.float32([[3.0, 4.0, 0.5]])
    assert R.approx_voxel_grid(one, LEAF).tobytes() == one.tobytes()
    holes = np.float32([[1, 2, 3], [np.nan, 0, 0], [1, 2, 3], [0, np.inf, 0]])
    assert R.approx_voxel_grid(holes, LEAF).tobytes() == np.float32([[1, 2, 3]]).tobytes()
    assert R.prefilter(holes, leaf=LEAF, use_distance_filter=False, downsample_method="APPROX_VOXELGRID").tolist() == [[1, 2, 3]]


def test_cell_indices_beyond_int_leave_the_cloud_as_it_is():
    p = np.float32([[90.0, 0.1, 0.2], [0.3, 0.2, 0.1], [0.3, 0.2, 0.1]])
    assert R.cells_overflow(p, 1e-9) and not R.cells_overflow(p[1:], 1e-9)
    assert R.approx_voxel_grid(p, 1e-9).tobytes() == p.tobytes()
    assert len(R.approx_voxel_grid(p[1:], 1e-9)) == 1


def _vectorised(xyz, leaf):
    """the parallel form: stable argsort by bucket, run heads, one scan over the triggers in input order, one over the buckets' last runs"""
    p = np.asarray(xyz, np.float32)
    p = p[np.isfinite(p).all(axis=1)]
    n = len(p)
    if n == 0:
        return p
    inv = np.float32(1.0) / np.float32(leaf)
    idx = np.floor(p * inv).astype(np.int64)
    bucket = (idx[:, 0] * 7171 + idx[:, 1] * 3079 + idx[:, 2] * 4231) & 511
    order = np.argsort(bucket, kind="stable")
    sb, sc = bucket[order], idx[order]
    head = np.ones(n, bool)
    head[1:] = (sb[1:] != sb[:-1]) | (sc[1:] != sc[:-1]).any(axis=1)
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    last = np.ones(len(starts), bool)
    last[:-1] = sb[starts[1:]] != sb[starts[:-1]]
    trig = np.zeros(n, np.int64)
    trig[order[ends[~last]]] = 1                               # the point that opens the next run of the bucket, by its input index
    tpos = np.cumsum(trig) - trig
    rank = np.empty(len(starts), np.int64)
    rank[~last] = tpos[order[ends[~last]]]
    rank[last] = trig.sum() + (np.cumsum(last) - last)[last]
    out = np.zeros((len(starts), 3), np.float32)
    for r, (s, e) in enumerate(zip(starts, ends)):
        run = np.vstack([np.zeros((1, 3), np.float32), p[order[s:e]]])
        out[rank[r]] = np.add.accumulate(run, axis=0, dtype=np.float32)[-1] / np.float32(e - s)
    return out


def test_restatement_equals_the_parallel_form():
    rng = np.random.default_rng(11)
    for scale, leaf, n in ((3.0, 0.25, 3000), (40.0, 0.5, 5000), (0.6, 0.1, 2500)):
        p = rng.normal(0, scale, (n, 3)).astype(np.float32)
        p[rng.integers(0, n, n // 3)] = p[rng.integers(0, n, n // 3)]          # repeated points: revisits of a cell far apart in the input
        p[::7] = p[0] + rng.uniform(0, leaf / 4, (len(p[::7]), 3)).astype(np.float32)
        p[5] = np.nan
        a, b = R.approx_voxel_grid(p, leaf), _vectorised(p, leaf)
        assert a.tobytes() == b.tobytes() and 0 < len(a) < n
        assert len(a) > len(np.unique(np.floor(p[np.isfinite(p).all(axis=1)] * (np.float32(1) / np.float32(leaf))), axis=0))   # some cell came out twice
    forced = np.array([at(c) for c in ([40, 8, 2], [47, 5, 2], [40, 8, 2], [40, 8, 2], [47, 5, 2])] * 3, np.float32)           # A B A A B ...
    assert R.approx_voxel_grid(forced, LEAF).tobytes() == _vectorised(forced, LEAF).tobytes()
    assert len(R.approx_voxel_grid(forced, LEAF)) == 12


# ---- the calibration ---------------------------------------------------------------------------------------
def test_calibration_against_mpmath():
    import mpmath as mp
    mp.mp.dps = 50
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.uniform(-60, 60, (200, 2)), rng.uniform(-6, 6, (200, 1))], axis=1).astype(np.float32)
    got = R.angle_calibration(p, R.ANGLE_RAD)
    d = mp.mpf(0.11) * mp.pi / 180
    worst = 0.0
    for row, out in zip(p, got):
        x, y, z = (mp.mpf(float(v)) for v in row)
        nrm = mp.sqrt(x * x + y * y)
        a = (y / nrm, -x / nrm, mp.mpf(0))                     # p x (0,0,1), normalised
        c, s = mp.cos(d), mp.sin(d)
        dot = a[0] * x + a[1] * y
        cross = (a[1] * z - a[2] * y, a[2] * x - a[0] * z, a[0] * y - a[1] * x)
        exact = [c * v + s * cr + (1 - c) * dot * ax for v, cr, ax in zip((x, y, z), cross, a)]          # Rodrigues
        for e, g in zip(exact, out):
            ulp = float(np.spacing(np.float32(abs(float(e)))))
            worst = max(worst, abs(float(mp.mpf(float(g)) - e)) / ulp)
    print("calibration: worst error", worst, "ulp of f32")
    assert worst <= 2.0
    assert not np.array_equal(got, p)
    # the angle the nodelet hard-codes
    assert R.ANGLE_RAD == 0.11 * math.pi / 180 == ndt.ANGLE_CALIBRATION_RAD


def test_calibration_special_rows():
    c = math.cos(R.ANGLE_RAD)
    p = np.float32([[0, 0, 7.5], [0, 0, -2.25], [0, 0, 0], [np.nan, 1, 2], [1, np.inf, 2], [3, -4, 0]])
    got = R.angle_calibration(p)
    assert got[0].tolist() == [0.0, 0.0, float(np.float32(c * 7.5))]           # on the z axis: a zero axis, the point scaled by cos
    assert got[1].tolist() == [0.0, 0.0, float(np.float32(c * -2.25))]
    assert got[2].tolist() == [0.0, 0.0, 0.0]
    assert got[3:5].tobytes() == p[3:5].tobytes()                              # non-finite rows stay as they are
    # a horizontal point is lifted by the angle: z = |p| sin(delta), to f32
    assert abs(float(got[5, 2]) - 5.0 * math.sin(R.ANGLE_RAD)) < 1e-9 and abs(float(np.hypot(got[5, 0], got[5, 1])) - 5.0 * c) < 1e-6
    assert R.angle_calibration(np.zeros((0, 3), np.float32)).shape == (0, 3)


def test_chain_order_and_the_oracle_routes():
    from oracle import oracle_py as O
    rng = np.random.default_rng(3)
    p = rng.uniform(-20, 20, (500, 3)).astype(np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [1.5, -0.5, 2.0]
    moved = R.move(p, T)
    assert np.array_equal(moved, p + T[:3, 3])
    cal = R.angle_calibration(moved)
    assert R.prefilter(p, transform=T, angle_calibration=True, leaf=0.5).tobytes() == O.prefilter(cal, 0.5, 100.0, 0.5, True).tobytes()
    assert R.prefilter(p, dict(leaf=0.0, use_distance_filter=False), angle_calibration=R.ANGLE_RAD).tobytes() == R.angle_calibration(p).tobytes()
    assert R.prefilter(p, transform=T, angle_calibration=True, leaf=0.5, downsample_method="APPROX_VOXELGRID").tobytes() == \
        R.approx_voxel_grid(R.gate(cal, 0.5, 100.0), 0.5).tobytes()
    with pytest.raises(ValueError):
        R.prefilter(p, downsample_method="NONE")
    with pytest.raises(ValueError):
        R.prefilter(p, resolution=0.1)


# ---- the C ABI and the wrappers, without a device --------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(ndt.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return ndt.load_library()


def test_defaults_fill_the_new_fields(lib):
    p = ndt.PrefilterParamsEx()
    C.memset(C.byref(p), 0xFF, C.sizeof(p))
    assert lib.mi355ndt_prefilter_params_ex_default(C.byref(p)) == ndt.OK
    assert p.downsample_method == ndt.DOWNSAMPLE_VOXELGRID == 0 and p.use_angle_calibration == 0
    assert p.angle_calibration_rad == 0.11 * math.pi / 180
    assert p.base.extended == ndt.PREFILTER_EXTENDED
    # the base is what mi355ndt_prefilter_params_default gives, but for the word that announces the extension
    q = ndt.PrefilterParams()
    C.memset(C.byref(q), 0xFF, C.sizeof(q))
    assert lib.mi355ndt_prefilter_params_default(C.byref(q)) == ndt.OK and q.extended == 0
    q.extended = ndt.PREFILTER_EXTENDED
    assert bytes(p.base) == bytes(q)
    assert lib.mi355ndt_prefilter_params_ex_default(None) == -2
    assert ndt.DOWNSAMPLE_APPROX_VOXELGRID == 1
    for name in ("mi355ndt_prefilter_p", "mi355ndt_prefilter_params_ex_default"):
        assert hasattr(lib, name) and name in ndt.SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mi355_ndt.h")).read()
    for s in ("MI355NDT_DOWNSAMPLE_VOXELGRID = 0", "MI355NDT_DOWNSAMPLE_APPROX_VOXELGRID = 1", "MI355NDT_PREFILTER_EXTENDED 0x%08X" % ndt.PREFILTER_EXTENDED):
        assert s in hdr


def test_struct_layout_matches_header(tmp_path):
    """the new fields live in mi355ndt_prefilter_params_ex; mi355ndt_prefilter_params keeps its size, `extended` lies in its former padding"""
    src = tmp_path / "pf.c"
    src.write_text('''
#include <stdio.h>
#include <stddef.h>
#include "mi355_ndt.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mi355ndt_prefilter_params), offsetof(mi355ndt_prefilter_params, extended),
         offsetof(mi355ndt_prefilter_params, distance_near), offsetof(mi355ndt_prefilter_params, transform_colmajor),
         sizeof(mi355ndt_prefilter_params_ex), offsetof(mi355ndt_prefilter_params_ex, downsample_method),
         offsetof(mi355ndt_prefilter_params_ex, use_angle_calibration), offsetof(mi355ndt_prefilter_params_ex, angle_calibration_rad));
  return 0;
}''')
    exe = tmp_path / "pf"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    P, X = ndt.PrefilterParams, ndt.PrefilterParamsEx
    assert got == [C.sizeof(P), P.extended.offset, P.distance_near.offset, P.transform_colmajor.offset,
                   C.sizeof(X), X.downsample_method.offset, X.use_angle_calibration.offset, X.angle_calibration_rad.offset]
    assert got[:4] == [96, 4, 8, 32] and got[4:] == [112, 96, 100, 104] and X.base.offset == 0


def test_null_handle_is_refused(lib):
    n = C.c_size_t(99)
    assert lib.mi355ndt_prefilter_p(None, None, 0, 12, None, None, 0, 12, C.byref(n)) == -1
    assert n.value == 99


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called the library ({name}) before refusing its arguments")


def test_wrappers_refuse_before_calling_the_library():
    eng = object.__new__(ndt.Engine)            # no mi355ndt_create: the checks below must not reach the library
    eng.lib, eng.h = _NoLibrary(), None
    a = np.zeros((10, 3), np.float32)
    for bad in (dict(downsample_method="NONE"), dict(downsample_method="approx"), dict(downsample_method=1), dict(angle_calibration=float("nan")),
                dict(angle_calibration=float("inf"))):
        with pytest.raises(ValueError):
            eng.batch_prefilter([a], None, **bad)
        with pytest.raises(ValueError):
            eng.sequence_run_raw([a, a], [0.0, 0.1], **bad)
        with pytest.raises(ValueError):
            eng.prefilter_p(a, **bad)
    p = ndt._prefilter_params(0.5, 100.0, 0.1, True, None, "APPROX_VOXELGRID", True)
    assert (p.downsample_method, p.use_angle_calibration, p.angle_calibration_rad) == (1, 1, ndt.ANGLE_CALIBRATION_RAD)
    p = ndt._prefilter_params(0.5, 100.0, 0.1, True, None, "VOXELGRID", 0.002)
    assert (p.downsample_method, p.use_angle_calibration, p.angle_calibration_rad) == (0, 1, 0.002)
    p = ndt._prefilter_params(0.5, 100.0, 0.1, True, None)
    assert (p.downsample_method, p.use_angle_calibration, p.base.extended) == (0, 0, ndt.PREFILTER_EXTENDED)
