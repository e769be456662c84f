"""GPU (-m gpu): the fourth channel of pcl::PointXYZI through the device prefilter -- mi355ndt_prefilter_p, mi355ndt_batch_prefilter,
mi355ndt_prefilter_outliers, mi355ndt_batch_remove_outliers, mi355ndt_sequence_run_raw with a mi355ndt_prefilter_params_ex2 -- against
tools/prefilter_xyzi_ref.py.  Every comparison is word for word (same_words: uint32 views), count and order included.  No tolerances.

One fixture of five raw [N,4] clouds:
  0  about 3,000 points on the 0.1 m lattice: 600 cells of 1..4 points and 18 of 50..130, shuffled -- more than 512 distinct cells with repeats
     (APPROX_VOXELGRID flushes entries mid-cloud and at the end), one voxel run longer than a wave, runs across the emit kernels' 256-lane
     tile edges, some cells inside distance_near
  1  40 points: less than one wave
  2  empty
  3  1,500 points with NaN / +-Inf coordinates and NaN / +Inf intensities sprinkled in
  4  301 points whose extent makes the leaf too small once the gate is off (a 300 m cube; one point at 3e8 m, which is APPROX's rule)
Intensities are i * 0.37f, some scaled by 1e7 and by -3e6: the order of an f32 sum shows in its words.  The non-finite intensities are NaN
and +Inf only: Inf - Inf makes a NEW NaN, and the sign x86 (the restatement) and gfx950 give a generated NaN differs by hardware convention --
no rule of PCL's is behind either word.

Not asserted: that a row's tail behind the new count is zero after the outlier removals.  No entry point reads past a cloud's count."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
BAD_ARG = -2
LEAF = 0.1


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(name, m)
    spec.loader.exec_module(m)
    return m


X = _load("prefilter_xyzi_ref")


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _intensity(n, rng):
    w = (np.arange(n, dtype=np.float32) * np.float32(0.37)).astype(np.float32)
    w[::13] *= np.float32(1e7)
    w[5::17] *= np.float32(-3e6)
    return w[rng.permutation(n)]


_CLOUDS, _REF = None, {}


def clouds():
    global _CLOUDS
    if _CLOUDS is None:
        rng = np.random.default_rng(2024)
        cells = np.unique(rng.integers(-30, 30, (700, 3)), axis=0)
        cells = cells[rng.permutation(len(cells))][:618]
        per = np.concatenate([rng.integers(1, 5, 600), [130, 120, 110, 100, 97, 90, 85, 80, 77, 70, 66, 65, 64, 63, 60, 55, 51, 50]])
        rows = np.repeat(cells, per, axis=0)
        rows = rows[rng.permutation(len(rows))]
        p0 = ((rows + 0.5) * 0.1 + rng.uniform(-0.03, 0.03, rows.shape)).astype(np.float32)
        c0 = np.concatenate([p0, _intensity(len(p0), rng)[:, None]], axis=1)
        c1 = np.concatenate([rng.uniform(-3, 3, (40, 3)).astype(np.float32), _intensity(40, rng)[:, None]], axis=1)
        c2 = np.zeros((0, 4), np.float32)
        c3 = np.concatenate([(rng.integers(-25, 25, (1500, 3)) * 0.1 + rng.uniform(0.01, 0.09, (1500, 3))).astype(np.float32),
                             _intensity(1500, rng)[:, None]], axis=1)
        for bad, col in ((np.nan, 0), (np.inf, 1), (-np.inf, 2), (np.nan, 2)):
            c3[rng.choice(1500, 40, replace=False), col] = bad
        c3[rng.choice(1500, 80, replace=False), 3] = np.nan
        c3[rng.choice(1500, 80, replace=False), 3] = np.inf
        c4 = np.concatenate([rng.uniform(-150, 150, (301, 3)).astype(np.float32), _intensity(301, rng)[:, None]], axis=1)
        c4[150, :3] = (3e8, 0.0, 0.0)
        _CLOUDS = [np.ascontiguousarray(c, np.float32) for c in (c0, c1, c2, c3, c4)]
        for c in _CLOUDS:
            c.setflags(write=False)
        assert 2900 < len(c0) < 3200 and len(np.unique(rows, axis=0)) > 512
    return _CLOUDS


MOVE = np.array([[0.96, -0.28, 0.0, 0.3], [0.28, 0.96, 0.0, -0.2], [0.0, 0.0, 1.0, 0.05], [0, 0, 0, 1]], np.float32)
CASES = {}
for _m, _leaf in (("VOXELGRID", LEAF), ("APPROX_VOXELGRID", LEAF), ("NONE", 0.0)):
    for _mv in (False, True):
        for _gate in (True, False):
            CASES[f"{_m}-{'move' if _mv else 'still'}-{'gate' if _gate else 'nogate'}"] = dict(
                downsample_method="VOXELGRID" if _m == "NONE" else _m, leaf=_leaf, transform=MOVE if _mv else None, use_distance_filter=_gate)
    CASES[f"{_m}-calibrated"] = dict(downsample_method="VOXELGRID" if _m == "NONE" else _m, leaf=_leaf, angle_calibration=True)
PLAIN = "VOXELGRID-still-gate"


def reference(k, case):
    """the restatement's answer for cloud k under a case; computed once, shared and left unchanged"""
    if (k, case) not in _REF:
        out = X.prefilter(clouds()[k], CASES[case])
        out.setflags(write=False)
        _REF[(k, case)] = out
    return _REF[(k, case)]


def kw_of(case):
    q = dict(CASES[case])
    q["downsample_resolution"] = q.pop("leaf")
    return q


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(**PRM))
    yield e
    e.close()


@pytest.mark.parametrize("case", list(CASES))
def test_prefilter_p_word_for_word(eng, case):
    """cases 1 and 2: [M,4] equals the restatement; its first three columns equal the call without the keyword"""
    for k, c in enumerate(clouds()):
        got = eng.prefilter_p(c, intensity=True, **kw_of(case))
        exp = reference(k, case)
        print(f"{case} cloud {k}: raw {len(c)} filtered {len(got)} expected {len(exp)}")
        assert got.shape == exp.shape, (case, k, got.shape, exp.shape)
        assert same_words(got, exp), (case, k, int((got.view(np.uint32) != exp.view(np.uint32)).any(axis=1).sum()))
        assert eng.prefilter_p(c, intensity=True, fetch=False, **kw_of(case)) == len(exp)
        xyz = eng.prefilter_p(c, **kw_of(case))
        assert xyz.shape == (len(exp), 3) and same_words(xyz, got[:, :3]), (case, k)
        assert same_words(xyz, eng.prefilter_p(c[:, :3], **kw_of(case))), (case, k)
        if "calibrated" in case:
            assert not got[:, 3].view(np.uint32).any()                       # +0.0f, the sign bit too
    # the edge cases occur
    big = reference(0, case)
    if case == PLAIN:
        assert len(big) <= 618 and not np.isfinite(reference(3, case)[:, 3]).all()
    if case == "VOXELGRID-still-nogate":
        assert len(big) == 618 and len(reference(4, case)) == 301               # the leaf is too small for cloud 4: it comes back whole
    if case == "APPROX_VOXELGRID-still-nogate":
        assert len(big) > 618 and len(reference(4, case)) == 301                # cells come out more than once; cloud 4: some index past 2^31


def test_equals_the_window_keyframe_of_one_scan(eng):
    """case 3: the two device paths agree"""
    for k, c in enumerate(clouds()):
        got = eng.prefilter_p(c, downsample_resolution=LEAF, use_distance_filter=False, intensity=True)
        kid, n = eng.window_keyframe([c], [np.eye(4)], LEAF, intensity=True)
        kf = eng.keyframe_get(kid, intensity=True)
        eng.keyframe_release(kid)
        assert n == len(got) and same_words(got, kf), k


SLOT_CAP = 3200


@pytest.fixture(scope="module")
def batch():
    """case 4's engine: five slots, every cloud on both sides (the sources in reverse order), groups of two raw clouds: five groups"""
    e = ndt.Engine(ndt.default_params(**PRM))
    e.set_option(ndt.OPT_PREFILTER_GROUP, 2)
    e.batch_reserve(5, SLOT_CAP, SLOT_CAP)
    cl = clouds()
    counts = e.batch_prefilter(cl, cl[::-1], intensity=True, **kw_of(PLAIN))
    yield e, counts
    e.close()


def test_batch_slots_word_for_word(batch):
    e, (tc, sc) = batch
    single = ndt.Engine(ndt.default_params(**PRM))
    for k in range(5):
        for tgt, src_k, cnt in ((True, k, tc[k]), (False, 4 - k, sc[k])):
            exp = reference(src_k, PLAIN)
            got = e.batch_get_cloud(k, tgt, intensity=True)
            assert cnt == len(exp) and got.shape == exp.shape and same_words(got, exp), (k, tgt)
            assert same_words(got, single.prefilter_p(clouds()[src_k], intensity=True, **kw_of(PLAIN)))
            # case 6: without the keyword, [M,3] with today's words
            xyz = e.batch_get_cloud(k, tgt)
            assert xyz.shape == (len(exp), 3) and same_words(xyz, exp[:, :3])
    # ... "today's words": the same call without the keyword on a fresh batch
    single.set_option(ndt.OPT_PREFILTER_GROUP, 2)
    single.batch_reserve(5, SLOT_CAP, SLOT_CAP)
    single.batch_prefilter([c[:, :3] for c in clouds()], None, **kw_of(PLAIN))
    for k in range(5):
        assert same_words(single.batch_get_cloud(k, True), e.batch_get_cloud(k, True))
        z = single.batch_get_cloud(k, True, intensity=True)                    # a slot without intensity reads zeros
        assert z.shape[1] == 4 and not z[:, 3].view(np.uint32).any()
    single.close()


@pytest.mark.parametrize("case", ["APPROX_VOXELGRID-move-nogate", "NONE-still-gate", "VOXELGRID-calibrated", "APPROX_VOXELGRID-calibrated"])
def test_batch_other_chains(case):
    e = ndt.Engine(ndt.default_params(**PRM))
    e.set_option(ndt.OPT_PREFILTER_GROUP, 2)
    e.batch_reserve(5, SLOT_CAP, 64)
    tc, _ = e.batch_prefilter(clouds(), None, intensity=True, **kw_of(case))
    for k in range(5):
        exp = reference(k, case)
        assert tc[k] == len(exp) and same_words(e.batch_get_cloud(k, True, intensity=True), exp), (case, k)
    e.close()


def test_refilled_slot_reads_zeros(batch):
    """case 5 (after case 4's reads: it changes slots 1 and 2)"""
    e, _ = batch
    raw = clouds()[1]
    e.batch_set_target(1, raw)
    e.batch_set_source(2, raw[:, :3])
    kid = e.keyframe_add(raw[:7], intensity=True)
    e.batch_set_source_keyframe(1, kid)
    e.keyframe_release(kid)
    for got, n in ((e.batch_get_cloud(1, True, intensity=True), 40), (e.batch_get_cloud(2, False, intensity=True), 40),
                   (e.batch_get_cloud(1, False, intensity=True), 7)):
        assert got.shape == (n, 4) and same_words(got[:, :3], raw[:n, :3]) and not got[:, 3].view(np.uint32).any()
    assert same_words(e.batch_get_cloud(0, True, intensity=True), reference(0, PLAIN))      # the other slots keep theirs
    # a prefilter without the keyword over a slot clears it as well
    e.batch_prefilter([clouds()[0]], None, first_pair=0, **kw_of(PLAIN))
    got = e.batch_get_cloud(0, True, intensity=True)
    assert same_words(got[:, :3], reference(0, PLAIN)[:, :3]) and not got[:, 3].view(np.uint32).any()


def test_overflowing_slot_fails_and_leaves_no_intensity():
    """case 7"""
    e = ndt.Engine(ndt.default_params(**PRM))
    e.batch_reserve(2, 256, 256)
    with pytest.raises(ndt.NDTError) as ex:
        e.batch_prefilter([clouds()[1], clouds()[0]], None, intensity=True, **kw_of(PLAIN))
    assert ex.value.code == BAD_ARG and "slot 1" in str(ex.value) and "more than its slot holds" in str(ex.value)
    for k in range(2):
        assert e.batch_get_cloud(k, True, intensity=True).shape == (0, 4)      # every touched slot is recorded as empty
    e.batch_set_target(0, clouds()[1])
    assert not e.batch_get_cloud(0, True, intensity=True)[:, 3].view(np.uint32).any()
    e.close()


def planted():
    """cloud 0's filtered points plus planted outliers far from everything, with intensities of their own"""
    rng = np.random.default_rng(9)
    base = reference(0, "NONE-still-gate")[:1200]
    far = np.concatenate([rng.uniform(20, 60, (25, 3)).astype(np.float32), (1000 + np.arange(25, dtype=np.float32))[:, None]], axis=1)
    out = np.concatenate([base, far])
    return np.ascontiguousarray(out[rng.permutation(len(out))])


OUTLIER = [dict(method="STATISTICAL", mean_k=4, stddev_mul=1.0), dict(method="RADIUS", radius=0.25, min_neighbors=3)]


def _ref_outliers(P, o):
    o = dict(o)
    if "radius" in o:
        o["radius_m"] = o.pop("radius")
    return X.remove_outliers(P, **o)[0]


@pytest.mark.parametrize("o", OUTLIER, ids=["statistical", "radius"])
def test_prefilter_outliers_keep_the_survivors_intensity(eng, o):
    """case 8"""
    for P in (planted(), np.ascontiguousarray(clouds()[3])):
        n = eng.prefilter_p(P, downsample_resolution=0.0, use_distance_filter=False, intensity=True, fetch=False)
        pre = X.prefilter(P, leaf=0.0, use_distance_filter=False)
        assert n == len(pre)
        got = eng.prefilter_outliers(intensity=True, **o)
        exp = _ref_outliers(pre, o)
        print(f"{o['method']}: {len(pre)} -> {len(got)} (expected {len(exp)})")
        assert 0 < len(exp) < len(pre) and got.shape == exp.shape and same_words(got, exp)
        assert same_words(eng.prefilter(P, downsample_resolution=0.0, use_distance_filter=False, outlier=o, intensity=True), exp)
        # over a resident result with an intensity row, the call without the keyword gives [M,3] -- and the library's own refusal has a text
        eng.prefilter_p(P, downsample_resolution=0.0, use_distance_filter=False, intensity=True, fetch=False)
        n3 = C.c_size_t()
        op = ndt._outlier_params(**o)
        buf = np.zeros((len(pre), 3), np.float32)
        assert eng.lib.mi355ndt_prefilter_outliers(eng.h, C.byref(op), None, buf.ctypes.data_as(C.c_void_p), len(pre), 12, C.byref(n3), None) == BAD_ARG
        assert b"cannot hold it" in eng.lib.mi355ndt_last_error(eng.h)
        assert same_words(eng.prefilter_outliers(**o), exp[:, :3])
        # x, y, z are what the xyz-only surface gives
        assert same_words(eng.prefilter(P[:, :3], downsample_resolution=0.0, use_distance_filter=False, outlier=o), exp[:, :3])


@pytest.mark.parametrize("o", OUTLIER, ids=["statistical", "radius"])
def test_batch_remove_outliers_compacts_the_intensity_rows(o):
    """case 9: both sides of three slots; one slot side is refilled without intensity first and reads zeros afterwards"""
    e = ndt.Engine(ndt.default_params(**PRM))
    e.set_option(ndt.OPT_PREFILTER_GROUP, 2)
    e.batch_reserve(3, 1600, 1600)
    raws = [planted(), np.ascontiguousarray(clouds()[3]), np.ascontiguousarray(clouds()[1])]
    kw = dict(downsample_resolution=0.0, use_distance_filter=False)
    e.batch_prefilter(raws, raws[::-1], intensity=True, **kw)
    e.batch_set_source(1, raws[1][:, :3])                                       # (source 1 held raws[1] with intensity)
    tc, sc = e.batch_remove_outliers(**o)
    for k in range(3):
        for tgt, P, cnt in ((True, raws[k], tc[k]), (False, raws[2 - k], sc[k])):
            exp = _ref_outliers(X.prefilter(P, leaf=0.0, use_distance_filter=False) if (tgt or k != 1) else P, o)
            got = e.batch_get_cloud(k, tgt, intensity=True)
            assert cnt == len(exp) and got.shape == exp.shape and same_words(got[:, :3], exp[:, :3]), (k, tgt)
            if tgt or k != 1:
                assert same_words(got, exp), (k, tgt)
            else:
                assert not got[:, 3].view(np.uint32).any()
    e.close()


def test_sequence_run_raw_frames_are_unchanged_and_slots_carry_intensity():
    """case 10: four of the smallest synthetic frames tests/test_sequence.py uses"""
    scans, _ = synth.make_sequence(4, 256, n_beams=32)
    rng = np.random.default_rng(4)
    recs = [np.ascontiguousarray(np.concatenate([s.numpy().astype(np.float32), _intensity(len(s), rng)[:, None]], axis=1)) for s in scans]
    stamps = [0.1 * k for k in range(4)]
    prm = ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=3, variant=1)
    kw = dict(keyframe_delta_trans=2.5, downsample_resolution=0.25, raw_records=True)
    a, b = ndt.Engine(prm), ndt.Engine(prm)
    (fa, ra), _, ca = a.sequence_run_raw([r[:, :3] for r in recs], stamps, **kw)
    (fb, rb), _, cb = b.sequence_run_raw(recs, stamps, intensity=True, **kw)
    assert ca == cb and bytes(fa) == bytes(fb) and bytes(ra) == bytes(rb)
    for k in range(4):
        exp = X.prefilter(recs[k], leaf=0.25)
        assert cb[k] == len(exp) and same_words(b.batch_get_cloud(k, True, intensity=True), exp), k
        assert not a.batch_get_cloud(k, True, intensity=True)[:, 3].view(np.uint32).any()
    a.close()
    b.close()


def test_bad_offsets_are_refused_and_change_nothing(batch, eng):
    """case 11"""
    e, _ = batch
    cl = np.ascontiguousarray(clouds()[1])
    rec20 = np.zeros((40, 5), np.float32)
    rec20[:, :4] = cl
    eng.prefilter_p(cl, intensity=True, **kw_of(PLAIN))
    kid = eng.keyframe_from_prefiltered()
    resident = eng.keyframe_get(kid, intensity=True)
    eng.keyframe_release(kid)
    before = [e.batch_get_cloud(k, t, intensity=True).tobytes() for k in range(5) for t in (True, False)]
    out, n = np.zeros((40, 5), np.float32), C.c_size_t()
    ptrs, cnts = np.array([rec20.ctypes.data], np.uint64), np.array([40], np.uint64)

    def params(off, reserved=0):
        x = ndt.PrefilterParamsEx2()
        assert eng.lib.mi355ndt_prefilter_params_ex2_default(C.byref(x)) == 0
        x.ex.base.distance_near = 0.5
        x.intensity_offset_bytes, x.reserved = off, reserved
        return x

    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for off, reserved, stride, out_stride in ((16, 0, 16, 20), (20, 0, 20, 20), (8, 0, 20, 20), (0, 0, 20, 20), (13, 0, 20, 20), (12, 1, 20, 20),
                                               (16, 0, 20, 16)):
        x = params(off, reserved)
        rc = eng.lib.mi355ndt_prefilter_p(eng.h, vp(rec20), 40, stride, C.byref(x.ex.base), vp(out), 40, out_stride, C.byref(n))
        assert rc == BAD_ARG, (off, reserved, stride, out_stride)
        if out_stride == 20:                                                    # (the out stride is the single-cloud surface's argument)
            rc = e.lib.mi355ndt_batch_prefilter(e.h, 0, 1, vp(ptrs), vp(cnts), None, None, stride, C.byref(x.ex.base), None, None)
            assert rc == BAD_ARG, (off, reserved, stride)
    # the accepted forms: offset 16 of 20-byte records, in and out; -1 is "no intensity"
    x = params(16)
    rec20[:, 4] = cl[:, 3]
    assert eng.lib.mi355ndt_prefilter_p(eng.h, vp(rec20), 40, 20, C.byref(x.ex.base), vp(out), 40, 20, C.byref(n)) == 0
    exp = reference(1, PLAIN)
    assert n.value == len(exp) and same_words(out[: n.value, :3], exp[:, :3]) and same_words(out[: n.value, 4], exp[:, 3])
    # prefilter_outliers writes the row at the same offset and refuses an out stride that cannot hold it
    op = ndt.OutlierParams(ndt.OUTLIER_RADIUS, 20, 1.0, 10.0, 0)
    assert eng.lib.mi355ndt_prefilter_outliers(eng.h, C.byref(op), None, vp(out), 40, 16, C.byref(n), None) == BAD_ARG
    out[:] = 0
    assert eng.lib.mi355ndt_prefilter_outliers(eng.h, C.byref(op), None, vp(out), 40, 20, C.byref(n), None) == 0
    assert n.value == len(exp) and same_words(out[: n.value, 4], exp[:, 3])
    # nothing the refused calls touched has changed
    eng.prefilter_p(cl, intensity=True, **kw_of(PLAIN))
    x = params(8)
    assert eng.lib.mi355ndt_prefilter_p(eng.h, vp(rec20), 40, 20, C.byref(x.ex.base), None, 0, 20, C.byref(n)) == BAD_ARG
    kid = eng.keyframe_from_prefiltered()
    assert same_words(eng.keyframe_get(kid, intensity=True), resident)
    eng.keyframe_release(kid)
    assert [e.batch_get_cloud(k, t, intensity=True).tobytes() for k in range(5) for t in (True, False)] == before
    m = C.c_size_t()
    assert e.lib.mi355ndt_batch_get_cloud_i(e.h, 0, 2, vp(out), 0, 20, 8, C.byref(m)) == BAD_ARG
    assert e.lib.mi355ndt_batch_get_cloud_i(e.h, 0, 2, vp(out), 0, 16, 16, C.byref(m)) == BAD_ARG
    assert e.lib.mi355ndt_batch_get_cloud_i(e.h, 0, 2, None, 0, 16, -1, C.byref(m)) == BAD_ARG
