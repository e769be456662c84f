"""GPU (-m gpu): resident scans -- mi355ndt_keyframe_from_prefiltered, mi355ndt_keyframe_from_slot, mi355ndt_window_keyframe_ids -- and
WindowKeyframer over ids.  The yardsticks: the prefilter's own output read back, mi355ndt_window_keyframe over the same clouds as host
records, and tools/window_map_ref.py.  Every comparison is word for word.  No tolerances."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import keyframes as KF
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
BAD_ARG, ERR_STATE = -2, -7


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(name, m)
    spec.loader.exec_module(m)
    return m


W = _load("window_map_ref")


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def drive():
    """four of the smallest synthetic frames tests/test_sequence.py uses (8,192 points), with intensities whose sum order shows"""
    scans, poses = synth.make_sequence(4, 256, n_beams=32)
    rng = np.random.default_rng(31)
    recs = []
    for s in scans:
        w = (np.arange(len(s), dtype=np.float32) * np.float32(0.37)).astype(np.float32)
        w[::13] *= np.float32(1e7)
        w[5::17] *= np.float32(-3e6)
        recs.append(np.ascontiguousarray(np.concatenate([s.numpy().astype(np.float32), w[rng.permutation(len(s))][:, None]], axis=1)))
    return recs, poses


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(**PRM))
    yield e
    e.close()


def test_keyframe_from_prefiltered(eng, drive):
    recs, _ = drive
    for intensity in (True, False):
        out = eng.prefilter_p(recs[0], downsample_resolution=0.25, intensity=intensity)
        kid = eng.keyframe_from_prefiltered()
        got = eng.keyframe_get(kid, intensity=True)
        assert len(out) > 500 and same_words(got[:, :3], out[:, :3])
        assert same_words(got[:, 3], out[:, 3]) if intensity else not got[:, 3].view(np.uint32).any()
        # the source is intact: the outlier stage runs over it as it would have, and its result makes another keyframe
        o = dict(method="STATISTICAL", mean_k=4, stddev_mul=1.0)
        surv = eng.prefilter_outliers(intensity=intensity, **o)
        other = ndt.Engine(ndt.default_params(**PRM))
        assert same_words(surv, other.prefilter(recs[0], downsample_resolution=0.25, distance_near=0.5, outlier=o, intensity=intensity)
                          if intensity else other.prefilter(recs[0][:, :3], downsample_resolution=0.25, outlier=o))
        other.close()
        kid2 = eng.keyframe_from_prefiltered()
        assert 0 < len(surv) < len(out) and same_words(eng.keyframe_get(kid2, intensity=intensity), surv)
        assert same_words(eng.keyframe_get(kid, intensity=True), got)            # the first keyframe owns its rows
        eng.keyframe_release(kid)
        eng.keyframe_release(kid2)
    # an empty result gives an empty keyframe
    assert eng.prefilter_p(np.zeros((0, 4), np.float32), intensity=True, fetch=False) == 0
    kid = eng.keyframe_from_prefiltered()
    assert eng.keyframe_get(kid, intensity=True).shape == (0, 4)
    eng.keyframe_release(kid)
    assert eng.prefilter_p(recs[0][:50] * np.float32(0.001), intensity=True, fetch=False) == 0      # everything inside distance_near
    kid = eng.keyframe_from_prefiltered()
    assert eng.keyframe_get(kid, fetch=False) == 0
    eng.keyframe_release(kid)


def test_keyframe_from_slot(drive):
    recs, _ = drive
    e = ndt.Engine(ndt.default_params(**PRM))
    e.batch_reserve(3, 8192, 8192)
    with pytest.raises(ndt.NDTError) as ex:
        e.keyframe_from_slot(0, True)                                           # a side never given a cloud
    assert ex.value.code == BAD_ARG
    empty = np.zeros((0, 4), np.float32)
    e.batch_prefilter([recs[0], recs[1], empty], [recs[2], empty, recs[3]], downsample_resolution=0.25, intensity=True)
    e.batch_set_source(0, recs[2][:700, :3])                                    # a slot without intensity: a keyframe of three channels
    before = [e.batch_get_cloud(k, t, intensity=True) for k in range(3) for t in (True, False)]
    ids = [e.keyframe_from_slot(k, t) for k in range(3) for t in (True, False)]
    for kid, cloud in zip(ids, before):
        assert same_words(e.keyframe_get(kid, intensity=True), cloud)
    assert len(before[0]) > 500 and before[3].shape == (0, 4) and before[4].shape == (0, 4)
    assert not before[1][:, 3].view(np.uint32).any() and before[0][:, 3].view(np.uint32).any()
    after = [e.batch_get_cloud(k, t, intensity=True) for k in range(3) for t in (True, False)]
    assert all(same_words(a, b) for a, b in zip(before, after))                  # the slots are intact
    # the keyframes own their rows: refilling the slot changes nothing in the store
    e.batch_set_target(0, recs[3][:100, :3])
    assert same_words(e.keyframe_get(ids[0], intensity=True), before[0])
    for bad in ((3, True), (-1, False)):
        with pytest.raises(ndt.NDTError) as ex:
            e.keyframe_from_slot(*bad)
        assert ex.value.code == BAD_ARG
    kid = C.c_int()
    assert e.lib.mi355ndt_keyframe_from_slot(e.h, 0, 3, C.byref(kid)) == BAD_ARG
    e.close()


def test_stream_mode_and_missing_result_are_state_errors():
    e = ndt.Engine(ndt.default_params(**PRM))
    with pytest.raises(ndt.NDTError) as ex:
        e.keyframe_from_prefiltered()
    assert ex.value.code == ERR_STATE and "no prefilter result" in str(ex.value)
    e.prefilter_p(np.ones((10, 4), np.float32), intensity=True)
    e.batch_reserve(1, 64, 64)
    e.batch_set_target(0, np.ones((10, 3), np.float32))
    a = e.keyframe_from_prefiltered()
    e.stream_begin(2, 4, 4096, 4096)
    for f in (e.keyframe_from_prefiltered, lambda: e.keyframe_from_slot(0, True), lambda: e.window_keyframe_ids([a], [np.eye(4)]),
              lambda: e.batch_get_cloud(0, True, intensity=True)):
        with pytest.raises(ndt.NDTError) as ex:
            f()
        assert ex.value.code == ERR_STATE
    e.stream_end()
    assert e.keyframe_get(a, fetch=False) == 1                                   # (ten copies of one point: one voxel)
    e.close()


def small_poses(k):
    out = [np.eye(4)]
    for j in range(1, k):
        T = np.eye(4)
        a = 0.01 * j
        T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        T[:3, 3] = [0.4 * j, -0.05 * j, 0.01 * j]
        out.append(T)
    return out


@pytest.mark.parametrize("leaf", [0.1, 0.0, 1e-4], ids=["leaf0.1", "leaf0", "leaf-too-small"])
def test_window_keyframe_ids(eng, drive, leaf):
    """three resident scans -- one of them empty, one id twice -- against window_keyframe over the downloaded arrays and the restatement"""
    recs, _ = drive
    filtered = [eng.prefilter_p(r[:3000], downsample_resolution=0.2, intensity=True) for r in recs[:2]]
    ids = []
    for r in recs[:2]:
        eng.prefilter_p(r[:3000], downsample_resolution=0.2, intensity=True, fetch=False)
        ids.append(eng.keyframe_from_prefiltered())
    eng.prefilter_p(np.zeros((0, 4), np.float32), intensity=True, fetch=False)
    ids.append(eng.keyframe_from_prefiltered())
    scans = [filtered[0], filtered[1], np.zeros((0, 4), np.float32), filtered[0]]
    win, rel = [ids[0], ids[1], ids[2], ids[0]], small_poses(4)
    stored = [eng.keyframe_get(i, intensity=True) for i in ids]
    for intensity in (True, False):
        before = eng.profile_get()
        kid, n = eng.window_keyframe_ids(win, rel, leaf, intensity=intensity)
        after = eng.profile_get()
        assert after["cloud_uploads"] == before["cloud_uploads"] and after["cloud_upload_bytes"] == before["cloud_upload_bytes"]
        got = eng.keyframe_get(kid, intensity=True)
        hid, hn = eng.window_keyframe(scans if intensity else [s[:, :3] for s in scans], rel, leaf, intensity=intensity)
        host = eng.keyframe_get(hid, intensity=True)
        exp = W.window_map(scans, rel, leaf, intensity=intensity)
        assert n == hn == len(exp) and same_words(got, host)
        assert same_words(got[:, : exp.shape[1]], exp)
        if not intensity:
            assert not got[:, 3].view(np.uint32).any()
        if leaf == 0.1:
            assert 100 < n < sum(len(s) for s in scans)
        else:
            assert n == sum(len(s) for s in scans)
        eng.keyframe_release(kid)
        eng.keyframe_release(hid)
    # a 3-channel scan read with an intensity contributes +0
    x3 = eng.keyframe_add(filtered[1][:, :3])
    kid, _ = eng.window_keyframe_ids([ids[0], x3], rel[:2], leaf, intensity=True)
    z = filtered[1].copy()
    z[:, 3] = 0.0
    assert same_words(eng.keyframe_get(kid, intensity=True), W.window_map([filtered[0], z], rel[:2], leaf, intensity=True))
    eng.keyframe_release(kid)
    # the scans' keyframes are unchanged
    assert all(same_words(eng.keyframe_get(i, intensity=True), s) for i, s in zip(ids, stored))
    # released and unknown ids are refused with the store's message
    eng.keyframe_release(x3)
    for bad, word in ((x3, "released"), (10 ** 6, "never given out")):
        with pytest.raises(ndt.NDTError) as ex:
            eng.window_keyframe_ids([ids[0], bad], rel[:2], leaf)
        assert ex.value.code == BAD_ARG and "no keyframe with id" in str(ex.value) and word in str(ex.value)
    for i in ids:
        eng.keyframe_release(i)


def test_raw_scans_to_keyframes_without_a_download(drive):
    """raw [N,4] scans -> sequence_run_raw(intensity=True) -> keyframe_from_slot -> WindowKeyframer over ids, against WindowKeyframer over host
    arrays of the same filtered scans; both keyframes give the same map cloud"""
    recs, _ = drive
    stamps = [0.1 * k for k in range(len(recs))]
    e = ndt.Engine(ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=3, variant=1))
    frames, _, counts = e.sequence_run_raw(recs, stamps, keyframe_delta_trans=2.5, downsample_resolution=0.25, intensity=True)
    host = [e.batch_get_cloud(k, True, intensity=True) for k in range(len(recs))]
    assert [len(h) for h in host] == counts
    up0 = e.profile_get()["cloud_uploads"]
    wa = KF.WindowKeyframer(e, delta_trans=0.8, delta_angle=2.0, leaf=0.3, intensity=True)
    a = [wa.push(f["odom"], e.keyframe_from_slot(k, True)) for k, f in enumerate(frames)] + [wa.flush()]
    assert e.profile_get()["cloud_uploads"] == up0                               # nothing crossed PCIe on the resident route
    wb = KF.WindowKeyframer(e, delta_trans=0.8, delta_angle=2.0, leaf=0.3, intensity=True)
    b = [wb.push(f["odom"], host[k]) for k, f in enumerate(frames)] + [wb.flush()]
    a, b = [r for r in a if r is not None], [r for r in b if r is not None]
    assert len(a) == len(b) >= 1 and sum(r.n_scans for r in a) == len(recs)
    for ra, rb in zip(a, b):
        assert (ra.n, ra.seq, ra.n_scans) == (rb.n, rb.seq, rb.n_scans)
        assert same_words(e.keyframe_get(ra.id, intensity=True), e.keyframe_get(rb.id, intensity=True))
    assert e.keyframe_count() == len(a) + len(b)                                 # the scans' ids were released when their windows closed
    poses = [r.odom for r in a]
    assert same_words(e.map_cloud_keyframes([r.id for r in a], poses, 0.5), e.map_cloud_keyframes([r.id for r in b], poses, 0.5))
    e.close()
