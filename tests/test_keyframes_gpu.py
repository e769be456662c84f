"""GPU (-m gpu): the keyframe store (mi355ndt_keyframe_*), the consumers that take ids (mi355ndt_map_cloud_keyframes,
mi355ndt_batch_set_target_keyframe / _source_keyframe, loop_closure.verify_candidates with ids) and the pipeline end to end
(WindowKeyframer -> ids -> map_cloud_keyframes).  Every comparison is an equality of words."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import keyframes as KF
from lv_slam_amd import loop_closure as LC
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


WR, MR = _tool("window_map_ref"), _tool("map_cloud_ref")


def same_words(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _res_words(r):
    return (r["final"].tobytes(), r["score"], r["iterations"], r["converged"], r["trans_probability"])


@pytest.fixture(scope="module")
def drive():
    """The map cloud tests' shape: every 5th frame of a 40-frame synthetic drive (65,536 points per scan) with its ground-truth poses."""
    scans, poses = synth.make_sequence(40)
    return [scans[k].numpy().astype(np.float32) for k in range(0, 40, 5)], [poses[k] for k in range(0, 40, 5)]


def test_add_get_round_trip_and_ids(drive):
    clouds, _ = drive
    e = ndt.Engine()
    rng = np.random.default_rng(41)
    c = clouds[0][:10007].copy()
    c[5] = [np.nan, np.inf, -np.inf]                              # a host cloud as it is: nothing filtered
    rec = np.concatenate([c, rng.uniform(0, 1, (len(c), 1)).astype(np.float32)], axis=1)
    a = e.keyframe_add(c)
    b = e.keyframe_add(rec, intensity=True)
    z = e.keyframe_add(np.zeros((0, 3), np.float32))
    assert (a, b, z) == (0, 1, 2) and e.keyframe_count() == 3
    assert same_words(e.keyframe_get(a), c) and e.keyframe_get(a, fetch=False) == len(c)
    assert same_words(e.keyframe_get(b, intensity=True), rec) and same_words(e.keyframe_get(b), c)
    got = e.keyframe_get(a, intensity=True)                       # no intensity carried: zeros
    assert same_words(got[:, :3], c) and (got[:, 3] == 0).all()
    assert e.keyframe_get(z).shape == (0, 3)
    e.keyframe_release(a)
    assert e.keyframe_count() == 2
    d = e.keyframe_add(c[:100])
    assert d == 3                                                 # ids are not reused
    kid, _ = e.window_keyframe([c[:1000]], [np.eye(4)], 0.1)
    assert kid == 4
    # a released id, and one never given out, are refused by every consumer
    for bad in (a, 99, -1):
        calls = [lambda: e.keyframe_get(bad), lambda: e.keyframe_get(bad, fetch=False), lambda: e.keyframe_release(bad),
                 lambda: e.map_cloud_keyframes([b, bad], [np.eye(4)] * 2, 0.5), lambda: LC.verify_candidates(e, b, [bad], np.eye(4)[None]),
                 lambda: LC.verify_candidates(e, bad, [b], np.eye(4)[None])]
        e.batch_reserve(1, 20000, 20000)
        calls += [lambda: e.batch_set_target_keyframe(0, bad), lambda: e.batch_set_source_keyframe(0, bad)]
        for f in calls:
            with pytest.raises(ndt.NDTError) as ex:
                f()
            assert ex.value.code == -2 and "keyframe" in str(ex.value)
    assert "released" in str(ex.value) or "never" in str(ex.value)
    # a keyframe larger than the reserved rows
    e.batch_reserve(1, 64, 64)
    with pytest.raises(ndt.NDTError) as ex:
        e.batch_set_source_keyframe(0, b)
    assert ex.value.code == -2
    assert same_words(e.keyframe_get(b, intensity=True), rec)     # the store is intact after all that
    e.close()


def test_refused_in_stream_mode(drive):
    clouds, _ = drive
    e = ndt.Engine(ndt.default_params(**PRM))
    c = clouds[0][:5000]
    kid = e.keyframe_add(c)
    e.stream_begin(2, 4, 4096, 4096)
    try:
        for f in (lambda: e.keyframe_add(c), lambda: e.keyframe_get(kid), lambda: e.keyframe_release(kid), lambda: e.keyframe_count(),
                  lambda: e.window_keyframe([c], [np.eye(4)], 0.1), lambda: e.map_cloud_keyframes([kid], [np.eye(4)], 0.5),
                  lambda: e.batch_set_target_keyframe(0, kid), lambda: e.batch_set_source_keyframe(0, kid)):
            with pytest.raises(ndt.NDTError) as ex:
                f()
            assert ex.value.code == -7
    finally:
        e.stream_end()
    assert e.keyframe_count() == 1 and same_words(e.keyframe_get(kid), c)
    e.close()


def test_resident_registration_is_left_as_it_was(drive):
    """After any of the new calls a resident single registration aligns to the same bits as before."""
    clouds, poses = drive
    t, s, _ = synth.make_pair(210, 256)
    t, s = t.numpy(), s.numpy()
    G = synth.default_guess()

    def run(with_keyframes):
        e = ndt.Engine(ndt.default_params(**PRM))
        pf = e.prefilter(clouds[0][:20000], 0.5, 100.0, 0.2)
        e.set_target(t)
        e.set_source(s)
        out = [_res_words(e.align(G))]
        if with_keyframes:
            a = e.keyframe_add(clouds[1])
            w, _ = e.window_keyframe(clouds[2:5], [np.linalg.inv(poses[2]) @ p for p in poses[2:5]], 0.1)
            mc = e.map_cloud(clouds[:2], poses[:2], 0.5)
        out.append(_res_words(e.align(G)))
        if with_keyframes:
            e.map_cloud_keyframes([a, w], [poses[1], poses[2]], 0.5)
            e.keyframe_get(w)
            e.keyframe_release(a)
            assert same_words(e.map_cloud(clouds[:2], poses[:2], 0.5), mc)      # the map cloud's own workspace serves both routes
        out.append(_res_words(e.align(G)))
        out.append(e.fitness_score())
        e.use_prefiltered(as_target=True)                         # the prefilter result is still the one from before
        out.append(_res_words(e.align(G)))
        e.close()
        return pf.tobytes(), out

    assert run(True) == run(False)


@pytest.mark.parametrize("r", [0.5, 0.05])
def test_map_cloud_keyframes_equals_map_cloud(drive, r):
    clouds, poses = drive
    e = ndt.Engine()
    exp = e.map_cloud(clouds, poses, r)
    ids = [e.keyframe_add(c) for c in clouds]
    e.synchronize()
    before = e.profile_get()
    got = e.map_cloud_keyframes(ids, poses, r)
    after = e.profile_get()
    assert after["cloud_uploads"] == before["cloud_uploads"] and after["cloud_upload_bytes"] == before["cloud_upload_bytes"]
    assert got.shape == exp.shape and same_words(got, exp)
    assert e.map_cloud_keyframes(ids, poses, r, fetch=False) == len(exp)
    # empty keyframes in between, a keyframe with intensity, a keyframe used twice
    z = e.keyframe_add(np.zeros((0, 3), np.float32))
    wi = e.keyframe_add(np.concatenate([clouds[1], np.ones((len(clouds[1]), 1), np.float32)], axis=1), intensity=True)
    empty = np.zeros((0, 3), np.float32)
    exp2 = e.map_cloud([empty, clouds[0], clouds[1], empty, clouds[0]], [poses[0], poses[0], poses[1], poses[2], poses[3]], r)
    got2 = e.map_cloud_keyframes([z, ids[0], wi, z, ids[0]], [poses[0], poses[0], poses[1], poses[2], poses[3]], r)
    assert same_words(got2, exp2)
    assert e.map_cloud_keyframes([], [], r) is None and e.map_cloud_keyframes([z, z], [np.eye(4)] * 2, r).shape == (0, 3)
    with pytest.raises(ndt.NDTError) as ex:
        e.map_cloud_keyframes(ids[:1], poses[:1], 0.0)
    assert ex.value.code == -2
    e.close()


@pytest.mark.parametrize("use_bow", [False, True])
@pytest.mark.parametrize("mr", [1.0, float("inf")])
def test_verify_candidates_with_ids_equals_arrays(use_bow, mr):
    """The shapes of tests/test_batch_fitness_gpu.py's loop-closure case: index, pose words and score bits are those of the array route."""
    t, s, _ = synth.make_pair(120, 256)
    target, src = t.numpy(), s.numpy()
    new_pose = np.eye(4)
    new_pose[:3, 3] = [10.0, 5.0, 0.0]
    offsets = [(0.2, 0.1, 0.0), (0.6, -0.3, 0.02), (25.0, 8.0, 0.6), (0.0, 0.0, 0.0), (-40.0, 12.0, -0.9)]
    cand_poses = []
    for dx, dy, yaw in offsets:
        P = new_pose.copy()
        P[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        P[:3, 3] += [dx, dy, 0.0]
        cand_poses.append(P)
    candidates = [src, src[:-100], src, src[50:], src]            # (different sizes: the slots' tails must be zero-filled alike)
    guesses = np.stack([LC.loop_guess(new_pose, P) for P in cand_poses])
    bow = [(0.5, 2), (0.3, 0), (0.2, 3), (0.1, 1), (0.03, 4)] if use_bow else None
    e1 = ndt.Engine(ndt.default_params(**PRM))
    exp = LC.verify_candidates(e1, target, candidates, guesses, mr, 0.5, bow)
    e2 = ndt.Engine(ndt.default_params(**PRM))
    tid = e2.keyframe_add(target)
    cids = [e2.keyframe_add(c) for c in candidates]
    e2.profile_reset()
    got = LC.verify_candidates(e2, tid, cids, guesses, mr, 0.5, bow)
    assert e2.profile_get()["cloud_uploads"] == 0
    assert got[0] == exp[0] and got[3] == exp[3]
    assert np.float64(got[2]).tobytes() == np.float64(exp[2]).tobytes()
    assert (got[1] is None and exp[1] is None) or got[1].tobytes() == exp[1].tobytes()
    # ids and arrays mixed
    mixed = LC.verify_candidates(e2, tid, [cids[0], candidates[1], cids[2], candidates[3], cids[4]], guesses, mr, 0.5, bow)
    assert mixed[0] == exp[0] and np.float64(mixed[2]).tobytes() == np.float64(exp[2]).tobytes()
    if mr == 1.0:
        assert exp[0] is not None
    e1.close()
    e2.close()


def test_window_keyframer_to_map_cloud_end_to_end():
    scans, poses = synth.make_sequence(40, 256)                   # 16,384 points per scan
    scans = [s.numpy().astype(np.float32) for s in scans]

    class RefEngine:                                              # the same pipeline through the CPU restatements
        def __init__(self):
            self.clouds = []

        def window_keyframe(self, sc, rel, leaf=0.1, intensity=False):
            self.clouds.append(WR.window_map(sc, rel, leaf, intensity))
            return len(self.clouds) - 1, len(self.clouds[-1])

    e, ref = ndt.Engine(), RefEngine()
    got_kf, exp_kf = [], []
    for eng, out in ((e, got_kf), (ref, exp_kf)):
        wk = KF.WindowKeyframer(eng, delta_trans=4.0, delta_angle=0.3, leaf=0.1)
        for k, (P, s) in enumerate(zip(poses, scans)):
            r = wk.push(P, s, seq=k)
            if r is not None:
                out.append(r)
        out.append(wk.flush())
    assert len(got_kf) == len(exp_kf) >= 4 and max(r.n_scans for r in got_kf) >= 3
    for g, x in zip(got_kf, exp_kf):
        assert (g.n, g.seq, g.n_scans, g.accum_distance) == (x.n, x.seq, x.n_scans, x.accum_distance) and np.array_equal(g.odom, x.odom)
        assert same_words(e.keyframe_get(g.id), ref.clouds[x.id])
    print("windows:", [(r.seq, r.n_scans, r.n) for r in got_kf])
    for res in (0.5, 0.05):
        got = e.map_cloud_keyframes([r.id for r in got_kf], [r.odom for r in got_kf], res)
        exp = MR.map_cloud([ref.clouds[r.id] for r in exp_kf], [r.odom for r in exp_kf], res)
        assert got.shape == exp.shape and same_words(got, exp)
    e.close()


def test_interleaved_surfaces_equal_fresh_engines():
    """The prefilter, both routes of the map cloud, the window map and the keyframe fitness scores (whose first look at a keyframe builds its
    index) share one scratch on the engine.  One engine runs them interleaved, every surface once right after a larger call and once right
    after a smaller one; every output equals, word for word, that of the same call alone on a fresh engine.  use_prefiltered then still
    hands over the prefilter result made before all of that -- and, after a second prefilter that follows a larger call, that one."""
    scans, poses = synth.make_sequence(6, 128, n_beams=48)        # 6,144 points per scan
    big = [c.numpy().astype(np.float32) for c in scans]
    small = [np.ascontiguousarray(c[::4]) for c in big]            # 1,536
    t, s, _ = synth.make_pair(210, 256, n_beams=16)                # 4,096
    t, s, s2 = t.numpy(), s.numpy(), np.ascontiguousarray(s.numpy()[::2])
    G = synth.default_guess()

    def pf(e, cloud):
        return e.prefilter(cloud, 0.5, 100.0, 0.2).tobytes()

    def mc(e, clouds, k0):
        return e.map_cloud(clouds[k0:k0 + 3], poses[k0:k0 + 3], 0.5).tobytes()

    def mk(e, clouds, k0):
        return e.map_cloud_keyframes([e.keyframe_add(c) for c in clouds[k0:k0 + 3]], poses[k0:k0 + 3], 0.5).tobytes()

    def wk(e, clouds, k0):
        kid, n = e.window_keyframe(clouds[k0:k0 + 2], [np.linalg.inv(poses[k0]) @ P for P in poses[k0:k0 + 2]], 0.1)
        return n, e.keyframe_get(kid).tobytes()

    def kff(e, clouds, k0):
        ids = [e.keyframe_add(c) for c in clouds[k0:k0 + 3]]
        rel = np.stack([np.linalg.inv(poses[k0 + i]) @ poses[k0 + i + 1] for i in range(2)])
        sc, inl = e.keyframe_fitness_scores(ids[:2], ids[1:], rel, 1.0)
        return np.float64(sc).tobytes(), np.int64(inl).tobytes()

    def handed(e):                                                 # the prefilter result as the target of a registration
        e.set_source(s)
        e.use_prefiltered(as_target=True)
        return _res_words(e.align(G)), e.fitness_score()

    def fresh(f, *a, then=None):
        e = ndt.Engine(ndt.default_params(**PRM))
        out = f(e, *a) if then is None else (f(e, *a), then(e))[1]
        e.close()
        return out

    # (call, arguments, points the call's scratch is sized for)
    order = [(wk, (small, 0), 3072), (pf, (t,), 4096), (mc, (big, 0), 18432), (wk, (small, 2), 3072), (mk, (big, 1), 18432),
             (kff, (small, 0), 1536), (wk, (big, 0), 12288), (mc, (small, 1), 4608), (kff, (big, 0), 6144), (mk, (small, 3), 4608)]
    tail = [(mc, (big, 3), 18432), (pf, (s2,), 2048)]
    for f in (pf, mc, mk, wk, kff):                                # every surface follows a larger and a smaller call
        seq = order + tail
        after = [seq[i - 1][2] - seq[i][2] for i in range(1, len(seq)) if seq[i][0] is f]
        assert min(after) < 0 < max(after), f.__name__
    e = ndt.Engine(ndt.default_params(**PRM))
    for i, (f, a, _) in enumerate(order):
        assert f(e, *a) == fresh(f, *a), (i, f.__name__)
    assert handed(e) == fresh(pf, t, then=handed)                  # the first prefilter's result, nine other calls later
    for i, (f, a, _) in enumerate(tail):
        assert f(e, *a) == fresh(f, *a), ("tail", i, f.__name__)
    assert handed(e) == fresh(pf, s2, then=handed)
    e.close()
