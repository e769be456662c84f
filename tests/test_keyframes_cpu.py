"""CPU: the keyframe policy of the global graph node (lv_slam_amd/keyframes.py: KeyframeUpdater, WindowKeyframer) on scripted pose lists,
with a fake engine recording the calls; and verify_candidates' id route against a fake engine."""
import numpy as np
import pytest

from lv_slam_amd import keyframes as KF
from lv_slam_amd import loop_closure as LC


def pose(x=0.0, y=0.0, yaw=0.0):
    P = np.eye(4)
    P[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    P[:3, 3] = [x, y, 0.0]
    return P


class FakeEngine:
    def __init__(self):
        self.calls = []

    def window_keyframe(self, scans, rel_poses, leaf=0.1, intensity=False):
        self.calls.append(dict(scans=list(scans), rel=[np.array(r) for r in rel_poses], leaf=leaf, intensity=intensity))
        return len(self.calls) - 1, sum(len(s) for s in scans)


def test_updater_first_pose_then_thresholds():
    u = KF.KeyframeUpdater(delta_trans=2.0, delta_angle=0.5)
    assert u.is_first and u.update(pose(5.0)) and not u.is_first        # the first pose, wherever it is
    assert u.accum_distance == 0.0
    assert not u.update(pose(6.9))                                      # dx = 1.9 < 2
    assert u.update(pose(7.0))                                          # dx = 2.0: not "< delta"
    assert u.accum_distance == 2.0
    assert not u.update(pose(7.5, 0.0, 0.9))                            # da = acos(w) = yaw / 2 = 0.45 < 0.5
    assert u.update(pose(7.5, 0.0, 1.0 + 1e-9))                         # da = 0.5 (+): a keyframe by angle alone
    assert u.accum_distance == 2.5
    assert np.array_equal(u.prev_keypose, pose(7.5, 0.0, 1.0 + 1e-9))
    # a rejected pose changes nothing
    before = (u.accum_distance, u.prev_keypose.copy())
    assert not u.update(pose(7.6, 0.0, 1.0))
    assert u.accum_distance == before[0] and np.array_equal(u.prev_keypose, before[1])


def test_quaternion_w_is_the_half_angle_cosine():
    for yaw in (0.0, 0.3, 1.5, 3.0, -2.5):                              # trace > 0 and the other branch (whose sign follows the matrix)
        assert abs(KF.quaterniond_w(pose(yaw=yaw)[:3, :3])) == pytest.approx(abs(np.cos(yaw / 2)), abs=1e-15)
    assert KF.quaterniond_w(pose(yaw=3.0)[:3, :3]) > 0 > KF.quaterniond_w(pose(yaw=-2.5)[:3, :3])
    rx = np.array([[1, 0, 0], [0, np.cos(3.0), -np.sin(3.0)], [0, np.sin(3.0), np.cos(3.0)]])
    assert KF.quaterniond_w(rx) == pytest.approx(np.cos(1.5), abs=1e-15)


def test_window_keyframer_scripted_drive():
    eng = FakeEngine()
    wk = KF.WindowKeyframer(eng, delta_trans=2.0, delta_angle=0.5, leaf=0.2, intensity=False)
    xs = [0.0, 0.5, 1.5, 2.5, 3.0, 4.4, 4.6, 7.0]                      # keyframes at 0.0, 2.5, 4.6 (dx 2.1 from 2.5), 7.0
    odoms = [pose(x, 0.1 * k, 0.01 * k) for k, x in enumerate(xs)]
    scans = [np.full((k + 1, 3), float(k), np.float32) for k in range(len(xs))]
    out = [wk.push(o, s, seq=100 + k) for k, (o, s) in enumerate(zip(odoms, scans))]
    closes = [k for k, r in enumerate(out) if r is not None]
    assert closes == [3, 6, 7]                                          # the frames that close a window (and open the next)
    assert len(eng.calls) == 3
    windows = [(0, [0, 1, 2]), (3, [3, 4, 5]), (6, [6])]
    acc = 0.0
    prev = None
    for w, (call, (first, members), k) in enumerate(zip(eng.calls, windows, closes)):
        r = out[k]
        assert [int(s[0, 0]) for s in call["scans"]] == members         # which scans, in order
        assert call["leaf"] == 0.2 and call["intensity"] is False
        assert np.array_equal(call["rel"][0], np.eye(4))
        for m, rel in zip(members[1:], call["rel"][1:]):
            assert np.array_equal(rel, KF.isometry_inverse(odoms[first]) @ odoms[m])    # w_odom.inverse() * odom
        if prev is not None:
            acc += float(np.linalg.norm((KF.isometry_inverse(odoms[prev]) @ odoms[first])[:3, 3]))
        prev = first
        assert r.seq == 100 + first and np.array_equal(r.odom, odoms[first]) and r.n_scans == len(members)
        assert r.accum_distance == acc                                  # as of the window's first frame
        assert r.id == w and r.n == sum(len(s) for s in call["scans"])
    # the open window (frame 7) closes on flush, once
    last = wk.flush()
    assert last.seq == 107 and last.n_scans == 1 and len(eng.calls) == 4
    assert wk.flush() is None and len(eng.calls) == 4


def test_window_keyframer_counts_frames_without_seq():
    eng = FakeEngine()
    wk = KF.WindowKeyframer(eng, delta_trans=1.0, delta_angle=2.0)
    got = [wk.push(pose(0.6 * k), np.zeros((1, 3), np.float32)) for k in range(6)]      # keyframes at frames 0, 2, 4
    assert [r.seq for r in got if r is not None] == [0, 2]
    assert eng.calls[0]["leaf"] == 0.1


class FakeBatchEngine:
    """Records which setter verify_candidates uses for which slot."""

    def __init__(self, sizes):
        self.sizes, self.log = sizes, []

    def keyframe_get(self, kid, intensity=False, fetch=True):
        assert not fetch
        return self.sizes[kid]

    def batch_reserve(self, n, mt, ms):
        self.log.append(("reserve", n, mt, ms))

    def batch_set_target(self, k, c):
        self.log.append(("tgt", k, len(c)))

    def batch_set_source(self, k, c):
        self.log.append(("src", k, len(c)))

    def batch_set_target_keyframe(self, k, kid):
        self.log.append(("tgt_id", k, kid))

    def batch_set_source_keyframe(self, k, kid):
        self.log.append(("src_id", k, kid))

    def batch_align(self, G):
        return [dict(converged=True, final=np.eye(4, dtype=np.float32)) for _ in G]

    def batch_fitness_scores(self, mr):
        n = self.log[0][1]
        return np.arange(n, dtype=np.float64) * 0.1 + 0.1, np.ones(n, np.int64)


def test_verify_candidates_routes_ids_and_arrays():
    eng = FakeBatchEngine({4: 300, 9: 120})
    arr = np.zeros((50, 3), np.float32)
    idx, _, score, n = LC.verify_candidates(eng, 4, [9, arr], np.stack([np.eye(4)] * 2))
    assert eng.log == [("reserve", 2, 300, 120), ("tgt_id", 0, 4), ("src_id", 0, 9), ("tgt_id", 1, 4), ("src", 1, 50)]
    assert idx == 0 and score == 0.1 and n == 2
    eng = FakeBatchEngine({})
    LC.verify_candidates(eng, arr, [arr], np.eye(4)[None])
    assert eng.log == [("reserve", 1, 50, 50), ("tgt", 0, 50), ("src", 0, 50)]
