"""Keyframe policy of lv_slam's global graph node, ROS-free: which frames become keyframes and which scans make up a keyframe's window map.

`KeyframeUpdater` restates include/global_graph/keyframe_updater.hpp:37-61; `WindowKeyframer` restates the three-way branch of
GlobalGraphNodelet::cloud_callback (src/global_graph/global_graph_nodelet.cpp:202-244).  Both are host-side policy, as they are in the
reference; the window map itself -- moving the scans into the window's first frame, appending them, the VoxelGrid -- is ONE call into the
engine (Engine.window_keyframe, mi355ndt_window_keyframe) when the window closes, and the keyframe's cloud stays on the device under the id
that call returns.  A scan may also be the id of a resident keyframe (Engine.keyframe_from_slot, keyframe_from_prefiltered): a window of
ids closes through Engine.window_keyframe_ids, no scan crosses PCIe again, and the scans' ids are released once the window has closed.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


def quaterniond_w(R) -> float:
    """w of Eigen::Quaterniond(R) (Eigen's rotation matrix -> quaternion assignment), f64."""
    m = np.asarray(R, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        return float(0.5 * np.sqrt(t + 1.0))
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    return float((m[k, j] - m[j, k]) * (0.5 / t))


def isometry_inverse(T) -> np.ndarray:
    """Eigen::Isometry3d::inverse(): [R^T, -R^T t]."""
    T = np.asarray(T, np.float64)
    inv = np.eye(4)
    inv[:3, :3] = T[:3, :3].T
    inv[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return inv


class KeyframeUpdater:
    """keyframe_updater.hpp: the first pose is always a keyframe; afterwards a pose is one when it lies at least `delta_trans` metres from
    the previous keyframe's or is turned by at least `delta_angle` against it (da = acos(w) of the relative rotation's quaternion, i.e.
    HALF the rotation angle, as the reference computes it).  `accum_distance` adds up the keyframe-to-keyframe distances."""

    def __init__(self, delta_trans: float = 2.0, delta_angle: float = 2.0):       # the in-code defaults (:26-27)
        self.delta_trans = float(delta_trans)
        self.delta_angle = float(delta_angle)
        self.is_first = True
        self.prev_keypose = np.eye(4)
        self.accum_distance = 0.0

    def update(self, pose) -> bool:
        pose = np.asarray(pose, np.float64)
        if self.is_first:
            self.is_first = False
            self.prev_keypose = pose.copy()
            return True
        delta = isometry_inverse(self.prev_keypose) @ pose
        dx = float(np.linalg.norm(delta[:3, 3]))
        with np.errstate(invalid="ignore"):
            da = float(np.arccos(quaterniond_w(delta[:3, :3])))
        if dx < self.delta_trans and da < self.delta_angle:       # too close to the previous keyframe (a NaN angle fails the compare: keyframe)
            return False
        self.accum_distance += dx
        self.prev_keypose = pose.copy()
        return True


@dataclass
class WindowKeyframe:
    """What cloud_callback hands to the keyframe queue when a window closes (:227): the window's first frame carries the pose, the
    sequence number and the accumulated distance; `id` names the window map on the device, `n` its point count."""
    id: int
    n: int
    odom: np.ndarray
    seq: int
    accum_distance: float
    n_scans: int


class WindowKeyframer:
    """cloud_callback's branch over (odom, scan) pairs.  The frame the updater accepts first opens a window (:202-211); a frame it rejects
    is appended to the open window with the relative pose w_odom.inverse() * odom (:237-244); the next frame it accepts closes the window
    -- the window map becomes a keyframe (:212-229) -- and opens the next one (:230-235).  The window is kept on the host as a list of scans
    and relative poses; nothing is computed until it closes.  A scan is an array or the int id of a resident keyframe -- one kind per
    window: a window that mixes them is a ValueError."""

    def __init__(self, engine, delta_trans: float = 2.0, delta_angle: float = 2.0, leaf: float = 0.1, intensity: bool = False):
        self.engine = engine
        self.updater = KeyframeUpdater(delta_trans, delta_angle)
        self.leaf = float(leaf)
        self.intensity = bool(intensity)
        self.w_odom = None
        self.w_seq = None
        self.w_accum = 0.0
        self.w_scans: list = []
        self.w_rel: list = []
        self.frames = 0

    def _open(self, odom, scan, seq):
        self.w_odom = np.asarray(odom, np.float64).copy()
        self.w_scans = [scan]
        self.w_rel = [np.eye(4)]
        self.w_seq = seq
        self.w_accum = self.updater.accum_distance                # (:209, :235: read after update())

    @staticmethod
    def _is_id(scan) -> bool:
        return isinstance(scan, (int, np.integer)) and not isinstance(scan, (bool, np.bool_))

    def _close(self) -> WindowKeyframe:
        by_id = [self._is_id(s) for s in self.w_scans]
        if any(by_id) and not all(by_id):
            raise ValueError("a window holds resident scan ids or host scans, not both")
        if by_id[0]:
            ids = [int(s) for s in self.w_scans]
            kid, n = self.engine.window_keyframe_ids(ids, self.w_rel, self.leaf, self.intensity)
            for i in dict.fromkeys(ids):                          # (an id may appear twice in a window: released once)
                self.engine.keyframe_release(i)
        else:
            kid, n = self.engine.window_keyframe(self.w_scans, self.w_rel, self.leaf, self.intensity)
        return WindowKeyframe(kid, n, self.w_odom, self.w_seq, self.w_accum, len(self.w_scans))

    def push(self, odom, scan, seq: int | None = None):
        """One (odom, scan) pair.  Returns the WindowKeyframe of the window this frame closed, else None."""
        if seq is None:
            seq = self.frames
        self.frames += 1
        first = self.updater.is_first
        if self.updater.update(odom):
            out = None if first else self._close()
            self._open(odom, scan, seq)
            return out
        if self._is_id(scan) != self._is_id(self.w_scans[0]):
            raise ValueError("a window holds resident scan ids or host scans, not both")
        self.w_scans.append(scan)
        self.w_rel.append(isometry_inverse(self.w_odom) @ np.asarray(odom, np.float64))
        return None

    def flush(self):
        """Close the open window without a next frame (the reference never does: its last window is lost when the node stops)."""
        if self.w_odom is None:
            return None
        out = self._close()
        self.w_odom, self.w_scans, self.w_rel = None, [], []
        return out
