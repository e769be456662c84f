"""GPU box: exact k-nearest and radius search over a resident window keyframe, against the route a host has without it.

    python tools/keyframe_knn_timing.py [--frames 40] [--azimuth 1024] [--points 100000] [--queries 65536] [--steps 9] [--warmup 2]
                                        [--radius 0.5] [--max-nn 16] [--workers 16]

The searched cloud is the window keyframe of a synth.make_sequence drive (WindowKeyframer, leaf 0.1 m) whose size is nearest --points; the
queries are the first --queries points of a neighbouring window keyframe, moved by the relative pose of the two.  Legs, each the median /
min / max of --steps synchronous calls after --warmup (host clock around the call, which ends in the call's one wait for the device), the
two query orders of a leg taken alternately in one loop:
  resident   Engine.keyframe_knn_ids: the queries are a resident keyframe, read in place        (k = 5, k = 20; input order, cell order)
  host       Engine.keyframe_knn: the queries come from the host and are staged                  (k = 5, k = 20; input order, cell order)
  shuffled   the host leg with the queries in a random order -- a window keyframe's points come out of the VoxelGrid in cell order, queries
             from elsewhere do not                                                               (k = 5, k = 20, the radius; both orders)
  radius     Engine.keyframe_radius_search, host queries                                         (input order, cell order)
  first      the first search of a fresh keyframe: the index build rides the call
  cpu        what a host does today: Engine.keyframe_get, scipy.spatial.cKDTree build, query(workers=--workers, at most 16) -- the
             download and the build timed on their own, then the queries alone (a host that keeps its tree pays those once per keyframe)
`identical` = the two query orders returned the same bytes; `agree_cpu` = the share of queries whose id lists equal the kd-tree's (f64
distances over the same f32 points: they part only where rounding makes or breaks a tie).  One JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools import knn_ref as R  # noqa: E402

PRM = dict(trans_epsilon=0.01, max_iterations=64)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3))


def timed_alternately(fs, warmup, steps):
    """the calls of `fs` in turn, warmup + steps rounds: [times of each], [last result of each]"""
    ts, out = [[] for _ in fs], [None] * len(fs)
    for i in range(warmup + steps):
        for j, f in enumerate(fs):
            t0 = time.perf_counter()
            out[j] = f()
            if i >= warmup:
                ts[j].append((time.perf_counter() - t0) * 1e3)
    return ts, out


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def cpu_route(cloud, moved, ks, radius, max_nn, workers, warmup, steps):
    """rows of the kd-tree route over a downloaded cloud: the build, then each query leg"""
    from scipy.spatial import cKDTree
    c64, q64 = cloud.astype(np.float64), moved.astype(np.float64)
    tb, (tree,) = timed_alternately([lambda: cKDTree(c64)], min(warmup, 1), max(3, steps // 2))
    rows = [dict(leg="cpu", what="cKDTree build", **stats(tb[0]))]
    ids = {}
    for k in ks:
        t, (res,) = timed_alternately([lambda: tree.query(q64, k, workers=workers)], min(warmup, 1), max(3, steps // 2))
        ids[k] = res[1].reshape(len(q64), k)
        rows.append(dict(leg="cpu", what=f"query k={k}", workers=workers, **stats(t[0])))
    t, _ = timed_alternately([lambda: tree.query(q64, max_nn, distance_upper_bound=radius, workers=workers)], min(warmup, 1), max(3, steps // 2))
    rows.append(dict(leg="cpu", what=f"query k={max_nn} within {radius} m", workers=workers, **stats(t[0])))
    return rows, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--azimuth", type=int, default=1024)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=float, default=0.5)
    ap.add_argument("--max-nn", type=int, default=16)
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    workers = max(1, min(16, a.workers))
    from lv_slam_amd import keyframes as KF
    from lv_slam_amd import ndt, synth
    scans, poses = synth.make_sequence(a.frames, a.azimuth)
    scans = [s.numpy().astype(np.float32) for s in scans]
    e = ndt.Engine(ndt.default_params(**PRM))
    wk = KF.WindowKeyframer(e, delta_trans=4.0, delta_angle=0.3, leaf=0.1)
    kfs = [r for r in (wk.push(P, s, seq=k) for k, (P, s) in enumerate(zip(poses, scans))) if r is not None] + [wk.flush()]
    sizes = [e.keyframe_get(r.id, fetch=False) for r in kfs]
    big = [i for i, n in enumerate(sizes) if n >= a.queries] or list(range(len(kfs)))
    it = min(big, key=lambda i: abs(sizes[i] - a.points))
    iq = min((i for i in big if i != it), key=lambda i: abs(i - it), default=it)
    cloud = e.keyframe_get(kfs[it].id)
    q = np.ascontiguousarray(e.keyframe_get(kfs[iq].id)[:a.queries])
    T64 = KF.isometry_inverse(kfs[it].odom) @ kfs[iq].odom
    T = T64.astype(np.float32)
    e.close()
    print(json.dumps(dict(window_keyframes=sizes, searched_points=len(cloud), queries=len(q), radius=a.radius, max_nn=a.max_nn)), flush=True)

    g = ndt.Engine(ndt.default_params(**PRM))
    kid, qid = g.keyframe_add(cloud), g.keyframe_add(q)
    g.synchronize()
    t0 = time.perf_counter()
    first = g.keyframe_knn(kid, q, 5, T=T, query_order=ndt.KNN_ORDER_INPUT)
    print(json.dumps(dict(leg="first", what="keyframe_knn k=5 with the index build", ms=round((time.perf_counter() - t0) * 1e3, 3))), flush=True)
    orders = (("input", ndt.KNN_ORDER_INPUT), ("cell", ndt.KNN_ORDER_CELL))
    got = {}
    for k in (5, 20):
        ts, out = timed_alternately([lambda o=o: g.keyframe_knn_ids([kid], [qid], [T64], k, query_order=o, total_queries=len(q)) for _, o in orders], a.warmup, a.steps)
        for (name, _), t in zip(orders, ts):
            print(json.dumps(dict(leg="resident", what=f"keyframe_knn_ids k={k}", order=name, **stats(t), identical=same(out[0], out[1]))), flush=True)
        ts, out2 = timed_alternately([lambda o=o: g.keyframe_knn(kid, q, k, T=T, query_order=o) for _, o in orders], a.warmup, a.steps)
        for (name, _), t in zip(orders, ts):
            print(json.dumps(dict(leg="host", what=f"keyframe_knn k={k}", order=name, **stats(t),
                                  identical=same(out2[0], out2[1]) and same(out2[0], out[0]))), flush=True)
        got[k] = out[0]
    assert same(first, got[5])
    ts, out = timed_alternately([lambda o=o: g.keyframe_radius_search(kid, q, a.radius, a.max_nn, T=T, query_order=o) for _, o in orders], a.warmup, a.steps)
    for (name, _), t in zip(orders, ts):
        print(json.dumps(dict(leg="radius", what=f"keyframe_radius_search r={a.radius} max_nn={a.max_nn}", order=name, **stats(t),
                              identical=same(out[0], out[1]), mean_found=round(float(out[0][2].mean()), 2))), flush=True)

    # queries that do not arrive in cell order
    perm = np.random.default_rng(0).permutation(len(q))
    qs = np.ascontiguousarray(q[perm])
    for k in (5, 20):
        ts, out = timed_alternately([lambda o=o: g.keyframe_knn(kid, qs, k, T=T, query_order=o) for _, o in orders], a.warmup, a.steps)
        for (name, _), t in zip(orders, ts):
            print(json.dumps(dict(leg="shuffled", what=f"keyframe_knn k={k}", order=name, **stats(t),
                                  identical=same(out[0], out[1]) and same(out[0], [x[perm] for x in got[k]]))), flush=True)
    ts, out = timed_alternately([lambda o=o: g.keyframe_radius_search(kid, qs, a.radius, a.max_nn, T=T, query_order=o) for _, o in orders], a.warmup, a.steps)
    for (name, _), t in zip(orders, ts):
        print(json.dumps(dict(leg="shuffled", what=f"keyframe_radius_search r={a.radius} max_nn={a.max_nn}", order=name, **stats(t),
                              identical=same(out[0], out[1]))), flush=True)

    # the route a host has today
    tg, (down,) = timed_alternately([lambda: g.keyframe_get(kid)], 1, max(3, a.steps // 2))
    print(json.dumps(dict(leg="cpu", what="keyframe_get", **stats(tg[0]))), flush=True)
    moved, _ = R.move(q, T)
    rows, ids = cpu_route(down, moved, (5, 20), a.radius, a.max_nn, workers, a.warmup, a.steps)
    for r in rows:
        print(json.dumps(r), flush=True)
    for k in (5, 20):
        print(json.dumps(dict(leg="cpu", what=f"agreement k={k}", agree_cpu=round(float((ids[k] == got[k][0]).all(axis=1).mean()), 5))), flush=True)
    g.close()


if __name__ == "__main__":
    main()
