"""GPU box: the fitness scores of graph edges between resident window keyframes, three routes on the same edges.

    python tools/keyframe_fitness_timing.py [--frames 60] [--azimuth 1024] [--steps 7] [--warmup 2] [--range 1.0] [--cells 100,250,500,1000]

Window keyframes come from a synth.make_sequence drive through WindowKeyframer (leaf 0.1 m).  Edge sets: `one` = one consecutive
(odometry) edge; `flush` = all consecutive edges; `loops` = a few far-apart, low-overlap (loop-like) edges; `flush+loops` = both.
Routes, per edge set (median / min / max of --steps calls after --warmup, host clock around the synchronous call):
  (a) Engine.keyframe_fitness_scores: `first` = the first call on fresh keyframes (it builds the indexes), `resident` = later calls;
  (b) the batch route: batch_reserve + batch_set_target_keyframe / batch_set_source_keyframe + batch_build_targets +
      batch_fitness_scores(T) -- row copies and a full NDT target build the score never reads;
  (c) the host route: two keyframe_get downloads per edge + set_target / set_source / fitness_score(T) on a one-pair engine.
`identical` = routes (b) and (c) return the same words as (a).  With --cells the new call is repeated on engines with other cell sizes
(MI355NDT_OPT_KF_FITNESS_CELL_MM).  One JSON line per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lv_slam_amd import keyframes as KF  # noqa: E402
from lv_slam_amd import ndt, synth  # noqa: E402

PRM = dict(trans_epsilon=0.01, max_iterations=64)


def stats(ts):
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3))


def timed(f, warmup, steps):
    ts, out = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out = f()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--azimuth", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--range", type=float, default=1.0)
    ap.add_argument("--cells", default="100,250,500,1000")
    a = ap.parse_args()
    mr = a.range
    scans, poses = synth.make_sequence(a.frames, a.azimuth)
    scans = [s.numpy().astype(np.float32) for s in scans]
    e = ndt.Engine(ndt.default_params(**PRM))
    wk = KF.WindowKeyframer(e, delta_trans=4.0, delta_angle=0.3, leaf=0.1)
    kfs = [r for r in (wk.push(P, s, seq=k) for k, (P, s) in enumerate(zip(poses, scans))) if r is not None] + [wk.flush()]
    clouds = [e.keyframe_get(r.id) for r in kfs]
    n = len(kfs)
    rel = lambda i, j: KF.isometry_inverse(kfs[i].odom) @ kfs[j].odom
    consecutive = [(i, i + 1) for i in range(n - 1)]
    loops = [(0, n - 1), (n - 1, 0), (1, n - 2), (0, n // 2)]
    sets = {"one": consecutive[:1], "flush": consecutive, "loops": loops, "flush+loops": consecutive + loops}
    print(json.dumps(dict(keyframes=n, points=[len(c) for c in clouds], scans=[r.n_scans for r in kfs], max_range=mr)), flush=True)

    def fresh(cell_mm=None):
        g = ndt.Engine(ndt.default_params(**PRM))
        if cell_mm is not None:
            g.set_option(ndt.OPT_KF_FITNESS_CELL_MM, cell_mm)
        ids = [g.keyframe_add(c) for c in clouds]
        g.synchronize()
        return g, ids

    for name, pairs in sets.items():
        T = [rel(i, j) for i, j in pairs]
        # (a) the new call: first (indexes built) and resident
        g, ids = fresh()
        a1, a2 = [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs]
        t0 = time.perf_counter()
        got = g.keyframe_fitness_scores(a1, a2, T, mr)
        first_ms = (time.perf_counter() - t0) * 1e3
        ta, again = timed(lambda: g.keyframe_fitness_scores(a1, a2, T, mr), a.warmup, a.steps)
        same = got[0].tobytes() == again[0].tobytes()
        res_med = float(np.median(ta))
        print(json.dumps(dict(edges=name, n_edges=len(pairs), route="a:keyframe_fitness_scores", first_ms=round(first_ms, 3),
                              index_build_share=round(max(0.0, 1.0 - res_med / first_ms), 3), **stats(ta), identical=same,
                              mean_inliers=float(np.mean(got[1])))), flush=True)

        # (b) the batch route that exists today
        def route_b():
            g.batch_reserve(len(pairs), max(len(clouds[i]) for i, _ in pairs), max(len(clouds[j]) for _, j in pairs))
            for p in range(len(pairs)):
                g.batch_set_target_keyframe(p, a1[p])
                g.batch_set_source_keyframe(p, a2[p])
            g.batch_build_targets()
            return g.batch_fitness_scores(mr, T=np.stack(T).astype(np.float32))
        tb, gb = timed(route_b, a.warmup, a.steps)
        print(json.dumps(dict(edges=name, n_edges=len(pairs), route="b:batch slots + target build", **stats(tb),
                              identical=gb[0].tobytes() == got[0].tobytes() and np.array_equal(gb[1], got[1]))), flush=True)

        # (c) two downloads per edge and the one-pair surface
        single = ndt.Engine(ndt.default_params(**PRM))

        def route_c():
            out = []
            for p in range(len(pairs)):
                c1, c2 = g.keyframe_get(a1[p]), g.keyframe_get(a2[p])
                single.set_target(c1)
                single.set_source(c2)
                out.append(single.fitness_score(mr, T=T[p].astype(np.float32)))
            return out
        tc, gc = timed(route_c, min(a.warmup, 1), max(3, a.steps // 2))
        print(json.dumps(dict(edges=name, n_edges=len(pairs), route="c:keyframe_get x2 + one-pair", **stats(tc),
                              identical=all(gc[k] == (got[0][k], got[1][k]) for k in range(len(pairs))))), flush=True)
        single.close()
        g.close()

    # the cell size (flush + loops, and the loops alone: far queries walk many rings)
    for cell in [int(x) for x in a.cells.split(",") if x]:
        for name in ("flush", "loops"):
            pairs = sets[name]
            T = [rel(i, j) for i, j in pairs]
            g, ids = fresh(cell)
            a1, a2 = [ids[i] for i, _ in pairs], [ids[j] for _, j in pairs]
            t0 = time.perf_counter()
            g.keyframe_fitness_scores(a1, a2, T, mr)
            first_ms = (time.perf_counter() - t0) * 1e3
            ta, _ = timed(lambda: g.keyframe_fitness_scores(a1, a2, T, mr), a.warmup, a.steps)
            print(json.dumps(dict(cell_mm=cell, edges=name, n_edges=len(pairs), first_ms=round(first_ms, 3), **stats(ta))), flush=True)
            g.close()
    e.close()


if __name__ == "__main__":
    main()
