"""GPU box: one mi355ndt_batch_fitness_scores call against the K single-surface calls it replaces (set_target + set_source +
fitness_score per pair: one re-upload, one target build and three host syncs each), on the same clouds and the same final poses.

    python tools/fitness_batch_timing.py [--pairs 5,271] [--ranges 1.0,inf] [--steps 5] [--warmup 1] [--azimuth 1024] [--single-call]

K pairs of synth.make_pair(k, azimuth) (65,536 points per cloud at 1024) are aligned once in a batch (DIRECT7, resolution 1.0, the
nodelet's epsilon / iteration cap); then, per max_range, the batched call is timed: `first_ms` = the first call after the target
build (it builds the occupied-cell index), `batch_ms` = median of --steps calls after --warmup.  `single_ms` = median of --steps
passes over the K pairs through one single-registration engine.  `identical` = every pair's (score, inliers) equal bit for bit.
One JSON line per (K, max_range).

--single-call adds, per max_range and before the batches, one line for the one-pair surface on its own: pair 0 resident and built on a
one-pair engine, `single_first_ms` = the first Engine.fitness_score after a target build (it holds the index build), `single_call_ms` =
median of --single-steps later calls (min / max beside it); nothing is uploaded or built between the calls."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lv_slam_amd import ndt, synth  # noqa: E402


def make(n, azimuth):
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    out = []
    for b in range(0, n, 16):
        t, s, _ = synth.make_pairs(list(range(b, min(b + 16, n))), azimuth, device=dev)
        t, s = t.cpu().numpy(), s.cpu().numpy()
        out += [(t[j], s[j]) for j in range(len(t))]
    return out


def single_call(a, prm):
    (t, s), = make(1, a.azimuth)
    e = ndt.Engine(ndt.default_params(**prm))
    e.set_target(t)
    e.set_source(s)
    F = e.align(synth.default_guess())["final"]
    cells = int(np.prod(e.get_grid(0)[2].astype(np.int64)))
    for mr in [float(x) for x in a.ranges.split(",")]:
        e.set_target(t)
        e.batch_build_targets()                         # a fresh build: the first call below builds what the score reads beside the grid
        e.synchronize()
        t0 = time.perf_counter()
        got = e.fitness_score(mr, F)
        first_ms = (time.perf_counter() - t0) * 1e3
        ts = []
        for i in range(a.warmup + a.single_steps):
            t0 = time.perf_counter()
            again = e.fitness_score(mr, F)
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps(dict(K=1, points=len(t), max_range=mr if mr != float("inf") else "DBL_MAX", single_first_ms=round(first_ms, 3),
                              single_call_ms=round(float(np.median(ts)), 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3),
                              identical=again == got, score_word=np.float64(got[0]).tobytes()[::-1].hex(), inliers=got[1], grid_cells=cells)), flush=True)
    e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="5,271")
    ap.add_argument("--ranges", default="1.0,inf")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--azimuth", type=int, default=1024)
    ap.add_argument("--single-call", action="store_true")
    ap.add_argument("--single-steps", type=int, default=51)
    a = ap.parse_args()
    prm = dict(trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7)
    if a.single_call:
        single_call(a, prm)
    for K in [int(x) for x in a.pairs.split(",") if x]:
        pairs = make(K, a.azimuth)
        eng = ndt.Engine(ndt.default_params(**prm))
        eng.batch_reserve(K, max(len(t) for t, _ in pairs), max(len(s) for _, s in pairs))
        for k, (t, s) in enumerate(pairs):
            eng.batch_set_target(k, t)
            eng.batch_set_source(k, s)
        res = eng.batch_align(synth.default_guess())
        finals = [r["final"] for r in res]
        single = ndt.Engine(ndt.default_params(**prm))
        for mr in [float(x) for x in a.ranges.split(",")]:
            eng.batch_build_targets()                   # a fresh build: the first call below builds the index again
            eng.synchronize()                           # (the build is asynchronous: first_ms times the index build, not the build's tail)
            t0 = time.perf_counter()
            got = eng.batch_fitness_scores(mr)
            first_ms = (time.perf_counter() - t0) * 1e3
            tb = []
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                eng.batch_fitness_scores(mr)
                if i >= a.warmup:
                    tb.append((time.perf_counter() - t0) * 1e3)
            ts, want = [], None
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                out = []
                for (t, s), F in zip(pairs, finals):
                    single.set_target(t)
                    single.set_source(s)
                    out.append(single.fitness_score(mr, F))
                if i >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
                want = out
            identical = all((got[0][k], got[1][k]) == want[k] for k in range(K))
            bm, sm = float(np.median(tb)), float(np.median(ts))
            print(json.dumps(dict(K=K, points=len(pairs[0][0]), max_range=mr if mr != float("inf") else "DBL_MAX", first_ms=round(first_ms, 3),
                                  batch_ms=round(bm, 3), single_ms=round(sm, 3), speedup=round(sm / bm, 2), identical=identical,
                                  mean_inliers=float(np.mean(got[1])), mean_score=float(np.mean(got[0][got[1] > 0])) if np.any(got[1] > 0) else None)),
                  flush=True)
        single.close()
        eng.close()


if __name__ == "__main__":
    main()
