"""GPU box: what the prefilter's two options cost -- batch_prefilter with VOXELGRID and with APPROX_VOXELGRID, the vertical-angle calibration
off and on, over the raw scans of tools/batch_prefilter_timing.py.

    python tools/prefilter_options_timing.py [--pairs 64] [--azimuth 2048] [--steps 15] [--warmup 3]

Clouds are the targets and sources of synth.make_pair(k, azimuth) (azimuth * 64 raw points a scan); the prefilter is the odometry's (0.5 .. 100 m,
0.1 m).  The slots are reserved for the raw counts: the approximate grid may emit a point per input point.  One JSON line per leg: median / min /
max of --steps calls after --warmup (host clock around the synchronous call, staging of the raw scans included, as the call is used; the four
legs alternate call by call) and the mean filtered counts of the targets and of the sources."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lv_slam_amd import ndt, synth  # noqa: E402

PF = dict(distance_near=0.5, distance_far=100.0, downsample_resolution=0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    raw = []
    for k in range(a.pairs):
        t, s, _ = synth.make_pair(k, a.azimuth, device="cuda")
        raw.append((np.ascontiguousarray(t.cpu().numpy()), np.ascontiguousarray(s.cpu().numpy())))
    tg, sr = [p[0] for p in raw], [p[1] for p in raw]
    n_raw = len(tg[0])
    eng = ndt.Engine(ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT1, variant=ndt.VARIANT_PCA))
    eng.batch_reserve(a.pairs, n_raw, n_raw)
    legs = [dict(PF, downsample_method=m, angle_calibration=c) for m in ("VOXELGRID", "APPROX_VOXELGRID") for c in (False, True)]
    ts, counts = [[] for _ in legs], [None] * len(legs)
    for i in range(a.warmup + a.steps):              # the legs alternate: a drift of the host or the card touches all four alike
        for j, kw in enumerate(legs):
            t0 = time.perf_counter()
            counts[j] = eng.batch_prefilter(tg, sr, **kw)
            if i >= a.warmup:
                ts[j].append((time.perf_counter() - t0) * 1e3)
    for kw, t, c in zip(legs, ts, counts):
        med = float(np.median(t))
        print(json.dumps(dict(pairs=a.pairs, raw_points=n_raw, downsample_method=kw["downsample_method"], angle_calibration=kw["angle_calibration"],
                              batch_prefilter_median_ms=round(med, 3), min_ms=round(float(np.min(t)), 3), max_ms=round(float(np.max(t)), 3),
                              clouds_per_s=round(2 * a.pairs / med * 1e3, 1), filtered_points=[int(np.mean(c[0])), int(np.mean(c[1]))])), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
