"""GPU box: outlier removal over the resident prefilter result against what a host has to do without it.

    python tools/outlier_timing.py [--azimuth 512,1024,2048] [--steps 7] [--warmup 2] [--cells 50,100,200,400,800] [--kernel-stats]

Scans are synth.make_pair sources, prefiltered as the odometry sees them (distance filter 0.5 .. 100 m, 0.1 m down-sampling).  Per size, one
JSON line each (median / min / max of --steps calls after --warmup, host clock around the synchronous calls):
  new           prefilter(fetch=False) + prefilter_outliers(fetch=False), and prefilter(fetch=False) alone: the difference is the new stage,
                for STATISTICAL 20 / 1.0 and RADIUS 0.5 / 5
  host          what a host does today: prefilter(fetch=True), an exact k-NN on the CPU (scipy's cKDTree on 16 threads when scipy is there --
                its distances are f64, so it stands for the cost, not for the words -- else tools/outlier_ref.py), and a new upload (set_source)
  cells         the new STATISTICAL call with other values of MI355NDT_OPT_OUTLIER_CELL_MM
`identical` = the survivors equal tools/outlier_ref.py's, word for word (sizes up to --check-max points).
--kernel-stats runs the STATISTICAL calls of the largest size once more in a child process under `rocprofv3 --kernel-trace --stats` and prints the
share of the index build (k_kfi_*, k_minmax, k_rs_*, k_fit_*) and of k_ol_knn in the kernel time."""
import argparse
import csv
import glob
import importlib.util
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lv_slam_amd import ndt, synth  # noqa: E402

spec = importlib.util.spec_from_file_location("outlier_ref", os.path.join(ROOT, "tools", "outlier_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)

STAT = dict(method="STATISTICAL", mean_k=20, stddev_mul=1.0)
RAD = dict(method="RADIUS", radius=0.5, min_neighbors=5)


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


def cpu_knn(cloud, k):
    """mean distance to the k nearest others, exact, on the CPU"""
    try:
        from scipy.spatial import cKDTree
        d, _ = cKDTree(cloud).query(cloud, k + 1, workers=16)
        return "scipy cKDTree, 16 workers", d[:, 1:].mean(axis=1)
    except ImportError:
        return "tools/outlier_ref.py", R.mean_distances(cloud, k)[0]


def profile_child(azimuth):
    scan = synth.make_pair(0, azimuth)[1].numpy()
    e = ndt.Engine()
    for _ in range(5):
        e.prefilter(scan, fetch=False)
        e.prefilter_outliers(fetch=False, **STAT)
    e.close()


def kernel_stats(azimuth):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--profile-child", str(azimuth)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            print(json.dumps(dict(kernel_stats="no kernel_stats.csv written")), flush=True)
            return
        tot, build, knn, pre = 0.0, 0.0, 0.0, 0.0
        for row in csv.DictReader(open(files[0])):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            tot += ns
            if name.startswith(("k_pfb_", "k_deint")):          # (the prefilter's own kernels; its sort passes count with the index build's)
                pre += ns
            elif name.startswith(("k_kfi_", "k_minmax", "k_rs_", "k_fit_")):
                build += ns
            elif name.startswith("k_ol_knn"):
                knn += ns
        print(json.dumps(dict(kernel_stats=os.path.basename(files[0]), azimuth=azimuth, kernel_ms_per_call=round(tot / 5e6, 3),
                              index_build_share=round(build / tot, 3), knn_share=round(knn / tot, 3), prefilter_share=round(pre / tot, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--azimuth", default="512,1024,2048")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cells", default="50,100,200,400,800")
    ap.add_argument("--check-max", type=int, default=40000)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--profile-child", type=int, default=0)
    a = ap.parse_args()
    if a.profile_child:
        return profile_child(a.profile_child)
    sizes = [int(x) for x in a.azimuth.split(",") if x]
    for az in sizes:
        scan = synth.make_pair(0, az)[1].numpy()
        e = ndt.Engine()
        pre = e.prefilter(scan)
        row = dict(azimuth=az, scan_points=len(scan), prefiltered_points=len(pre))
        t0, _ = timed(lambda: e.prefilter(scan, fetch=False), a.warmup, a.steps)
        print(json.dumps(dict(row, route="prefilter(fetch=False) alone", **stats(t0))), flush=True)
        for name, kw in (("STATISTICAL 20 / 1.0", STAT), ("RADIUS 0.5 / 5", RAD)):
            def new():
                e.prefilter(scan, fetch=False)
                return e.prefilter_outliers(fetch=False, **kw)
            ts, n = timed(new, a.warmup, a.steps)
            same = None
            if len(pre) <= a.check_max:
                x = R.statistical(pre, 20, 1.0) if kw is STAT else R.radius(pre, 0.5, 5)
                same = e.prefilter(scan, outlier=kw).tobytes() == pre[x["kept"]].tobytes()
            print(json.dumps(dict(row, route="new: prefilter + prefilter_outliers, " + name, kept=n, identical=same,
                                  stage_median_ms=round(float(np.median(ts) - np.median(t0)), 3), **stats(ts))), flush=True)

        def host():
            c = e.prefilter(scan)
            who, d = cpu_knn(c, 20)
            keep = d <= d.mean() + d.std(ddof=1)
            e.set_source(c[keep])
            e.synchronize()
            return who
        ts, who = timed(host, 1, max(3, a.steps // 2))
        print(json.dumps(dict(row, route="host: prefilter(fetch=True) + " + who + " + set_source", **stats(ts))), flush=True)
        e.close()
        for cell in [int(x) for x in a.cells.split(",") if x]:
            g = ndt.Engine()
            g.set_option(ndt.OPT_OUTLIER_CELL_MM, cell)

            def swept():
                g.prefilter(scan, fetch=False)
                return g.prefilter_outliers(fetch=False, **STAT)
            ts, _ = timed(swept, a.warmup, a.steps)
            tr, _ = timed(lambda: (g.prefilter(scan, fetch=False), g.prefilter_outliers(fetch=False, **RAD)), a.warmup, a.steps)
            print(json.dumps(dict(row, cell_mm=cell, statistical=stats(ts), radius=stats(tr))), flush=True)
            g.close()
    if a.kernel_stats:
        kernel_stats(sizes[-1])


if __name__ == "__main__":
    main()
