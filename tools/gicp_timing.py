"""GPU box: the GICP surface (mi355ndt_gicp_*) against the restatement's stages on one CPU thread.

    python tools/gicp_timing.py [--azimuth 64,256] [--steps 5] [--warmup 1] [--pair 0] [--no-cpu]

Clouds are synth.make_pair(pair, azimuth) (64 beams: 4,096 / 16,384 points), factory parameters (registrations.cpp:47-51).  One JSON line each
(median / min / max of --steps calls after --warmup, host clock around the synchronous calls):
  covariances     gicp_set_target + gicp_covariances(fetch=False): upload, index build and k_gc_cov of one cloud
  covariances_k64 the same with k_correspondences = 64 (the CAP 64 instantiation)
  correspondences one pass of the matching loop with both clouds' covariances resident (results not fetched by the align; fetched here)
  cost            one evaluation of the thirteen sums (two launches, one wait)
  align           gicp_align from default_guess() with the covariances resident, and its outer iterations
  align_cold      set both clouds, then align: what a loop candidate costs when neither cloud has been seen
  cpu_*           tools/gicp_ref.py's covariances / correspondences / cost / align, one call each, on one thread (--no-cpu skips them)"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lv_slam_amd import ndt, synth  # noqa: E402

spec = importlib.util.spec_from_file_location("gicp_ref", os.path.join(ROOT, "tools", "gicp_ref.py"))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)


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
    ap.add_argument("--azimuth", default="64,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pair", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    G = synth.default_guess()
    I4 = np.eye(4, dtype=np.float32)
    prm = {k: R.FACTORY[k] for k in R.DEFAULTS}
    for az in [int(x) for x in a.azimuth.split(",") if x]:
        tgt, src, _ = synth.make_pair(a.pair, az)
        tgt, src = tgt.numpy(), src.numpy()
        row = dict(azimuth=az, points=len(tgt))
        e = ndt.Engine()
        for name, k in (("covariances", 20), ("covariances_k64", 64)):
            e.gicp_set_params(ndt.default_gicp_params(**dict(prm, k_correspondences=k)))

            def cov():
                e.gicp_set_target(tgt)
                e.gicp_covariances(ndt.GICP_TARGET, fetch=False)
            ts, _ = timed(cov, a.warmup, a.steps)
            print(json.dumps(dict(row, stage=name, **stats(ts))), flush=True)
        e.gicp_set_params(ndt.default_gicp_params(**prm))
        e.gicp_set_target(tgt)
        e.gicp_set_source(src)
        e.gicp_covariances(ndt.GICP_TARGET, fetch=False)
        e.gicp_covariances(ndt.GICP_SOURCE, fetch=False)
        ts, (idx, M, m) = timed(lambda: e.gicp_correspondences(G), a.warmup, a.steps)
        print(json.dumps(dict(row, stage="correspondences", matched=m, **stats(ts))), flush=True)
        ts, _ = timed(lambda: e.gicp_cost([0.0] * 6, G), a.warmup, 10 * a.steps)
        print(json.dumps(dict(row, stage="cost", **stats(ts))), flush=True)
        ts, r = timed(lambda: e.gicp_align(G), a.warmup, a.steps)
        print(json.dumps(dict(row, stage="align", iterations=r["iterations"], converged=r["converged"], **stats(ts))), flush=True)

        def cold():
            e.gicp_set_target(tgt)
            e.gicp_set_source(src)
            return e.gicp_align(G)
        ts, _ = timed(cold, a.warmup, a.steps)
        print(json.dumps(dict(row, stage="align_cold", **stats(ts))), flush=True)
        if not a.no_cpu:
            cs, ct = e.gicp_covariances(ndt.GICP_SOURCE), e.gicp_covariances(ndt.GICP_TARGET)
            for name, f in (("cpu_covariances", lambda: R.covariances(tgt, 20, 1e-3)),
                            ("cpu_correspondences", lambda: R.correspondences(src, tgt, cs, ct, G, I4, 5.0)),
                            ("cpu_cost", lambda: R.cost(src, tgt, idx, M, [0.0] * 6, G)),
                            ("cpu_align", lambda: R.align(src, tgt, G, prm, cov_src=cs, cov_tgt=ct))):
                ts, _ = timed(f, 0, 1)
                print(json.dumps(dict(row, stage=name, **stats(ts))), flush=True)
        e.close()


if __name__ == "__main__":
    main()
