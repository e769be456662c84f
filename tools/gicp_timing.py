"""GPU box: the GICP surface (mi355ndt_gicp_*) against the restatement's stages on one CPU thread.

    python tools/gicp_timing.py [--azimuth 64,256] [--steps 5] [--warmup 1] [--pair 0] [--no-cpu] [--batch 1,2,5,16 [--baseline-lib PATH]]

Clouds are synth.make_pair(pair, azimuth) (64 beams: 4,096 / 16,384 points), factory parameters (registrations.cpp:47-51).  One JSON line each
(median / min / max of --steps calls after --warmup, host clock around the synchronous calls):
  covariances     gicp_set_target + gicp_covariances(fetch=False): upload, index build and k_gc_cov of one cloud
  covariances_k64 the same with k_correspondences = 64 (the CAP 64 instantiation)
  correspondences one pass of the matching loop with both clouds' covariances resident (results not fetched by the align; fetched here)
  cost            one evaluation of the thirteen sums (two launches, one wait)
  align           gicp_align from default_guess() with the covariances resident, and its outer iterations
  align_cold      set both clouds, then align: what a loop candidate costs when neither cloud has been seen
  cpu_*           tools/gicp_ref.py's covariances / correspondences / cost / align, one call each, on one thread (--no-cpu skips them)
--batch K,...: only the loop check.  The K candidates are the source under K small rigid motions, resident keyframes with their covariances
computed; one line per K, medians of --steps alternating repetitions:
  sequential_ms   K x (gicp_set_source(keyframe) + gicp_align), one candidate after the other
  batch_ms        K x gicp_batch_set_source(keyframe) + ONE gicp_batch_align, with its rounds and the sum of the slots' requests; every slot's
                  final transformation is compared with its sequential one (equal_bytes)
  baseline_ms     the sequential loop through another build of the library (--baseline-lib, e.g. the parent commit's), in the same run"""
import argparse
import ctypes as C
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


SINGLE_PAIR_CALLS = ("mi355ndt_create", "mi355ndt_destroy", "mi355ndt_last_error", "mi355ndt_keyframe_add", "mi355ndt_keyframe_get",
                     "mi355ndt_gicp_set_params", "mi355ndt_gicp_set_target", "mi355ndt_gicp_set_source", "mi355ndt_gicp_set_target_keyframe",
                     "mi355ndt_gicp_set_source_keyframe", "mi355ndt_gicp_covariances", "mi355ndt_gicp_align")


def engine_over(path):
    """an Engine over another build of the library, for the calls the sequential loop makes (the build need not have the batch calls)"""
    ours, L = ndt.load_library(), C.CDLL(path)
    for name in SINGLE_PAIR_CALLS:
        f, g = getattr(L, name), getattr(ours, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    e = ndt.Engine.__new__(ndt.Engine)
    e.lib, e.h, e._keep, e._gicp_n, e._gicp_batch_n = L, C.c_void_p(), [], [0, 0], []
    rc = L.mi355ndt_create(None, 0, C.byref(e.h))
    if rc != ndt.OK:
        raise ndt.NDTError(rc, "mi355ndt_create")
    return e


def candidates(src, G, K):
    """the source under K small rigid motions, each with the guess that undoes it"""
    out = []
    for k in range(K):
        D = np.eye(4)
        D[:3, :3] = synth.rot_zyx(0.001 * (k % 5), -0.0015 * (k % 3), 0.002 * (k % 7))
        D[:3, 3] = [0.02 * (k % 4), -0.01 * (k % 6), 0.005 * (k % 3)]
        Gk = (G.astype(np.float64) @ np.linalg.inv(D)).astype(np.float32)
        Gk[3] = [0, 0, 0, 1]
        out.append((R.move_f32(D.astype(np.float32), src), Gk))
    return out


def loop_check(a, prm, az, Ks):
    tgt, src, _ = synth.make_pair(a.pair, az)
    tgt, src = tgt.numpy(), src.numpy()
    G = synth.default_guess()
    engines = [ndt.Engine()] + ([engine_over(a.baseline_lib)] if a.baseline_lib else [])
    cand = candidates(src, G, max(Ks))
    ids = []
    for e in engines:                               # every cloud resident, its index built and its covariances computed
        e.gicp_set_params(ndt.default_gicp_params(**prm))
        kt = e.keyframe_add(tgt)
        e.gicp_set_target(keyframe=kt)
        e.gicp_covariances(ndt.GICP_TARGET, fetch=False)
        ids.append([e.keyframe_add(c) for c, _ in cand])
        for i in ids[-1]:
            e.gicp_set_source(keyframe=i)
            e.gicp_covariances(ndt.GICP_SOURCE, fetch=False)

    def sequential(e, kid, K):
        out = []
        for k in range(K):
            e.gicp_set_source(keyframe=kid[k])
            out.append(e.gicp_align(cand[k][1]))
        return out

    def batch(K):
        e = engines[0]
        e.gicp_batch_reserve(K)
        for k in range(K):
            e.gicp_batch_set_source(k, keyframe=ids[0][k])
        return e.gicp_batch_align(np.stack([g for _, g in cand[:K]]))
    for K in Ks:
        ts = {"sequential_ms": [], "batch_ms": [], "baseline_ms": []}
        for i in range(a.warmup + a.steps):          # the three alternate inside every repetition
            t0 = time.perf_counter()
            seq = sequential(engines[0], ids[0], K)
            t1 = time.perf_counter()
            bat = batch(K)
            t2 = time.perf_counter()
            if a.baseline_lib:
                base = sequential(engines[1], ids[1], K)
            t3 = time.perf_counter()
            if i >= a.warmup:
                ts["sequential_ms"].append((t1 - t0) * 1e3); ts["batch_ms"].append((t2 - t1) * 1e3); ts["baseline_ms"].append((t3 - t2) * 1e3)
        rounds, req = engines[0].gicp_batch_stats()
        equal = all(b["final"].tobytes() == s["final"].tobytes() and b["iterations"] == s["iterations"] for b, s in zip(bat, seq))
        row = dict(azimuth=az, points=len(src), stage="batch", K=K, rounds=rounds, requests_sum=int(req.sum()), equal_bytes=equal,
                   iterations=[r["iterations"] for r in bat])
        for name, v in ts.items():
            if name != "baseline_ms" or a.baseline_lib:
                row[name] = round(float(np.median(v)), 3)
        if a.baseline_lib:
            row["baseline_equal_bytes"] = all(b["final"].tobytes() == s["final"].tobytes() for b, s in zip(base, seq))
        row["batch_ms_per_round"] = round(row["batch_ms"] / max(rounds, 1), 4)
        print(json.dumps(row), flush=True)
    for e in engines:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="", help="K,...: time the loop check (K sequential aligns against one batch align) and nothing else")
    ap.add_argument("--baseline-lib", default="", help="another build of libmi355ndt.so for the sequential baseline of --batch")
    ap.add_argument("--azimuth", default="64,256")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pair", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    G = synth.default_guess()
    I4 = np.eye(4, dtype=np.float32)
    prm = {k: R.FACTORY[k] for k in R.DEFAULTS}
    if a.batch:
        for az in [int(x) for x in a.azimuth.split(",") if x]:
            loop_check(a, prm, az, [int(x) for x in a.batch.split(",") if x])
        return
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
