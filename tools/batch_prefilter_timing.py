"""GPU box: raw scans into registrations -- the batch prefilter against the single surface, on the workload of `bench.py --prefiltered`.

    python tools/batch_prefilter_timing.py [--pairs 64] [--azimuth 2048] [--frames 64] [--steps 5] [--warmup 2] [--arith 0] [--outliers]

Pairs are synth.make_pair(k, azimuth) (azimuth * 64 raw points a scan), registered with ndt_pca, DIRECT1, 1.0 m, eps 0.01, 64 iterations, from
synth.default_guess(); the prefilter is the odometry's (0.5 .. 100 m, 0.1 m).  One JSON line per route (median / min / max of --steps runs after
--warmup, host clock around synchronous calls; registrations/s from the median):
  a          what the single surface offers: per cloud prefilter(fetch=False) + use_prefiltered, one align at a time (latency mode on)
  b          batch_prefilter + batch_build_targets + batch_align over all pairs, with the time of batch_prefilter alone beside it
  seq_host   per frame prefilter(fetch=True), then sequence_run over the downloaded clouds
  seq_raw    sequence_run_raw over the raw frames
`identical`: route b's result records equal route a's finals, iterations and scores when route a aligns with the batch align's work items (latency
mode off; the timed route a runs in latency mode as `bench.py --prefiltered` does, whose finer work items sum in another order:
max_abs_diff_to_latency_mode is the largest difference of a final-transformation entry to that run).  seq_raw: its frame records equal
seq_host's, as bytes.

--outliers: the nodelet's three stages (STATISTICAL, mean_k 20, stddev_mul 1.0) in place of the legs above:
  o_host     the route without the batch stage: per cloud prefilter(outlier={}) with the survivors downloaded, batch_set_clouds, build, align
  o_batch    batch_prefilter + batch_remove_outliers + batch_build_targets + batch_align, with the time of batch_remove_outliers alone beside it;
             `identical`: its result records equal o_host's, as bytes
  o_one      batch_remove_outliers over a batch of ONE filtered scan against one prefilter_outliers call on the same cloud (the stage alone is
             timed: the upload and the prefilter in front of it are not); slower_by_ms against the single call's own max - min spread
  o_raw      batch_remove_outliers over one scan that was NOT down-sampled (the longest serial chain of the statistics kernel); the kernel's own
             time comes from a kernel trace of this leg (rocprofv3 --kernel-trace --stats -- python tools/batch_prefilter_timing.py --outliers --pairs 0)"""
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


def stats(ts, n):
    med = float(np.median(ts))
    return dict(median_ms=round(med, 3), min_ms=round(float(np.min(ts)), 3), max_ms=round(float(np.max(ts)), 3), per_s=round(n / med * 1e3, 1))


def timed(f, warmup, steps):
    ts, out = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out = f()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts, out


def outliers_leg(a):
    prm = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT1, variant=ndt.VARIANT_PCA)
    G = synth.default_guess()
    steps = max(a.steps, 5)
    if a.pairs > 0:
        raw = []
        for k in range(a.pairs):
            t, s, _ = synth.make_pair(k, a.azimuth, device="cuda")
            raw.append((np.ascontiguousarray(t.cpu().numpy()), np.ascontiguousarray(s.cpu().numpy())))
        tg, sr = [p[0] for p in raw], [p[1] for p in raw]
        row = dict(pairs=a.pairs, raw_points=len(raw[0][0]), arith=a.arith, outlier="STATISTICAL 20 1.0")
        gc = np.ascontiguousarray(np.broadcast_to(G.T.reshape(1, 16), (a.pairs, 16)))
        # slot sizes: the filtered counts, learnt from a first call into slots of the raw size
        eb = ndt.Engine(ndt.default_params(**prm))
        eb.set_option(ndt.OPT_ARITH, a.arith)
        eb.batch_reserve(a.pairs, len(raw[0][0]), len(raw[0][0]))
        tc, sc = eb.batch_prefilter(tg, sr, **PF)
        cap_t, cap_s = (max(tc) + 4095) // 4096 * 4096, (max(sc) + 4095) // 4096 * 4096
        eh = ndt.Engine(ndt.default_params(**prm))
        eh.set_option(ndt.OPT_ARITH, a.arith)
        eh.batch_reserve(a.pairs, cap_t, cap_s)
        res_h, res_b = (ndt.Result * a.pairs)(), (ndt.Result * a.pairs)()

        def o_host():
            ft = [eh.prefilter(c, outlier={}, **PF) for c in tg]
            fs = [eh.prefilter(c, outlier={}, **PF) for c in sr]
            eh.batch_set_clouds_raw(0, [c.ctypes.data for c in ft], [len(c) for c in ft], [c.ctypes.data for c in fs], [len(c) for c in fs], 12)
            eh.batch_build_targets()
            eh.batch_align_raw(gc, res_h)
            return ft, fs
        th, (ft, fs) = timed(o_host, a.warmup, steps)
        print(json.dumps(dict(row, route="o_host: per cloud prefilter(outlier={}) downloaded + batch_set_clouds + build + align", **stats(th, a.pairs))), flush=True)
        eh.close()
        eb.batch_reserve(a.pairs, cap_t, cap_s)
        t_ol = []

        def o_batch():
            eb.batch_prefilter(tg, sr, **PF)
            t0 = time.perf_counter()
            out = eb.batch_remove_outliers()
            t_ol.append((time.perf_counter() - t0) * 1e3)
            eb.batch_build_targets()
            eb.batch_align_raw(gc, res_b)
            return out
        tb, (oc_t, oc_s) = timed(o_batch, a.warmup, steps)
        print(json.dumps(dict(row, route="o_batch: batch_prefilter + batch_remove_outliers + batch_build_targets + batch_align",
                              identical=bytes(res_b) == bytes(res_h) and oc_t == [len(c) for c in ft] and oc_s == [len(c) for c in fs],
                              filtered_points=[int(np.mean(tc)), int(np.mean(sc))], surviving_points=[int(np.mean(oc_t)), int(np.mean(oc_s))],
                              batch_remove_outliers_median_ms=round(float(np.median(t_ol[a.warmup:])), 3), **stats(tb, a.pairs))), flush=True)
        eb.close()
    # a batch of one against one call of the single surface, the stage alone
    scan = np.ascontiguousarray(synth.make_pair(0, a.azimuth, device="cuda")[0].cpu().numpy())
    e1 = ndt.Engine(ndt.default_params(**prm))
    for leg, pf in (("o_one", PF), ("o_raw", dict(PF, downsample_resolution=0.0))):
        filtered = e1.prefilter(scan, **pf)
        e1.batch_reserve(1, len(scan), 64)
        ts, tb1, kept = [], [], None
        for i in range(a.warmup + steps):
            e1.prefilter(scan, fetch=False, **pf)
            t0 = time.perf_counter()
            m = e1.prefilter_outliers(fetch=False)
            t1 = time.perf_counter()
            e1.batch_set_clouds_raw(0, [filtered.ctypes.data], [len(filtered)], None, None, 12)
            e1.synchronize()
            t2 = time.perf_counter()
            tc1, _ = e1.batch_remove_outliers(sources=False)
            t3 = time.perf_counter()
            assert tc1 == [m], (tc1, m)
            kept = m
            if i >= a.warmup:
                ts.append((t1 - t0) * 1e3)
                tb1.append((t3 - t2) * 1e3)
        spread = float(np.max(ts) - np.min(ts))
        slower = float(np.median(tb1) - np.median(ts))
        print(json.dumps(dict(route=f"{leg}: batch_remove_outliers over one cloud against one prefilter_outliers call", points=len(filtered), kept=kept,
                              down_sampled=pf["downsample_resolution"] > 0, single=stats(ts, 1), batch_of_one=stats(tb1, 1),
                              single_spread_ms=round(spread, 3), slower_by_ms=round(slower, 3), slower_than_the_spread=bool(slower > spread))), flush=True)
    e1.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arith", type=int, default=0)
    ap.add_argument("--outliers", action="store_true")
    a = ap.parse_args()
    if a.outliers:
        return outliers_leg(a)
    prm = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT1, variant=ndt.VARIANT_PCA)
    G = synth.default_guess()
    if a.pairs > 0:
        raw = []
        for k in range(a.pairs):
            t, s, _ = synth.make_pair(k, a.azimuth, device="cuda")
            raw.append((np.ascontiguousarray(t.cpu().numpy()), np.ascontiguousarray(s.cpu().numpy())))
        row = dict(pairs=a.pairs, raw_points=len(raw[0][0]), arith=a.arith)
        # route a
        ea = ndt.Engine(ndt.default_params(**prm))
        ea.set_option(ndt.OPT_ARITH, a.arith)
        ea.set_latency_mode(True)

        def route_a():
            out = []
            for tg, sr in raw:
                ea.prefilter(tg, fetch=False, **PF)
                ea.use_prefiltered(as_target=True)
                ea.prefilter(sr, fetch=False, **PF)
                ea.use_prefiltered(as_target=False)
                out.append(ea.align(G))
            return out
        ta, ra = timed(route_a, a.warmup, a.steps)
        print(json.dumps(dict(row, route="a: per cloud prefilter(fetch=False) + use_prefiltered, one align at a time", **stats(ta, a.pairs))), flush=True)
        ea.set_latency_mode(False)                   # (untimed: the batch align's work items, for the identity check below)
        ra_batch_items = route_a()
        ea.close()
        # route b: the slots are reserved for the filtered clouds (learnt from a first call into slots of the raw size)
        eb = ndt.Engine(ndt.default_params(**prm))
        eb.set_option(ndt.OPT_ARITH, a.arith)
        tg, sr = [p[0] for p in raw], [p[1] for p in raw]
        eb.batch_reserve(a.pairs, len(raw[0][0]), len(raw[0][0]))
        tc, sc = eb.batch_prefilter(tg, sr, **PF)
        cap_t, cap_s = (max(tc) + 4095) // 4096 * 4096, (max(sc) + 4095) // 4096 * 4096
        eb.batch_reserve(a.pairs, cap_t, cap_s)
        gc = np.ascontiguousarray(np.broadcast_to(G.T.reshape(1, 16), (a.pairs, 16)))
        res = (ndt.Result * a.pairs)()
        t_pf = []

        def route_b():
            t0 = time.perf_counter()
            eb.batch_prefilter(tg, sr, **PF)
            t_pf.append((time.perf_counter() - t0) * 1e3)
            eb.batch_build_targets()
            eb.batch_align_raw(gc, res)
            return res
        tb, _ = timed(route_b, a.warmup, a.steps)
        finals = [np.array(r.final_colmajor, np.float32).reshape(4, 4).T for r in res]
        same = all(np.array_equal(f, x["final"]) and r.iterations == x["iterations"] and r.score == x["score"] for f, r, x in zip(finals, res, ra_batch_items))
        drift = max(float(np.abs(f.astype(np.float64) - x["final"]).max()) for f, x in zip(finals, ra))
        print(json.dumps(dict(row, route="b: batch_prefilter + batch_build_targets + batch_align", identical=bool(same), max_abs_diff_to_latency_mode=drift, slot_points=[cap_t, cap_s],
                              filtered_points=[int(np.mean(tc)), int(np.mean(sc))], batch_prefilter_median_ms=round(float(np.median(t_pf[a.warmup:])), 3),
                              **stats(tb, a.pairs))), flush=True)
        eb.close()
    if a.frames > 0:
        scans = [np.ascontiguousarray(s.cpu().numpy()) for s in synth.make_sequence(a.frames, a.azimuth, device="cuda")[0]]
        stamps = [0.1 * k for k in range(a.frames)]
        row = dict(frames=a.frames, raw_points=len(scans[0]), arith=a.arith)
        eh = ndt.Engine(ndt.default_params(**prm))
        eh.set_option(ndt.OPT_ARITH, a.arith)

        def seq_host():
            return eh.sequence_run([eh.prefilter(s, **PF) for s in scans], stamps, raw_records=True)
        th, ((fh, _), sh) = timed(seq_host, a.warmup, a.steps)
        print(json.dumps(dict(row, route="seq_host: per frame prefilter(fetch=True), then sequence_run", last_stats=sh, **stats(th, a.frames))), flush=True)
        eh.close()
        er = ndt.Engine(ndt.default_params(**prm))
        er.set_option(ndt.OPT_ARITH, a.arith)
        tr, ((fr, _), sr_, _) = timed(lambda: er.sequence_run_raw(scans, stamps, raw_records=True, **PF), a.warmup, a.steps)
        print(json.dumps(dict(row, route="seq_raw: sequence_run_raw", identical=bytes(fr) == bytes(fh), last_stats=sr_, **stats(tr, a.frames))), flush=True)
        er.close()


if __name__ == "__main__":
    main()
