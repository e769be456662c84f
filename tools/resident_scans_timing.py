"""GPU box: a drive of raw PointXYZI scans into window keyframes -- the resident chain against the route a host has without it -- and the
xyz-only prefilter surfaces at this commit against a library built from the parent commit.

    python tools/resident_scans_timing.py [--frames 64] [--azimuth 2048] [--steps 5] [--warmup 2] [--parent-root DIR]

Frames are synth.make_sequence(frames, azimuth) (azimuth * 64 = 131,072 raw points a scan at the default), each with a fourth column of
intensities; the prefilter is the odometry's (0.5 .. 100 m, 0.1 m), the window policy the global graph's defaults at leaf 0.1.  One JSON
line per leg (median / min / max of --steps runs after --warmup, host clock around synchronous calls):
  a   sequence_run_raw(intensity=True) -> keyframe_from_slot per frame -> WindowKeyframer over ids: each point crosses PCIe once, raw
  b   the route without resident scans: sequence_run_raw -> batch_get_cloud per frame -> WindowKeyframer over the host arrays (window_keyframe
      uploads them again); this route has no intensity.  `identical`: its keyframes' x, y, z equal leg a's, as words
  c   batch_prefilter over the frames, xyz only: this tree and, with --parent-root (a checkout of the parent commit with its library
      built), the parent's package and library, each in a child process of its own, alternating, `--repeats` runs of each: the medians
      and the spread between repeated runs of one library
  d   the same for batch_remove_outliers (STATISTICAL, mean_k 20, 1.0) over the slots leg c filled"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                          # (a child of legs c and d: the package of another checkout)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)

PF = dict(distance_near=0.5, distance_far=100.0, downsample_resolution=0.1)
PRM = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=3, variant=1)


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


def frames_xyzi(n, azimuth):
    from lv_slam_amd import synth
    scans, _ = synth.make_sequence(n, azimuth, device="cuda")
    rng = np.random.default_rng(1)
    return [np.ascontiguousarray(np.concatenate([s.cpu().numpy().astype(np.float32), rng.uniform(0, 255, (len(s), 1)).astype(np.float32)], axis=1))
            for s in scans]


def xyz_child(a):
    """legs c and d in this process, with the package and library of --root: one JSON line"""
    from lv_slam_amd import ndt
    raw = [np.ascontiguousarray(r[:, :3]) for r in frames_xyzi(a.frames, a.azimuth)]
    e = ndt.Engine(ndt.default_params(**PRM))
    e.batch_reserve(a.frames, len(raw[0]), 64)
    tc, _ = timed(lambda: e.batch_prefilter(raw, None, **PF), a.warmup, a.steps)
    t_ol = []
    for i in range(a.warmup + a.steps):
        e.batch_prefilter(raw, None, **PF)
        t0 = time.perf_counter()
        e.batch_remove_outliers(sources=False)
        if i >= a.warmup:
            t_ol.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(lib=ndt.LIB_PATH, batch_prefilter=stats(tc), batch_remove_outliers=stats(t_ol))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--azimuth", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=None)
    ap.add_argument("--xyz-child", action="store_true")
    a = ap.parse_args()
    if a.xyz_child:
        return xyz_child(a)
    from lv_slam_amd import keyframes as KF
    from lv_slam_amd import ndt
    recs = frames_xyzi(a.frames, a.azimuth)
    xyz = [np.ascontiguousarray(r[:, :3]) for r in recs]
    stamps = [0.1 * k for k in range(a.frames)]
    row = dict(frames=a.frames, raw_points=len(recs[0]))
    e = ndt.Engine(ndt.default_params(**PRM))

    def close_all(wk, scans, frames):
        out = [wk.push(f["odom"], s) for f, s in zip(frames, scans)] + [wk.flush()]
        return [r for r in out if r is not None]

    def leg_a():
        frames, _, _ = e.sequence_run_raw(recs, stamps, intensity=True, **PF)
        ids = [e.keyframe_from_slot(k, True) for k in range(a.frames)]
        return close_all(KF.WindowKeyframer(e, leaf=0.1, intensity=True), ids, frames)

    def leg_b():
        frames, _, _ = e.sequence_run_raw(xyz, stamps, **PF)
        host = [e.batch_get_cloud(k, True) for k in range(a.frames)]
        return close_all(KF.WindowKeyframer(e, leaf=0.1), host, frames)

    def release(keys):
        for r in keys:
            e.keyframe_release(r.id)

    ta, tb, ka, kb = [], [], None, None
    for i in range(a.warmup + a.steps):
        for leg, ts in ((leg_a, ta), (leg_b, tb)):
            t0 = time.perf_counter()
            keys = leg()
            e.synchronize()
            if i >= a.warmup:
                ts.append((time.perf_counter() - t0) * 1e3)
            if i == a.warmup + a.steps - 1:
                ka, kb = (keys, kb) if leg is leg_a else (ka, keys)
            else:
                release(keys)
    same = len(ka) == len(kb) and all(e.keyframe_get(x.id).tobytes() == e.keyframe_get(y.id).tobytes() for x, y in zip(ka, kb))
    print(json.dumps(dict(row, leg="a: sequence_run_raw(intensity) + keyframe_from_slot + WindowKeyframer over ids", keyframes=len(ka), **stats(ta))), flush=True)
    print(json.dumps(dict(row, leg="b: sequence_run_raw + batch_get_cloud + WindowKeyframer over host arrays (no intensity)", keyframes=len(kb),
                          identical=bool(same), **stats(tb))), flush=True)
    e.close()
    # legs c and d: a fresh child per run and library, alternating
    libs = [("this", ROOT)] + ([("parent", a.parent_root)] if a.parent_root else [])
    runs = {name: [] for name, _ in libs}
    for _ in range(a.repeats):
        for name, path in libs:
            env = dict(os.environ)
            env.pop("MI355NDT_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--xyz-child", "--root", os.path.abspath(path), "--frames", str(a.frames), "--azimuth", str(a.azimuth),
                                  "--steps", str(a.steps), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(json.dumps(dict(leg="c/d", lib=name, error=out.stderr[-400:])), flush=True)
                return 1
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    for key, leg in (("batch_prefilter", "c"), ("batch_remove_outliers", "d")):
        res = dict(row, leg=f"{leg}: {key}, xyz only")
        for name in runs:
            med = [r[key]["median_ms"] for r in runs[name]]
            res[name] = dict(medians_ms=med, spread_ms=round(max(med) - min(med), 3))
        if "parent" in runs:
            res["this_minus_parent_ms"] = round(float(np.median([r[key]["median_ms"] for r in runs["this"]]) -
                                                      np.median([r[key]["median_ms"] for r in runs["parent"]])), 3)
        print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
