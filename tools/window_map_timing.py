"""Times the window map and the id route of the map cloud on one GPU.

  (a) Engine.window_keyframe (host scans in, count out) for 8 and 32 scans of 65,536 points at 0.1 m, against tools/window_map_ref.py on
      one CPU thread; the run-length distribution of the windows' voxels (one lane of the emit kernel walks one run), and -- under
      rocprofv3 --kernel-trace --stats, when it is installed -- the emit kernel's share of the call's kernel time, for a driving window
      and for one that stands still (long runs);
  (b) Engine.map_cloud_keyframes (resident keyframes) against Engine.map_cloud (the host route) for 200 keyframes of 65,536 points at
      0.5 m and 0.05 m.

Medians of --runs runs (at least five) with min / max, after one warm-up call that also sizes the workspaces.  The driver opens no GPU
itself: every step is ONE child process under its own `timeout`, run one after the other; a step that fails ends the run.

  python tools/window_map_timing.py [--runs 7] [--keyframes 200] [--skip-cpu]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _stats(ts):
    import numpy as np
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=float(np.median(ts)), min_ms=float(ts.min()), max_ms=float(ts.max()), runs=len(ts))


def _window(n_scans, still=False):
    """A window of a synthetic drive (or of one scan repeated with 5 mm noise: a vehicle that stands still)."""
    import numpy as np
    from lv_slam_amd import synth
    if still:
        scans, _ = synth.make_sequence(1)
        base = scans[0].numpy().astype(np.float32)
        rng = np.random.default_rng(7)
        return [base + rng.normal(0, 0.005, base.shape).astype(np.float32) for _ in range(n_scans)], [np.eye(4)] * n_scans
    scans, poses = synth.make_sequence(n_scans)
    return [s.numpy().astype(np.float32) for s in scans], [np.linalg.inv(poses[0]) @ p for p in poses]


def _histogram(rl):
    import numpy as np
    edges = [1, 2, 3, 5, 9, 17, 33, 65, 129, 257, 1 << 30]
    h = {}
    for lo, hi in zip(edges[:-1], edges[1:]):
        name = f"{lo}" if hi == lo + 1 else (f"{lo}-{hi - 1}" if hi < (1 << 30) else f"{lo}+")
        h[name] = int(((rl >= lo) & (rl < hi)).sum())
    return dict(voxels=int(len(rl)), mean=float(rl.mean()) if len(rl) else 0.0, max=int(rl.max()) if len(rl) else 0, histogram=h)


def step_window(args):
    import numpy as np
    import window_map_ref as R
    from lv_slam_amd import ndt
    eng = ndt.Engine()
    for n_scans, still in ((8, False), (32, False), (20, True)):
        scans, rel = _window(n_scans, still)
        kid, n = eng.window_keyframe(scans, rel, 0.1)              # warm-up: sizes the workspace and the staging slots
        eng.keyframe_release(kid)
        ts = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            kid, n = eng.window_keyframe(scans, rel, 0.1)
            eng.synchronize()                                      # (the emit kernel is enqueued when the call returns)
            ts.append(time.perf_counter() - t0)
            eng.keyframe_release(kid)
        row = dict(step="window_keyframe", scans=n_scans, still=still, points_in=int(sum(len(s) for s in scans)), points_out=int(n), gpu=_stats(ts),
                   run_lengths=_histogram(R.run_lengths(scans, rel, 0.1)))
        if not args.skip_cpu:
            tc = []
            for _ in range(1 if n_scans > 8 else 3):
                t0 = time.perf_counter()
                ref = R.window_map(scans, rel, 0.1)
                tc.append(time.perf_counter() - t0)
            row["cpu_numpy_one_thread"] = _stats(tc)
            row["same_count"] = bool(len(ref) == n)
        print(json.dumps(row), flush=True)
    eng.close()


def step_mapcloud(args):
    import numpy as np
    from lv_slam_amd import ndt, synth
    K = args.keyframes
    base_scans, base_poses = synth.make_sequence(8)
    base_scans = [s.numpy().astype(np.float32) for s in base_scans]
    clouds, poses = [], []
    for k in range(K):                                             # 200 keyframes along a line: the eight scans in turn, 8 m apart
        T = base_poses[k % 8].copy()
        T[0, 3] += 8.0 * (k // 8)
        clouds.append(base_scans[k % 8])
        poses.append(T)
    eng = ndt.Engine()
    ids = [eng.keyframe_add(c) for c in clouds]
    eng.synchronize()
    for r in (0.5, 0.05):
        a = eng.map_cloud(clouds, poses, r)                        # warm-ups
        b = eng.map_cloud_keyframes(ids, poses, r)
        same = a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
        t_host, t_ids = [], []
        for _ in range(args.runs):                                 # interleaved, so that drift hits both alike
            t0 = time.perf_counter()
            eng.map_cloud(clouds, poses, r, fetch=False)
            t_host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            eng.map_cloud_keyframes(ids, poses, r, fetch=False)
            t_ids.append(time.perf_counter() - t0)
        print(json.dumps(dict(step="map_cloud", keyframes=K, points=int(sum(len(c) for c in clouds)), resolution=r, centres=int(len(a)),
                              equal_words=same, host_route=_stats(t_host), id_route=_stats(t_ids))), flush=True)
    eng.close()


def step_profiled(args):
    """The body of the rocprofv3 child: a few window calls, nothing else."""
    from lv_slam_amd import ndt
    eng = ndt.Engine()
    scans, rel = _window(20 if args.still else 8, args.still)
    for _ in range(4):
        kid, _ = eng.window_keyframe(scans, rel, 0.1)
        eng.synchronize()
        eng.keyframe_release(kid)
    eng.close()


def emit_share(args, still):
    """rocprofv3 --kernel-trace --stats over a child that only builds windows: k_kf_emit's share of the kernel time."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return dict(step="emit_share", still=still, error="rocprofv3 not found")
    out = tempfile.mkdtemp(prefix="wm_prof_")
    cmd = ["timeout", "-k", "10", "240", prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
           sys.executable, os.path.abspath(__file__), "--step", "profiled"] + (["--still"] if still else [])
    rc = subprocess.call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    row = dict(step="emit_share", still=still, rc=rc)
    if rc == 0:
        tot, kern = 0.0, {}
        for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                ns = float(r.get("TotalDurationNs") or 0)
                name = (r.get("Name") or "").split("(")[0]
                tot += ns
                kern[name] = kern.get(name, 0.0) + ns
        if tot > 0:
            row["kernel_ms_per_call"] = tot / 4e6
            row["share"] = {k: round(v / tot, 4) for k, v in sorted(kern.items(), key=lambda kv: -kv[1])[:8]}
            row["k_kf_emit_share"] = round(sum(v for k, v in kern.items() if "k_kf_emit" in k) / tot, 4)
        else:
            row["error"] = "no kernel statistics in rocprofv3's output"
    shutil.rmtree(out, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--skip-cpu", action="store_true")
    ap.add_argument("--step", choices=["window", "mapcloud", "profiled"])
    ap.add_argument("--still", action="store_true")
    args = ap.parse_args()
    args.runs = max(args.runs, 5)
    if args.step:
        {"window": step_window, "mapcloud": step_mapcloud, "profiled": step_profiled}[args.step](args)
        return 0
    common = ["--runs", str(args.runs), "--keyframes", str(args.keyframes)] + (["--skip-cpu"] if args.skip_cpu else [])
    for step, limit in (("window", 420), ("mapcloud", 420)):
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step] + common)
        if rc != 0:
            print(json.dumps(dict(step=step, error=f"exit status {rc}; stopping")), flush=True)
            return rc
    for still in (False, True):
        row = emit_share(args, still)
        print(json.dumps(row), flush=True)
        if row.get("rc", 0) != 0:
            return row["rc"]
    return 0


if __name__ == "__main__":
    sys.exit(main())
