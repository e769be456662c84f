"""GPU box: one mi355ndt_map_cloud call (MapCloudGenerator::generate on the device) against the CPU restatement it equals bit for bit
(tools/map_cloud_ref.py), on the keyframes of a synthetic drive.

    python tools/map_cloud_timing.py [--keyframes 40,200] [--every 1] [--resolutions 0.5,0.05] [--steps 5] [--warmup 1] [--azimuth 1024]

Keyframes are frames 0, every, 2 * every, ... of synth.make_sequence (--azimuth x 64 points per scan) with their ground-truth poses,
cast on the GPU when torch sees one.  `gpu_ms` = median of --steps Engine.map_cloud calls after --warmup (host clouds in, centres out:
staging, transfer, kernels and copy-out), `gpu_min_ms` their minimum; `cpu_ms` = one run of the restatement (NumPy, one thread);
`identical` = the two outputs equal word for word.  One JSON line per (K, resolution)."""
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

_spec = importlib.util.spec_from_file_location("map_cloud_ref", os.path.join(ROOT, "tools", "map_cloud_ref.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)


def keyframes(n, every, azimuth):
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    scans, poses = synth.make_sequence((n - 1) * every + 1, azimuth, device=dev)
    return [scans[k].cpu().numpy().astype(np.float32) for k in range(0, len(scans), every)], [poses[k] for k in range(0, len(scans), every)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="40,200")
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--resolutions", default="0.5,0.05")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--azimuth", type=int, default=1024)
    ap.add_argument("--no-cpu", action="store_true", help="skip the restatement (no cpu_ms / identical)")
    a = ap.parse_args()
    ks = [int(x) for x in a.keyframes.split(",")]
    clouds, poses = keyframes(max(ks), a.every, a.azimuth)
    eng = ndt.Engine()
    for K in ks:
        cl, ps = clouds[:K], poses[:K]
        n = sum(len(c) for c in cl)
        for r in (float(x) for x in a.resolutions.split(",")):
            for _ in range(a.warmup):
                eng.map_cloud(cl, ps, r)
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                got = eng.map_cloud(cl, ps, r)
                ts.append((time.perf_counter() - t0) * 1e3)
            line = dict(keyframes=K, points=n, resolution=r, centres=int(len(got)), gpu_ms=round(float(np.median(ts)), 3),
                        gpu_min_ms=round(float(np.min(ts)), 3), steps=a.steps, warmup=a.warmup)
            if not a.no_cpu:
                t0 = time.perf_counter()
                exp, box = R.map_cloud(cl, ps, r, return_box=True)
                line.update(cpu_ms=round((time.perf_counter() - t0) * 1e3, 1), depth=box.depth,
                            identical=bool(exp.shape == got.shape and np.array_equal(exp.view(np.uint32), got.view(np.uint32))))
            print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
