"""GPU box: what MI355NDT_OPT_NDT_CLASS = 1 (pcl::NormalDistributionsTransform: radius search, f64 evaluation) costs against the f32 models on
the SAME search and the SAME path.

    python tools/ndt_pcl_timing.py [--pairs 271] [--azimuth 1024] [--steps 5] [--warmup 1] [--resolution 1.0]

The batch is BASELINE config 3's clouds: --pairs pairs of synth.make_pair(k, --azimuth) (64 beams: 65,536 points a cloud), trans_epsilon 0.01,
64 iterations, every pair from default_guess(); the clouds are cast on the device and bound, the target grids built once (under class 1, whose
grids -- centroids and f64 inverse covariances -- serve the other two runs as well).  Class 1 always takes the lockstep (update, sweep) rounds
and always the radius search, so the fair parents are MI355NDT_OPT_POSE_MODEL = 1 and = 0 with neighbor_mode = KDTREE and
MI355NDT_OPT_ASYNC_ALIGN = 0: the same probes, the same rounds, the f32 evaluations.  The three alternate inside every repetition; host clock
around the synchronous batch_align (which ends in a device synchronise).  One JSON line: medians in ms, the sweeps each run took (three
different registrations: their iteration counts differ), us per (pair, sweep), and the ratios of those.  No threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lv_slam_amd import ndt, synth  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=271)
    ap.add_argument("--azimuth", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--resolution", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ndt_pcl_timing.py measures on the GPU: no device found")
    B, N = a.pairs, a.azimuth * 64
    T = torch.empty(B, 3, N, device="cuda", dtype=torch.float32)
    S = torch.empty(B, 3, N, device="cuda", dtype=torch.float32)
    for b0 in range(0, B, 16):
        ks = list(range(b0, min(b0 + 16, B)))
        t, s, _ = synth.make_pairs(ks, a.azimuth, device="cuda")
        T[ks[0]:ks[-1] + 1] = t.permute(0, 2, 1)
        S[ks[0]:ks[-1] + 1] = s.permute(0, 2, 1)
    torch.cuda.synchronize()
    eng = ndt.Engine(ndt.default_params(resolution=a.resolution, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.KDTREE))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, 0)
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    eng.batch_bind_device(T.data_ptr(), [N] * B, N, S.data_ptr(), [N] * B, N)
    eng.batch_build_targets()
    G = np.ascontiguousarray(np.broadcast_to(synth.default_guess().T.reshape(1, 16), (B, 16)), dtype=np.float32)
    res = (ndt.Result * B)()
    runs = {"pcl_f64": (1, 0), "euler_f32_kdtree": (0, 1), "se3_f32_kdtree": (0, 0)}          # name: (OPT_NDT_CLASS, OPT_POSE_MODEL)
    ts = {k: [] for k in runs}
    info = {}
    for i in range(a.warmup + a.steps):
        for name, (cls, model) in runs.items():
            eng.set_option(ndt.OPT_NDT_CLASS, cls)
            eng.set_option(ndt.OPT_POSE_MODEL, model)
            t0 = time.perf_counter()
            eng.batch_align_raw(G, res)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                ts[name].append(dt)
            info[name] = dict(sweeps=int(sum(r.sweeps for r in res)), iterations_max=int(max(r.iterations for r in res)), converged=int(sum(r.converged for r in res)),
                              hits_last=int(sum(r.hits_last for r in res)))
    row = dict(pairs=B, points=N, resolution=a.resolution, steps=a.steps)
    for name in runs:
        ms = float(np.median(ts[name]))
        row[name] = dict(median_ms=round(ms, 3), min_ms=round(float(np.min(ts[name])), 3), max_ms=round(float(np.max(ts[name])), 3),
                         us_per_pair_sweep=round(1e3 * ms / max(info[name]["sweeps"], 1), 4), **info[name])
    for other in ("euler_f32_kdtree", "se3_f32_kdtree"):
        row[f"ratio_ms_pcl_over_{other}"] = round(row["pcl_f64"]["median_ms"] / row[other]["median_ms"], 4)
        row[f"ratio_per_pair_sweep_pcl_over_{other}"] = round(row["pcl_f64"]["us_per_pair_sweep"] / row[other]["us_per_pair_sweep"], 4)
    print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
