"""GPU box: what MI355NDT_OPT_GROUND_CLASS = 1 / 2 / 3 (pclomp_ground's classes) cost against class 0, ndt_omp, on the SAME path.

    python tools/ndt_ground_timing.py [--pairs 271] [--azimuth 1024] [--steps 5] [--warmup 1] [--search DIRECT7]

The batch is BASELINE config 3's: --pairs pairs of synth.make_pair(k, --azimuth) (64 beams: 65,536 points a cloud), ndt_omp, 1 m, DIRECT1 or
DIRECT7, trans_epsilon 0.01, 64 iterations, every pair from default_guess(); the clouds are cast on the device and bound.  The target grids
are built once, under class 1, so that they carry the leaves' class codes and serve all four classes: no align of the loop rebuilds them.
A ground class always takes the lockstep (update, sweep) rounds, so the fair parent figure is class 0 with MI355NDT_OPT_ASYNC_ALIGN = 0 --
the same rounds.  The four alternate inside every repetition; host clock around the synchronous batch_align.  One JSON line: medians in ms,
the sweeps and hits each class took (they are different registrations: their iteration counts differ), us per (pair, sweep), and the ratios
of those to class 0's.  No threshold."""
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
    ap.add_argument("--search", default="DIRECT7", choices=["DIRECT1", "DIRECT7", "DIRECT26"])
    a = ap.parse_args()
    B, N = a.pairs, a.azimuth * 64
    T = torch.empty(B, 3, N, device="cuda", dtype=torch.float32)
    S = torch.empty(B, 3, N, device="cuda", dtype=torch.float32)
    for b0 in range(0, B, 16):
        ks = list(range(b0, min(b0 + 16, B)))
        t, s, _ = synth.make_pairs(ks, a.azimuth, device="cuda")
        T[ks[0]:ks[-1] + 1] = t.permute(0, 2, 1)
        S[ks[0]:ks[-1] + 1] = s.permute(0, 2, 1)
    torch.cuda.synchronize()
    eng = ndt.Engine(ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=getattr(ndt, a.search)))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, 0)
    eng.batch_bind_device(T.data_ptr(), [N] * B, N, S.data_ptr(), [N] * B, N)
    eng.set_option(ndt.OPT_GROUND_CLASS, 1)
    eng.batch_build_targets()
    G = np.ascontiguousarray(np.broadcast_to(synth.default_guess().T.reshape(1, 16), (B, 16)), dtype=np.float32)
    res = (ndt.Result * B)()
    runs = {"class0_rounds": 0, "class1_horizontal": 1, "class2_vertical": 2, "class3_all": 3}   # name: MI355NDT_OPT_GROUND_CLASS
    ts = {k: [] for k in runs}
    info = {}
    for i in range(a.warmup + a.steps):
        for name, cls in runs.items():
            eng.set_option(ndt.OPT_GROUND_CLASS, cls)
            t0 = time.perf_counter()
            eng.batch_align_raw(G, res)
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                ts[name].append(dt)
            info[name] = dict(sweeps=int(sum(r.sweeps for r in res)), iterations_max=int(max(r.iterations for r in res)), converged=int(sum(r.converged for r in res)),
                              hits_last=int(sum(r.hits_last for r in res)))
    row = dict(pairs=B, points=N, search=a.search, steps=a.steps)
    for name in runs:
        ms = float(np.median(ts[name]))
        row[name] = dict(median_ms=round(ms, 3), min_ms=round(float(np.min(ts[name])), 3), max_ms=round(float(np.max(ts[name])), 3),
                         us_per_pair_sweep=round(1e3 * ms / max(info[name]["sweeps"], 1), 4), **info[name])
    for name in list(runs)[1:]:
        row["ratio_ms_" + name] = round(row[name]["median_ms"] / row["class0_rounds"]["median_ms"], 4)
        row["ratio_per_pair_sweep_" + name] = round(row[name]["us_per_pair_sweep"] / row["class0_rounds"]["us_per_pair_sweep"], 4)
    print(json.dumps(row), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
