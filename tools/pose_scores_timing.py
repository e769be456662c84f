"""What a search over start poses costs: 5 loop candidates of ~100 k points against one window keyframe, a 9 x 9 x 5 lattice (405 poses a
candidate, 2,025 items).  Times, on cuda:0,
  * one Engine.batch_score_poses over all items,
  * the same scores through repeated Engine.derivatives_T on one-pair engines (what a caller could do before), and checks them bit for bit,
  * loop_closure.verify_candidates_search end to end against loop_closure.verify_candidates.
Prints one JSON line.  No threshold is attached to any of the figures (DESIGN.md 8 records a run).

  python tools/pose_scores_timing.py [--azimuth 1600] [--repeat 5] [--single-items 405]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lv_slam_amd import loop_closure as LC  # noqa: E402
from lv_slam_amd import ndt, synth  # noqa: E402

DX = DY = tuple(np.linspace(-4.0, 4.0, 9))
DYAW = tuple(np.linspace(-0.2, 0.2, 5))


def best_of(fn, repeat):
    out, ts = None, []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts) * 1e3, float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--azimuth", type=int, default=1600, help="azimuth steps of the 64-beam scans: 1600 = 102,400 points a cloud")
    ap.add_argument("--candidates", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--single-items", type=int, default=405, help="items per candidate that also go through derivatives_T")
    a = ap.parse_args()
    K = a.candidates
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    clouds = [synth.make_pair(k, a.azimuth, device=dev) for k in range(K)]
    tgt = clouds[0][0].cpu().numpy()
    cands = [c[1].cpu().numpy() for c in clouds]
    guesses = []
    for k in range(K):                                       # the true motion of pair 0 for every candidate, displaced: what a drifted graph hands over
        G = clouds[0][2].copy()
        G[:3, 3] += (1.5 - 0.7 * k, 0.4 * k - 0.8, 0.0)
        guesses.append(LC.loop_guess(np.eye(4), G))
    guesses = np.stack(guesses)
    lattice = dict(dx=DX, dy=DY, dyaw=DYAW)
    L = np.stack([LC.pose_lattice(g, **lattice) for g in guesses])
    n_poses = L.shape[1]
    prm = ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7)
    eng = ndt.Engine(prm)
    eng.batch_reserve(K, len(tgt), max(len(c) for c in cands))
    for k, c in enumerate(cands):
        eng.batch_set_target(k, tgt)
        eng.batch_set_source(k, c)
    eng.batch_build_targets()
    eng.synchronize()
    pairs = np.repeat(np.arange(K, dtype=np.int32), n_poses)
    poses = L.reshape(-1, 4, 4)
    eng.batch_score_poses(pairs, poses)                      # (allocations, first launch)
    (s, h), batch_ms, batch_med = best_of(lambda: eng.batch_score_poses(pairs, poses), a.repeat)
    # the same through derivatives_T, one call and one host round trip per item
    m = min(a.single_items, n_poses)
    single_s, single_ms = np.zeros((K, m)), 0.0
    I3 = np.eye(3, dtype=np.float32)
    for k, c in enumerate(cands):
        e1 = ndt.Engine(prm)
        e1.set_target(tgt)
        e1.set_source(c)
        e1.derivatives_T(L[k, 0], I3)
        t0 = time.perf_counter()
        for j in range(m):
            single_s[k, j] = e1.derivatives_T(L[k, j], I3)[0]
        single_ms += (time.perf_counter() - t0) * 1e3
        e1.close()
    same_bits = bool(np.array_equal(single_s.view(np.int64), s.reshape(K, n_poses)[:, :m].view(np.int64)))
    # the loop check, end to end (uploads, grids, scores, aligns, fitness scores)
    def run(f, *x):
        e = ndt.Engine(prm)
        try:
            return f(e, tgt, cands, guesses, *x, 25.0, 0.5)
        finally:
            e.close()
    run(LC.verify_candidates)
    plain, plain_ms, _ = best_of(lambda: run(LC.verify_candidates), a.repeat)
    searched, search_ms, _ = best_of(lambda: run(LC.verify_candidates_search, lattice), a.repeat)
    print(json.dumps(dict(points=len(tgt), candidates=K, poses_per_candidate=n_poses, items=int(len(pairs)),
                          batch_score_poses_ms=round(batch_ms, 3), batch_score_poses_median_ms=round(batch_med, 3),
                          us_per_item=round(1e3 * batch_ms / len(pairs), 3), hits_total=int(h.sum()),
                          derivatives_T_items=K * m, derivatives_T_ms=round(single_ms, 3), derivatives_T_us_per_item=round(1e3 * single_ms / (K * m), 3),
                          same_bits=same_bits, verify_candidates_ms=round(plain_ms, 3), verify_candidates_search_ms=round(search_ms, 3),
                          picked=searched[4], loop_plain=plain[0], loop_search=searched[0])))
    assert same_bits


if __name__ == "__main__":
    main()
