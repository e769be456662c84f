"""GPU box: the ICP surface (mi355ndt_icp_*) against the restatement's stages on one CPU thread.

    python tools/icp_timing.py [--azimuth 64,256] [--steps 5] [--warmup 1] [--pair 0] [--no-cpu | --cpu-only] [--cells 200,400] [--batch 1,2,5,16 [--baseline-lib PATH]]

Clouds are synth.make_pair(pair, azimuth) (64 beams: 4,096 / 16,384 points).  One JSON line each (median / min / max of --steps calls after
--warmup, host clock around the synchronous calls), the target's index resident:
  step            icp_correspondences from default_guess(): one move, match and sum (two launches, one wait), the results fetched
  align_factory   icp_align at the factory's values (registrations.cpp:21-29) from default_guess(), and its iterations
  align_eps1e-6   icp_align at transformation_epsilon 1e-6 from the identity, and its iterations
  align_cold      set both clouds, then align_eps1e-6: what a loop candidate costs when neither cloud has been seen
  cpu_*           tools/icp_ref.py's one_step / align (exhaustive search), one call each, on one thread (--no-cpu skips them)
--batch K,...: only the loop check, at transformation_epsilon 1e-6.  The K candidates are the source under K small rigid motions, resident
keyframes; one line per K, medians of --steps alternating repetitions:
  sequential_ms   K x (icp_set_source(keyframe) + icp_align), one candidate after the other
  batch_ms        K x icp_batch_set_source(keyframe) + ONE icp_batch_align, with its rounds and the sum of the slots' requests; every slot's
                  final transformation is compared with its sequential one (equal_bytes)
  baseline_ms     the sequential loop through another build of the library that has the ICP surface (--baseline-lib), in the same run; a
                  build without it (any commit before the surface existed) is reported as such"""
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

spec = importlib.util.spec_from_file_location("icp_ref", os.path.join(ROOT, "tools", "icp_ref.py"))
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


def params(**kw):
    prm = dict(R.FACTORY, **kw)
    prm.pop("use_reciprocal_correspondences")
    return ndt.default_icp_params(**prm)


SINGLE_PAIR_CALLS = ("mi355ndt_create", "mi355ndt_destroy", "mi355ndt_last_error", "mi355ndt_keyframe_add", "mi355ndt_keyframe_get",
                     "mi355ndt_icp_set_params", "mi355ndt_icp_set_target", "mi355ndt_icp_set_source", "mi355ndt_icp_set_target_keyframe",
                     "mi355ndt_icp_set_source_keyframe", "mi355ndt_icp_align")


def engine_over(path):
    """an Engine over another build of the library, for the calls the sequential loop makes; None when the build has no ICP surface"""
    ours, L = ndt.load_library(), C.CDLL(path)
    if not all(hasattr(L, name) for name in SINGLE_PAIR_CALLS):
        return None
    for name in SINGLE_PAIR_CALLS:
        f, g = getattr(L, name), getattr(ours, name)
        f.argtypes, f.restype = g.argtypes, g.restype
    e = ndt.Engine.__new__(ndt.Engine)
    e.lib, e.h, e._keep, e._gicp_n, e._gicp_batch_n, e._icp_n, e._icp_batch_n = L, C.c_void_p(), [], [0, 0], [], [0, 0], []
    rc = L.mi355ndt_create(None, 0, C.byref(e.h))
    if rc != ndt.OK:
        raise ndt.NDTError(rc, "mi355ndt_create")
    return e


def candidates(src, K):
    """the source under K small rigid motions, each from the identity"""
    out = []
    for k in range(K):
        D = np.eye(4)
        D[:3, :3] = synth.rot_zyx(0.001 * (k % 5), -0.0015 * (k % 3), 0.002 * (k % 7))
        D[:3, 3] = [0.02 * (k % 4), -0.01 * (k % 6), 0.005 * (k % 3)]
        out.append((R.move_f32(D.astype(np.float32), src), np.eye(4, dtype=np.float32)))
    return out


def loop_check(a, az, Ks):
    tgt, src, _ = synth.make_pair(a.pair, az)
    tgt, src = tgt.numpy(), src.numpy()
    engines = [ndt.Engine()]
    if a.baseline_lib:
        b = engine_over(a.baseline_lib)
        if b is None:
            print(json.dumps(dict(stage="batch", baseline_lib=a.baseline_lib, note="this build has no mi355ndt_icp_* surface: no baseline")), flush=True)
        else:
            engines.append(b)
    cand = candidates(src, max(Ks))
    ids = []
    for e in engines:                               # every cloud resident, the target's index built
        e.icp_set_params(params(transformation_epsilon=1e-6))
        kt = e.keyframe_add(tgt)
        e.icp_set_target(keyframe=kt)
        ids.append([e.keyframe_add(c) for c, _ in cand])
        e.icp_set_source(keyframe=ids[-1][0])
        e.icp_align(cand[0][1])

    def sequential(e, kid, K):
        out = []
        for k in range(K):
            e.icp_set_source(keyframe=kid[k])
            out.append(e.icp_align(cand[k][1]))
        return out

    def batch(K):
        e = engines[0]
        e.icp_batch_reserve(K)
        for k in range(K):
            e.icp_batch_set_source(k, keyframe=ids[0][k])
        return e.icp_batch_align(np.stack([g for _, g in cand[:K]]))
    for K in Ks:
        ts = {"sequential_ms": [], "batch_ms": [], "baseline_ms": []}
        for i in range(a.warmup + a.steps):          # the three alternate inside every repetition
            t0 = time.perf_counter()
            seq = sequential(engines[0], ids[0], K)
            t1 = time.perf_counter()
            bat = batch(K)
            t2 = time.perf_counter()
            if len(engines) > 1:
                base = sequential(engines[1], ids[1], K)
            t3 = time.perf_counter()
            if i >= a.warmup:
                ts["sequential_ms"].append((t1 - t0) * 1e3); ts["batch_ms"].append((t2 - t1) * 1e3); ts["baseline_ms"].append((t3 - t2) * 1e3)
        rounds, req = engines[0].icp_batch_stats()
        equal = all(b["final"].tobytes() == s["final"].tobytes() and b["iterations"] == s["iterations"] for b, s in zip(bat, seq))
        row = dict(azimuth=az, points=len(src), stage="batch", K=K, rounds=rounds, requests_sum=int(req.sum()), equal_bytes=equal,
                   iterations=[r["iterations"] for r in bat])
        for name, v in ts.items():
            if name != "baseline_ms" or len(engines) > 1:
                row[name] = round(float(np.median(v)), 3)
        if len(engines) > 1:
            row["baseline_equal_bytes"] = all(b["final"].tobytes() == s["final"].tobytes() for b, s in zip(base, seq))
        row["batch_ms_per_round"] = round(row["batch_ms"] / max(rounds, 1), 4)
        row["sequential_ms_per_request"] = round(row["sequential_ms"] / max(int(req.sum()), 1), 4)
        print(json.dumps(row), flush=True)
    for e in engines:
        e.close()


def engine_stages(a, row, tgt, src, G, I4, cell=None):
    e = ndt.Engine()
    if cell is not None:
        e.set_option(ndt.OPT_KF_FITNESS_CELL_MM, cell)
    e.icp_set_params(params())
    e.icp_set_target(tgt)
    e.icp_set_source(src)
    ts, (_, _, _, m) = timed(lambda: e.icp_correspondences(G), a.warmup, 4 * a.steps)
    print(json.dumps(dict(row, stage="step", matched=m, **stats(ts))), flush=True)
    ts, r = timed(lambda: e.icp_align(G), a.warmup, a.steps)
    print(json.dumps(dict(row, stage="align_factory", iterations=r["iterations"], state=ndt.ICP_STATES[r["state"]], **stats(ts))), flush=True)
    e.icp_set_params(params(transformation_epsilon=1e-6))
    ts, r = timed(lambda: e.icp_align(I4), a.warmup, a.steps)
    print(json.dumps(dict(row, stage="align_eps1e-6", iterations=r["iterations"], state=ndt.ICP_STATES[r["state"]], **stats(ts))), flush=True)

    def cold():
        e.icp_set_target(tgt)
        e.icp_set_source(src)
        return e.icp_align(I4)
    ts, _ = timed(cold, a.warmup, a.steps)
    print(json.dumps(dict(row, stage="align_cold", **stats(ts))), flush=True)
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
    ap.add_argument("--cpu-only", action="store_true", help="only the cpu_* lines (needs no GPU)")
    ap.add_argument("--cells", default="", help="mm,...: repeat the engine's stages with these cell sizes of the target's index (MI355NDT_OPT_KF_FITNESS_CELL_MM; no result bit depends on it)")
    a = ap.parse_args()
    G = synth.default_guess()
    I4 = np.eye(4, dtype=np.float32)
    if a.batch:
        for az in [int(x) for x in a.azimuth.split(",") if x]:
            loop_check(a, az, [int(x) for x in a.batch.split(",") if x])
        return
    tight = dict(R.FACTORY, transformation_epsilon=1e-6)
    for az in [int(x) for x in a.azimuth.split(",") if x]:
        tgt, src, _ = synth.make_pair(a.pair, az)
        tgt, src = tgt.numpy(), src.numpy()
        row = dict(azimuth=az, points=len(tgt))
        if not a.cpu_only:
            for cell in [None] + [int(x) for x in a.cells.split(",") if x]:
                engine_stages(a, row if cell is None else dict(row, cell_mm=cell), tgt, src, G, I4, cell)
        if not a.no_cpu:
            for name, f in (("cpu_step", lambda: R.one_step(src, tgt, G)), ("cpu_align_factory", lambda: R.align(src, tgt, G, R.FACTORY)),
                            ("cpu_align_eps1e-6", lambda: R.align(src, tgt, I4, tight))):
                ts, out = timed(f, 0, 1)
                print(json.dumps(dict(row, stage=name, iterations=out.get("iterations"), **stats(ts))), flush=True)


if __name__ == "__main__":
    main()
