#!/usr/bin/env python3
"""The target build beside the align launch, from a rocprofv3 --kernel-trace csv of a bench.py run.

usage: tools/stream_build_trace.py <..._kernel_trace.csv>

Prints (1) every build kernel's duration split into calls that ran with the GPU to themselves and calls that ran inside a k_align_async launch
(the streamed builds, in the launch's reserved slots), and (2) for the last streamed launches: start-to-start, launch, gap to the next launch
and how long after the end of the launch the build it covered ended.
"""
import csv
import re
import statistics
import sys

BUILD = ("k_minmax", "k_griddesc", "k_word_offsets", "k_build_check", "k_rs_hist", "k_rs_scan", "k_rs_scatter", "k_mark", "k_rank", "k_leafsum", "k_voxels")


def short(name):
    n = name.replace("void ", "")
    m = re.match(r"([\w:]+)(<[^(]*>)?", n)
    return (m.group(1) + (m.group(2) or "")) if m else n


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])) for r in rows)
    launches = [e for e in ev if e[2].startswith("k_align_async")]
    builds = [e for e in ev if e[2].startswith(BUILD)]

    def inside(e):                                   # the launch that covers more than half of the kernel, if any
        for L in launches:
            if L[0] > e[1]:
                break
            if min(L[1], e[1]) - max(L[0], e[0]) > (e[1] - e[0]) / 2:
                return L
        return None

    alone, beside = {}, {}
    for e in builds:
        (beside if inside(e) else alone).setdefault(e[2], []).append((e[1] - e[0]) / 1e3)
    print(f"{'build kernel':44s} {'alone: calls':>12s} {'median us':>10s} {'beside a launch: calls':>23s} {'median us':>10s} {'ratio':>6s}")
    for n in sorted(set(alone) | set(beside), key=lambda n: -sum(beside.get(n, [0]))):
        a, b = alone.get(n, []), beside.get(n, [])
        ma, mb = (statistics.median(a) if a else float("nan")), (statistics.median(b) if b else float("nan"))
        print(f"{n[:44]:44s} {len(a):12d} {ma:10.1f} {len(b):23d} {mb:10.1f} {mb / ma if a and b else float('nan'):6.1f}")
    tot = sum(sum(v) for v in beside.values())
    nb = int(statistics.median(len(v) for v in beside.values())) if beside else 0      # (k_rs_scan runs twice per build, a late k_voxels seldom)
    if nb:
        print(f"sum of the build kernels beside a launch: {tot / nb:.0f} us per build ({nb} builds)")

    print("\n# streamed launches (us): start-to-start, launch, gap to the next launch, end of the build after the end of the launch | last build kernel")
    out = []
    for i, L in enumerate(launches[:-1]):
        nxt = launches[i + 1]
        mine = [e for e in builds if L[0] <= e[0] < nxt[0]]
        if not mine or not any(inside(e) is L for e in mine):
            continue
        last = max(mine, key=lambda e: e[1])
        out.append(f"{(nxt[0] - L[0]) / 1e3:9.1f} {(L[1] - L[0]) / 1e3:9.1f} {(nxt[0] - L[1]) / 1e3:8.1f} {(last[1] - L[1]) / 1e3:8.1f} | {last[2][:28]}")
    print("\n".join(out[-12:]))

    # the last two streamed launches kernel by kernel: where the build's time goes, and whether its stream stands idle
    streamed = [i for i, L in enumerate(launches[:-1]) if any(inside(e) is L for e in builds if L[0] <= e[0] < launches[i + 1][0])]
    for i in streamed[-2:]:
        L, nxt = launches[i], launches[i + 1]
        print(f"\n# launch of {(L[1] - L[0]) / 1e3:.1f} us: build kernels started before the next launch (start after the launch's start, duration, idle before; us)")
        prev = None
        for e in (e for e in builds if L[0] <= e[0] < nxt[0]):
            print(f"  {e[2][:40]:40s} {(e[0] - L[0]) / 1e3:9.1f} {(e[1] - e[0]) / 1e3:9.1f} {((e[0] - prev) / 1e3 if prev else 0.0):9.1f}")
            prev = e[1]


if __name__ == "__main__":
    main()
