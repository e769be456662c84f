"""GPU box: record what Engine.fitness_score (mi355ndt_fitness_score_T) returns over a fixed list of cases, as words.

    python tools/record_fitness_words.py [--out tests/golden/fitness_single_parent.json]

tests/golden/fitness_single_parent.json was written by this script with the library of the commit BEFORE the one-pair score moved onto
the batch path (k_fitness over the dense cstart / cend table); tests/test_batch_fitness_gpu.py::test_one_pair_words_equal_the_parents
recomputes every case with the current library and compares word for word.  Run it again only to extend the list, with a library whose
words are known to be right: the file is the anchor, not a cache.

A case = (clouds, transform, max_range); the score is stored as the hex of its 64-bit word, the inlier count as an int.  Clouds come
from synth alone, transforms are given explicitly, so nothing depends on an align."""
import argparse
import json
import os
import struct
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RANGES = (0.04, 1.0, 25.0, float("inf"))
# (name, pair index, azimuth steps, what is done to the target)
CLOUDS = (("p40", 40, 256, None), ("p90", 90, 256, None), ("p91", 91, 256, None), ("p0_full", 0, 1024, None),
          ("p91_stray", 91, 256, "stray"), ("p90_nan", 90, 256, "nan"))


def transforms():
    off = np.eye(4, dtype=np.float32)
    off[:3, 3] = [0.3, 0.0, 0.0]
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 5000.0
    return (("identity", np.eye(4, dtype=np.float32)), ("offset", off), ("far", far))


def clouds(k, n_az, kind):
    from lv_slam_amd import synth
    t, s, _ = synth.make_pair(k, n_az)
    t, s = t.numpy(), s.numpy()
    if kind == "stray":                        # the leaf-too-small guard: no grid, the exhaustive kernel
        t = t.copy()
        t[7] = [1e30, 0.0, 0.0]
    elif kind == "nan":                        # points, none finite: an empty grid
        t = np.full((500, 3), np.nan, np.float32)
    return t, s


def word(x: float) -> str:
    return struct.pack(">d", x).hex()


def compute():
    """{case name: [score word, inliers]} with the library that is loaded."""
    from lv_slam_amd import ndt
    out = {}
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    for name, k, n_az, kind in CLOUDS:
        t, s = clouds(k, n_az, kind)
        eng.set_target(t)
        eng.set_source(s)
        for tname, T in transforms():
            for mr in RANGES:
                score, n = eng.fitness_score(mr, T)
                out[f"{name}/{tname}/{mr}"] = [word(score), int(n)]
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("tests", "golden", "fitness_single_parent.json"))
    a = ap.parse_args()
    got = compute()
    with open(a.out, "w") as f:                  # one case per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(got[k])}" for k in sorted(got)) + "\n}\n")
    print(f"{len(got)} cases -> {a.out}")


if __name__ == "__main__":
    main()
