"""Reference-originated vectors, when somebody has produced them (tools/pin_reference/README.md).

The reference (PCL + Eigen + Sophus + FLANN) cannot be built in this repository's environment, so every parity statement elsewhere
in tests/ rests on the oracle, which is pinned only by an independent NumPy restatement ("parity unpinned").  tools/pin_reference/
dump_golden.cpp is the way out: built on a ROS / PCL host against lv_slam's own headers it runs the committed clouds of
tests/golden/pin/ through the REAL pclomp:: / pclpca::NormalDistributionsTransform and writes tests/golden/ref_<case>.bin.  This module
consumes those files: the oracle on the CPU, the HIP path (both f32 sum orders) under -m gpu.  Without them the oracle's cases SKIP
with a message that says what to do, and the HIP path's cases are held to the same bars against the oracle; the kit itself (file format,
reader, the dumper's own logic) is tested regardless:
  * CPU: oracle results written in the dumper's format and read back compare clean; a corrupted leaf or pose is caught;
  * CPU: dump_golden.cpp compiles (-Wall -Werror, -DPIN_SELFCHECK_MI355) with the mi355ndt adaptor standing in for the reference classes;
  * GPU: that self-check build runs every case of cases.txt and its files pass the same comparison against the oracle.

Bars against a reference file: leaf set / cell indices / point counts exact; mean 1e-13, cov / icov / evals 1e-9 relative (eigen-solver
and inverse algorithms differ); one sweep 2e-6 of its largest entry (the f32 summation order inside Eigen's products is exactly what is
being pinned); align: same iteration count and converged flag, SE(3) inside (1e-4 m, 1e-5 rad) -- the north-star tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PIN = os.path.join(GOLDEN, "pin")
sys.path.insert(0, GOLDEN)
import ref_format as RF                                   # noqa: E402
from conftest import se3_err                              # noqa: E402
from oracle import oracle_py as O                         # noqa: E402

CASES = RF.read_cases(PIN)
SKIP_MSG = ("no reference-originated vectors for this case: build tools/pin_reference/dump_golden.cpp on a ROS/PCL host against lv_slam's "
            "headers, run it on tests/golden/pin/ and commit tests/golden/ref_{name}.bin (tools/pin_reference/README.md)")


def params_of(c, mod):
    return mod.default_params(resolution=c["resolution"], step_size=c["step_size"], outlier_ratio=c["outlier_ratio"], trans_epsilon=c["trans_epsilon"],
                              max_iterations=c["max_iterations"], neighbor_mode=c["mode"], variant=c["variant"])


def clouds_of(c):
    return RF.load_cloud(os.path.join(PIN, c["target"])), RF.load_cloud(os.path.join(PIN, c["source"]))


def first_sweep_pose(guess):
    """computeTransformation's first sweep (ndt_omp_impl2.hpp:102-129): the cloud is moved by the f32 guess itself, the Jacobian uses exp(log(guess))."""
    p = O.se3_log(np.asarray(guess, np.float64))
    return p, np.asarray(O.se3_exp(p), np.float32)[:3, :3]


def oracle_dump(c):
    """What dump_golden.cpp writes, computed by the oracle."""
    tgt, src = clouds_of(c)
    prm = params_of(c, O)
    grid = O.Grid(tgt, prm)
    lv = grid.leaves()
    leaves = np.zeros(len(lv), RF.LEAF_DT)
    for k in ("idx", "n", "mean", "cov", "icov", "evals"):
        leaves[k] = lv[k]
    leaves["weight"] = lv["weight"] if c["variant"] == 1 else 0
    p, Rj = first_sweep_pose(c["guess"])
    s, g, H, _ = O.derivatives(grid, src, c["guess"], Rj)
    r = O.align(grid, src, c["guess"])
    moved = (src.astype(np.float32) @ r["final"][:3, :3].T.astype(np.float32))      # (only for calculateScore: the PCL-form transform is the engine's job)
    out = np.empty_like(src)
    F = r["final"].astype(np.float32)
    for a in range(3):
        out[:, a] = ((F[a, 0] * src[:, 0] + F[a, 1] * src[:, 1]) + F[a, 2] * src[:, 2]) + F[a, 3]
    del moved
    return dict(variant=c["variant"], mode=c["mode"], n_target=len(tgt), n_source=len(src), max_iterations=c["max_iterations"], flags=RF.HAS_SWEEP | RF.ALL_LEAVES | RF.HAS_COV,
                resolution=c["resolution"], step_size=c["step_size"], outlier_ratio=c["outlier_ratio"], trans_epsilon=c["trans_epsilon"], leaves=leaves,
                p=p, score=s, g=g, H=H, final=r["final"], last_inc=r["transformation"], iterations=r["iterations"], converged=int(r["converged"]),
                trans_probability=r["trans_probability"], calc_score=O.calculate_score(grid, out))


def compare(ref, got, min_points=6, sweep_rtol=2e-6):
    """`ref` (a reference file, or a file of the kit's self-test) against `got` (oracle or HIP path, same dict layout)."""
    assert (ref["variant"], ref["mode"], ref["n_target"], ref["n_source"]) == (got["variant"], got["mode"], got["n_target"], got["n_source"])
    rl, gl = ref["leaves"], got["leaves"]
    # compare on the coarser of the two leaf lists: searchable leaves (nr_points >= min_points, or -1 = eigen / inverse failure) are in both
    if not (ref["flags"] & RF.ALL_LEAVES and got["flags"] & RF.ALL_LEAVES):
        rl = rl[(rl["n"] >= min_points) | (rl["n"] == -1)]
        gl = gl[(gl["n"] >= min_points) | (gl["n"] == -1)]
    assert len(rl) == len(gl) and np.array_equal(rl["idx"], gl["idx"]), "leaf sets differ"
    assert np.array_equal(rl["n"], gl["n"]), "point counts differ"
    assert np.allclose(rl["mean"], gl["mean"], rtol=1e-13, atol=1e-13)
    live = rl["n"] >= min_points
    assert np.allclose(rl["icov"][live], gl["icov"][live], rtol=1e-9, atol=1e-9 * np.abs(rl["icov"][live]).max(initial=1.0)) or \
        np.allclose(rl["icov"][live].astype(np.float32), gl["icov"][live].astype(np.float32), rtol=2e-6)
    if ref["flags"] & RF.HAS_COV and got["flags"] & RF.HAS_COV:
        assert np.allclose(rl["cov"][live], gl["cov"][live], rtol=1e-9, atol=1e-12)
        assert np.allclose(rl["evals"][live], gl["evals"][live], rtol=1e-9, atol=1e-12)
    if ref["variant"] == 1:
        assert np.array_equal(rl["weight"][live], gl["weight"][live]), "ndt_pca integer weights differ"
    if ref["flags"] & RF.HAS_SWEEP and got["flags"] & RF.HAS_SWEEP:
        assert np.allclose(ref["p"], got["p"], rtol=0, atol=1e-12)
        scale = max(1.0, abs(ref["score"]), np.abs(ref["g"]).max(), np.abs(ref["H"]).max())
        assert abs(ref["score"] - got["score"]) <= sweep_rtol * scale
        assert np.abs(ref["g"] - got["g"]).max() <= sweep_rtol * scale and np.abs(ref["H"] - got["H"]).max() <= sweep_rtol * scale
    assert ref["iterations"] == got["iterations"] and ref["converged"] == got["converged"], (ref["iterations"], got["iterations"])
    dt, dr = se3_err(ref["final"], got["final"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    dt, dr = se3_err(ref["last_inc"], got["last_inc"])
    assert dt < 1e-5 and dr < 1e-5, (dt, dr)
    assert abs(ref["trans_probability"] - got["trans_probability"]) <= 1e-5 * max(1.0, abs(ref["trans_probability"]))
    assert abs(ref["calc_score"] - got["calc_score"]) <= 1e-5 * max(1.0, abs(ref["calc_score"]))


# ---------------------------------------------------------------------------------------------- the kit itself (always runs)
def test_pin_inputs_are_complete():
    assert len(CASES) >= 9 and {c["name"] for c in CASES} >= {"omp_direct7_r1", "pca_direct1_r05", "omp_kdtree_r1", "full_omp_direct7", "full_pca_direct1"}
    for c in CASES:
        t, s = clouds_of(c)
        assert len(t) > 1000 and len(s) > 100 and np.isfinite(t).all() and np.isfinite(s).all()
        assert c["guess"].shape == (4, 4) and c["guess"][3, 3] == 1.0 and c["guess"][0, 3] == 1.0      # the benchmark's guess: identity with x = +1 m
    full = [c for c in CASES if c["name"].startswith("full_")]
    assert all(len(clouds_of(c)[0]) == 65536 for c in full)
    # the small cases ARE the clouds of the committed npz fixtures
    z = np.load(os.path.join(GOLDEN, "omp_direct7_r1.npz"))
    t, s = clouds_of([c for c in CASES if c["name"] == "omp_direct7_r1"][0])
    assert np.array_equal(t, z["target"]) and np.array_equal(s, z["src_align"])


@pytest.mark.parametrize("name", ["omp_direct7_r1", "pca_direct1_r05", "omp_kdtree_r1"])
def test_format_round_trip_and_the_comparison_has_teeth(tmp_path, name):
    c = [x for x in CASES if x["name"] == name][0]
    d = oracle_dump(c)
    path = str(tmp_path / f"ref_{name}.bin")
    RF.write_ref(path, d)
    back = RF.read_ref(path)
    assert os.path.getsize(path) == 64 + 208 * len(d["leaves"]) + 544
    compare(back, d)                                       # the oracle against its own file: clean
    assert np.array_equal(back["leaves"]["mean"], d["leaves"]["mean"]) and np.array_equal(back["H"], d["H"]) and np.array_equal(back["final"], d["final"])
    for field, tweak in (("leaf", lambda r: r["leaves"]["mean"].__setitem__((3, 0), r["leaves"]["mean"][3, 0] + 1e-9)),
                         ("pose", lambda r: r["final"].__setitem__((0, 3), r["final"][0, 3] + np.float32(2e-4))),
                         ("iterations", lambda r: r.__setitem__("iterations", r["iterations"] + 1)),
                         ("sweep", lambda r: r["H"].__setitem__(np.unravel_index(np.abs(r["H"]).argmax(), (6, 6)), np.abs(r["H"]).max() * (1 + 1e-4)))):
        bad = RF.read_ref(path)
        tweak(bad)
        with pytest.raises(AssertionError):
            compare(bad, d)
    open(path, "ab").write(b"\0")
    with pytest.raises(ValueError):
        RF.read_ref(path)


def build_selfcheck():
    import __graft_entry__ as entry
    entry.build()
    return entry.build_pin_selfcheck()


def test_dumper_compiles_with_the_adaptor_standing_in():
    exe = build_selfcheck()
    assert os.path.exists(exe)
    src = open(os.path.join(ROOT, "tools", "pin_reference", "dump_golden.cpp")).read()
    for needle in ("ndt_omp/ndt_omp_impl2.hpp", "ndt_pca/ndt_pca_impl2.hpp", "target_cells_.getLeaves()", "computeDerivatives(g, H, cloud, p, true)", "calculateScore(out)"):
        assert needle in src                               # the reference-side code path is there, not only the self-check one
    cm = open(os.path.join(ROOT, "tools", "pin_reference", "CMakeLists.txt")).read()
    assert "-msse4.2" in cm and "LV_SLAM_DIR" in cm        # lv_slam's own flags (CMakeLists.txt:6,11)


# ---------------------------------------------------------------------------------------------- reference files, when present
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_oracle_vs_reference_file(c):
    path = os.path.join(GOLDEN, f"ref_{c['name']}.bin")
    if not os.path.exists(path):
        pytest.skip(SKIP_MSG.format(name=c["name"]))
    ref = RF.read_ref(path)
    errs = []
    for flags in (0, 1):                                   # canonical f32 sum order, then the Eigen 3.3 SSE predux pairing (ORA_VAR_SUM3_02_1)
        try:
            O.lib().ora_set_variant(flags, 256)
            compare(ref, oracle_dump(c))
            print(f"{c['name']}: the oracle matches the reference file with f32 sum order {flags}")
            return
        except AssertionError as e:
            errs.append(e)
        finally:
            O.lib().ora_set_variant(0, 256)
    raise errs[0]


def engine_dump(c, order):
    from lv_slam_amd import ndt
    tgt, src = clouds_of(c)
    eng = ndt.Engine(params_of(c, ndt))
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    eng.set_target(tgt)
    eng.set_source(src)
    v = eng.get_voxels()
    leaves = np.zeros(len(v), RF.LEAF_DT)
    for k in ("idx", "n", "mean", "weight"):
        leaves[k] = v[k]
    leaves["icov"] = v["icov"]
    leaves["cov"] = np.nan
    leaves["evals"] = np.nan
    if c["variant"] == 0:
        leaves["weight"] = 0
    p, Rj = first_sweep_pose(c["guess"])
    s, g, H, _ = eng.derivatives_T(c["guess"], Rj)
    r = eng.align(c["guess"])
    inc, _ = eng.get_incremental()
    d = dict(variant=c["variant"], mode=c["mode"], n_target=len(tgt), n_source=len(src), max_iterations=c["max_iterations"], flags=RF.HAS_SWEEP,
             resolution=c["resolution"], step_size=c["step_size"], outlier_ratio=c["outlier_ratio"], trans_epsilon=c["trans_epsilon"], leaves=leaves,
             p=p, score=s, g=g, H=H, final=r["final"], last_inc=inc, iterations=r["iterations"], converged=int(r["converged"]),
             trans_probability=r["trans_probability"], calc_score=eng.calculate_score(eng.get_aligned()))
    eng.close()
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_hip_path_vs_reference_file(c):
    """The HIP path against the case's reference file with the bars above (either f32 sum order may be the reference's).  Until that file
    is committed, the same comparison runs against the oracle's dump of the case -- the statement of the reference every other parity test
    rests on -- for EACH sum order against the oracle's matching variant (ndt_pca + KDTREE: order 0 only, as in
    test_gpu_parity.py::test_full_size_pair_vs_oracle), so the HIP side of the kit is held to those bars case by case either way."""
    path = os.path.join(GOLDEN, f"ref_{c['name']}.bin")
    if not os.path.exists(path):
        print(f"{c['name']}: {SKIP_MSG.format(name=c['name'])}; comparing with the oracle instead")
        orders = (0,) if (c["variant"] == 1 and c["mode"] == 0) else (0, 1)
        for order in orders:
            try:
                O.lib().ora_set_variant(order, 256)
                want = oracle_dump(c)
            finally:
                O.lib().ora_set_variant(0, 256)
            compare(want, engine_dump(c, order))
        return
    ref = RF.read_ref(path)
    errs = []
    for order in (0, 1):
        try:
            compare(ref, engine_dump(c, order))
            print(f"{c['name']}: the HIP path matches the reference file with MI355NDT_OPT_F32_SUM_ORDER = {order}")
            return
        except AssertionError as e:
            errs.append(e)
    raise errs[0]


@pytest.mark.gpu
def test_dumper_selfcheck_files_pass_the_comparison(tmp_path):
    """dump_golden.cpp itself, with the mi355ndt adaptor where the reference classes go: every case of cases.txt, the files it writes read back
    by ref_format.py and held against the oracle with the bars a reference file is held to (and against the HIP path through the C-ABI)."""
    exe = build_selfcheck()
    out = subprocess.run([exe, PIN, str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    for c in CASES:
        ref = RF.read_ref(str(tmp_path / f"ref_{c['name']}.bin"))
        assert ref["flags"] == 0 and ref["n_leaves"] == len(ref["leaves"]) > 0
        if c["variant"] == 1 and c["mode"] in (0, 1):
            continue                                       # ndt_pca with KDTREE / DIRECT26: chaotic runs, not comparable pose by pose
        compare(ref, oracle_dump(c))
        d = engine_dump(c, 0)
        assert np.array_equal(ref["final"], d["final"]) and ref["iterations"] == d["iterations"] and ref["calc_score"] == d["calc_score"]
