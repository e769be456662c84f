"""GPU (-m gpu): every stage of the target build alone -- k_minmax, k_griddesc, k_word_offsets, the segment sort's result, k_mark, k_rank,
k_sorted_points, the five leaf-sum kernels and k_voxels (lv_slam_amd/csrc/ndt_build.hpp, driven by ndt_host_build.hpp) -- read through
mi355ndt_get_build_buffer directly after a synchronous batch_build_targets and compared with tests/build_ref.py, the plain NumPy / mpmath
restatement of VoxelGridCovariance::applyFilter.  The cases are tests/build_cases.py's, one edge each; tests/test_build_stages_cpu.py checks the
reference against the oracle, that the cases reach their edges and that they tell a wrong build from a right one.

Word for word: the decoded extremes, every GridDesc field, the sorted keys and ids over the whole pitch, the bitmap bits and prefixes with the
all-zero landing word, head_cnt and the heads of every slice, n_voxels, seg_start, vox_idx, vox_n, kd_weight and the pca weights (these three
against the oracle, whose integer outputs hold on a discontinuity too), the batch's word total, largest grid and word offsets.
Bit for bit: the nine ordered sums, the f32 centroid, the means -- in k_leafsum with and without centroid and in both MI355NDT_LEAF_SORTED = 1
forms.  Inside derived bars: the tree sums (gamma_m * sum |terms| against math.fsum), icov and icov64 (build_ref.K_ICOV * majorant against mpmath
from the device's own sums; K measured on the oracle in test_build_stages_cpu.py), the tolerance records (head + tail to 2^-48 |mean|; c[] exactly
the f32 symmetrisation).  Every test prints its worst ratio to its bar, per quantity."""
import os

import numpy as np
import pytest
import torch                     # (before the library is loaded: torch brings its own HIP runtime and wants to be the first to open it)

import build_cases as BC
import build_ref as R
from lv_slam_amd import ndt
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

CASES = BC.all_cases()
BY_NAME = {c.name: c for c in CASES}
LEAFSUM = [c for c in CASES if c.group == "leafsum"]
INT_MIN = -2 ** 31

# what makes the build take each leaf-sum kernel (ndt_grid_state.hpp: grid_extras; ndt_host_build.hpp)
CONFIGS = {
    "base": dict(prm=dict(neighbor_mode=ndt.DIRECT7, variant=ndt.VARIANT_OMP), arith=0, sorted=False),                # k_leafsum<false>
    "full": dict(prm=dict(neighbor_mode=ndt.KDTREE, variant=ndt.VARIANT_PCA, step_size=0.01, trans_epsilon=0.1), arith=0, sorted=False),   # k_leafsum<true>, icov64, kd_weight
    "tree": dict(prm=dict(neighbor_mode=ndt.DIRECT7, variant=ndt.VARIANT_PCA), arith=1, sorted=False),                # k_leafsum_tree, recs_fast
    "sorted": dict(prm=dict(neighbor_mode=ndt.DIRECT7, variant=ndt.VARIANT_OMP), arith=0, sorted=True),               # k_sorted_points, k_leafsum<false, true>
    "sorted_full": dict(prm=dict(neighbor_mode=ndt.KDTREE, variant=ndt.VARIANT_PCA, step_size=0.01, trans_epsilon=0.1), arith=0, sorted=True),
}
MADE = {"base": (), "full": ("cent", "icov64", "kd_weight"), "tree": ("recs_fast",), "sorted": ("sorted_points",),
        "sorted_full": ("cent", "icov64", "kd_weight", "sorted_points")}


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(name):
        if name not in made:
            cfg = CONFIGS[name]
            old = os.environ.pop("MI355NDT_LEAF_SORTED", None)
            if cfg["sorted"]:
                os.environ["MI355NDT_LEAF_SORTED"] = "1"                 # read when the engine is created
            try:
                made[name] = ndt.Engine(ndt.default_params(**cfg["prm"]))
            finally:
                os.environ.pop("MI355NDT_LEAF_SORTED", None)
                if old is not None:
                    os.environ["MI355NDT_LEAF_SORTED"] = old
            if cfg["arith"]:
                made[name].set_option(ndt.OPT_ARITH, 1)
        return made[name]
    yield get
    for e in made.values():
        e.close()


def build(eng, case):
    """the case's batch through the library's own build; returns what has to stay alive while the buffers are read"""
    p = eng.get_params()
    p.resolution, p.min_points_per_voxel = case.leaf, case.min_points
    eng.set_params(p)
    K, P = len(case.clouds), case.eff_pitch
    keep = None
    if case.mode == "set":
        eng.batch_reserve(K, max(1, max(len(c) for c in case.clouds)), 64)
        for b, c in enumerate(case.clouds):
            eng.batch_set_target(b, c.reshape(-1, 3))
    else:
        rows = np.stack([r.T for r, n in case.rows()])                   # [K][3][pitch], padding included
        keep = (torch.from_numpy(np.ascontiguousarray(rows)).cuda(), torch.zeros(K * 3 * 64, device="cuda"))
        torch.cuda.synchronize()
        eng.batch_bind_device(keep[0].data_ptr(), [len(c) for c in case.clouds], P, keep[1].data_ptr(), [0] * K, 64)
    eng.batch_build_targets()
    return keep


def decode_extremes(w):
    """the six words of a target -> (min[3], max[3]) f32, or None for "no finite point yet" """
    if not w.any():
        return None
    o = np.concatenate([~w[:3] ^ np.uint32(0x80000000), w[3:] ^ np.uint32(0x80000000)]).astype(np.uint32).view(np.int32)
    f = np.where(o >= 0, o, o ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(np.float32)
    return f[:3], f[3:]


def oracle_leaves(case, b, pca):
    lv = O.Grid(case.clouds[b], O.default_params(resolution=case.leaf, min_points_per_voxel=case.min_points, variant=1 if pca else 0)).leaves()
    return lv[lv["n_pushed"] >= case.min_points]


class Worst(dict):
    def see(self, what, ratio, where):
        if ratio >= self.get(what, (-1.0,))[0]:
            self[what] = (float(ratio), where)

    def __str__(self):
        return "; ".join(f"{k} {v[0]:.3g} {v[1]}" for k, v in self.items()) or "integers only"


def check_integers(eng, case, cfg):
    """every integer buffer of every target, word for word; returns the per-target device buffers the float checks go on with"""
    T, cb, word_off, total, largest = BC.reference(case)
    P, K, mp = case.eff_pitch, len(case.clouds), case.min_points
    pca = CONFIGS[cfg]["prm"]["variant"] == ndt.VARIANT_PCA
    geo = eng.get_build_buffer("geometry")
    rpp, nsl, scap = P // mp + 1, -(-P // 256), 256 // mp + 2
    assert tuple(int(v) for v in geo) == (P, rpp, nsl, scap, cb), (case.name, geo)
    assert tuple(eng.get_build_buffer("info")) == (total, largest), case.name              # k_word_offsets: the total and the largest grid
    out = []
    for b, t in enumerate(T):
        at = (case.name, cfg, b)
        g = eng.get_build_buffer("griddesc", b)[0]
        mm = decode_extremes(eng.get_build_buffer("minmax", b))
        assert (mm is None) == (t.mm is None), at
        if mm is not None:
            assert np.array_equal(mm[0], t.mm[0]) and np.array_equal(mm[1], t.mm[1]), (at, mm, t.mm)      # (by value: -0.0 and +0.0 are one extreme)
        r = t.grid
        assert g["status"] == r.status and np.array_equal(g["min_b"], r.min_b) and np.array_equal(g["max_b"], r.max_b) and np.array_equal(g["div_b"], r.div_b), (at, g)
        assert (g["mul1"], g["mul2"], g["ncells"], g["nwords"]) == (r.mul1, r.mul2, r.ncells, r.nwords), (at, g)
        assert g["leaf"] == np.float32(r.leaf) and g["inv_leaf"] == np.float32(r.inv_leaf), at
        assert g["word_off"] == word_off[b] and g["rec_off"] == b * rpp and g["n_voxels"] == t.n_voxels, (at, g, word_off[b])
        assert np.array_equal(eng.get_build_buffer("keys", b), t.keys), at
        assert np.array_equal(eng.get_build_buffer("ids", b), t.ids), at
        w = eng.get_build_buffer("words", b)
        assert len(w) == r.nwords and np.array_equal(w["bits"], t.bits) and np.array_equal(w["prefix"], t.prefix) and not w["pad"].any(), at
        if r.nwords:
            assert w["bits"][-1] == 0 and w["prefix"][-1] == t.n_voxels, at                 # the landing word of out-of-grid probes
        hc = eng.get_build_buffer("head_cnt", b)
        assert np.array_equal(hc, t.head_cnt), (at, np.flatnonzero(hc != t.head_cnt)[:8])
        H = eng.get_build_buffer("heads", b).reshape(nsl, scap)
        for q in np.flatnonzero(t.head_cnt):
            assert np.array_equal(H[q, :t.head_cnt[q]], t.heads[q]), (at, q)
        assert np.array_equal(eng.get_build_buffer("seg_start", b), t.seg_start), at
        assert np.array_equal(eng.get_build_buffer("vox_idx", b), t.leaf_cells), at
        d = dict(t=t, vox_n=eng.get_build_buffer("vox_n", b), sums=eng.get_build_buffer("sums", b).reshape(-1, 9), vox=eng.get_voxels(b) if r.status == R.GRID_OK else None)
        if r.status == R.GRID_OK:
            lv = oracle_leaves(case, b, pca)
            assert np.array_equal(lv["idx"], t.leaf_cells), at
            assert np.array_equal(d["vox_n"], lv["n"]), (at, d["vox_n"], lv["n"])             # the count, -1 for a dead leaf
            assert np.array_equal(d["vox"]["idx"], t.leaf_cells) and np.array_equal(d["vox"]["n"], lv["n"]), at
            assert np.array_equal(d["vox"]["weight"], np.where(lv["n"] == -1, 0, lv["weight"] if pca else 1)), at
            if "kd_weight" in MADE[cfg]:
                assert np.array_equal(eng.get_build_buffer("kd_weight", b), lv["weight"]), at
            d["oracle"] = lv
        else:
            assert t.n_voxels == 0 and len(d["vox_n"]) == 0, at
        for name in ("cent", "icov64", "kd_weight", "recs_fast", "sorted_points"):
            if name in MADE[cfg]:
                d[name] = eng.get_build_buffer(name, b)
            else:
                with pytest.raises(ndt.NDTError) as e:                                       # a buffer this build did not make
                    eng.get_build_buffer(name, b)
                assert e.value.code == -2, (at, name)
        out.append(d)
    return out


def check_ordered(case, cfg, dev, worst):
    """sums, centroid and means bit for bit (the four ordered kernels)"""
    for b, d in enumerate(dev):
        t = d["t"]
        assert d["sums"].tobytes() == t.sums.tobytes(), (case.name, cfg, b, np.argwhere(d["sums"] != t.sums)[:4])
        if "cent" in d:
            assert d["cent"].tobytes() == t.cent.tobytes(), (case.name, cfg, b)
        if t.n_voxels:
            assert d["vox"]["mean"].tobytes() == (t.sums[:, :3] / t.counts[:, None]).tobytes(), (case.name, cfg, b)
    worst.see("sums |dev - ref| (bits)", 0.0, case.name)


def check_tree(case, cfg, dev, worst):
    """k_leafsum_tree: the same f64 terms in another order -- |got - exact| <= gamma_m sum |terms|, m = count + 1 (the seed); derived, not measured"""
    rows = case.rows()
    for b, d in enumerate(dev):
        t = d["t"]
        for v in range(t.n_voxels):
            P = rows[b][0][t.ids[t.seg_start[v]:t.seg_start[v] + t.counts[v]]]
            exact, mag = R.exact_sums(P)
            bar = R.gamma(int(t.counts[v]) + 1) * mag
            err = np.abs(d["sums"][v] - exact)
            worst.see("tree sums / (gamma_m sum|terms|)", float((err / bar).max()), (case.name, b, v))
            assert (err <= bar).all(), (case.name, b, v, err, bar)
        if t.n_voxels:
            assert d["vox"]["mean"].tobytes() == (d["sums"][:, :3] / t.counts[:, None]).tobytes(), (case.name, b)


def check_model(case, cfg, dev, worst):
    """icov (f32), icov64, the pca label's weight and the tolerance records against the mpmath evaluation FROM THE DEVICE'S OWN SUMS"""
    pca = CONFIGS[cfg]["prm"]["variant"] == ndt.VARIANT_PCA
    left_out = n = 0
    for b, d in enumerate(dev):
        t = d["t"]
        for v in range(t.n_voxels):
            m = R.model_cached(d["sums"][v], int(t.counts[v]), 0.01, True)
            n += 1
            if m.near_guard:
                left_out += 1                                            # (its integer outputs were compared with the oracle's)
                continue
            at = (case.name, cfg, b, v)
            vox = d["vox"][v]
            assert (vox["n"] == -1) == m.dead, at
            if "recs_fast" in d:
                f = d["recs_fast"][v]
                mean = vox["mean"]
                gap = np.abs(f["mh"].astype(np.float64) + f["ml"].astype(np.float64) - mean)
                worst.see("recs_fast head + tail / (2^-48 |mean|)", float((gap / (2.0 ** -48 * np.abs(mean))).max()), at)
                assert (gap <= 2.0 ** -48 * np.abs(mean)).all(), (at, gap)
                ic = vox["icov"]
                sym = np.array([ic[0], np.float32(0.5) * (ic[1] + ic[3]), np.float32(0.5) * (ic[2] + ic[6]), ic[4], np.float32(0.5) * (ic[5] + ic[7]), ic[8]], np.float32)
                assert f["c"].tobytes() == sym.tobytes() and not f["pad"].any() and f["weight"] == (INT_MIN if vox["n"] == -1 else vox["weight"]), (at, f)
            if m.dead:
                assert not vox["icov"].any() and vox["weight"] == 0, at
                if "icov64" in d:
                    assert not d["icov64"].reshape(-1, 9)[v].any(), at
                continue
            if pca:
                assert vox["weight"] == int(m.dim2d), (at, vox["weight"], m.dim2d)
            r32 = np.abs(vox["icov"].reshape(3, 3).astype(np.float64) - m.icov) / R.icov_majorant(m.icov, m.a, m.kappa, True)
            worst.see("icov f32 / majorant", float(r32.max()), at)
            assert r32.max() <= R.K_ICOV, (at, r32)
            if "icov64" in d:
                r64 = np.abs(d["icov64"].reshape(-1, 3, 3)[v] - m.icov) / R.icov_majorant(m.icov, m.a, m.kappa, False)
                worst.see("icov64 / majorant", float(r64.max()), at)
                assert r64.max() <= R.K_ICOV, (at, r64)
    assert left_out == 0, (case.name, left_out, n)                       # every model case is a named one


def check_sorted_points(case, dev):
    """k_sorted_points: position j holds the point ids[j] (x, y, z, 0); a bound buffer's padding rows are known too"""
    rows = case.rows()
    for b, d in enumerate(dev):
        t, P4 = d["t"], d["sorted_points"].reshape(-1, 4)
        sel = np.arange(case.eff_pitch) if case.mode == "bind" else np.flatnonzero(t.ids < rows[b][1])
        assert P4[sel, :3].tobytes() == rows[b][0][t.ids[sel]].tobytes() and not P4[:, 3].any(), (case.name, b)


def run_case(engines, case, cfg):
    eng = engines(cfg)
    keep = build(eng, case)
    worst = Worst()
    dev = check_integers(eng, case, cfg)
    (check_tree if cfg == "tree" else check_ordered)(case, cfg, dev, worst)
    if "sorted_points" in MADE[cfg]:
        check_sorted_points(case, dev)
    if case.model:
        check_model(case, cfg, dev, worst)
    del keep
    print(f"{case.name} [{cfg}]: worst ratio to its bar: {worst}")
    return dev


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_every_stage_of_the_default_build(engines, case):
    run_case(engines, case, "base")


@pytest.mark.parametrize("cfg", ["full", "tree", "sorted", "sorted_full"])
@pytest.mark.parametrize("case", LEAFSUM, ids=[c.name for c in LEAFSUM])
def test_every_leaf_sum_kernel(engines, case, cfg):
    run_case(engines, case, cfg)


@pytest.mark.parametrize("cfg", ["full", "tree", "sorted"])
@pytest.mark.parametrize("name", ["markrank_mp6", "markrank_mp12", "bitmap_sparse_over_262144_cells", "griddesc_statuses", "minmax_n3077_K3"])
def test_the_other_stages_under_the_other_builds(engines, name, cfg):
    run_case(engines, BY_NAME[name], cfg)


@pytest.mark.parametrize("pair", [("base", "sorted"), ("full", "sorted_full")], ids=["no_centroid", "centroid"])
def test_sorted_leaf_sums_equal_the_default_byte_for_byte(engines, pair):
    """MI355NDT_LEAF_SORTED = 1 (k_sorted_points + k_leafsum<..., SORTED = true>) against the default engine on ragged batches"""
    for name in ("leafsum_n_voxels", "leafsum_K9", "leafsum_sizes_at_580m"):
        case = BY_NAME[name]
        got = []
        for cfg in pair:
            eng = engines(cfg)
            keep = build(eng, case)
            got.append([(eng.get_voxels(b).tobytes(), eng.get_build_buffer("sums", b).tobytes(), eng.get_build_buffer("vox_n", b).tobytes(),
                         eng.get_build_buffer("cent", b).tobytes() if "cent" in MADE[cfg] else b"") for b in range(len(case.clouds))])
            del keep
        assert got[0] == got[1], name
    print(f"sorted vs default {pair}: voxels, sums, counts and centroids equal byte for byte")


def test_hook_refuses_what_it_cannot_serve(engines):
    eng = engines("base")
    build(eng, BY_NAME["leafsum_K1"])
    nb = ndt.C.c_size_t(0)
    L, h = eng.lib, eng.h
    assert L.mi355ndt_get_build_buffer(h, 99, 0, None, 0, ndt.C.byref(nb)) == -2            # an unknown buffer
    assert L.mi355ndt_get_build_buffer(h, 0, 1, None, 0, ndt.C.byref(nb)) == -2             # no such pair
    assert L.mi355ndt_get_build_buffer(h, 3, 0, None, 0, ndt.C.byref(nb)) == 0 and nb.value == 4 * BY_NAME["leafsum_K1"].eff_pitch
    small = np.zeros(4, np.uint8)
    assert L.mi355ndt_get_build_buffer(h, 3, 0, small.ctypes.data_as(ndt.C.c_void_p), 4, ndt.C.byref(nb)) == -2       # too small
    fresh = ndt.Engine(ndt.default_params())
    fresh.batch_reserve(1, 64, 64)
    assert L.mi355ndt_get_build_buffer(fresh.h, 0, 0, None, 0, ndt.C.byref(nb)) == -7       # nothing built: MI355NDT_ERR_STATE
    fresh.stream_begin(2, 1, 64, 64)
    assert L.mi355ndt_get_build_buffer(fresh.h, 0, 0, None, 0, ndt.C.byref(nb)) == -7       # a stream session
    fresh.stream_end()
    fresh.close()


# ------------------------------------------------------------------------------------------------ tests/hip/build_check: what points cannot reach
MAGIC, GUARD, FILL = 0x31434C42, 64, 0xA5A5A5A5
REC_DTYPE = np.dtype([("mean", "<f8", 3), ("icov", "<f4", 9), ("weight", "<i4")])


class Results:
    """the helper's output file: buffer after buffer as [n] [64 guard words] [n words] [64 guard words]"""

    def __init__(self, path):
        self.w = np.fromfile(path, np.uint32)
        self.at = 0

    def buf(self):
        n = int(self.w[self.at])
        lo, body, hi = np.split(self.w[self.at + 1:self.at + 1 + n + 2 * GUARD], [GUARD, GUARD + n])
        assert len(hi) == GUARD, "short result file"
        self.at += 1 + n + 2 * GUARD
        assert (lo == FILL).all() and (hi == FILL).all(), "a guard word was written"
        return body

    def done(self):
        return self.at == len(self.w)


def run_helper(tmp_path, mode, cases):
    import subprocess
    import __graft_entry__ as entry
    exe = entry.build_build_check()
    blob = np.concatenate([np.array([MAGIC, mode, len(cases)], np.uint32)] + [np.ascontiguousarray(p).view(np.uint32).ravel() for c in cases for p in c])
    blob.tofile(tmp_path / "in.u32")
    run = subprocess.run([exe, "run", str(tmp_path / "in.u32"), str(tmp_path / "out.u32")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return Results(tmp_path / "out.u32")


def test_k_voxels_alone_on_synthetic_sums(tmp_path):
    """k_voxels launched directly (one thread per record slot; two blocks): every output between its guard words, entries past n_voxels untouched,
    both eig_mult, pca on and off, and once with no optional output at all"""
    VC = BC.voxel_cases() * 6                                            # 276 leaves: the second block
    nv, cap = len(VC), len(VC) + 9
    sums = np.stack([s for _, _, s, _ in VC])
    counts = np.array([n for _, n, _, _ in VC], np.int32)
    runs = [(pca, 7, em) for pca in (0, 1) for em in BC.EIG_MULTS] + [(1, 0, 0.01)]
    res = run_helper(tmp_path, 1, [(np.array([nv, cap, pca, opt], np.uint32), np.array([em], np.float64), sums, counts) for pca, opt, em in runs])
    worst = Worst()
    for pca, opt, em in runs:
        recs, vox_n = res.buf().view(REC_DTYPE), res.buf().view(np.int32)
        icov64, kdw, fast = res.buf().view(np.float64).reshape(-1, 9), res.buf().view(np.int32), res.buf().view(ndt.RECF_DTYPE)
        assert len(recs) == cap and len(vox_n) == cap and len(icov64) == len(kdw) == len(fast) == (cap if opt else 0)
        for b in (recs, vox_n, icov64, kdw, fast):                       # entries past n_voxels: untouched
            assert (b[nv:].view(np.uint32) == FILL).all() if len(b) else True
        for v, (name, n, s, expect) in enumerate(VC):
            at = (name, pca, em)
            m = R.model_cached(s, n, em, True)
            r = recs[v]
            assert r["mean"].tobytes() == (s[:3] / n).tobytes(), at
            if expect == "bad_inverse":                                  # alive through the eigenvalue test (m.dead is False), 0 / 0 in the cofactor inverse
                assert not m.dead and vox_n[v] == -1 and r["weight"] == INT_MIN and not np.isfinite(r["icov"]).any(), (at, r, vox_n[v])
                if opt:
                    assert not np.isfinite(icov64[v]).any() and kdw[v] == (int(m.dim2d) if pca else 0) and fast[v]["weight"] == INT_MIN, at
                continue
            assert not m.near_guard, at                                  # a named case: never left out
            assert vox_n[v] == (-1 if m.dead else n), (at, vox_n[v])
            want_w = INT_MIN if m.dead else (int(m.dim2d) if pca else 1)
            assert r["weight"] == want_w, (at, r["weight"], want_w, m.dim2d)
            if opt:
                assert kdw[v] == (0 if m.dead or not pca else int(m.dim2d)), at
                f, ic = fast[v], r["icov"]
                gap = np.abs(f["mh"].astype(np.float64) + f["ml"].astype(np.float64) - r["mean"])
                assert (gap <= 2.0 ** -48 * np.abs(r["mean"])).all(), (at, gap)
                worst.see("recs_fast head + tail / (2^-48 |mean|)", float((gap / np.maximum(2.0 ** -48 * np.abs(r["mean"]), 1e-300)).max()), at)
                sym = np.array([ic[0], np.float32(0.5) * (ic[1] + ic[3]), np.float32(0.5) * (ic[2] + ic[6]), ic[4], np.float32(0.5) * (ic[5] + ic[7]), ic[8]], np.float32)
                assert f["c"].tobytes() == sym.tobytes() and not f["pad"].any() and f["weight"] == want_w, (at, f)
            if m.dead:
                assert not r["icov"].any() and (not opt or not icov64[v].any()), at
                continue
            r32 = np.abs(r["icov"].reshape(3, 3).astype(np.float64) - m.icov) / R.icov_majorant(m.icov, m.a, m.kappa, True)
            worst.see("icov f32 / majorant", float(r32.max()), at)
            assert r32.max() <= R.K_ICOV, (at, r32)
            if opt:
                r64 = np.abs(icov64[v].reshape(3, 3) - m.icov) / R.icov_majorant(m.icov, m.a, m.kappa, False)
                worst.see("icov64 / majorant", float(r64.max()), at)
                assert r64.max() <= R.K_ICOV, (at, r64)
    assert res.done()
    print(f"k_voxels alone: worst ratio to its bar: {worst}")


def test_k_build_check_alone(tmp_path):
    """the planned build's fit test: the three status words, and every grid of a misfit batch turned to GRID_CAP with zero words, cells and voxels"""
    cases, inputs = BC.build_check_cases(), []
    rng = np.random.default_rng(20261020)
    for name, B, plan_words, plan_cb, total, largest in cases:
        gd = np.stack([rng.integers(0, 2, B), rng.integers(1, 5000, B), rng.integers(1, 80, B), rng.integers(0, 70000, B), rng.integers(0, 900, B)], axis=1).astype(np.uint32)
        nwords = gd[:, 2].copy()
        inputs.append((np.array([B, plan_words, plan_cb, total, largest], np.uint32), gd, nwords))
    res = run_helper(tmp_path, 2, inputs)
    for (name, B, plan_words, plan_cb, total, largest), (_, gd, nwords) in zip(cases, inputs):
        fits = total <= plan_words and (plan_cb >= 31 or largest + 1 <= (1 << plan_cb))
        assert fits == name.startswith(("fits", "plan_cb")), name
        stat, g, nw = res.buf(), res.buf().view(ndt.GRIDDESC_DTYPE), res.buf()
        assert tuple(stat) == (total, largest, 0 if fits else 1), (name, stat)
        assert np.array_equal(g["rec_off"], 7 * np.arange(B)) and np.array_equal(g["mul1"], 1 + np.arange(B)) and not g["min_b"].any() and not g["leaf"].any(), name
        got = np.stack([g["status"], g["ncells"], g["nwords"], g["word_off"], g["n_voxels"]], axis=1)
        want = gd if fits else np.tile(np.array([R.GRID_CAP, 0, 0, 0, 0], np.uint32), (B, 1))
        assert np.array_equal(got, want) and np.array_equal(nw, nwords if fits else np.zeros(B, np.uint32)), name
    assert res.done()
