"""GPU (-m gpu): mi355ndt_batch_remove_outliers / mi355ndt_sequence_run_raw_outliers -- PrefilteringNodelet::outlier_removal over whole batches
of slot clouds on the device.  The yardsticks are tools/outlier_ref.py, applied to what batch_get_cloud returned before the call, and the
single surface on a second engine (prefilter with the distance filter off and no down-sampling + prefilter_outliers).  Every comparison is
word for word: counts, order, the survivors as bytes, mean / stddev / threshold as f64 bytes.  No tolerances, no excluded cases.  (Where the
restatement's statistic is NaN -- a cloud with no valid point -- the engine's must be NaN too: a NaN's sign and payload are the producing
hardware's and say nothing, so NaNs are compared as NaNs.)

Timings: tools/batch_prefilter_timing.py --outliers, DESIGN.md section 8 (batch outlier removal)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
BAD_ARG, ERR_STATE = -2, -7
STAT20 = dict(mean_k=20, stddev_mul=1.0)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("outlier_ref")
_REF = {}


def ref(cloud, method, **kw):
    """the restatement's answer, computed once per (cloud bytes, parameters) and shared by every test; left unchanged"""
    key = (np.ascontiguousarray(cloud, np.float32).tobytes(), method, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = R.statistical(cloud, **kw) if method == "STATISTICAL" else R.radius(cloud, **kw)
    return _REF[key]


def second_engine(**prm):
    key = ("engine", tuple(sorted(prm.items())))
    if key not in _REF:
        _REF[key] = ndt.Engine(ndt.default_params(**dict(PRM, **prm)))
    return _REF[key]


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(**PRM))
    yield e
    e.close()
    for k in [k for k in _REF if k[0] == "engine"]:
        _REF.pop(k).close()


def blobs():
    """the 3,000-point cloud of test_outlier_gpu.py: 2,900 points in three dense blobs on a 0.1 m jittered lattice, 100 isolated points 5-60 m away"""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3) * 0.1
    parts = [(g[:m] + rng.uniform(-0.03, 0.03, (m, 3)) + c) for m, c in ((967, (0, 0, 0)), (967, (8, 3, 0)), (966, (-5, 10, 1)))]
    d = rng.normal(size=(100, 3))
    far = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(5, 60, (100, 1))
    p = np.concatenate(parts + [far]).astype(np.float32)
    return p[rng.permutation(len(p))]


BLOBS = blobs()


def sheet():
    """the 0.5 m sheet of test_points_on_cell_boundaries_and_duplicates with its 50 duplicates"""
    i, j = np.meshgrid(np.arange(40), np.arange(40), indexing="ij")
    s = np.stack([i.ravel() * 0.5, j.ravel() * 0.5 - 10.0, np.full(1600, 1.5)], 1).astype(np.float32)
    return np.concatenate([s, s[np.random.default_rng(3).choice(1600, 50, replace=False)]])


def set_slots(e, targets, sources, cap):
    """batch_reserve + mi355ndt_batch_set_clouds over slots 0 .. n - 1 (either side may be None); returns what batch_get_cloud gives back"""
    side = [None if cl is None else [np.ascontiguousarray(c, np.float32) for c in cl] for cl in (targets, sources)]
    n = len(side[0] if side[0] is not None else side[1])
    e.batch_reserve(n, cap, cap)
    tab = [(None, None) if s is None else ([c.ctypes.data for c in s], [len(c) for c in s]) for s in side]
    e.batch_set_clouds_raw(0, tab[0][0], tab[0][1], tab[1][0], tab[1][1], 12)
    e.synchronize()
    held = {(k, t): e.batch_get_cloud(k, t) for t, s in ((True, side[0]), (False, side[1])) if s is not None for k in range(n)}
    for (k, t), got in held.items():
        assert got.tobytes() == side[0 if t else 1][k].tobytes(), (k, t)        # the slots hold the clouds as given, NaN and inf rows included
    return held


def f64w(x):
    return np.float64(x).tobytes()


def same_stats(st, x, where):
    assert (st["n_in"], st["n_valid"]) == (x["n_in"], x["n_valid"]), where
    for key in ("mean", "stddev", "threshold"):
        if np.isnan(x[key]):
            assert np.isnan(st[key]), (where, key)
        else:
            assert f64w(st[key]) == f64w(x[key]), (where, key, st[key], x[key])


def check_slots(e, held, keys, counts, stats, method, **kw):
    """slots `keys` ((slot, is_target)) after a call against the restatement over what they held before; counts / stats: {key: value}"""
    for key in keys:
        before = held[key]
        if len(before) == 0:
            assert counts[key] == 0 and e.batch_get_cloud(*key).shape == (0, 3), key
            assert set(stats[key].values()) == {0}, (key, stats[key])
            continue
        x = ref(before, method, **kw)
        got = e.batch_get_cloud(*key)
        print(f"{key} {method} {kw}: n_in {len(before)} kept {len(got)} stats {stats[key]} | restatement kept {len(x['kept'])} threshold {x['threshold']!r}")
        assert counts[key] == len(got) == len(x["kept"]), (key, counts[key], len(got), len(x["kept"]))
        assert got.tobytes() == before[x["kept"]].tobytes(), key
        if method == "STATISTICAL":
            same_stats(stats[key], x, key)
        else:
            assert set(stats[key].values()) == {0}, (key, stats[key])


def run(e, n, method="STATISTICAL", first_pair=0, targets=True, sources=True, **kw):
    """batch_remove_outliers with stats; returns ({key: count}, {key: stats})"""
    tc, sc, ts, ss = e.batch_remove_outliers(first_pair, n, targets, sources, method=method, return_stats=True, **kw)
    counts, stats = {}, {}
    for t, c, s in ((True, tc, ts), (False, sc, ss)):
        if c is not None:
            assert len(c) == len(s) == n
            counts.update({(first_pair + k, t): c[k] for k in range(n)})
            stats.update({(first_pair + k, t): s[k] for k in range(n)})
    return counts, stats


def slot_bytes(e, n):
    return [e.batch_get_cloud(k, t).tobytes() for k in range(n) for t in (True, False)]


# ---- 1
@pytest.mark.parametrize("method,kw", [("STATISTICAL", STAT20), ("RADIUS", dict(radius=0.5, min_neighbors=5))])
def test_ragged_counts_in_one_launch(eng, method, kw):
    # 1: one lane; 20 = mean_k: nothing valid, NaN threshold, all kept; 21: every list exactly full; 257: a fifth block with one live lane; 0: stays empty
    small = {n: np.random.default_rng(n).normal(0, 0.5, (n, 3)).astype(np.float32) for n in (1, 20, 21, 257, 0)}
    order_t, order_s = (1, 20, 21, 257, 0), (257, 0, 21, 1, 20)
    held = set_slots(eng, [small[n] for n in order_t], [small[n] for n in order_s], 320)
    counts, stats = run(eng, 5, method, **kw)
    check_slots(eng, held, list(held), counts, stats, method, **kw)
    if method == "STATISTICAL":
        for k in range(5):
            for t, n in ((True, order_t[k]), (False, order_s[k])):
                st = stats[(k, t)]
                if n == 0:
                    continue
                assert st["n_in"] == n and st["n_valid"] == (n if n > 20 else 0)
                assert np.isnan(st["threshold"]) == (n <= 20)
                if n <= 20:
                    assert counts[(k, t)] == n
        assert counts[(3, True)] < 257                                          # the stage removes something


# ---- 2
@pytest.mark.parametrize("mean_k", [1, 32, 33, 64])
def test_both_list_capacities(eng, mean_k):
    rolls = (0, 1, 777, 2048)
    held = set_slots(eng, [np.roll(BLOBS, r, axis=0) for r in rolls], None, 3008)
    counts, stats = run(eng, 4, sources=False, mean_k=mean_k, stddev_mul=1.0)
    check_slots(eng, held, list(held), counts, stats, "STATISTICAL", mean_k=mean_k, stddev_mul=1.0)
    kept = [np.unique(eng.batch_get_cloud(k, True), axis=0) for k in range(4)]
    assert 2000 < len(kept[0]) < 3000
    for k in range(1, 4):                                                       # other ids, the same kept set
        assert kept[k].tobytes() == kept[0].tobytes(), k
        assert stats[(k, True)]["n_valid"] == 3000


# ---- 3
@pytest.mark.parametrize("method,kw", [("STATISTICAL", STAT20), ("RADIUS", dict(radius=0.5, min_neighbors=5))])
def test_lattice_and_no_lattice_together(eng, method, kw):
    stray = np.concatenate([BLOBS, np.array([[1e12, 0, 0]], np.float32)])      # no lattice: the exhaustive variant
    holes = BLOBS[:600].copy()
    holes[100, 0] = np.nan
    holes[433, 2] = np.nan
    holes[17, 1] = np.inf
    holes[250] = -np.inf
    held = set_slots(eng, [BLOBS, stray, np.roll(BLOBS, 5, axis=0), holes], None, 3008)
    counts, stats = run(eng, 4, method, sources=False, **kw)
    check_slots(eng, held, list(held), counts, stats, method, **kw)
    x = ref(holes, method, **kw)
    bad = [17, 100, 250, 433]
    if method == "STATISTICAL":                                                # not searchable: dist 0, not valid, kept
        assert all(x["dist"][i] == 0 for i in bad) and set(bad) <= set(x["kept"].tolist()) and x["n_valid"] == 596
        assert not np.isfinite(eng.batch_get_cloud(3, True)).all()
    else:                                                                      # RADIUS removes them
        assert not set(bad) & set(x["kept"].tolist())
        assert np.isfinite(eng.batch_get_cloud(3, True)).all()


# ---- 4
@pytest.mark.parametrize("method,kw", [("STATISTICAL", dict(mean_k=20, stddev_mul=0.5)), ("STATISTICAL", dict(mean_k=4, stddev_mul=1.0)),
                                       ("RADIUS", dict(radius=0.5, min_neighbors=1)), ("RADIUS", dict(radius=0.75, min_neighbors=5))])
def test_ties(eng, method, kw):
    p = sheet()
    eng.set_option(ndt.OPT_OUTLIER_CELL_MM, 500)                               # the sheet's points sit on the cells' boundaries
    try:
        held = set_slots(eng, [p, BLOBS, p], None, 3008)
        counts, stats = run(eng, 3, method, sources=False, **kw)
        check_slots(eng, held, list(held), counts, stats, method, **kw)
        assert eng.batch_get_cloud(0, True).tobytes() == eng.batch_get_cloud(2, True).tobytes()
    finally:
        eng.set_option(ndt.OPT_OUTLIER_CELL_MM, 100)


# ---- 5
def test_sides_offsets_untouched_slots(eng):
    tg = [BLOBS[400 * k: 400 * k + 1000] for k in range(6)]
    sr = [BLOBS[300 * k: 300 * k + 800] for k in range(6)]
    held = set_slots(eng, tg, sr, 1024)
    tc, sc = eng.batch_remove_outliers(first_pair=2, n=3, targets=True, sources=False)
    assert sc is None and len(tc) == 3
    touched = [(k, True) for k in (2, 3, 4)]
    counts, stats = run(eng, 3, first_pair=2, sources=False, method="RADIUS", min_neighbors=0)   # (every survivor is searchable: the counts again, nothing removed)
    assert [counts[k] for k in touched] == tc
    x = {k: ref(held[k], "STATISTICAL", **STAT20) for k in touched}
    for j, k in enumerate(touched):
        assert tc[j] == len(x[k]["kept"]) and eng.batch_get_cloud(*k).tobytes() == held[k][x[k]["kept"]].tobytes(), k
    assert any(tc[j] < 1000 for j in range(3))
    for k in range(6):
        assert eng.batch_get_cloud(k, False).tobytes() == held[(k, False)].tobytes(), k
        if k not in (2, 3, 4):
            assert eng.batch_get_cloud(k, True).tobytes() == held[(k, True)].tobytes(), k


# ---- 6
def test_groups_change_no_word(eng):
    ref_eng = second_engine()
    clouds = [ref_eng.prefilter(c.numpy()) for k in (60, 61, 62, 63) for c in synth.make_pair(k, 65)[:2]]
    assert all(3000 < len(c) < 4160 for c in clouds)
    want = None
    for group in (3, 0):
        eng.set_option(ndt.OPT_PREFILTER_GROUP, group)
        try:
            held = set_slots(eng, clouds[0::2], clouds[1::2], 4160)
            counts, stats = run(eng, 4, **STAT20)
        finally:
            eng.set_option(ndt.OPT_PREFILTER_GROUP, 0)
        got = (counts, {k: {n: f64w(v) for n, v in s.items()} for k, s in stats.items()}, slot_bytes(eng, 4))
        if want is None:
            want = got
            keys = [(0, True), (3, False)]                                      # the first cloud of the first group and the last of the last
            check_slots(eng, held, keys, counts, stats, "STATISTICAL", **STAT20)
            assert all(0 < counts[k] < len(held[k]) for k in held)
        assert got == want, group


# ---- 7
@pytest.mark.parametrize("method,kw,kept51", [("STATISTICAL", {}, (7008, 7138)), ("RADIUS", dict(method="RADIUS"), (6989, 6992))])
def test_aligns_follow(eng, method, kw, kept51):
    pairs = [[c.numpy() for c in synth.make_pair(k, 128)[:2]] for k in (51, 52)]
    ref_eng = second_engine()
    survivors = []
    for p in pairs:
        for c in p:
            f = ref_eng.prefilter(c)                                            # 0.5 / 100 m, 0.1 m: the keyword defaults of batch_prefilter
            x = ref(f, method, **(STAT20 if method == "STATISTICAL" else dict(radius=0.8, min_neighbors=2)))
            survivors.append(f[x["kept"]])
    assert (len(survivors[0]), len(survivors[1])) == kept51                    # of 7,563 and 7,612: the stage removes something and not everything
    eng.batch_reserve(2, 8192, 8192)
    tc, sc = eng.batch_prefilter([p[0] for p in pairs], [p[1] for p in pairs], outlier=kw)
    assert tc == [len(survivors[0]), len(survivors[2])] and sc == [len(survivors[1]), len(survivors[3])]
    set_slots(ref_eng, survivors[0::2], survivors[1::2], 8192)
    G = np.ascontiguousarray(np.transpose(np.broadcast_to(synth.default_guess(), (2, 4, 4)), (0, 2, 1))).reshape(2, 16)
    out = []
    for e in (eng, ref_eng):
        e.batch_build_targets()
        res = (ndt.Result * 2)()
        e.batch_align_raw(G, res)
        out.append(bytes(res))
        assert all(r.iterations > 0 for r in res)
    assert out[0] == out[1]


# ---- 8
def test_the_fused_keywords(eng):
    """the ragged shapes of test_batch_prefilter_gpu.py: a scan one past a sort tile and one of two tiles exactly, a 32-byte-record cloud, a 1-point
    and a 0-point cloud, a cloud wholly inside distance_near, a cloud with NaN / inf rows"""
    small = [[c.numpy() for c in synth.make_pair(k, 65)[:2]] for k in (50, 52)]
    big = [[c.numpy() for c in synth.make_pair(k, 128)[:2]] for k in (51, 52)]
    holes = big[1][1].copy()
    holes[::97] = np.nan
    holes[5::211, 1] = np.inf
    holes[11::301, 2] = -np.inf
    rec32 = np.zeros((len(small[1][0]), 8), np.float32)
    rec32[:, :3] = small[1][0]
    rec32[:, 3:] = 7.0
    targets = [small[0][0], big[0][0], rec32, np.float32([[3.0, 4.0, 0.5]]), np.random.default_rng(77).uniform(-0.2, 0.2, (300, 3)).astype(np.float32)]
    sources = [small[0][1], big[0][1], big[1][0], np.zeros((0, 3), np.float32), holes]
    eng.batch_reserve(5, 8192, 8192)
    tc, sc = eng.batch_prefilter(targets, sources, outlier={})
    ref_eng = second_engine()
    for k in range(5):
        for t, cloud, cnt in ((True, targets[k], tc[k]), (False, sources[k], sc[k])):
            exp = ref_eng.prefilter(np.ascontiguousarray(cloud[:, :3]), outlier={}) if len(cloud) else np.zeros((0, 3), np.float32)
            got = eng.batch_get_cloud(k, t)
            assert cnt == len(exp) == len(got), (k, t, cnt, len(exp), len(got))
            assert got.tobytes() == exp.tobytes(), (k, t)
    assert tc[3] == 1 and sc[3] == 0 and tc[4] == 0


# ---- 9
def test_sequence(eng):
    scans = [s.numpy() for s in synth.make_sequence(6, 256, n_beams=32)[0]]
    assert all(s.shape == (8192, 3) for s in scans)
    stamps = [0.1 * k for k in range(len(scans))]
    a = second_engine()
    # with the third stage: per-frame prefilter(outlier={}) + sequence_run
    filtered = [a.prefilter(s, outlier={}) for s in scans]
    (rf, rr), _ = a.sequence_run(filtered, stamps, keyframe_delta_trans=2.5, raw_records=True)
    (f, r), stats, counts = eng.sequence_run_raw(scans, stamps, keyframe_delta_trans=2.5, raw_records=True, outlier={})
    assert counts == [len(c) for c in filtered]
    assert bytes(f) == bytes(rf) and bytes(r) == bytes(rr)
    assert stats["prefilter_ms"] > 0 and stats["aligns"] == len(scans)
    plain = [a.prefilter(s) for s in scans]
    assert all(len(x) < len(y) for x, y in zip(filtered, plain))               # the stage removed points from every frame
    # without it: the slots and the records of batch_prefilter + sequence_run
    (f0, r0), _, counts0 = eng.sequence_run_raw(scans, stamps, keyframe_delta_trans=2.5, raw_records=True)
    slots = [eng.batch_get_cloud(k, True).tobytes() for k in range(len(scans))]
    a.batch_reserve(len(scans), 8192, 64)
    tc, _ = a.batch_prefilter(scans, None)
    assert counts0 == tc == [len(c) for c in plain]
    assert slots == [a.batch_get_cloud(k, True).tobytes() for k in range(len(scans))] == [c.tobytes() for c in plain]
    (pf, pr), _ = a.sequence_run(plain, stamps, keyframe_delta_trans=2.5, raw_records=True)
    assert bytes(f0) == bytes(pf) and bytes(r0) == bytes(pr)
    assert bytes(f0) != bytes(f)


# ---- 10
def test_refusals(eng):
    held = set_slots(eng, [BLOBS[:500], BLOBS[500:1000]], [BLOBS[1000:1500], BLOBS[1500:2000]], 512)
    before = slot_bytes(eng, 2)
    for kw in (dict(mean_k=0), dict(mean_k=65), dict(stddev_mul=float("nan")), dict(method="RADIUS", radius=-1.0), dict(method="RADIUS", radius=float("nan")),
               dict(method="RADIUS", min_neighbors=65), dict(method="NO_SUCH_METHOD"), dict(first_pair=1, n=2), dict(first_pair=-1, n=1), dict(n=0)):
        with pytest.raises(ndt.NDTError) as ex:
            eng.batch_remove_outliers(**kw)
        assert ex.value.code == BAD_ARG, kw
        assert "batch_remove_outliers:" in str(ex.value), str(ex.value)
        assert slot_bytes(eng, 2) == before, kw
    prm = ndt.OutlierParams(ndt.OUTLIER_STATISTICAL, 20, 1.0, 0.8, 2)
    for sides in (0, 4, -1):                                                   # (the wrapper refuses "no side" itself: the library's own answer)
        assert eng.lib.mi355ndt_batch_remove_outliers(eng.h, 0, 2, sides, C.byref(prm), None, None, None, None) == BAD_ARG, sides
        assert slot_bytes(eng, 2) == before, sides
    assert eng.lib.mi355ndt_batch_remove_outliers(eng.h, 0, 2, 3, None, None, None, None, None) == ndt.OK      # NULL params: the defaults
    x = [ref(held[(k, t)], "STATISTICAL", **STAT20) for k in range(2) for t in (True, False)]
    assert slot_bytes(eng, 2) == [held[(k, t)][x[2 * k + (0 if t else 1)]["kept"]].tobytes() for k in range(2) for t in (True, False)]
    # a side that has never been given a cloud
    e1 = ndt.Engine(ndt.default_params(**PRM))
    set_slots(e1, [BLOBS[:100]], None, 128)
    with pytest.raises(ndt.NDTError) as ex:
        e1.batch_remove_outliers(targets=False, sources=True)
    assert ex.value.code == BAD_ARG
    assert e1.batch_remove_outliers(sources=False)[0] == [len(ref(BLOBS[:100], "STATISTICAL", **STAT20)["kept"])]
    e1.close()
    # a bound device batch
    import torch
    e2 = ndt.Engine(ndt.default_params(**PRM))
    dt = torch.ones(2, 3, 64, dtype=torch.float32, device="cuda")
    ds = torch.ones(2, 3, 64, dtype=torch.float32, device="cuda")
    e2.batch_bind_device(dt.data_ptr(), [2, 2], 64, ds.data_ptr(), [2, 2], 64)
    with pytest.raises(ndt.NDTError) as ex:
        e2.batch_remove_outliers()
    assert ex.value.code == BAD_ARG
    torch.cuda.synchronize()
    assert bool((dt == 1).all()) and bool((ds == 1).all())
    e2.close()
    # stream mode
    e3 = ndt.Engine(ndt.default_params(**PRM))
    e3.batch_reserve(2, 64, 64)
    e3.stream_begin(2, 2, 64, 64)
    with pytest.raises(ndt.NDTError) as ex:
        e3.batch_remove_outliers(n=2)
    assert ex.value.code == ERR_STATE
    e3.stream_end()
    e3.close()
