"""GPU (-m gpu): downsample_method = APPROX_VOXELGRID and use_angle_calibration on the prefilter surfaces -- mi355ndt_batch_prefilter,
mi355ndt_prefilter_p, mi355ndt_sequence_run_raw.  The yardstick is tools/prefilter_options_ref.py (the literal history-table loop, the f64
recipe; VOXELGRID cases through oracle_py.prefilter); every comparison is word for word (bytes), count and order included.  No tolerances.

Shapes: 4,160 points (one past a sort tile), 8,192 (two tiles), 9,000 with the 512 bucket words behind them (three tiles), 0 and 1.
Timings: tools/prefilter_options_timing.py, DESIGN.md section 8."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
BAD_ARG = -2
APPROX = "APPROX_VOXELGRID"
PARAM_SETS = [(0.5, 100.0, 0.1, True), (1.0, 40.0, 0.25, True), (0.5, 100.0, 0.2, False)]      # (near, far, leaf, gate)
SLOT_CAP = 8192          # the approximate grid can emit a point per input point: the largest raw cloud


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("prefilter_options_ref")
_BATCH, _REF = None, {}


def ragged_batch():
    """five pair slots: scans one past a sort tile (4,160 points) and of two tiles exactly (8,192), a 1-point cloud, a 0-point cloud, a cloud
    wholly inside distance_near, a cloud with NaN / inf rows mixed in, one cloud as 32-byte records"""
    global _BATCH
    if _BATCH is None:
        small = [[c.numpy() for c in synth.make_pair(k, 65)[:2]] for k in (50, 51, 52)]
        big = [[c.numpy() for c in synth.make_pair(k, 128)[:2]] for k in (50, 51, 52)]
        assert small[0][0].shape == (4160, 3) and big[0][0].shape == (8192, 3)
        rng = np.random.default_rng(77)
        holes = big[2][1].copy()
        holes[::97] = np.nan
        holes[5::211, 1] = np.inf
        holes[11::301, 2] = -np.inf
        rec32 = np.zeros((len(small[2][0]), 8), np.float32)
        rec32[:, :3] = small[2][0]
        rec32[:, 3:] = 7.0
        targets = [small[0][0], big[1][0], rec32, np.float32([[3.0, 4.0, 0.5]]), rng.uniform(-0.2, 0.2, (300, 3)).astype(np.float32)]
        sources = [small[0][1], big[1][1], big[2][0], np.zeros((0, 3), np.float32), holes]
        _BATCH = (targets, sources)
    return _BATCH


def reference(name, cloud, **params):
    """the restatement's answer for one cloud and parameter set; computed once, shared and left unchanged"""
    key = (name,) + tuple(sorted((k, v if np.isscalar(v) or v is None else np.asarray(v).tobytes()) for k, v in params.items()))
    if key not in _REF:
        out = R.prefilter(np.asarray(cloud, np.float32)[:, :3], params)
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def slot_bytes(eng, n):
    return [eng.batch_get_cloud(k, t).tobytes() for k in range(n) for t in (True, False)]


def run_ragged(eng, near, far, leaf, gate):
    targets, sources = ragged_batch()
    eng.batch_reserve(len(targets), SLOT_CAP, SLOT_CAP)
    return eng.batch_prefilter(targets, sources, distance_near=near, distance_far=far, downsample_resolution=leaf, use_distance_filter=gate,
                               downsample_method=APPROX)


@pytest.mark.parametrize("near,far,leaf,gate", PARAM_SETS)
def test_ragged_batch_word_for_word(near, far, leaf, gate):
    targets, sources = ragged_batch()
    eng = ndt.Engine(ndt.default_params(**PRM))
    tc, sc = run_ragged(eng, near, far, leaf, gate)
    twice = 0
    for k in range(len(targets)):
        for is_tgt, cloud, cnt in ((True, targets[k], tc[k]), (False, sources[k], sc[k])):
            exp = reference(("ragged", k, is_tgt), cloud, distance_near=near, distance_far=far, leaf=leaf, use_distance_filter=gate, downsample_method=APPROX)
            got = eng.batch_get_cloud(k, is_tgt)
            print(f"slot {k} {'target' if is_tgt else 'source'}: raw {len(cloud)} filtered {cnt} expected {len(exp)}")
            assert cnt == len(exp) == len(got), (k, is_tgt, cnt, len(exp), len(got))
            assert got.tobytes() == exp.tobytes(), (k, is_tgt)
            if len(exp):
                twice += len(exp) - len(np.unique(np.floor(exp * (np.float32(1) / np.float32(leaf))), axis=0))
    assert sc[3] == 0 and tc[3] == 1                                           # the 0-point and the 1-point cloud (|p| = 5.02 m passes every gate here)
    if gate:
        assert tc[4] == 0                                                      # wholly inside distance_near
    assert twice > 0                                                           # some cell came out more than once: this is not the VoxelGrid
    eng.close()


def lattice(cells, rng=None):
    """points in cells of the 0.25 m lattice: the centres, +- 0.05 with `rng`, so no product sits on a cell edge"""
    c = (np.asarray(cells, np.float64) + 0.5) * 0.25
    if rng is not None:
        c = c + rng.uniform(-0.05, 0.05, c.shape)
    return c.astype(np.float32)


def test_collisions_and_revisits():
    rng = np.random.default_rng(21)
    A = np.array([40, 8, 2])
    B = A + (7, -3, 0)                                                         # 7 * 3 - 3 * 7 = 0 (mod 512): A's bucket
    alternating = lattice([A if i % 2 == 0 else B for i in range(9000)], rng)
    abaab = lattice([(A, B, A, A, B)[i % 5] for i in range(4160)], rng)
    others = [A + (1 + i % 37, i % 11, 0) for i in range(100)]
    long_run = lattice(others + [A] * 5000 + others[::-1] + [B] * 3 + [A] * 2, rng)   # 5,000 consecutive points of one cell from position 100 on
    all_buckets = lattice([A + (i, 0, 0) for i in range(600)], rng)            # bucket = h(A) + 3 i: i < 512 touches every bucket, the rest revisit
    assert len({(3 * i) % 512 for i in range(600)}) == 512
    clouds = [alternating, abaab, long_run, all_buckets]
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(len(clouds), 9024, 64)
    tc, _ = eng.batch_prefilter(clouds, None, downsample_resolution=0.25, use_distance_filter=False, downsample_method=APPROX)
    for k, c in enumerate(clouds):
        exp = reference(("lattice", k), c, leaf=0.25, use_distance_filter=False, downsample_method=APPROX)
        got = eng.batch_get_cloud(k, True)
        assert tc[k] == len(exp) == len(got), (k, tc[k], len(exp))
        assert got.tobytes() == exp.tobytes(), k
    assert tc[0] == 9000 and eng.batch_get_cloud(0, True).tobytes() == alternating.tobytes()      # every point its own run, in trigger order
    assert tc[1] == 4160 // 5 * 4                                                                  # A | B | A A | B per five points
    assert tc[3] == 600                                                                            # 88 cells share a bucket with an earlier one
    eng.close()


def test_groups_change_no_word():
    want = None
    for group in (1, 2, 0):
        eng = ndt.Engine(ndt.default_params(**PRM))
        eng.set_option(ndt.OPT_PREFILTER_GROUP, group)
        counts = run_ragged(eng, 0.5, 100.0, 0.1, True)
        got = (counts, slot_bytes(eng, 5))
        if want is None:
            want = got
        assert got == want, group
        eng.close()


def test_leaf_guard_for_one_cloud_only():
    rng = np.random.default_rng(9)
    d = rng.normal(0, 1, (2, 400, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    near = (d[0] * rng.uniform(0.6, 0.95, (400, 1))).astype(np.float32)        # inside 1 m: |coord * 1e9| < 2^31
    near[100:200] = near[100]                                                   # (one run of a hundred points)
    far = (d[1] * rng.uniform(0.6, 0.95, (400, 1))).astype(np.float32)
    far[7] = [90.0, 0.0, 0.0]                                                  # 9e10 cells out
    far[9] = [150.0, 0.0, 0.0]                                                 # (gated away: it does not count)
    clouds = [far, near]
    assert R.cells_overflow(R.gate(far, 0.5, 100.0), 1e-9) and not R.cells_overflow(R.gate(near, 0.5, 100.0), 1e-9)
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(2, 512, 64)
    tc, _ = eng.batch_prefilter(clouds, None, downsample_resolution=1e-9, downsample_method=APPROX)
    msg = (eng.lib.mi355ndt_last_error(eng.h) or b"").decode()
    assert "slot 0" in msg and "too small" in msg, msg
    for k, c in enumerate(clouds):
        exp = reference(("guard", k), c, leaf=1e-9, downsample_method=APPROX)
        assert tc[k] == len(exp) and eng.batch_get_cloud(k, True).tobytes() == exp.tobytes(), k
    assert eng.batch_get_cloud(0, True).tobytes() == R.gate(far, 0.5, 100.0).tobytes()          # its gated input, in input order
    assert tc[0] == 399 and tc[1] == 301                                                        # the second went through the table
    eng.close()


def test_slot_overflow():
    scan = synth.make_pair(50, 65)[0].numpy()
    tiny = np.float32([[3.0, 4.0, 0.5], [6.0, 1.0, 0.2]])
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(3, 1024, 1024)
    with pytest.raises(ndt.NDTError) as ex:
        eng.batch_prefilter([tiny, tiny, tiny], [tiny, scan, tiny], downsample_method=APPROX)
    assert ex.value.code == BAD_ARG and "slot 1" in str(ex.value) and "source" in str(ex.value), str(ex.value)
    for k in range(3):
        assert eng.batch_get_cloud(k, True).shape == (0, 3) and eng.batch_get_cloud(k, False).shape == (0, 3)
    eng.close()


def calibration_cloud():
    c = synth.make_pair(51, 128)[0].numpy().copy()
    c[3] = [0.0, 0.0, 7.5]                                                     # on the z axis
    c[4] = [0.0, 0.0, -2.25]
    c[5] = [-0.0, 0.0, 3.0]
    c[6] = [0.0, 0.0, 0.0]                                                     # the origin
    c[40] = np.nan
    c[41, 2] = np.inf
    c[4100, 0] = -np.inf
    return c


def test_calibration_alone():
    c = calibration_cloud()
    assert len(c) == 8192
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(1, SLOT_CAP, 64)
    for cal, rad in ((True, R.ANGLE_RAD), (0.01, 0.01)):
        tc, _ = eng.batch_prefilter([c], None, downsample_resolution=0.0, use_distance_filter=False, angle_calibration=cal)
        exp = R.angle_calibration(c, rad)
        exp = exp[np.isfinite(exp).all(axis=1)]                                # (the finite test drops the three rows)
        got = eng.batch_get_cloud(0, True)
        assert tc[0] == len(exp) == 8189
        assert got.tobytes() == exp.tobytes(), cal
    assert not np.array_equal(got, c[np.isfinite(c).all(axis=1)])
    eng.close()


def the_move():
    cy, sy, cr, sr = np.cos(0.3), np.sin(0.3), np.cos(0.02), np.sin(0.02)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T[:3, 3] = [1.2, -0.4, 1.73]
    return T.astype(np.float32)


def test_calibration_in_the_chain():
    c, T = calibration_cloud(), the_move()
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(2, SLOT_CAP, 64)
    tc, _ = eng.batch_prefilter([c, c[:4160]], None, transform=T, angle_calibration=True, downsample_method=APPROX, downsample_resolution=0.2)
    for k, cloud in enumerate((c, c[:4160])):
        exp = reference(("chain", k), cloud, transform=T, angle_calibration=True, downsample_method=APPROX, leaf=0.2)
        assert tc[k] == len(exp) and eng.batch_get_cloud(k, True).tobytes() == exp.tobytes(), k
    # the VoxelGrid behind it: the oracle over the calibrated cloud
    tc, _ = eng.batch_prefilter([c, c[:4160]], None, angle_calibration=True)
    for k, cloud in enumerate((c, c[:4160])):
        exp = O.prefilter(R.angle_calibration(cloud), 0.5, 100.0, 0.1, True)
        assert tc[k] == len(exp) and eng.batch_get_cloud(k, True).tobytes() == exp.tobytes(), k
    assert eng.batch_get_cloud(0, True).tobytes() != O.prefilter(c, 0.5, 100.0, 0.1, True).tobytes()
    eng.close()


def test_single_surface():
    c, T = calibration_cloud(), the_move()
    scan = synth.make_pair(50, 65)[0].numpy()
    eng = ndt.Engine(ndt.default_params(**PRM))
    for cloud, kw in ((scan, {}), (c, dict(distance_near=1.0, distance_far=40.0, downsample_resolution=0.25)), (c, dict(downsample_resolution=0.0)),
                      (c[:0], {}), (c[:1], {})):
        want = O.prefilter(cloud, **{"leaf" if k == "downsample_resolution" else k: v for k, v in kw.items()})
        plain = eng.prefilter(cloud, **kw)               # (the two entry points run one chain: each is held to the oracle, and to the other)
        got = eng.prefilter_p(cloud, **kw)
        assert plain.tobytes() == want.tobytes() and plain.shape == want.shape
        assert got.tobytes() == want.tobytes() and got.shape == want.shape
        assert got.tobytes() == plain.tobytes() and got.shape == plain.shape
    # the whole chain: the batch slot's words, resident for the third stage
    kw = dict(transform=T, angle_calibration=True, downsample_method=APPROX, downsample_resolution=0.2)
    got = eng.prefilter_p(c, **kw)
    eng.batch_reserve(1, SLOT_CAP, 64)
    tc, _ = eng.batch_prefilter([c], None, **kw)
    assert tc[0] == len(got) and eng.batch_get_cloud(0, True).tobytes() == got.tobytes()
    assert got.tobytes() == reference(("chain", 0), c, transform=T, angle_calibration=True, downsample_method=APPROX, leaf=0.2).tobytes()
    kept = eng.prefilter_outliers()
    bc, _ = eng.batch_remove_outliers(sources=False)
    assert 0 < len(kept) < len(got) and bc[0] == len(kept) and eng.batch_get_cloud(0, True).tobytes() == kept.tobytes()
    eng.use_prefiltered(as_target=True)
    eng.use_prefiltered(as_target=False)
    assert eng.align(synth.default_guess())["iterations"] > 0 and eng.get_aligned().shape == kept.shape
    eng.close()


def test_sequence_run_raw():
    scans = [s.numpy() for s in synth.make_sequence(6, 256, n_beams=32)[0]]
    stamps = [0.1 * k for k in range(len(scans))]
    prm = dict(resolution=1.0, neighbor_mode=ndt.DIRECT1, variant=ndt.VARIANT_PCA, **PRM)
    filtered = [reference(("seq", k), s, angle_calibration=True, downsample_method=APPROX) for k, s in enumerate(scans)]
    ref_eng = ndt.Engine(ndt.default_params(**prm))
    (rf, rr), _ = ref_eng.sequence_run(filtered, stamps, keyframe_delta_trans=2.5, raw_records=True)
    eng = ndt.Engine(ndt.default_params(**prm))
    (f, r), stats, counts = eng.sequence_run_raw(scans, stamps, keyframe_delta_trans=2.5, raw_records=True, angle_calibration=True, downsample_method=APPROX)
    assert counts == [len(c) for c in filtered]
    assert bytes(f) == bytes(rf) and bytes(r) == bytes(rr)
    assert stats["prefilter_ms"] > 0 and stats["aligns"] == len(scans)
    eng.close()
    ref_eng.close()


def test_argument_errors(monkeypatch):
    tiny = np.float32([[3.0, 4.0, 0.5], [6.0, 1.0, 0.2]])
    scan = synth.make_pair(50, 65)[0].numpy()
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(2, 4160, 64)
    eng.batch_prefilter([tiny, tiny], None, downsample_method=APPROX)
    before = slot_bytes(eng, 2)
    make = ndt._prefilter_params
    for field, value in (("downsample_method", 2), ("downsample_method", -1), ("angle_calibration_rad", float("nan"))):
        def bad(*a, **k):
            p = make(*a, **k)
            setattr(p, field, value)
            return p
        monkeypatch.setattr(ndt, "_prefilter_params", bad)
        with pytest.raises(ndt.NDTError) as ex:
            eng.batch_prefilter([scan, scan], None)
        assert ex.value.code == BAD_ARG and slot_bytes(eng, 2) == before, (field, value)
        with pytest.raises(ndt.NDTError) as ex:
            eng.prefilter_p(scan)
        assert ex.value.code == BAD_ARG
    # without the word that announces it the extension is not looked at: a plain mi355ndt_prefilter_params, whatever lies behind it
    def plain(*a, **k):
        p = make(*a, **k)
        p.base.extended, p.downsample_method, p.angle_calibration_rad = 0, 7, float("nan")
        return p
    monkeypatch.setattr(ndt, "_prefilter_params", plain)
    tc, _ = eng.batch_prefilter([scan, scan], None, downsample_method=APPROX, angle_calibration=True)
    exp = O.prefilter(scan, 0.5, 100.0, 0.1, True)
    assert tc == [len(exp)] * 2 and eng.batch_get_cloud(1, True).tobytes() == exp.tobytes()
    monkeypatch.setattr(ndt, "_prefilter_params", make)
    eng.close()


# ---- mi355ndt_prefilter as a group of one: the 64-point pitch and the 4,096-point sort tile / scan chunk, where the segmented chain's tile
# and chunk counts change
GROUP_OF_ONE_N = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
GATE = (1.5, 3.5)
LEAF_TOO_SMALL = "prefilter: leaf size too small for the cloud's extent, voxel indices would overflow; cloud not down-sampled"


def clustered_cloud():
    """8,193 points in clusters of four within a centimetre (voxels of several points from the first rows on), inside and outside the
    1.5 .. 3.5 m gate, two rows not finite; row 0 passes the gate"""
    rng = np.random.default_rng(20261020)
    base = np.repeat(rng.uniform([-3.0, -3.0, -0.5], [3.0, 3.0, 0.5], (2049, 3)), 4, axis=0)
    c = (base + rng.normal(0.0, 0.01, base.shape)).astype(np.float32)[:8193]
    c[0] = [2.0, 0.5, 0.1]
    c[5] = np.nan
    c[40, 1] = np.inf
    c.setflags(write=False)
    return c


def last_error(eng):
    return (eng.lib.mi355ndt_last_error(eng.h) or b"").decode()


@pytest.fixture(scope="module")
def one_eng():
    e = ndt.Engine(ndt.default_params(**PRM))
    yield e
    e.close()


@pytest.mark.parametrize("n", GROUP_OF_ONE_N)
def test_plain_prefilter_at_pitch_and_tile_edges(one_eng, n):
    c = clustered_cloud()[:n]
    exp = {}
    for gate in (True, False):
        for leaf in (0.1, 0.0):
            exp[gate, leaf] = O.prefilter(c, *GATE, leaf, gate)
            got = one_eng.prefilter(c, *GATE, leaf, gate)
            assert got.shape == exp[gate, leaf].shape and got.tobytes() == exp[gate, leaf].tobytes(), (n, gate, leaf)
    if n > 1:                                             # the oracle's own answers are not trivial: the gate rejects, voxels hold several points
        assert 0 < len(exp[True, 0.0]) < len(exp[False, 0.0]) <= n
        assert len(exp[True, 0.1]) < len(exp[True, 0.0]) and len(exp[False, 0.1]) < len(exp[False, 0.0])
    else:
        assert len(exp[True, 0.1]) == 1


def test_plain_prefilter_leaf_too_small():
    rng = np.random.default_rng(9)
    pts = rng.uniform(-120, 120, (4097, 3)).astype(np.float32)            # 2.4e6 cells of 1e-4 m per axis
    eng = ndt.Engine(ndt.default_params(**PRM))
    assert last_error(eng) == ""
    got = eng.prefilter(pts, 0.5, 100.0, 1e-4, True)                      # (returns: the code is OK)
    d = np.sqrt((pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1]) + pts[:, 2] * pts[:, 2]).astype(np.float64)
    kept = pts[(d > 0.5) & (d < 100.0)]
    assert 0 < len(kept) < len(pts)
    assert got.shape == kept.shape and got.tobytes() == kept.tobytes()    # the gated input in input order
    assert got.tobytes() == O.prefilter(pts, 0.5, 100.0, 1e-4, True).tobytes()
    assert last_error(eng) == LEAF_TOO_SMALL
    eng.close()


def test_resident_result_follows_each_call():
    """one engine, large cloud, 1-point cloud, all-rejected cloud, large again: the count and the resident rows are those of the last call
    (read back through the stage that consumes them, RADIUS outlier removal with min_neighbors = 0: every finite point stays)"""
    c = clustered_cloud()
    rng = np.random.default_rng(78)
    inside = rng.uniform(-0.2, 0.2, (300, 3)).astype(np.float32)
    eng = ndt.Engine(ndt.default_params(**PRM))
    for cloud in (c, c[:1], inside, c[:4097]):
        exp = O.prefilter(cloud, *GATE, 0.1, True)
        got = eng.prefilter(cloud, *GATE, 0.1, True)
        assert got.shape == exp.shape and got.tobytes() == exp.tobytes()
        assert eng.prefilter(cloud, *GATE, 0.1, True, fetch=False) == len(exp)
        resident = eng.prefilter_outliers(method="RADIUS", min_neighbors=0)
        assert resident.shape == exp.shape and resident.tobytes() == exp.tobytes()
    assert len(O.prefilter(inside, *GATE, 0.1, True)) == 0 and len(O.prefilter(c[:1], *GATE, 0.1, True)) == 1
    eng.close()
