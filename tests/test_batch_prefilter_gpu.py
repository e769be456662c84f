"""GPU (-m gpu): mi355ndt_batch_prefilter / mi355ndt_batch_get_cloud / mi355ndt_sequence_run_raw -- whole batches of RAW scans through the
prefilter on the device, into the batch slots.  The yardsticks are the single surface (Engine.prefilter of a second engine) and
oracle_py.prefilter; every comparison is word for word (np.array_equal, bytes), count and order included.  No tolerances.

Timings: tools/batch_prefilter_timing.py, DESIGN.md section 8 (batch prefilter)."""
import numpy as np
import pytest

from lv_slam_amd import ndt, synth
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
BAD_ARG, ERR_STATE = -2, -7
# (near, far, leaf, gate): the sets of test_prefilter_next_row_n2
PARAM_SETS = [(0.5, 100.0, 0.1, True), (0.5, 100.0, 0.0, True), (1.0, 40.0, 0.25, True), (0.5, 100.0, 0.2, False)]
SLOT_CAP = 8192          # these scans filter to at most 7,638 points at 0.1 m; without down-sampling a cloud keeps at most its 8,192 raw points

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


def reference(name, cloud, near, far, leaf, gate):
    """the single surface's answer (a second engine) for one cloud and parameter set, checked against the oracle; computed once and shared"""
    key = (name, near, far, leaf, gate)
    if key not in _REF:
        if "eng" not in _REF:
            _REF["eng"] = ndt.Engine(ndt.default_params(**PRM))
        xyz = np.ascontiguousarray(np.asarray(cloud, np.float32)[:, :3])
        got = _REF["eng"].prefilter(xyz, near, far, leaf, gate)
        assert np.array_equal(got, O.prefilter(xyz, near, far, leaf, gate))
        got.setflags(write=False)
        _REF[key] = got
    return _REF[key]


def slot_bytes(eng, n):
    return [eng.batch_get_cloud(k, t).tobytes() for k in range(n) for t in (True, False)]


def set_clouds(eng, targets, sources):
    """mi355ndt_batch_set_clouds over slots 0 .. n - 1"""
    t = [np.ascontiguousarray(c, np.float32) for c in targets]
    s = [np.ascontiguousarray(c, np.float32) for c in sources]
    eng.batch_set_clouds_raw(0, [c.ctypes.data for c in t], [len(c) for c in t], [c.ctypes.data for c in s], [len(c) for c in s], 12)
    eng.synchronize()                                                           # (t and s are staged before the call returns; this keeps the test simple)


def run_ragged(eng, near, far, leaf, gate):
    targets, sources = ragged_batch()
    eng.batch_reserve(len(targets), SLOT_CAP, SLOT_CAP)
    return eng.batch_prefilter(targets, sources, distance_near=near, distance_far=far, downsample_resolution=leaf, use_distance_filter=gate)


@pytest.mark.parametrize("near,far,leaf,gate", PARAM_SETS)
def test_ragged_batch_word_for_word(near, far, leaf, gate):
    targets, sources = ragged_batch()
    eng = ndt.Engine(ndt.default_params(**PRM))
    tc, sc = run_ragged(eng, near, far, leaf, gate)
    for k in range(len(targets)):
        for is_tgt, cloud, cnt in ((True, targets[k], tc[k]), (False, sources[k], sc[k])):
            exp = reference(("ragged", k, is_tgt), cloud, near, far, leaf, gate)
            got = eng.batch_get_cloud(k, is_tgt)
            assert cnt == len(exp) == len(got), (k, is_tgt, cnt, len(exp), len(got))
            assert np.array_equal(got, exp), (k, is_tgt)
    assert sc[3] == 0 and tc[3] == 1                                           # the 0-point and the 1-point cloud (|p| = 5.02 m passes every gate here)
    if gate:
        assert tc[4] == 0                                                      # wholly inside distance_near
    eng.close()


def test_leaf_too_small_for_one_cloud_only():
    rng = np.random.default_rng(9)
    wide = rng.uniform(-120, 120, (4000, 3)).astype(np.float32)                # 1.5e19 cells at 1e-4 m: test_leaf_too_small_guards_beyond_the_int64_range
    tiny = [(np.float32([10.0, -3.0, 1.0]) + rng.uniform(0.0, 0.01, (50, 3))).astype(np.float32) for _ in range(2)]
    clouds = [tiny[0], wide, tiny[1]]
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(3, 4096, 64)
    tc, sc = eng.batch_prefilter(clouds, None, downsample_resolution=1e-4)
    assert sc is None
    msg = (eng.lib.mi355ndt_last_error(eng.h) or b"").decode()
    assert "slot 1" in msg and "too small" in msg, msg
    for k, cloud in enumerate(clouds):
        exp = reference(("leaf", k), cloud, 0.5, 100.0, 1e-4, True)
        assert tc[k] == len(exp) and np.array_equal(eng.batch_get_cloud(k, True), exp), k
    d = np.sqrt((wide[:, 0] * wide[:, 0] + wide[:, 1] * wide[:, 1]) + wide[:, 2] * wide[:, 2]).astype(np.float64)
    assert np.array_equal(eng.batch_get_cloud(1, True), wide[(d > 0.5) & (d < 100.0)])     # its gated input, in input order
    for k in (0, 2):                                                           # the others went through the voxel grid: voxel order, not input order
        assert not np.array_equal(eng.batch_get_cloud(k, True), clouds[k])
    eng.close()


def test_groups_change_no_word():
    want = None
    for group in (1, 2, 0):
        eng = ndt.Engine(ndt.default_params(**PRM))
        eng.set_option(ndt.OPT_PREFILTER_GROUP, group)
        assert eng.get_option(ndt.OPT_PREFILTER_GROUP) == group
        counts = run_ragged(eng, 0.5, 100.0, 0.1, True)
        got = (counts, slot_bytes(eng, 5))
        if want is None:
            want = got
        assert got == want, group
        eng.close()


@pytest.mark.parametrize("variant,mode", [(ndt.VARIANT_OMP, ndt.DIRECT7), (ndt.VARIANT_PCA, ndt.DIRECT1)])
def test_rows_behind_a_count_are_zero(variant, mode):
    """larger clouds first (batch_set_clouds' route), then smaller ones prefiltered into the same slots: build + align must not see the old rows"""
    prm = dict(PRM, variant=variant, neighbor_mode=mode)
    pairs = [[c.numpy() for c in synth.make_pair(k, 128)[:2]] for k in (50, 51, 52)]
    G = np.broadcast_to(synth.default_guess(), (3, 4, 4))
    eng = ndt.Engine(ndt.default_params(**prm))
    eng.batch_reserve(3, SLOT_CAP, SLOT_CAP)
    set_clouds(eng, [p[0] + np.float32(0.37) for p in pairs], [p[1] - np.float32(0.21) for p in pairs])   # 8,192 points each, more than any filtered cloud
    eng.batch_prefilter([p[0] for p in pairs], [p[1] for p in pairs])
    fresh = ndt.Engine(ndt.default_params(**prm))
    fresh.batch_reserve(3, SLOT_CAP, SLOT_CAP)
    set_clouds(fresh, [reference(("pair128", k, True), p[0], 0.5, 100.0, 0.1, True) for k, p in enumerate(pairs)],
               [reference(("pair128", k, False), p[1], 0.5, 100.0, 0.1, True) for k, p in enumerate(pairs)])
    out = []
    for e in (eng, fresh):
        e.batch_build_targets()
        res = (ndt.Result * 3)()
        e.batch_align_raw(np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(3, 16), res)
        out.append(bytes(res))
        e.close()
    assert out[0] == out[1]
    assert all(r.iterations > 0 for r in res)


def test_the_move():
    """T = yaw 0.3, roll 0.02, translation (1.2, -0.4, 1.73) as f32; the yardstick moves the cloud in NumPy, every product and sum its own f32 operation"""
    cy, sy, cr, sr = np.cos(0.3), np.sin(0.3), np.cos(0.02), np.sin(0.02)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T[:3, 3] = [1.2, -0.4, 1.73]
    T = T.astype(np.float32)
    clouds = [synth.make_pair(50, 65)[0].numpy(), synth.make_pair(51, 65)[1].numpy().copy()]
    clouds[1][40] = np.nan
    clouds[1][41, 2] = np.inf

    def moved(c):
        x, y, z = (c[:, a].astype(np.float32) for a in range(3))
        with np.errstate(invalid="ignore"):
            out = np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)
        assert out.dtype == np.float32
        return out

    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(2, SLOT_CAP, 64)
    tc, _ = eng.batch_prefilter(clouds, None, transform=T)
    for k, c in enumerate(clouds):
        exp = reference(("moved", k), moved(c), 0.5, 100.0, 0.1, True)
        assert tc[k] == len(exp) and np.array_equal(eng.batch_get_cloud(k, True), exp), k
    assert not np.array_equal(eng.batch_get_cloud(0, True), reference(("unmoved", 0), clouds[0], 0.5, 100.0, 0.1, True))
    eng.close()


def test_overflow_and_argument_errors():
    scan = synth.make_pair(50, 65)[0].numpy()
    tiny = np.float32([[3.0, 4.0, 0.5], [6.0, 1.0, 0.2]])
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.prefilter(scan, fetch=False)                                           # the resident single-cloud result, to be installed at the end
    n_single = eng._pf_count
    # slot 1's target filters to ~3,800 points, its slot holds 1,024
    eng.batch_reserve(3, 1024, 1024)
    with pytest.raises(ndt.NDTError) as ex:
        eng.batch_prefilter([tiny, scan, tiny], [tiny, tiny, tiny])
    assert ex.value.code == BAD_ARG and "slot 1" in str(ex.value) and "target" in str(ex.value), str(ex.value)
    for k in range(3):
        assert eng.batch_get_cloud(k, True).shape == (0, 3) and eng.batch_get_cloud(k, False).shape == (0, 3)
    # NaN resolution / NaN in the transform: refused, the batch unchanged
    eng.batch_prefilter([tiny] * 3, [tiny] * 3, downsample_resolution=0.0)
    before = slot_bytes(eng, 3)
    bad_T = np.eye(4, dtype=np.float32)
    bad_T[1, 2] = np.nan
    for kw in (dict(downsample_resolution=float("nan")), dict(transform=bad_T)):
        with pytest.raises(ndt.NDTError) as ex:
            eng.batch_prefilter([scan] * 3, [scan] * 3, **kw)
        assert ex.value.code == BAD_ARG
        assert slot_bytes(eng, 3) == before
    with pytest.raises(ndt.NDTError) as ex:
        eng.batch_prefilter([tiny] * 3, None, first_pair=1)                    # slots outside the batch
    assert ex.value.code == BAD_ARG and slot_bytes(eng, 3) == before
    with pytest.raises(ndt.NDTError) as ex:
        eng.batch_get_cloud(3, True)
    assert ex.value.code == BAD_ARG
    # the resident single-cloud prefilter result is still installable
    eng.use_prefiltered(as_target=True)
    eng.use_prefiltered(as_target=False)
    assert eng.align(synth.default_guess())["iterations"] > 0 and eng.get_aligned().shape == (n_single, 3)
    eng.close()
    # a bound device batch
    import torch
    e2 = ndt.Engine(ndt.default_params(**PRM))
    dt = torch.zeros(2, 3, 64, dtype=torch.float32, device="cuda")
    ds = torch.zeros(2, 3, 64, dtype=torch.float32, device="cuda")
    e2.batch_bind_device(dt.data_ptr(), [2, 2], 64, ds.data_ptr(), [2, 2], 64)
    with pytest.raises(ndt.NDTError) as ex:
        e2.batch_prefilter([tiny, tiny], None)
    assert ex.value.code == BAD_ARG
    e2.close()
    # stream mode
    e3 = ndt.Engine(ndt.default_params(**PRM))
    e3.batch_reserve(2, 64, 64)
    e3.stream_begin(2, 2, 64, 64)
    with pytest.raises(ndt.NDTError) as ex:
        e3.batch_prefilter([tiny, tiny], None)
    assert ex.value.code == ERR_STATE
    e3.stream_end()
    e3.close()


def test_sequence_run_raw():
    scans = [s.numpy() for s in synth.make_sequence(8, 256, n_beams=32)[0]]
    stamps = [0.1 * k for k in range(len(scans))]
    prm = dict(resolution=1.0, neighbor_mode=ndt.DIRECT1, variant=ndt.VARIANT_PCA, **PRM)
    filtered = [reference(("seq", k), s, 0.5, 100.0, 0.1, True) for k, s in enumerate(scans)]
    ref_eng = ndt.Engine(ndt.default_params(**prm))
    (rf, rr), _ = ref_eng.sequence_run(filtered, stamps, keyframe_delta_trans=2.5, raw_records=True)
    assert sum(f.new_keyframe for f in rf) >= 2                                 # the run switches keyframes
    eng = ndt.Engine(ndt.default_params(**prm))
    for rep in range(2):                                                       # the second run on the same handle gives the same bytes
        (f, r), stats, counts = eng.sequence_run_raw(scans, stamps, keyframe_delta_trans=2.5, raw_records=True)
        assert counts == [len(c) for c in filtered]
        assert bytes(f) == bytes(rf), rep
        assert bytes(r) == bytes(rr), rep
        assert stats["prefilter_ms"] > 0 and stats["aligns"] == len(scans)
    # the handle serves an ordinary registration afterwards
    G = synth.default_guess()
    eng.set_target(filtered[0])
    eng.set_source(filtered[1])
    got = eng.align(G)
    ref_eng.set_target(filtered[0])
    ref_eng.set_source(filtered[1])
    want = ref_eng.align(G)
    assert got["iterations"] == want["iterations"] > 0 and np.array_equal(got["final"], want["final"]) and got["score"] == want["score"]
    eng.close()
    ref_eng.close()
