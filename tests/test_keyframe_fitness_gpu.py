"""GPU (-m gpu): mi355ndt_keyframe_fitness_scores -- InformationMatrixCalculator::calc_fitness_score for graph edges between resident
keyframes -- and the information matrices made from it.  Every edge is compared: with the one-pair surface (Engine.fitness_score(T=...) on a
fresh engine fed the downloaded clouds) word for word, and with the brute-force oracle to 1e-12 * max(1, expected)."""
import numpy as np
import pytest

from lv_slam_amd import information
from lv_slam_amd import keyframes as KF
from lv_slam_amd import ndt, synth
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
PRM = dict(trans_epsilon=0.01, max_iterations=64)
DBL_MAX = 1.7976931348623157e308
RANGES = [float("inf"), 1.0, 0.01]


def words(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def perturb(T, k):
    """ground truth, moved by a few centimetres and milliradians (a registration result, not the truth)"""
    rng = np.random.default_rng(1000 + k)
    yaw, dt = rng.normal(0, 4e-3), rng.normal(0, 0.04, 3)
    D = np.eye(4)
    D[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    D[:3, 3] = dt
    return np.asarray(T, np.float64) @ D


def one_pair(c1, c2, T, ranges=RANGES):
    """the one-pair surface on a fresh engine: [(score, inliers)] per max_range"""
    e = ndt.Engine(ndt.default_params(**PRM))
    e.set_target(c1)
    e.set_source(c2)
    out = [e.fitness_score(mr, T=np.asarray(T, np.float64).astype(np.float32)) for mr in ranges]
    e.close()
    return out


def windows(engine, n_frames, n_azimuth, **kw):
    scans, poses = synth.make_sequence(n_frames, n_azimuth)
    wk = KF.WindowKeyframer(engine, leaf=0.1, **kw)
    out = []
    for k, (P, s) in enumerate(zip(poses, scans)):
        r = wk.push(P, s.numpy().astype(np.float32), seq=k)
        if r is not None:
            out.append(r)
    out.append(wk.flush())
    return out


def drive_edges(kfs):
    """consecutive (odometry) edges, ground truth and perturbed, plus far-apart (loop-like) ones; (i, j, relpose): j moved into i's frame"""
    rel = lambda i, j: KF.isometry_inverse(kfs[i].odom) @ kfs[j].odom
    edges = []
    for i in range(len(kfs) - 1):
        edges.append((i, i + 1, rel(i, i + 1)))
        edges.append((i, i + 1, perturb(rel(i, i + 1), i)))
    n = len(kfs)
    for i, j in ((0, n - 1), (n - 1, 0), (1, n - 2), (0, n // 2)):
        edges.append((i, j, rel(i, j)))
        edges.append((i, j, perturb(rel(i, j), 100 + i)))
    return edges


def test_equals_one_pair_surface_on_a_drive():
    e = ndt.Engine()
    kfs = windows(e, 40, 256, delta_trans=4.0, delta_angle=0.3)   # the keyframe tests' drive: 16,384 points per scan
    assert len(kfs) >= 4
    clouds = [e.keyframe_get(r.id) for r in kfs]
    print("keyframes:", [len(c) for c in clouds])
    edges = drive_edges(kfs)
    ids1, ids2, rel = [kfs[i].id for i, _, _ in edges], [kfs[j].id for _, j, _ in edges], [T for _, _, T in edges]
    before = e.profile_get()
    got = {mr: e.keyframe_fitness_scores(ids1, ids2, rel, mr) for mr in RANGES}
    after = e.profile_get()
    assert after["cloud_uploads"] == before["cloud_uploads"] and after["cloud_upload_bytes"] == before["cloud_upload_bytes"]
    for k, (i, j, T) in enumerate(edges):
        exp = one_pair(clouds[i], clouds[j], T)
        for mr, (xs, xn) in zip(RANGES, exp):
            s, n = got[mr][0][k], got[mr][1][k]
            print(f"edge {k} ({i}<-{j}) max_range {mr}: score {s!r} inliers {n} | one-pair {xs!r} {xn}")
            assert words(s) == words(xs) and n == xn, (k, i, j, mr)
    assert (got[float("inf")][1] > 0).all()
    # a second identical call returns identical words (the indexes are resident now)
    again = e.keyframe_fitness_scores(ids1, ids2, rel, 1.0)
    assert words(again[0]) == words(got[1.0][0]) and np.array_equal(again[1], got[1.0][1])
    # the cell size is about speed only: another engine with other cells gives the same words
    e2 = ndt.Engine()
    e2.set_option(ndt.OPT_KF_FITNESS_CELL_MM, 700)
    assert e2.get_option(ndt.OPT_KF_FITNESS_CELL_MM) == 700
    m = {r.id: e2.keyframe_add(c) for r, c in zip(kfs, clouds)}
    other = e2.keyframe_fitness_scores([m[a] for a in ids1], [m[b] for b in ids2], rel, 1.0)
    assert words(other[0]) == words(got[1.0][0]) and np.array_equal(other[1], got[1.0][1])
    with pytest.raises(ndt.NDTError):
        e2.set_option(ndt.OPT_KF_FITNESS_CELL_MM, 0)
    e2.close()
    e.close()


def test_agrees_with_oracle():
    e = ndt.Engine()
    kfs = windows(e, 30, 64, delta_trans=4.0, delta_angle=0.3)    # 4,096 points per scan: the brute-force oracle stays in seconds
    clouds = [e.keyframe_get(r.id) for r in kfs]
    assert len(kfs) >= 4 and max(len(c) for c in clouds) <= 32000
    edges = drive_edges(kfs)
    ids1, ids2, rel = [kfs[i].id for i, _, _ in edges], [kfs[j].id for _, j, _ in edges], [T for _, _, T in edges]
    for mr in RANGES:
        s, n = e.keyframe_fitness_scores(ids1, ids2, rel, mr)
        for k, (i, j, T) in enumerate(edges):
            exp, m = O.fitness_score(clouds[i], clouds[j], np.asarray(T, np.float64).astype(np.float32), mr)
            print(f"edge {k} ({i}<-{j}) max_range {mr}: score {s[k]!r} inliers {n[k]} | oracle {exp!r} {m}")
            assert n[k] == m, (k, mr)
            assert abs(s[k] - exp) <= 1e-12 * max(1.0, exp), (k, mr, s[k], exp)
    e.close()


def test_degenerate_inputs():
    t, s, dT = synth.make_pair(33, 256)
    t, s = t.numpy().astype(np.float32), s.numpy().astype(np.float32)
    t, s = t[:9000].copy(), s[:7000].copy()
    T = np.asarray(dT, np.float64)
    I = np.eye(4)
    e = ndt.Engine()
    empty = e.keyframe_add(np.zeros((0, 3), np.float32))
    kt, ks = e.keyframe_add(t), e.keyframe_add(s)
    # an empty keyframe on either side (and on both)
    sc, n = e.keyframe_fitness_scores([empty, kt, empty], [ks, empty, empty], [I, I, I], 1.0)
    assert (sc == DBL_MAX).all() and (n == 0).all()
    # a one-point keyframe, on either side
    one = t[4321:4322].copy()
    k1 = e.keyframe_add(one)
    sc, n = e.keyframe_fitness_scores([k1, kt, k1], [ks, k1, k1], [T, I, I])
    for k, (a, b, P) in enumerate([(one, s, T), (t, one, I), (one, one, I)]):
        (xs, xn), = one_pair(a, b, P, [float("inf")])
        assert words(sc[k]) == words(xs) and n[k] == xn, k
    assert sc[2] == 0.0 and n[2] == 1
    # NaN / +-inf points on both sides
    tn, sn = t.copy(), s.copy()
    tn[::97, 0] = np.nan; tn[5::131, 1] = np.inf; tn[7::211, 2] = -np.inf
    sn[::89, 2] = np.nan; sn[3::127, 0] = -np.inf; sn[11::151, 1] = np.inf
    ktn, ksn = e.keyframe_add(tn), e.keyframe_add(sn)
    for mr in RANGES:
        sc, n = e.keyframe_fitness_scores([ktn, kt, ktn], [ksn, ksn, ks], [T, T, T], mr)
        for k, (a, b) in enumerate([(tn, sn), (t, sn), (tn, s)]):
            (xs, xn), = one_pair(a, b, T, [mr])
            assert words(sc[k]) == words(xs) and n[k] == xn, (k, mr)
            xo, no = O.fitness_score(a[np.isfinite(a).all(1)], b[np.isfinite(b).all(1)], T.astype(np.float32), mr)
            assert n[k] == no and abs(sc[k] - xo) <= 1e-12 * max(1.0, xo), (k, mr)
    allnan = np.full((100, 3), np.nan, np.float32)
    kn = e.keyframe_add(allnan)
    sc, n = e.keyframe_fitness_scores([kn, kt], [ks, kn], [T, T])
    assert (sc == DBL_MAX).all() and (n == 0).all()
    # a stray point at 1e12 m in cloud1 (no lattice: the exhaustive kernel) and in cloud2
    ts, ss = t.copy(), s.copy()
    ts[100] = [1e12, -3.0, 2.0]
    ss[200] = [-2.0, 1e12, 1.0]
    kts, kss = e.keyframe_add(ts), e.keyframe_add(ss)
    for mr in RANGES:
        sc, n = e.keyframe_fitness_scores([kts, kt, kts], [ks, kss, kss], [T, T, T], mr)
        for k, (a, b) in enumerate([(ts, s), (t, ss), (ts, ss)]):
            (xs, xn), = one_pair(a, b, T, [mr])
            assert words(sc[k]) == words(xs) and n[k] == xn, (k, mr)
    # two keyframes with no overlap, searched with a small max_range; and with none
    far = np.eye(4)
    far[:3, 3] = [500.0, -300.0, 40.0]
    for mr in (0.25, float("inf")):
        sc, n = e.keyframe_fitness_scores([kt], [ks], [far], mr)
        (xs, xn), = one_pair(t, s, far, [mr])
        assert words(sc[0]) == words(xs) and n[0] == xn
        if mr == 0.25:
            assert sc[0] == DBL_MAX and n[0] == 0
    # a self-edge with the identity pose
    sc, n = e.keyframe_fitness_scores([kt, ktn], [kt, ktn], [I, I], 1.0)
    assert sc[0] == 0.0 and n[0] == len(t)
    assert sc[1] == 0.0 and n[1] == int(np.isfinite(tn).all(1).sum())
    # one keyframe named in many edges and on both sides
    ids1 = [kt, ks, kt, kt, ks, kt]
    ids2 = [ks, kt, ks, kt, ks, ksn]
    Ts = [T, np.linalg.inv(T), perturb(T, 5), I, I, T]
    cl = {kt: t, ks: s, ksn: sn}
    sc, n = e.keyframe_fitness_scores(ids1, ids2, Ts, 1.0)
    for k in range(len(ids1)):
        (xs, xn), = one_pair(cl[ids1[k]], cl[ids2[k]], Ts[k], [1.0])
        assert words(sc[k]) == words(xs) and n[k] == xn, k
    e.close()


def test_errors():
    t, s, dT = synth.make_pair(34, 128)
    t, s = t.numpy().astype(np.float32), s.numpy().astype(np.float32)
    e = ndt.Engine(ndt.default_params(**PRM))
    kt, ks, gone = e.keyframe_add(t), e.keyframe_add(s), e.keyframe_add(s[:100])
    e.keyframe_release(gone)
    I = np.eye(4)
    import ctypes as C
    for bad in (gone, 99, -1):
        for ids1, ids2 in (([kt, bad], [ks, ks]), ([kt, kt], [ks, bad])):
            with pytest.raises(ndt.NDTError) as ex:
                e.keyframe_fitness_scores(ids1, ids2, [I, I], 1.0)
            assert ex.value.code == -2 and "keyframe" in str(ex.value)
            # the outputs are untouched
            a, b = np.array(ids1, np.int32), np.array(ids2, np.int32)
            P = np.ascontiguousarray(np.stack([I.T, I.T]).reshape(2, 16))
            sc, n = np.full(2, -7.5), np.full(2, -7, np.int64)
            rc = e.lib.mi355ndt_keyframe_fitness_scores(e.h, 2, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                                        1.0, sc.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p))
            assert rc == -2 and (sc == -7.5).all() and (n == -7).all()
    sc, n = e.keyframe_fitness_scores([], [], np.zeros((0, 4, 4)), 1.0)     # n_edges == 0 is OK
    assert len(sc) == 0 and len(n) == 0
    assert e.lib.mi355ndt_keyframe_fitness_scores(e.h, 0, None, None, None, 1.0, None, None) == 0
    assert e.lib.mi355ndt_keyframe_fitness_scores(e.h, -1, None, None, None, 1.0, None, None) == -2
    # n_inliers may be NULL
    a, b = np.array([kt], np.int32), np.array([ks], np.int32)
    P = np.ascontiguousarray(np.asarray(dT, np.float64).T.reshape(1, 16))
    sc = np.zeros(1)
    assert e.lib.mi355ndt_keyframe_fitness_scores(e.h, 1, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), P.ctypes.data_as(C.c_void_p),
                                                  1.0, sc.ctypes.data_as(C.c_void_p), None) == 0
    assert words(sc[0]) == words(e.keyframe_fitness_scores([kt], [ks], [dT], 1.0)[0][0])
    e.stream_begin(2, 4, 4096, 4096)
    try:
        with pytest.raises(ndt.NDTError) as ex:
            e.keyframe_fitness_scores([kt], [ks], [I], 1.0)
        assert ex.value.code == -7
    finally:
        e.stream_end()
    e.close()


def _res_words(r):
    return (r["final"].tobytes(), r["score"], r["iterations"], r["converged"], r["trans_probability"])


def test_isolation():
    """A resident registration and a reserved batch align to the same bits before and after; the other consumers of a keyframe give the same
    words before and after its index exists; releasing one indexed keyframe leaves the others' results unchanged."""
    scans, poses = synth.make_sequence(12, 256)
    clouds = [scans[k].numpy().astype(np.float32) for k in (0, 3, 6, 9)]
    P = [poses[k] for k in (0, 3, 6, 9)]
    t, s, _ = synth.make_pair(210, 256)
    t, s = t.numpy(), s.numpy()
    G = synth.default_guess()
    rel = lambda i, j: KF.isometry_inverse(P[i]) @ P[j]

    def run(with_scores):
        out = []
        e = ndt.Engine(ndt.default_params(**PRM))                 # a resident single registration, a prefilter result, a map cloud, a window
        pf = e.prefilter(clouds[0][:20000], 0.5, 100.0, 0.2)
        e.set_target(t)
        e.set_source(s)
        out.append(_res_words(e.align(G)))
        ids = [e.keyframe_add(c) for c in clouds]
        w, _ = e.window_keyframe(clouds[1:3], [np.eye(4), rel(1, 2)], 0.1)
        out.append(e.map_cloud_keyframes(ids, P, 0.5).tobytes())
        if with_scores:
            up = e.profile_get()["cloud_uploads"]
            e.keyframe_fitness_scores([ids[0], ids[1], w], [ids[1], ids[2], ids[3]], [rel(0, 1), rel(1, 2), rel(1, 3)], 1.0)
            assert e.profile_get()["cloud_uploads"] == up
        out.append(_res_words(e.align(G)))
        out.append(e.fitness_score())
        out.append(e.map_cloud_keyframes(ids, P, 0.5).tobytes())  # keyframes with and without an index, through the map cloud
        out.append(e.keyframe_get(w).tobytes())
        w2, _ = e.window_keyframe(clouds[1:3], [np.eye(4), rel(1, 2)], 0.1)
        out.append(e.keyframe_get(w2).tobytes())
        e.use_prefiltered(as_target=True)
        out.append(_res_words(e.align(G)))
        e.close()
        eb = ndt.Engine(ndt.default_params(**PRM))                # a reserved batch, filled by the keyframe setters
        ids = [eb.keyframe_add(c) for c in clouds]
        eb.batch_reserve(2, 65536, 65536)
        if with_scores:
            eb.keyframe_fitness_scores([ids[0]], [ids[1]], [rel(0, 1)], 1.0)
        for p in range(2):
            eb.batch_set_target_keyframe(p, ids[p])
            eb.batch_set_source_keyframe(p, ids[p + 1])
        if with_scores:
            eb.keyframe_fitness_scores([ids[1], ids[2]], [ids[2], ids[3]], [rel(1, 2), rel(2, 3)], 1.0)
        out += [_res_words(r) for r in eb.batch_align(np.stack([rel(0, 1), rel(1, 2)]).astype(np.float32))]
        if with_scores:
            eb.keyframe_fitness_scores([ids[0], ids[3]], [ids[3], ids[0]], [rel(0, 3), rel(3, 0)], 1.0)
        sc, n = eb.batch_fitness_scores(1.0)
        out += [words(sc), n.tobytes()]
        out += [_res_words(r) for r in eb.batch_align(np.stack([rel(0, 1), rel(1, 2)]).astype(np.float32))]
        eb.close()
        return pf.tobytes(), out

    assert run(True) == run(False)

    e = ndt.Engine()
    ids = [e.keyframe_add(c) for c in clouds]
    ed1, ed2, T = [ids[0], ids[1], ids[2], ids[0]], [ids[1], ids[2], ids[3], ids[2]], [rel(0, 1), rel(1, 2), rel(2, 3), rel(0, 2)]
    first = e.keyframe_fitness_scores(ed1, ed2, T, 1.0)
    e.keyframe_release(ids[1])                                    # (indexed: it was searched by edge 1)
    keep = [0, 2, 3]
    with pytest.raises(ndt.NDTError):
        e.keyframe_fitness_scores(ed1, ed2, T, 1.0)
    again = e.keyframe_fitness_scores([ed1[k] for k in (2, 3)], [ed2[k] for k in (2, 3)], [T[k] for k in (2, 3)], 1.0)
    assert words(again[0]) == words(first[0][2:]) and np.array_equal(again[1], first[1][2:])
    assert e.keyframe_count() == len(keep)
    e.close()


def test_window_keyframer_to_information_matrices_end_to_end():
    e = ndt.Engine()
    kfs = windows(e, 30, 256, delta_trans=4.0, delta_angle=0.3)
    assert len(kfs) >= 4
    rel = lambda i, j: KF.isometry_inverse(kfs[i].odom) @ kfs[j].odom
    # what flush_keyframe_queue hands over (prev -> new for every new keyframe) and a loop block's accepted loops
    pairs = [(i, i + 1) for i in range(len(kfs) - 1)] + [(0, len(kfs) - 1), (len(kfs) - 2, 0)]
    edges = [(kfs[i].id, kfs[j].id, rel(i, j)) for i, j in pairs]
    for prm in (dict(), dict(fitness_score_thresh=2.5, max_range=2.0), dict(use_const_inf_matrix=1)):
        calc = information.InformationMatrixCalculator(**prm)
        up = e.profile_get()["cloud_uploads"]
        got = calc.calc_information_matrices(e, edges)
        assert e.profile_get()["cloud_uploads"] == up
        assert len(got) == len(edges)
        for (i, j), (_, _, T), m in zip(pairs, edges, got):       # the host route: keyframe_get + the one-pair fitness + ndt.information_matrix
            if calc.use_const_inf_matrix:
                exp = ndt.information_matrix(0.0, calc.params)
            else:
                (sc, _), = one_pair(e.keyframe_get(kfs[i].id), e.keyframe_get(kfs[j].id), T, [calc.max_range])
                exp = ndt.information_matrix(sc, calc.params)
            assert m.shape == (6, 6) and m.tobytes() == exp.tobytes(), (i, j)
        one = calc.calc_information_matrix(e, *edges[0])
        assert one.tobytes() == got[0].tobytes()
    e.close()
