"""GPU (-m gpu): getFitnessScore(max_range) on the batch surface (mi355ndt_batch_fitness_scores, Engine.batch_fitness_scores) and the
loop-closure verification built on it (lv_slam_amd/loop_closure.py).  Every pair's score and inlier count must be word for word what the
single-registration surface (mi355ndt_fitness_score_T) returns for the same clouds and transform."""
import importlib.util
import json
import os

import numpy as np
import pytest

from lv_slam_amd import ndt, synth
from lv_slam_amd import loop_closure as LC
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
PRM = dict(trans_epsilon=0.01, max_iterations=64)
RANGES = (0.04, 1.0, 25.0, float("inf"))


def batch_engine(pairs, **kw):
    eng = ndt.Engine(ndt.default_params(**{**PRM, **kw}))
    eng.batch_reserve(len(pairs), max(max(len(t) for t, _ in pairs), 1), max(max(len(s) for _, s in pairs), 1))
    for k, (t, s) in enumerate(pairs):
        eng.batch_set_target(k, t)
        eng.batch_set_source(k, s)
    return eng


def single_scores(pairs, Ts, mr):
    """(score, inliers) of every pair through a one-pair engine (mi355ndt_fitness_score_T)."""
    e = ndt.Engine(ndt.default_params(**PRM))
    out = []
    for (t, s), T in zip(pairs, Ts):
        e.set_target(t)
        e.set_source(s)
        out.append(e.fitness_score(mr, T))
    e.close()
    return out


def small_pairs(ids, n_az=256):
    out = []
    for k in ids:
        t, s, _ = synth.make_pair(k, n_az)
        out.append((t.numpy(), s.numpy()))
    return out


def full_size_pairs(n):
    """make_pair(k, 1024) for k < n (65,536 points per cloud), cast 16 pairs at a time on the device (synth.make_pairs: bit for bit)."""
    import torch
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    out = []
    for b in range(0, n, 16):
        t, s, _ = synth.make_pairs(list(range(b, min(b + 16, n))), 1024, device=dev)
        t, s = t.cpu().numpy(), s.cpu().numpy()
        out += [(t[j], s[j]) for j in range(len(t))]
    return out


def test_batch_fitness_after_align_matches_single_and_oracle():
    pairs = small_pairs(range(70, 76))
    eng = batch_engine(pairs)
    res = eng.batch_align(synth.default_guess())
    finals = [r["final"] for r in res]
    for mr in RANGES:
        s, n = eng.batch_fitness_scores(mr)                                # T = None: the final poses of the align
        assert s.dtype == np.float64 and n.dtype == np.int64 and s.shape == n.shape == (len(pairs),)
        single = single_scores(pairs, finals, mr)
        for k, (t, src) in enumerate(pairs):
            exp, m = O.fitness_score(t, src, finals[k], mr)
            assert n[k] == m, (mr, k, n[k], m)
            assert abs(s[k] - exp) <= 1e-12 * max(1.0, exp), (mr, k, s[k], exp)
            assert (s[k], n[k]) == single[k], (mr, k, s[k], n[k], single[k])      # bit for bit
        s2, n2 = eng.batch_fitness_scores(mr, np.stack(finals))            # the same poses given explicitly
        assert np.array_equal(s, s2) and np.array_equal(n, n2)
    assert n[0] > 0 and s[0] < DBL_MAX


def test_batch_fitness_explicit_transforms_far_sources_and_identity_default():
    pairs = small_pairs(range(80, 83))
    eng = batch_engine(pairs)
    # T = None before any align: the identity
    s0, n0 = eng.batch_fitness_scores(25.0)
    s1, n1 = eng.batch_fitness_scores(25.0, np.eye(4, dtype=np.float32))
    assert np.array_equal(s0, s1) and np.array_equal(n0, n1) and n0.min() > 0
    # 5 km away: nothing within max_range 4, every point at max_range inf
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 5000.0
    s, n = eng.batch_fitness_scores(4.0, far)
    assert np.all(s == DBL_MAX) and np.all(n == 0)
    s, n = eng.batch_fitness_scores(float("inf"), far)
    single = single_scores(pairs, [far] * len(pairs), float("inf"))
    for k, (t, src) in enumerate(pairs):
        exp, m = O.fitness_score(t, src, far, float("inf"))
        assert n[k] == m == len(src) and abs(s[k] - exp) <= 1e-12 * exp
        assert (s[k], n[k]) == single[k]
    # source points 1e7 / 1e12 m out are matched; the one at 1e30 overflows to inf and is not counted
    t, src = pairs[1]
    far_src = src[:300].copy()
    far_src[5] = [1e7, -1e7, 1e7]
    far_src[9] = [-1e12, 1e12, 1e12]
    far_src[11] = [1e30, 0.0, 0.0]
    mixed = [pairs[0], (t, far_src), pairs[2]]
    e2 = batch_engine(mixed)
    Ts = np.stack([np.eye(4, dtype=np.float32)] * 3)
    Ts[2, :3, 3] = [0.4, -0.3, 0.05]
    for mr in (1.0, 1e16, float("inf")):
        s, n = e2.batch_fitness_scores(mr, Ts)
        single = single_scores(mixed, Ts, mr)
        for k, (tt, ss) in enumerate(mixed):
            exp, m = O.fitness_score(tt, ss, Ts[k], mr)
            assert n[k] == m and abs(s[k] - exp) <= 1e-12 * max(1.0, exp), (mr, k)
            assert (s[k], n[k]) == single[k], (mr, k)
    assert n[1] == 299


def test_batch_fitness_mixed_grid_brute_force_and_empty_targets():
    (t0, s0), (t1, s1) = small_pairs([90, 91])
    stray = t1.copy()
    stray[7] = [1e30, 0.0, 0.0]                                            # the leaf-too-small guard: no grid, exhaustive search
    nan_tgt = np.full((500, 3), np.nan, np.float32)                        # points, none finite: an empty grid
    empty = np.zeros((0, 3), np.float32)
    pairs = [(t0, s0), (stray, s1[:3000]), (empty, s0[:1000]), (nan_tgt, s1[:700]), (t1, s1)]
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.3, -0.2, 0.1]
    eng = batch_engine(pairs)
    eng.batch_build_targets()
    with pytest.raises(ndt.NDTError) as ex:
        eng.get_grid(1)
    assert ex.value.code == -4
    for mr in (0.5, 25.0, float("inf")):
        s, n = eng.batch_fitness_scores(mr, T)
        assert (s[2], n[2]) == (DBL_MAX, 0) and (s[3], n[3]) == (DBL_MAX, 0)
        single = single_scores([p for k, p in enumerate(pairs) if k != 2], [T] * 4, mr)
        for k, want in zip((0, 1, 3, 4), single):
            assert (s[k], n[k]) == want, (mr, k)
        exp, m = O.fitness_score(stray, s1[:3000], T, mr)
        assert n[1] == m > 0 and abs(s[1] - exp) <= 1e-12 * max(1.0, exp)
        # permuted batch, and every pair alone in a batch of its own
        perm = [3, 1, 4, 0, 2]
        ep = batch_engine([pairs[p] for p in perm])
        sp, np_ = ep.batch_fitness_scores(mr, T)
        for j, p in enumerate(perm):
            assert (sp[j], np_[j]) == (s[p], n[p]), (mr, p)
        ep.close()
        for k, p in enumerate(pairs):
            e1 = batch_engine([p])
            assert tuple(x[0] for x in e1.batch_fitness_scores(mr, T)) == (s[k], n[k]), (mr, k)
            e1.close()


def test_batch_fitness_empty_sources_then_sources_set_later():
    """Slots whose target is set but whose source is empty (never set, or set to no points) score (DBL_MAX, 0) -- the last slot among
    them, whose target sits at the end of the index pool -- and once their sources arrive they score what the single surface does,
    without a target rebuild in between (the index built by the first call already covers them)."""
    pairs = small_pairs(range(130, 134))
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.25, -0.1, 0.05]
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.batch_reserve(len(pairs), max(len(t) for t, _ in pairs), max(len(s) for _, s in pairs))
    for k, (t, s) in enumerate(pairs):
        eng.batch_set_target(k, t)
    eng.batch_set_source(0, pairs[0][1])
    eng.batch_set_source(1, np.zeros((0, 3), np.float32))               # slot 1: no points; slots 2 and 3: never set
    single = single_scores(pairs, [T] * len(pairs), float("inf"))
    for mr in (1.0, float("inf")):
        s, n = eng.batch_fitness_scores(mr, T)
        assert s[1:].tolist() == [DBL_MAX] * 3 and n[1:].tolist() == [0] * 3
        if mr == float("inf"):
            assert (s[0], n[0]) == single[0]
    for k in (1, 2, 3):
        eng.batch_set_source(k, pairs[k][1])                           # sources only: the targets (and their index) stay
    s, n = eng.batch_fitness_scores(float("inf"), T)
    for k in range(len(pairs)):
        assert (s[k], n[k]) == single[k], k
    eng.close()


@pytest.mark.parametrize("variant", [ndt.VARIANT_OMP, ndt.VARIANT_PCA])
def test_batch_fitness_independent_of_ndt_configuration(variant):
    pairs = small_pairs(range(100, 104))
    Ts = np.stack([synth.default_guess()] * len(pairs))
    Ts[1, :3, 3] = [0.2, 0.1, -0.05]
    want = None
    G = synth.default_guess()
    for mode in (ndt.DIRECT1, ndt.DIRECT7, ndt.DIRECT26, ndt.KDTREE):
        for arith in (0, 1):
            eng = batch_engine(pairs, neighbor_mode=mode, variant=variant)
            eng.set_option(ndt.OPT_ARITH, arith)
            first_fitness = (mode + arith) % 2 == 0                        # fitness on unbuilt targets (it builds them) or after an align
            if first_fitness:                                              # the align before: an engine that never scored
                e0 = batch_engine(pairs, neighbor_mode=mode, variant=variant)
                e0.set_option(ndt.OPT_ARITH, arith)
                before = e0.batch_align(G)
                e0.close()
            else:
                before = eng.batch_align(G)
            got = [eng.batch_fitness_scores(mr, Ts) for mr in (1.0, float("inf"))]
            if want is None:
                want = got
            for (a, b), (c, d) in zip(got, want):
                assert np.array_equal(a, c) and np.array_equal(b, d), (mode, arith)
            after = eng.batch_align(G)
            for r0, r1 in zip(before, after):                              # the fitness call leaves the align alone
                assert np.array_equal(r0["final"], r1["final"]) and r0["score"] == r1["score"] and r0["iterations"] == r1["iterations"]
            eng.close()


def test_batch_fitness_271_full_size_pairs_match_single_surface():
    n_pairs = 271
    pairs = full_size_pairs(n_pairs)
    assert len(pairs[0][0]) == 65536
    eng = batch_engine(pairs)
    Ts = np.stack([synth.default_guess()] * n_pairs)
    Ts[:, 1, 3] = np.linspace(-0.5, 0.5, n_pairs, dtype=np.float32)
    got = {mr: eng.batch_fitness_scores(mr, Ts) for mr in (float("inf"), 1.0)}
    e = ndt.Engine(ndt.default_params(**PRM))
    for k, (t, s) in enumerate(pairs):
        e.set_target(t)
        e.set_source(s)
        for mr, (sc, n) in got.items():
            assert (sc[k], n[k]) == e.fitness_score(mr, Ts[k]), (mr, k)
    e.close()
    assert np.all(got[float("inf")][1] == 65536) and np.all(got[1.0][1] > 0)


def offset_and_far():
    off = np.eye(4, dtype=np.float32)
    off[:3, 3] = [0.3, 0.0, 0.0]
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 5000.0
    return off, far


@pytest.mark.parametrize("n_src", [1, 256, 257, 2500])
def test_one_pair_ragged_sources_match_the_oracle(n_src):
    """The one-pair surface is the batch of one, and a lone pair is cut into pieces that spread over the XCDs: one point, one full block,
    one block and a point, and ten blocks with the last holding 196 points (five pieces of two)."""
    t, s, _ = synth.make_pair(40, 256)
    target, src = t.numpy()[:3000], s.numpy()[:n_src]
    off, far = offset_and_far()
    e = ndt.Engine(ndt.default_params(resolution=1.0, **PRM))
    e.set_target(target)
    e.set_source(src)
    for name, T in (("identity", np.eye(4, dtype=np.float32)), ("offset", off), ("far", far)):
        for mr in (0.04, 1.0, float("inf")):
            sc, n = e.fitness_score(mr, T)
            exp, m = O.fitness_score(target, src, T, mr)
            assert n == m, (name, mr, n, m)
            assert abs(sc - exp) <= 1e-12 * max(1.0, exp), (name, mr, sc, exp)
    assert e.fitness_score(float("inf"), far)[1] == n_src
    assert e.fitness_score(4.0, far) == (DBL_MAX, 0)
    e.close()


def test_cutting_a_big_pair_does_not_enter_any_result():
    """One 16,384-point pair (64 blocks) among eight 700-point pairs (3 blocks each): 88 blocks, so pairs of more than 11 are cut -- the big
    one into six pieces, the others not.  Every pair's words are those of the same pair alone in a batch of one and on the one-pair
    surface, wherever the big pair sits, and with a target that takes the exhaustive kernel in the batch."""
    big = small_pairs([140])[0]
    small = [(t[:700], s[:700]) for t, s in small_pairs(range(141, 149))]
    stray = small[3][0].copy()
    stray[7] = [1e30, 0.0, 0.0]                                            # the leaf-too-small guard: no grid, exhaustive search
    with_stray = small[:3] + [(stray, small[3][1])] + small[4:]
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = [0.3, -0.2, 0.1]
    ranges = (1.0, float("inf"))

    def alone(pair):
        """{max_range: (score, inliers)} of one pair: a batch of one and the one-pair surface, which must agree"""
        e1 = batch_engine([pair])
        out = {}
        for mr in ranges:
            out[mr] = tuple(x[0] for x in e1.batch_fitness_scores(mr, T))
            assert out[mr] == single_scores([pair], [T], mr)[0], mr
        e1.close()
        return out

    want_big, want_small, want_stray = alone(big), [alone(p) for p in small], alone(with_stray[3])
    assert want_big[1.0][1] > 0 and want_stray[float("inf")][1] == 700
    for smalls, wants in ((small, want_small), (with_stray, want_small[:3] + [want_stray] + want_small[4:])):
        for pairs, want in (([big] + smalls, [want_big] + wants), (smalls + [big], wants + [want_big])):
            eng = batch_engine(pairs)
            for mr in ranges:
                sc, n = eng.batch_fitness_scores(mr, T)
                for k in range(len(pairs)):
                    assert (sc[k], n[k]) == want[k][mr], (mr, k)
            eng.close()


def test_one_pair_words_equal_the_parents():
    """tests/golden/fitness_single_parent.json holds what Engine.fitness_score returned, as words, from the library of the commit before
    the one-pair score became the batch of one (its own kernel over a dense cell table): tools/record_fitness_words.py wrote it and
    states the cases.  Batch and keyframe tests compare against the one-pair surface; this is what the one-pair surface is held to."""
    spec = importlib.util.spec_from_file_location("record_fitness_words", os.path.join(ROOT, "tools", "record_fitness_words.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(os.path.join(ROOT, "tests", "golden", "fitness_single_parent.json")) as f:
        want = json.load(f)
    assert len(want) == len(rec.CLOUDS) * 3 * len(rec.RANGES) == 72
    got = rec.compute()
    assert sorted(got) == sorted(want)
    for case in sorted(want):
        assert got[case] == want[case], (case, got[case], want[case])


@pytest.mark.parametrize("use_bow", [False, True])
@pytest.mark.parametrize("mr", [1.0, float("inf")])
def test_verify_candidates_equals_sequential_loop_detector(use_bow, mr):
    t, s, _ = synth.make_pair(120, 256)
    target, src = t.numpy(), s.numpy()
    new_pose = np.eye(4)
    new_pose[:3, 3] = [10.0, 5.0, 0.0]
    # (dx, dy, yaw) of the candidates' recorded poses against the new keyframe's: two close, one exact, two far off and turned
    offsets = [(0.2, 0.1, 0.0), (0.6, -0.3, 0.02), (25.0, 8.0, 0.6), (0.0, 0.0, 0.0), (-40.0, 12.0, -0.9)]
    cand_poses, candidates = [], []
    for dx, dy, yaw in offsets:
        P = new_pose.copy()
        P[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
        P[:3, 3] += [dx, dy, 0.0]
        cand_poses.append(P)
        candidates.append(src)                                             # the same scan, recorded at different poses
    guesses = np.stack([LC.loop_guess(new_pose, P) for P in cand_poses])
    thresh = 0.5
    bow = [(0.5, 2), (0.3, 0), (0.2, 3), (0.1, 1), (0.03, 4)] if use_bow else None
    # the reference: one registration object, the new keyframe as target, the candidates one after the other
    reg = ndt.NormalDistributionsTransform()
    reg.setTransformationEpsilon(PRM["trans_epsilon"])
    reg.setMaximumIterations(PRM["max_iterations"])
    reg.setInputTarget(target)
    best, matched, pose, aligns = DBL_MAX, None, None, 0
    order = [(1.0, k) for k in range(len(candidates))] if bow is None else bow
    for b, k in order:
        if bow is not None and (b < 0.04 or best <= thresh):
            break
        if bow is not None:
            matched = k
        reg.setInputSource(candidates[k])
        reg.align(guesses[k])
        aligns += 1
        score = reg.getFitnessScore(mr)
        if not reg.hasConverged() or score > best:
            continue
        best = score
        if bow is None:
            matched = k
        pose = reg.getFinalTransformation()
    if best > thresh:
        matched, pose = None, None
    eng = ndt.Engine(ndt.default_params(**PRM))
    idx, rel, score, n_aligns = LC.verify_candidates(eng, target, candidates, guesses, mr, thresh, bow)
    assert idx == matched and score == best and n_aligns == aligns
    assert (rel is None and pose is None) or np.array_equal(rel, pose)
    if mr == 1.0:
        assert matched is not None                                         # the test data holds a loop
