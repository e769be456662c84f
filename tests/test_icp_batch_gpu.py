"""GPU (-m gpu): the ICP batch (mi355ndt_icp_batch_*) against the single-pair surface, byte for byte, and verify_candidates_icp against the
sequential loop of the reference's loop detector.  The batch is one loop on the calling thread: a round serves every slot that has not
ended, so rounds = the steps of the longest slot and requests[k] = the steps of slot k -- its iterations, plus the one step that found too
few correspondences when it ended on that."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT
from lv_slam_amd import loop_closure, ndt, synth

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


R = _load("icp_ref")
G0 = synth.default_guess()
I4 = np.eye(4, dtype=np.float32)
KEYS = ("converged", "iterations", "state", "matches", "mse")
_PAIR = {}


def pair(p):
    if p not in _PAIR:
        tgt, src, dT = synth.make_pair(p, n_azimuth=64)
        _PAIR[p] = (tgt.numpy(), src.numpy(), dT)
    return _PAIR[p]


@pytest.fixture(scope="module")
def eng():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    yield e
    e.close()


def set_params(e, **kw):
    e.icp_set_params(ndt.default_icp_params(**kw))


def single(e, source, guess):
    """(result, aligned cloud) of the single-pair surface; source = ("cloud", array) or ("id", keyframe)"""
    if source[0] == "id":
        e.icp_set_source(keyframe=source[1])
    else:
        e.icp_set_source(source[1])
    r = e.icp_align(guess)
    return r, e.icp_get_aligned()


def batch(e, sources, guesses):
    e.icp_batch_reserve(len(sources))
    for k, s in enumerate(sources):
        if s[0] == "id":
            e.icp_batch_set_source(k, keyframe=s[1])
        else:
            e.icp_batch_set_source(k, s[1])
    res = e.icp_batch_align(np.stack(guesses))
    return res, [e.icp_batch_get_aligned(k) for k in range(len(sources))], e.icp_batch_stats()


def same(a, b):
    return a["final"].tobytes() == b["final"].tobytes() and all(a[k] == b[k] for k in KEYS)


def check_stats(res, stats):
    rounds, req = stats
    steps = [r["iterations"] + (1 if r["state"] == R.NO_CORRESPONDENCES else 0) for r in res]
    print("iterations", [r["iterations"] for r in res], "states", [ndt.ICP_STATES[r["state"]] for r in res], "rounds", rounds, "requests", list(req))
    assert list(req) == steps and rounds == max(steps)


def test_five_mixed_slots_equal_the_single_pair_surface(eng):
    tgt, src, _ = pair(0)
    set_params(eng, transformation_epsilon=1e-6, corr_dist_threshold=1.0, max_iterations=12)
    kt, k257, kfull = eng.keyframe_add(tgt), eng.keyframe_add(src[:257]), eng.keyframe_add(src)
    eng.icp_set_target(keyframe=kt)
    G4 = G0.copy()
    G4[:3, :3] = synth.rot_zyx(0.01, 0.0, 0.0).astype(np.float32)
    sources = [("cloud", src), ("id", k257), ("cloud", src[:1]), ("id", kfull), ("cloud", src[::3].copy())]
    guesses = [G0, I4, I4, I4, G4]
    want = [single(eng, s, g) for s, g in zip(sources, guesses)]
    res, moved, stats = batch(eng, sources, guesses)
    for k in range(5):
        assert same(res[k], want[k][0]), k
        assert moved[k].tobytes() == want[k][1].tobytes(), k
    states = [r["state"] for r in res]
    assert states[2] == R.NO_CORRESPONDENCES and not res[2]["converged"] and res[2]["iterations"] == 0
    assert R.ITERATIONS in states and R.TRANSFORM in states and res[0]["iterations"] == 12
    assert len({r["iterations"] for r in res}) >= 3               # the slots end in different rounds
    check_stats(res, stats)
    res2, moved2, _ = batch(eng, sources, guesses)               # again from scratch: the same bytes
    assert all(same(a, b) for a, b in zip(res, res2)) and all(a.tobytes() == b.tobytes() for a, b in zip(moved, moved2))
    assert eng.keyframe_get(kfull).tobytes() == src.tobytes() and eng.keyframe_get(k257).tobytes() == src[:257].tobytes()   # sources are never written
    r, a = single(eng, sources[3], guesses[3])                    # the single-pair surface is as it was
    assert same(r, want[3][0]) and a.tobytes() == want[3][1].tobytes()
    for k in (kt, k257, kfull):
        eng.keyframe_release(k)
    with pytest.raises(ndt.NDTError) as err:                      # the target and two slots are released ids now
        eng.icp_batch_align(np.stack(guesses))
    assert err.value.code == -2 and "released" in str(err.value)


def test_batch_of_one_equals_the_single_call(eng):
    tgt, src, _ = pair(1)
    set_params(eng, transformation_epsilon=1e-6, max_iterations=64)
    eng.icp_set_target(tgt)
    want = single(eng, ("cloud", src), G0)
    res, moved, stats = batch(eng, [("cloud", src)], [G0])
    assert same(res[0], want[0]) and moved[0].tobytes() == want[1].tobytes() and res[0]["iterations"] > 3
    check_stats(res, stats)


def test_two_slots_on_an_exhaustive_target(eng):
    tgt, src, _ = pair(3)
    tgt = np.concatenate([tgt[::4], np.array([[1e12, 0, 0]], np.float32)])       # no lattice
    set_params(eng, transformation_epsilon=1e-4, max_iterations=8)
    eng.icp_set_target(tgt)
    sources = [("cloud", src[::4].copy()), ("cloud", src[1::8].copy())]
    guesses = [G0, I4]
    want = [single(eng, s, g) for s, g in zip(sources, guesses)]
    res, moved, stats = batch(eng, sources, guesses)
    for k in range(2):
        assert same(res[k], want[k][0]) and moved[k].tobytes() == want[k][1].tobytes(), k
        assert res[k]["iterations"] >= 2
    check_stats(res, stats)


def test_verify_candidates_icp_selects_what_the_sequential_loop_selects(eng):
    tgt, src, _ = pair(0)
    rng = np.random.default_rng(7)
    far = src + np.float32([40.0, 0, 0])                                            # a candidate from elsewhere
    cands = [src[::2].copy(), far, src.copy(), (src + rng.normal(0, 0.05, src.shape)).astype(np.float32)]
    guesses = np.stack([G0, G0, G0, I4])
    set_params(eng, transformation_epsilon=1e-6, max_iterations=64, corr_dist_threshold=2.0)
    conv, scores, finals = [], [], []
    for c, g in zip(cands, guesses):                                                # the reference's loop: align, score, one by one
        kt, kc = eng.keyframe_add(tgt), eng.keyframe_add(c)
        eng.icp_set_target(keyframe=kt)
        eng.icp_set_source(keyframe=kc)
        r = eng.icp_align(g)
        sc, _ = eng.keyframe_fitness_scores([kt], [kc], [r["final"]], 1.0)
        conv.append(r["converged"]); scores.append(float(sc[0])); finals.append(r["final"])
        eng.keyframe_release(kt); eng.keyframe_release(kc)
    print("converged", conv, "scores", scores)
    n_kf = eng.keyframe_count()
    want = loop_closure.select_matching(conv, scores, finals, 0.5)
    got = loop_closure.verify_candidates_icp(eng, tgt, cands, guesses, 1.0, 0.5)
    assert want[0] is not None and got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:]
    bow = [(0.5, 3), (0.3, 0), (0.2, 1), (0.01, 2)]                                # candidate 3 is within the threshold: the walk stops after it
    want = loop_closure.select_matching_and_bow(conv, scores, finals, bow, 0.5)
    got = loop_closure.verify_candidates_icp(eng, tgt, cands, guesses, 1.0, 0.5, bow=bow)
    assert want[0] == 3 and want[3] == 1 and scores[0] < scores[3]                 # (the walk never reaches the better candidate 0)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:]
    assert eng.keyframe_count() == n_kf                                             # the call's own keyframes are released
    assert loop_closure.verify_candidates_icp(eng, tgt, [], np.zeros((0, 4, 4), np.float32))[0] is None


def test_batch_state_and_argument_errors():
    e = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=64))
    p = pair(0)[1][:300]
    for call in (lambda: e.icp_batch_set_source(0, p), lambda: e.icp_batch_align(np.zeros((0, 4, 4), np.float32)), lambda: e.icp_batch_stats(),
                 lambda: e.icp_batch_get_aligned(0)):
        with pytest.raises(ndt.NDTError) as err:                # nothing is reserved
            call()
        assert err.value.code == -7
    for n in (0, ndt.ICP_BATCH_MAX + 1, -3):
        with pytest.raises(ndt.NDTError) as err:
            e.icp_batch_reserve(n)
        assert err.value.code == -2 and "n_slots" in str(err.value)
    e.icp_batch_reserve(2)
    for slot in (-1, 2):
        with pytest.raises(ndt.NDTError) as err:
            e._chk(e.lib.mi355ndt_icp_batch_set_source(e.h, slot, p.ctypes.data, len(p), 12), "icp_batch_set_source")
        assert err.value.code == -2 and "slot" in str(err.value)
    with pytest.raises(ndt.NDTError) as err:
        e.icp_batch_set_source(1, keyframe=9)                   # never given out
    assert err.value.code == -2
    e.icp_batch_set_source(0, p)
    with pytest.raises(ndt.NDTError) as err:                    # slot 1 is unset
        e.icp_batch_align(np.stack([I4, I4]))
    assert err.value.code == -7 and "slot 1" in str(err.value)
    e.icp_batch_set_source(1, p[:50])
    with pytest.raises(ndt.NDTError) as err:                    # no target
        e.icp_batch_align(np.stack([I4, I4]))
    assert err.value.code == -7 and "no target" in str(err.value)
    e.icp_set_target(p)
    with pytest.raises(ndt.NDTError) as err:
        e.icp_batch_get_aligned(0)                              # no batch align has run
    assert err.value.code == -7
    e.stream_begin(2, 4, 1024, 1024)
    for call in (lambda: e.icp_batch_reserve(2), lambda: e.icp_batch_set_source(0, p), lambda: e.icp_batch_align(np.stack([I4, I4])),
                 lambda: e.icp_batch_stats(), lambda: e.icp_batch_get_aligned(0)):
        with pytest.raises(ndt.NDTError) as err:
            call()
        assert err.value.code == -7
    e.stream_end()
    res = e.icp_batch_align(np.stack([I4, I4]))                 # the refused calls changed nothing
    assert all(r["converged"] and r["mse"] == 0.0 for r in res) and [r["matches"] for r in res] == [300, 50]
    e.close()
