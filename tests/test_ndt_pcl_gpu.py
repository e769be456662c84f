"""GPU (-m gpu): MI355NDT_OPT_NDT_CLASS = 1, pcl::NormalDistributionsTransform (registration_method = NDT), against tools/ndt_pcl_ref.py.

Bars: a sweep (score, g, H) -- test_gpu_parity.check_sweep at its own rtol of 1e-11 of the largest entry, equal hit counts (both sides f64: they
differ in sum order and in the last bits of exp / sin / cos); an align -- equal converged / iterations / sweeps / hits_last, the final pose
within 1e-4 m and 1e-5 rad, transformation_ / previous_transformation_ within 1e-6; batches, class switches, refusals and the loop check --
result records byte for byte.  The restatement's values come from the fixture tests/golden/ndt_pcl.npz, which the tool writes
(tests/test_ndt_pcl_cpu.py regenerates cases of it and shows that the f32 Euler model with KDTREE is 100 bars away from it)."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import loop_closure, ndt
from test_gpu_parity import check_sweep

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


P = _load("ndt_pcl_ref")
E = P.E
BASE = dict(trans_epsilon=0.01, max_iterations=64)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_pcl.npz"))


def pcl_engine(**kw):
    eng = ndt.Engine(ndt.default_params(**BASE, **kw))
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    return eng


def fixture_sweep(fx, key):
    return float(fx[key + "/score"]), fx[key + "/g"], fx[key + "/H"], int(fx[key + "/hits"])


def record(r):
    """every word of a result record"""
    return (r["final"].tobytes(), np.float64(r["score"]).tobytes(), np.float64(r["trans_probability"]).tobytes(), r["iterations"], r["converged"], r["sweeps"],
            r["hits_last"], r["status"])


def test_option_is_known():
    """1 (fails on the parent commit, where 13 is an unknown option)"""
    eng = ndt.Engine(ndt.default_params(**BASE))
    assert eng.get_option(ndt.OPT_NDT_CLASS) == 0
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    assert eng.get_option(ndt.OPT_NDT_CLASS) == 1
    eng.close()
    reg = ndt.NormalDistributionsTransform(ndt_class="pcl")
    assert reg.engine.get_option(ndt.OPT_NDT_CLASS) == 1
    assert not hasattr(reg, "setNeighborhoodSearchMethod") and not hasattr(reg, "setNumThreads")       # PCL's class has neither
    assert hasattr(ndt.NormalDistributionsTransform(), "setNeighborhoodSearchMethod")


def test_one_sweep_shapes(fx):
    """2: one lane, one tile, a tile and one point, an item (512 points) and one point, a chunk (2048 points) and one point"""
    tgt, _ = E.clouds(P.SHAPE_PAIR)
    eng = pcl_engine(resolution=P.SHAPE_RES)
    eng.set_target(tgt)
    assert all(0.1 < a < 1 for a in P.SHAPE_POSE[3:])
    assert int(fx["shape/1/hits"]) >= 1                              # the one-point case has a hit
    for n in P.SHAPE_SIZES:
        s = P.shape_source(n)
        assert len(s) == n
        eng.set_source(s)
        got = eng.derivatives(P.SHAPE_POSE)
        ref = fixture_sweep(fx, f"shape/{n}")
        print(f"shapes: n = {n}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.15g} / {ref[0]:.15g}")
        check_sweep(got, ref)
    eng.close()


def test_one_sweep_poses(fx):
    """3: 500 points, > 1000 hits; all angles zero, one angle inside the snap (5e-5) and just outside it (2e-4), roll near pi, pitch 1.5; and
    neighbor_mode is not consulted: DIRECT1 and KDTREE give the same words"""
    cases = P.pose_cases()
    assert sorted(cases) == ["pitch_1.5", "roll_pi", "snapped", "unsnapped", "zero"]
    assert cases["snapped"][1][4] == 5e-5 and cases["unsnapped"][1][4] == 2e-4 and abs(cases["roll_pi"][1][3] - np.pi) < 0.31 and cases["pitch_1.5"][1][4] == 1.5
    for name in cases:                                              # on the restatement alone: no comparison of near-empty sums
        assert int(fx[f"pose/{name}/hits"]) > 1000
    tgt, _ = E.clouds(P.POSE_PAIR)
    words = {}
    for mode in (ndt.DIRECT1, ndt.KDTREE):
        eng = pcl_engine(neighbor_mode=mode, resolution=P.POSE_RES)
        eng.set_target(tgt)
        for name, (s, p) in cases.items():
            assert len(s) == P.POSE_N
            eng.set_source(s)
            got = eng.derivatives(p)
            ref = fixture_sweep(fx, f"pose/{name}")
            print(f"poses: {name} mode {mode}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.15g} / {ref[0]:.15g}, "
                  f"max |dH| / scale {np.abs(got[2] - ref[2]).max() / max(1.0, np.abs(ref[2]).max()):.2e}")
            check_sweep(got, ref)
            words.setdefault(name, []).append((np.float64(got[0]).tobytes(), got[1].tobytes(), got[2].tobytes(), got[3]))
        eng.close()
    for name, w in words.items():
        assert w[0] == w[1], name


@pytest.mark.parametrize("i", range(len(P.ALIGNS)))
def test_aligns(fx, i):
    """4: four pairs of 500 points from default_guess(), a guess with roll -0.3, one with yaw 1.3, and one at the factory's resolution 0.5"""
    steps = fx[f"align/{i}/steps"]
    # an equal iteration count is a fair demand only away from a convergence decision: asserted on the restatement before the device is looked at
    assert (np.abs(steps - BASE["trans_epsilon"]) > 0.05 * BASE["trans_epsilon"]).all()
    tgt, s, G, res = P.align_inputs(i)
    assert len(s) == P.ALIGNS[i][4]
    if res == P.FACTORY_RES:                                         # hits on most source points
        assert int(fx[f"align/{i}/points_with_hits"]) > 0.75 * len(s)
    eng = pcl_engine(resolution=res)
    eng.set_target(tgt)
    eng.set_source(s)
    r = eng.align(G)
    inc, prev = eng.get_incremental(0)
    dt, dr = se3_err(fx[f"align/{i}/final"], r["final"])
    print(f"align {i} {P.ALIGNS[i]}: iterations gpu {r['iterations']} restatement {int(fx[f'align/{i}/iterations'])}, sweeps {r['sweeps']} / {int(fx[f'align/{i}/sweeps'])}, "
          f"hits {r['hits_last']} / {int(fx[f'align/{i}/hits'])}, dtrans {dt:.3e} drot {dr:.3e}, d inc {np.abs(inc - fx[f'align/{i}/inc']).max():.2e}, "
          f"d prev_inc {np.abs(prev - fx[f'align/{i}/prev_inc']).max():.2e}")
    assert r["converged"] == int(fx[f"align/{i}/converged"]) and r["iterations"] == int(fx[f"align/{i}/iterations"]) and r["sweeps"] == int(fx[f"align/{i}/sweeps"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert np.abs(inc - fx[f"align/{i}/inc"]).max() <= 1e-6 and np.abs(prev - fx[f"align/{i}/prev_inc"]).max() <= 1e-6
    assert r["hits_last"] == int(fx[f"align/{i}/hits"])
    eng.close()


def nine_pairs():
    """sizes of tests 2 and 4 mixed, different guesses (two of them turned: the chart near roll = pi, a large yaw)"""
    out = []
    for k, (n, axis, angle) in enumerate([(500, None, 0), (1, None, 0), (64, (1, 0, 0), -0.3), (65, None, 0), (513, (0, 0, 1), 1.3), (2049, None, 0), (500, (0, 1, 0), 0.4),
                                          (2049, (1, 0, 0), -0.3), (500, None, 0)]):
        tgt, src = E.clouds(1 + k)
        s, G = E.turned(E.subsample(src[E.SHAPE_START:], n), axis, angle)
        G = G.copy()
        G[1, 3] += np.float32(0.05 * k)
        out.append((tgt, s, G))
    return out


def load_batch(eng, pairs):
    eng.batch_reserve(len(pairs), 8192, 2049)
    for b, (tgt, s, _) in enumerate(pairs):
        eng.batch_set_target(b, tgt)
        eng.batch_set_source(b, s)


def test_batch_independence():
    """5: nine pairs in one batch: every slot's record equals, byte for byte, that of an engine holding that pair alone"""
    pairs = nine_pairs()
    eng = pcl_engine()
    load_batch(eng, pairs)
    eng.profile_enable(True)
    rb = eng.batch_align(np.stack([G for _, _, G in pairs]))
    assert eng.profile_get()["async_fallbacks"] == 0
    eng.close()
    for b, (tgt, s, G) in enumerate(pairs):
        one = pcl_engine()
        one.set_target(tgt)
        one.set_source(s)
        r1 = one.align(G)
        one.close()
        print(f"batch slot {b}: n = {len(s)}, iterations {rb[b]['iterations']} / {r1['iterations']}, hits {rb[b]['hits_last']}")
        assert record(rb[b]) == record(r1), b
    assert len({r["iterations"] for r in rb}) > 1                 # the slots end in different rounds


@pytest.mark.parametrize("async_align", [1, 2])
def test_no_leak_between_classes(async_align):
    """6: class 1, class 0, class 1 again, and class 1 <-> POSE_MODEL = 1, on one engine whose target was built under class 0 / DIRECT7 (no
    centroids, no f64 inverse covariances: rebuilt, not misread -- a misread would not repeat the words of an engine that built under class 1)"""
    pairs = nine_pairs()[:3]
    G = np.stack([g for _, _, g in pairs])

    def fresh(cls, model):
        e = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
        e.set_option(ndt.OPT_ASYNC_ALIGN, async_align)
        e.set_option(ndt.OPT_NDT_CLASS, cls)
        e.set_option(ndt.OPT_POSE_MODEL, model)
        load_batch(e, pairs)
        out = [record(r) for r in e.batch_align(G)]
        e.close()
        return out

    want0, want1, want_euler = fresh(0, 0), fresh(1, 0), fresh(0, 1)
    assert want1 != want0 and want1 != want_euler                   # (three different registrations)
    eng = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, async_align)
    eng.profile_enable(True)
    load_batch(eng, pairs)
    assert [record(r) for r in eng.batch_align(G)] == want0          # the target is resident as class 0 / DIRECT7 built it
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    assert [record(r) for r in eng.batch_align(G)] == want1
    eng.set_option(ndt.OPT_NDT_CLASS, 0)
    assert [record(r) for r in eng.batch_align(G)] == want0
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    assert [record(r) for r in eng.batch_align(G)] == want1          # ... and back
    eng.set_option(ndt.OPT_POSE_MODEL, 1)                          # not consulted under class 1
    assert [record(r) for r in eng.batch_align(G)] == want1
    eng.set_option(ndt.OPT_NDT_CLASS, 0)
    assert [record(r) for r in eng.batch_align(G)] == want_euler
    eng.set_option(ndt.OPT_NDT_CLASS, 1)
    assert [record(r) for r in eng.batch_align(G)] == want1
    assert eng.profile_get()["async_fallbacks"] == 0
    eng.close()


def test_refusals():
    """7: every entry of the refusal list returns its code with a message and leaves the next class-1 align's words unchanged"""
    tgt, s, G = nine_pairs()[0]
    eng = pcl_engine()
    eng.set_target(tgt)
    eng.set_source(s)
    want = record(eng.align(G))
    p = np.array([1.0, 0, 0, 0.1, 0.2, 0.3])

    def refused(code, f, *a, **kw):
        with pytest.raises(ndt.NDTError) as e:
            f(*a, **kw)
        assert e.value.code == code, (e.value.code, code)
        assert "(" in str(e.value) and len(str(e.value).split("(", 1)[1]) > 10, str(e.value)       # a message from the engine
        assert eng.get_option(ndt.OPT_NDT_CLASS) == 1
        assert record(eng.align(G)) == want

    def with_params(f, **kw):
        keep = eng.get_params()
        eng.set_params(ndt.default_params(**BASE, **kw))
        try:
            f()
        finally:
            eng.set_params(keep)
            eng.set_target(tgt)                                    # (the grids of the configuration the aligns use)

    UNSUPPORTED, STATE, BAD_ARG = -6, -7, -2
    assert (ndt.ERR[UNSUPPORTED], ndt.ERR[-7]) == ("unsupported configuration", "target/source not set")
    refused(UNSUPPORTED, with_params, lambda: eng.align(G), variant=ndt.VARIANT_PCA)
    refused(UNSUPPORTED, with_params, lambda: eng.align(G), step_size=0.004)                     # live More-Thuente: step_size <= eps / 2
    refused(UNSUPPORTED, eng.compute_hessian, p)
    refused(UNSUPPORTED, eng.derivatives_T, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32))
    frames = [s, s]
    refused(UNSUPPORTED, eng.sequence_run, frames, [0.0, 0.1])
    refused(UNSUPPORTED, eng.sequence_run_raw, frames, [0.0, 0.1])
    refused(UNSUPPORTED, eng.stream_begin, 2, 4, 8192, 2049)
    # value 2 is no class
    with pytest.raises(ndt.NDTError) as e:
        eng.set_option(ndt.OPT_NDT_CLASS, 2)
    assert e.value.code == BAD_ARG and eng.get_option(ndt.OPT_NDT_CLASS) == 1
    assert record(eng.align(G)) == want
    # the tolerance arithmetic and the f32 sum order are not consulted: the same words, no warning status
    eng.set_option(ndt.OPT_ARITH, 1)
    assert record(eng.align(G)) == want and want[-1] == ndt.OK
    eng.set_option(ndt.OPT_ARITH, 0)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, 1)
    assert record(eng.align(G)) == want
    eng.close()
    # setting the option while a stream is open: a state error, the stream's class unchanged
    st = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    st.stream_begin(2, 4, 8192, 2049)
    with pytest.raises(ndt.NDTError) as e:
        st.set_option(ndt.OPT_NDT_CLASS, 1)
    assert e.value.code == STATE and "stream" in str(e.value)
    assert st.get_option(ndt.OPT_NDT_CLASS) == 0
    st.stream_end()
    st.close()


def test_loop_check():
    """8: verify_candidates with three candidates against one target on a class-1 engine: the (converged, score, final) triples are those of three
    single aligns plus fitness_score at the final pose, byte for byte -- host clouds, and keyframe ids in their place"""
    pairs = nine_pairs()
    tgt = pairs[0][0]
    cands = [pairs[0][1], pairs[4][1][:300], pairs[5][1]]            # 500, 300 and 2049 points
    G = np.stack([pairs[0][2], pairs[0][2], pairs[0][2]])
    singles = []
    for s, g in zip(cands, G):
        one = pcl_engine()
        one.set_target(tgt)
        one.set_source(s)
        r = one.align(g)
        singles.append((r["converged"], one.fitness_score(5.0, T=r["final"])[0], r["final"].tobytes()))
        one.close()
    want = loop_closure.select_matching([c for c, _, _ in singles], [s for _, s, _ in singles], [np.frombuffer(f, np.float32).reshape(4, 4) for _, _, f in singles], 1e9)
    for use_ids in (False, True):
        eng = pcl_engine()
        t, c = (eng.keyframe_add(tgt), [eng.keyframe_add(s) for s in cands]) if use_ids else (tgt, cands)
        idx, pose, best, aligns = loop_closure.verify_candidates_ndt(eng, t, c, G, max_range=5.0, thresh=1e9)
        res = eng.batch_align(G)                                   # (the batch is still loaded: the same call again, for the triples)
        sc, _ = eng.batch_fitness_scores(5.0)
        got = [(r["converged"], float(s), r["final"].tobytes()) for r, s in zip(res, sc)]
        print("loop check", "ids" if use_ids else "host clouds", [(g[0], g[1]) for g in got], "selected", idx, best)
        assert got == singles
        assert (idx, best, aligns) == (want[0], want[2], want[3]) and pose.tobytes() == want[1].tobytes()
        eng.close()
    plain = ndt.Engine(ndt.default_params(**BASE))                   # a class-0 engine does not answer for NDT
    with pytest.raises(ValueError):
        loop_closure.verify_candidates_ndt(plain, tgt, cands, G)
    plain.close()
