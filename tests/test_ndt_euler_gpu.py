"""GPU (-m gpu): MI355NDT_OPT_POSE_MODEL = 1, the Euler-angle NDT of include/ndt_omp/ndt_omp_impl.hpp, against tools/ndt_euler_ref.py.

Bars: a sweep (score, g, H) -- test_gpu_parity.check_sweep at its own rtol of 1e-11 of the largest entry, equal hit counts; an align -- equal
converged / iterations / sweeps, the final pose within 1e-4 m and 1e-5 rad (README, north_star), transformation_ / previous_transformation_
equal to 1e-6; batches, model switches and refusals -- result records byte for byte.  The restatement's values come from the fixture
tests/golden/ndt_euler.npz, which the tool writes (tests/test_ndt_euler_cpu.py regenerates a case of it): every hit is evaluated in Python."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import ndt, synth
from test_gpu_parity import check_sweep

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


E = _load("ndt_euler_ref")
MODES = {E.DIRECT1: ndt.DIRECT1, E.DIRECT7: ndt.DIRECT7, E.DIRECT26: ndt.DIRECT26, E.KDTREE: ndt.KDTREE}
BASE = dict(trans_epsilon=0.01, max_iterations=64)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_euler.npz"))


def euler_engine(order=0, **kw):
    eng = ndt.Engine(ndt.default_params(**BASE, **kw))
    eng.set_option(ndt.OPT_POSE_MODEL, 1)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    return eng


def fixture_sweep(fx, key):
    return float(fx[key + "/score"]), fx[key + "/g"], fx[key + "/H"], int(fx[key + "/hits"])


def record(r):
    """every word of a result record"""
    return (r["final"].tobytes(), np.float64(r["score"]).tobytes(), np.float64(r["trans_probability"]).tobytes(), r["iterations"], r["converged"], r["sweeps"],
            r["hits_last"], r["status"])


def test_option_is_known():
    """1 (fails on the parent commit, where 12 is an unknown option)"""
    eng = ndt.Engine(ndt.default_params(**BASE))
    assert eng.get_option(ndt.OPT_POSE_MODEL) == 0
    eng.set_option(ndt.OPT_POSE_MODEL, 1)
    assert eng.get_option(ndt.OPT_POSE_MODEL) == 1
    eng.close()
    reg = ndt.NormalDistributionsTransform(pose_model="euler")
    assert reg.engine.get_option(ndt.OPT_POSE_MODEL) == 1


def test_one_sweep_shapes(fx):
    """2: DIRECT1; one lane, one tile, a tile and one point, an item (512 points) and one point, a chunk (2048 points) and one point"""
    tgt, _ = E.clouds(E.SHAPE_PAIR)
    eng = euler_engine(neighbor_mode=ndt.DIRECT1)
    eng.set_target(tgt)
    assert all(0.1 < a < 1 for a in E.SHAPE_POSE[3:])
    for n in E.SHAPE_SIZES:
        s = E.shape_source(n)
        assert len(s) == n
        eng.set_source(s)
        got = eng.derivatives(E.SHAPE_POSE)
        ref = fixture_sweep(fx, f"shape/{n}")
        print(f"shapes: n = {n}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.12g} / {ref[0]:.12g}")
        check_sweep(got, ref)
    eng.close()


@pytest.mark.parametrize("mode", list(E.POSE_MODES))
def test_one_sweep_poses(fx, mode):
    """3: 500 points; all angles zero, one angle inside the snap (5e-5) and just outside it (2e-4), roll near pi (the chart a guess with negative
    roll starts in), pitch 1.5; both f32 sum orders against the restatement run in the same order"""
    m, res = E.POSE_MODES[mode]
    cases = E.pose_cases()
    assert sorted(cases) == ["pitch_1.5", "roll_pi", "snapped", "unsnapped", "zero"]
    assert cases["snapped"][1][4] == 5e-5 and cases["unsnapped"][1][4] == 2e-4 and abs(cases["roll_pi"][1][3] - np.pi) < 0.31 and cases["pitch_1.5"][1][4] == 1.5
    for order in (0, 1):                                            # on the restatement alone: no comparison of near-empty sums
        for name in cases:
            assert int(fx[f"pose/{mode}/{name}/{order}/hits"]) > 1000
    tgt, _ = E.clouds(E.POSE_PAIR)
    for order in (0, 1):
        eng = euler_engine(order, neighbor_mode=MODES[m], resolution=res)
        eng.set_target(tgt)
        for name, (s, p) in cases.items():
            assert len(s) == E.POSE_N
            eng.set_source(s)
            got = eng.derivatives(p)
            ref = fixture_sweep(fx, f"pose/{mode}/{name}/{order}")
            print(f"poses: {mode} {name} order {order}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.12g} / {ref[0]:.12g}")
            check_sweep(got, ref)
        eng.close()
    # the two orders are different evaluations (else the second loop showed nothing)
    assert float(fx[f"pose/{mode}/zero/0/score"]) != float(fx[f"pose/{mode}/zero/1/score"])


@pytest.mark.parametrize("i", range(len(E.ALIGNS)))
def test_aligns(fx, i):
    """4: four pairs from default_guess() with DIRECT7, a guess with roll -0.3 and one with yaw 1.3 (test_large_rotation_gpu.turned) with DIRECT1"""
    steps = fx[f"align/{i}/steps"]
    # an equal iteration count is a fair demand only away from a convergence decision: asserted on the restatement before the device is looked at
    assert (np.abs(steps - BASE["trans_epsilon"]) > 0.05 * BASE["trans_epsilon"]).all()
    tgt, s, G, mode = E.align_inputs(i)
    assert len(s) == E.ALIGN_N
    eng = euler_engine(neighbor_mode=MODES[mode])
    eng.set_target(tgt)
    eng.set_source(s)
    r = eng.align(G)
    inc, prev = eng.get_incremental(0)
    dt, dr = se3_err(fx[f"align/{i}/final"], r["final"])
    print(f"align {i} {E.ALIGNS[i]}: iterations gpu {r['iterations']} restatement {int(fx[f'align/{i}/iterations'])}, sweeps {r['sweeps']} / {int(fx[f'align/{i}/sweeps'])}, "
          f"dtrans {dt:.3e} drot {dr:.3e}, d inc {np.abs(inc - fx[f'align/{i}/inc']).max():.2e}, d prev_inc {np.abs(prev - fx[f'align/{i}/prev_inc']).max():.2e}")
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


def test_batch_independence():
    """5: nine pairs in one batch: every slot's record equals, byte for byte, that of an engine holding that pair alone"""
    pairs = nine_pairs()
    eng = euler_engine(neighbor_mode=ndt.DIRECT7)
    eng.batch_reserve(len(pairs), 8192, 2049)
    for b, (tgt, s, _) in enumerate(pairs):
        eng.batch_set_target(b, tgt)
        eng.batch_set_source(b, s)
    eng.profile_enable(True)
    rb = eng.batch_align(np.stack([G for _, _, G in pairs]))
    assert eng.profile_get()["async_fallbacks"] == 0
    eng.close()
    for b, (tgt, s, G) in enumerate(pairs):
        one = euler_engine(neighbor_mode=ndt.DIRECT7)
        one.set_target(tgt)
        one.set_source(s)
        r1 = one.align(G)
        one.close()
        print(f"batch slot {b}: n = {len(s)}, iterations {rb[b]['iterations']} / {r1['iterations']}, hits {rb[b]['hits_last']}")
        assert record(rb[b]) == record(r1), b
    assert len({r["iterations"] for r in rb}) > 1                 # the slots end in different rounds


@pytest.mark.parametrize("async_align", [1, 2])
def test_no_leak_between_models(async_align):
    """6: model 1, align, model 0, align: the words of a fresh engine under model 0 -- with OPT_ASYNC_ALIGN = 2 the one-launch route is re-entered"""
    pairs = nine_pairs()[:3]
    G = np.stack([g for _, _, g in pairs])

    def load(eng):
        eng.batch_reserve(len(pairs), 8192, 2049)
        for b, (tgt, s, _) in enumerate(pairs):
            eng.batch_set_target(b, tgt)
            eng.batch_set_source(b, s)

    fresh = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    fresh.set_option(ndt.OPT_ASYNC_ALIGN, async_align)
    load(fresh)
    want = [record(r) for r in fresh.batch_align(G)]
    fresh.close()
    eng = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, async_align)
    eng.profile_enable(True)
    load(eng)
    eng.set_option(ndt.OPT_POSE_MODEL, 1)
    r1 = [record(r) for r in eng.batch_align(G)]
    assert eng.profile_get()["async_fallbacks"] == 0
    eng.set_option(ndt.OPT_POSE_MODEL, 0)
    r0 = [record(r) for r in eng.batch_align(G)]
    assert eng.profile_get()["async_fallbacks"] == 0
    assert r0 == want
    assert r1 != want                                              # (the two models are different registrations)
    eng.set_option(ndt.OPT_POSE_MODEL, 1)
    assert [record(r) for r in eng.batch_align(G)] == r1           # ... and back
    eng.close()


def test_refusals():
    """7: every entry of the refusal list returns its code with a message and leaves the next model-1 align's words unchanged"""
    tgt, s, G = nine_pairs()[0]
    eng = euler_engine(neighbor_mode=ndt.DIRECT7)
    eng.set_target(tgt)
    eng.set_source(s)
    want = record(eng.align(G))
    p = np.array([1.0, 0, 0, 0.1, 0.2, 0.3])

    def refused(code, f, *a, **kw):
        with pytest.raises(ndt.NDTError) as e:
            f(*a, **kw)
        assert e.value.code == code, (e.value.code, code)
        assert "(" in str(e.value) and len(str(e.value).split("(", 1)[1]) > 10, str(e.value)       # a message from the engine
        assert eng.get_option(ndt.OPT_POSE_MODEL) == 1
        assert record(eng.align(G)) == want

    def with_params(f, **kw):
        keep = eng.get_params()
        eng.set_params(ndt.default_params(**dict(BASE, neighbor_mode=ndt.DIRECT7), **kw))
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
    # value 2 is no model
    with pytest.raises(ndt.NDTError) as e:
        eng.set_option(ndt.OPT_POSE_MODEL, 2)
    assert e.value.code == BAD_ARG and eng.get_option(ndt.OPT_POSE_MODEL) == 1
    assert record(eng.align(G)) == want
    # the tolerance arithmetic is ignored: the same words, no warning status
    eng.set_option(ndt.OPT_ARITH, 1)
    assert record(eng.align(G)) == want and want[-1] == ndt.OK
    eng.set_option(ndt.OPT_ARITH, 0)
    eng.close()
    # setting the option while a stream is open: a state error, the stream's model unchanged
    st = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    st.stream_begin(2, 4, 8192, 2049)
    with pytest.raises(ndt.NDTError) as e:
        st.set_option(ndt.OPT_POSE_MODEL, 1)
    assert e.value.code == STATE and "stream" in str(e.value)
    assert st.get_option(ndt.OPT_POSE_MODEL) == 0
    st.stream_end()
    st.close()
