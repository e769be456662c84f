"""GPU (-m gpu): MI355NDT_OPT_GROUND_CLASS, pclomp_ground::NormalDistributionsTransformGround (ndt_ground_impl.hpp), against tools/ndt_ground_ref.py.

Bars: the leaves' class codes -- equal on every record; a sweep (score, g, H) -- test_gpu_parity.check_sweep at its own rtol of 1e-11 of the
largest entry, equal hit counts, masked entries exactly 0.0; class 3 against the option-0 engine -- bit for bit; an align -- equal converged /
iterations / sweeps, the final pose within 1e-4 m and 1e-5 rad, transformation_ / previous_transformation_ equal to 1e-6; batches, switches
and refusals -- result records byte for byte.  The restatement's values come from the fixture tests/golden/ndt_ground.npz, which the tool
writes (tests/test_ndt_ground_cpu.py regenerates cases of it and re-asserts its scene conditions); the hand-made scenes are a dozen points
and are restated here."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT, se3_err
from lv_slam_amd import ndt
from test_gpu_parity import check_sweep

pytestmark = pytest.mark.gpu


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


G = _load("ndt_ground_ref")
mg = G.mg
MODES = {G.DIRECT1: ndt.DIRECT1, G.DIRECT7: ndt.DIRECT7, G.DIRECT26: ndt.DIRECT26}
BASE = dict(trans_epsilon=0.01, max_iterations=64)
HELD = {1: [0, 1, 5], 2: [2, 3, 4], 3: []}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "ndt_ground.npz"))


def ground_engine(cls, order=0, **kw):
    eng = ndt.Engine(ndt.default_params(**BASE, **kw))
    eng.set_option(ndt.OPT_GROUND_CLASS, cls)
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    return eng


def fixture_sweep(fx, key):
    return float(fx[key + "/score"]), fx[key + "/g"], fx[key + "/H"], int(fx[key + "/hits"])


def restated(r):
    score, g, H, hits, _ = r
    return float(score), g, H, int(hits)


def record(r):
    """every word of a result record"""
    return (r["final"].tobytes(), np.float64(r["score"]).tobytes(), np.float64(r["trans_probability"]).tobytes(), r["iterations"], r["converged"], r["sweeps"],
            r["hits_last"], r["status"])


def check_masked(got, cls):
    """masked entries are +0.0 exactly (not -0.0, not a small number)"""
    _, g, H, _ = got
    H = np.asarray(H).reshape(6, 6)
    held = HELD[cls]
    for a in (np.asarray(g)[held], H[held, :], H[:, held]):
        assert (a == 0).all() and not np.signbit(a).any()


def test_option_is_known():
    """1 (fails on the parent commit, where 15 is an unknown option)"""
    eng = ndt.Engine(ndt.default_params(**BASE))
    assert eng.get_option(ndt.OPT_GROUND_CLASS) == 0
    for v in (1, 2, 3, 0):
        eng.set_option(ndt.OPT_GROUND_CLASS, v)
        assert eng.get_option(ndt.OPT_GROUND_CLASS) == v
    eng.close()
    reg = ndt.NormalDistributionsTransform(ground_class="vertical")
    assert reg.engine.get_option(ndt.OPT_GROUND_CLASS) == 2
    reg = ndt.NormalDistributionsTransformGround()
    assert reg.engine.get_option(ndt.OPT_GROUND_CLASS) == 1 and reg.getFlagClass() == 1
    assert ndt.NormalDistributionsTransformGround(flag_class=0).engine.get_option(ndt.OPT_GROUND_CLASS) == 3


def test_leaf_classes(fx):
    """2: the code array, read alone through the build buffer, on every record of the fixture scenes and of the three-leaf scene"""
    for pair, res in G.fixture_scenes():
        tgt, _ = G.clouds(pair)
        eng = ground_engine(1, neighbor_mode=ndt.DIRECT7, resolution=res)
        eng.set_target(tgt)
        eng.batch_build_targets()
        codes = eng.get_build_buffer("leaf_class")
        want = fx[f"codes/{pair}/{res}"]
        print(f"pair {pair} resolution {res}: {len(codes)} records, codes 0..3: {np.bincount(codes, minlength=4)}")
        assert codes.dtype == np.uint8 and len(codes) == len(want) == len(eng.get_build_buffer("vox_n")) and (codes == want).all()
        assert ((codes == 0) == (eng.get_build_buffer("vox_n") == -1)).all()
        eng.close()
    tgt, want = G.three_leaf_scene()
    eng = ground_engine(2, neighbor_mode=ndt.DIRECT1)
    eng.set_target(tgt)
    eng.batch_build_targets()
    assert list(eng.get_build_buffer("leaf_class")) == want == [1, 2, 3]          # the five-point cell is no record
    eng.close()
    # a build that does not need the codes does not make them
    eng = ground_engine(3, neighbor_mode=ndt.DIRECT1)
    eng.set_target(tgt)
    eng.batch_build_targets()
    with pytest.raises(ndt.NDTError) as e:
        eng.get_build_buffer("leaf_class")
    assert e.value.code == -2
    eng.close()


@pytest.mark.parametrize("cls", [1, 2, 3])
def test_one_sweep_shapes(fx, cls):
    """3: DIRECT1; one lane, one tile, a tile and one point, an item (512 points) and one point, a chunk (2048 points) and one point"""
    tgt, _ = G.clouds(G.SHAPE_PAIR)
    p, _ = G.sweep_pose()
    eng = ground_engine(cls, neighbor_mode=ndt.DIRECT1, resolution=G.SHAPE_RES)
    eng.set_target(tgt)
    for n in G.SHAPE_SIZES:
        s = G.shape_source(n)
        assert len(s) == n
        eng.set_source(s)
        got = eng.derivatives(p)
        ref = fixture_sweep(fx, f"shape/{n}/{cls}")
        print(f"shapes: class {cls} n = {n}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.12g} / {ref[0]:.12g}")
        check_sweep(got, ref)
        check_masked(got, cls)
    assert int(fx[f"shape/2049/{cls}/hits"]) > 50
    eng.close()


@pytest.mark.parametrize("mode", [ndt.DIRECT1, ndt.DIRECT7, ndt.DIRECT26])
def test_class_all_is_twice_the_engine(mode):
    """4: class 3 against the engine itself: g and H bit for bit 2 * the option-0 engine's derivatives at the same pose, the score bit for bit
    equal; both f32 sum orders"""
    tgt, src = G.clouds(2)
    s = G.subsample(src, 2049)
    p, _ = G.sweep_pose()
    for order in (0, 1):
        plain = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=mode))
        plain.set_option(ndt.OPT_F32_SUM_ORDER, order)
        plain.set_target(tgt)
        plain.set_source(s)
        s0, g0, H0, h0 = plain.derivatives(p)
        plain.close()
        eng = ground_engine(3, order, neighbor_mode=mode)
        eng.set_target(tgt)
        eng.set_source(s)
        s3, g3, H3, h3 = eng.derivatives(p)
        eng.close()
        print(f"mode {mode} order {order}: hits {h3}, score {s3:.12g}")
        assert h3 == h0 > 500 and np.float64(s3).tobytes() == np.float64(s0).tobytes()
        assert (2 * np.asarray(g0)).tobytes() == np.asarray(g3).tobytes() and (2 * np.asarray(H0)).tobytes() == np.asarray(H3).tobytes()


@pytest.mark.parametrize("name", list(G.LAST_SCENES))
def test_the_last_neighbour_decides(fx, name):
    """5a: DIRECT7 and DIRECT26 sweeps on scenes in which the tool counted at least 20 source points whose first and last live neighbours
    have different codes: a gate on the first neighbour, or on any neighbour, gives other sums"""
    pair, res, mode = G.LAST_SCENES[name]
    assert int(fx[f"last/{name}/differing"]) >= 20
    tgt, _ = G.clouds(pair)
    p, _ = G.sweep_pose()
    s = G.last_source(name)
    for cls in (1, 2, 3):
        eng = ground_engine(cls, neighbor_mode=MODES[mode], resolution=res)
        eng.set_target(tgt)
        eng.set_source(s)
        got = eng.derivatives(p)
        ref = fixture_sweep(fx, f"last/{name}/{cls}")
        print(f"{name} class {cls}: hits gpu {got[3]} restatement {ref[3]}, score {got[0]:.12g} / {ref[0]:.12g}")
        check_sweep(got, ref)
        check_masked(got, cls)
        eng.close()
    assert int(fx[f"last/{name}/1/hits"]) + int(fx[f"last/{name}/2/hits"]) < int(fx[f"last/{name}/3/hits"])


@pytest.mark.parametrize("mode", [G.DIRECT1, G.DIRECT7])
def test_floor_next_to_wall(mode):
    """5b: the hand-made scene: points whose first neighbour is the floor and whose last is a wall (and the other way round), a point whose
    only neighbour is a dead leaf, points outside the grid -- they add nothing under class 2 and zeros under class 1"""
    tgt, src = G.floor_wall_scene()
    want = G.hand_sweeps(mode)
    for flag, cls in G.OPTION_OF_FLAG.items():
        eng = ground_engine(cls, neighbor_mode=MODES[mode], min_points_per_voxel=G.HAND_MIN_POINTS)
        eng.set_target(tgt)
        eng.set_source(src)
        got = eng.derivatives(G.IDENTITY_P)
        print(f"floor / wall mode {mode} class {cls}: hits gpu {got[3]} restatement {want[flag][3]}, score {got[0]:.12g} / {want[flag][0]:.12g}")
        check_sweep(got, restated(want[flag]))
        check_masked(got, cls)
        # the points without a live neighbour alone: no hit, every sum zero
        eng.set_source(src[7:])
        s, g, H, hits = eng.derivatives(G.IDENTITY_P)
        assert hits == 0 and s == 0 and not np.asarray(g).any() and not np.asarray(H).any()
        eng.close()
    if mode == G.DIRECT7:
        assert want[1][3] == 8 and want[2][3] == 6 and want[0][3] == 15     # (a first-neighbour gate would give 6 / 8)


@pytest.mark.parametrize("i", range(len(G.ALIGNS)))
def test_aligns(fx, i):
    """6: classes 1, 2 and 3 with DIRECT1 and DIRECT7; case 0 is the nodelet's ground_s2k configuration, case 1 ends after one iteration"""
    steps = fx[f"align/{i}/steps"]
    assert (np.abs(steps - BASE["trans_epsilon"]) > 0.05 * BASE["trans_epsilon"]).all()
    tgt, s, G0, res, mode, flag = G.align_inputs(i)
    assert len(s) == G.ALIGN_N
    eng = ground_engine(G.OPTION_OF_FLAG[flag], neighbor_mode=MODES[mode], resolution=res)
    eng.set_target(tgt)
    eng.set_source(s)
    r = eng.align(G0)
    inc, prev = eng.get_incremental(0)
    dt, dr = se3_err(fx[f"align/{i}/final"], r["final"])
    print(f"align {i} {G.ALIGNS[i]}: iterations gpu {r['iterations']} restatement {int(fx[f'align/{i}/iterations'])}, sweeps {r['sweeps']} / {int(fx[f'align/{i}/sweeps'])}, "
          f"dtrans {dt:.3e} drot {dr:.3e}, d inc {np.abs(inc - fx[f'align/{i}/inc']).max():.2e}, d prev_inc {np.abs(prev - fx[f'align/{i}/prev_inc']).max():.2e}")
    assert r["converged"] == int(fx[f"align/{i}/converged"]) and r["iterations"] == int(fx[f"align/{i}/iterations"]) and r["sweeps"] == int(fx[f"align/{i}/sweeps"])
    assert dt < 1e-4 and dr < 1e-5, (dt, dr)
    assert np.abs(inc - fx[f"align/{i}/inc"]).max() <= 1e-6 and np.abs(prev - fx[f"align/{i}/prev_inc"]).max() <= 1e-6
    assert r["hits_last"] == int(fx[f"align/{i}/hits"])
    if i == 1:
        assert r["iterations"] == 1
    if i == 0:
        assert (res, mode, flag) == (10.0, G.DIRECT1, 1)
    eng.close()


def four_pairs():
    out = []
    for k, n in enumerate((500, 1, 65, 2049)):
        tgt, src = G.clouds(1 + k)
        Gk = G.default_guess().copy()
        Gk[1, 3] += np.float32(0.05 * k)
        out.append((tgt, G.subsample(src[G.SHAPE_START:], n), Gk))
    return out


@pytest.mark.parametrize("cls", [1, 3])
def test_batch_equals_single_pairs(cls):
    """7a: four pairs of mixed sizes in one batch -- host clouds, then the same targets as resident keyframes -- equal the single-pair aligns
    byte for byte"""
    pairs = four_pairs()
    singles = []
    for tgt, s, Gk in pairs:
        one = ground_engine(cls, neighbor_mode=ndt.DIRECT7)
        one.set_target(tgt)
        one.set_source(s)
        singles.append(record(one.align(Gk)))
        one.close()
    eng = ground_engine(cls, neighbor_mode=ndt.DIRECT7)
    eng.batch_reserve(len(pairs), 8192, 2049)
    for b, (tgt, s, _) in enumerate(pairs):
        eng.batch_set_target(b, tgt)
        eng.batch_set_source(b, s)
    Gs = np.stack([g for _, _, g in pairs])
    rb = eng.batch_align(Gs)
    assert [record(r) for r in rb] == singles
    kids = [eng.keyframe_add(tgt) for tgt, _, _ in pairs]
    for b, kid in enumerate(kids):
        eng.batch_set_target_keyframe(b, kid)
    assert [record(r) for r in eng.batch_align(Gs)] == singles
    eng.close()
    assert len({r["iterations"] for r in rb}) > 1


def test_no_leak_between_classes():
    """7b: option 0 -> 1 -> 0 on one engine: the class-0 records are byte for byte those of an engine that never set it"""
    pairs = four_pairs()
    Gs = np.stack([g for _, _, g in pairs])

    def load(eng):
        eng.batch_reserve(len(pairs), 8192, 2049)
        for b, (tgt, s, _) in enumerate(pairs):
            eng.batch_set_target(b, tgt)
            eng.batch_set_source(b, s)

    fresh = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    load(fresh)
    want = [record(r) for r in fresh.batch_align(Gs)]
    fresh.close()
    eng = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    load(eng)
    assert [record(r) for r in eng.batch_align(Gs)] == want
    eng.set_option(ndt.OPT_GROUND_CLASS, 1)
    r1 = [record(r) for r in eng.batch_align(Gs)]
    eng.set_option(ndt.OPT_GROUND_CLASS, 0)
    assert [record(r) for r in eng.batch_align(Gs)] == want
    assert r1 != want
    eng.set_option(ndt.OPT_GROUND_CLASS, 1)
    assert [record(r) for r in eng.batch_align(Gs)] == r1
    eng.close()


def test_scores_are_unchanged():
    """calculateScore and the fitness score do not depend on the option"""
    tgt, s, Gk = four_pairs()[0]
    out = []
    for cls in (0, 1):
        eng = ground_engine(cls, neighbor_mode=ndt.DIRECT7)
        eng.set_target(tgt)
        eng.set_source(s)
        out.append((np.float64(eng.calculate_score(s)).tobytes(), np.float64(eng.fitness_score(T=Gk)[0]).tobytes()))
        eng.close()
    assert out[0] == out[1]


def test_refusals():
    """8: every entry of the refusal list returns its code with a message and leaves the next ground align's words unchanged"""
    tgt, s, Gk = four_pairs()[0]
    eng = ground_engine(1, neighbor_mode=ndt.DIRECT7)
    eng.set_target(tgt)
    eng.set_source(s)
    want = record(eng.align(Gk))
    p = np.array([1.0, 0, 0, 0.1, 0.2, 0.3])

    def refused(code, f, *a, **kw):
        with pytest.raises(ndt.NDTError) as e:
            f(*a, **kw)
        assert e.value.code == code, (e.value.code, code)
        assert "(" in str(e.value) and len(str(e.value).split("(", 1)[1]) > 10, str(e.value)       # a message from the engine
        assert eng.get_option(ndt.OPT_GROUND_CLASS) == 1
        assert record(eng.align(Gk)) == want

    def with_params(f, **kw):
        keep = eng.get_params()
        eng.set_params(ndt.default_params(**dict(dict(BASE, neighbor_mode=ndt.DIRECT7), **kw)))
        try:
            f()
        finally:
            eng.set_params(keep)
            eng.set_target(tgt)

    def with_option(f, opt, v):
        eng.set_option(opt, v)
        try:
            f()
        finally:
            eng.set_option(opt, 0)

    UNSUPPORTED, STATE, BAD_ARG = -6, -7, -2
    refused(UNSUPPORTED, with_params, lambda: eng.align(Gk), variant=ndt.VARIANT_PCA)
    refused(UNSUPPORTED, with_params, lambda: eng.align(Gk), step_size=0.004)                     # live More-Thuente: step_size <= eps / 2
    refused(UNSUPPORTED, with_params, lambda: eng.align(Gk), neighbor_mode=ndt.KDTREE)
    refused(UNSUPPORTED, with_params, lambda: eng.derivatives(p), neighbor_mode=ndt.KDTREE)
    refused(UNSUPPORTED, with_option, lambda: eng.align(Gk), ndt.OPT_POSE_MODEL, 1)
    refused(UNSUPPORTED, with_option, lambda: eng.align(Gk), ndt.OPT_NDT_CLASS, 1)
    refused(UNSUPPORTED, eng.compute_hessian, p)
    refused(UNSUPPORTED, eng.derivatives_T, np.eye(4, dtype=np.float32), np.eye(3, dtype=np.float32))
    frames = [s, s]
    refused(UNSUPPORTED, eng.sequence_run, frames, [0.0, 0.1])
    refused(UNSUPPORTED, eng.sequence_run_raw, frames, [0.0, 0.1])
    refused(UNSUPPORTED, eng.stream_begin, 2, 4, 8192, 2049)
    for bad in (4, -1, 99):
        with pytest.raises(ndt.NDTError) as e:
            eng.set_option(ndt.OPT_GROUND_CLASS, bad)
        assert e.value.code == BAD_ARG and eng.get_option(ndt.OPT_GROUND_CLASS) == 1
    assert record(eng.align(Gk)) == want
    # the tolerance arithmetic and latency mode are ignored: the same words, no warning status
    eng.set_option(ndt.OPT_ARITH, 1)
    assert record(eng.align(Gk)) == want and want[-1] == ndt.OK
    eng.set_option(ndt.OPT_ARITH, 0)
    eng.set_latency_mode(True)
    assert record(eng.align(Gk)) == want
    eng.close()
    # setting the option while a stream is open: a state error, the stream's class unchanged
    st = ndt.Engine(ndt.default_params(**BASE, neighbor_mode=ndt.DIRECT7))
    st.stream_begin(2, 4, 8192, 2049)
    with pytest.raises(ndt.NDTError) as e:
        st.set_option(ndt.OPT_GROUND_CLASS, 1)
    assert e.value.code == STATE and "stream" in str(e.value)
    assert st.get_option(ndt.OPT_GROUND_CLASS) == 0
    st.stream_end()
    st.close()
