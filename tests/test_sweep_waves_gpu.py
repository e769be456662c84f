"""GPU (-m gpu): MI355NDT_OPT_SWEEP_WAVES.  The exact ndt_omp / DIRECT7 item body of the one-launch align exists twice -- at two waves per SIMD
(mid-evaluation record prefetch, two tiles probed together) and, lean, at three (no prefetch, one tile probed at a time; ndt_sweep.hpp:
SweepTune) -- and the host picks one per launch (ndt_sweep_waves.hpp).  No word a caller can read may depend on the choice:
  * every result word of the synchronous batch align and of a three-batch stream, and every partial row the aligns leave on the device
    (mi355ndt_get_partial_rows), with the option at 2 and at 3 -- batches of 1, 3 and 9 pairs, sources of 2,048, 2,049 and 5,000 points (64 and
    512 do not divide the latter two), one source that is mostly far from its target (fewer than 64 hits per work item, all of them from the
    item's first super-tile: the queue's partial drains of the older staging half occur, which the hit counts show), one empty target, both
    f32 sum orders, the score-only last sweep on and off;
  * the automatic choice: three waves at 1 m / 4,096 points, two above the threshold, and never for ndt_pca, DIRECT1, KDTREE, the Euler model
    or the tolerance arithmetic (mi355ndt_profile: async_waves_per_simd, async_launch_slots)."""
import numpy as np
import pytest

from lv_slam_amd import ndt, synth
from test_stream_gpu import colmajor, same

pytestmark = pytest.mark.gpu

NAZ = 80                       # 5,120-point clouds
COUNTS = (2048, 2049, 5000)    # source points, in turn
NEAR = 8                       # points of every 512-point work item the far source keeps near its target


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def roles(B):
    """(pair with the far source, pair with the empty target) of a batch of B pairs; None: the batch has none"""
    return (None, None) if B < 3 else (B // 3, B - 1)


def make_batch(first_id, B):
    """B resident pairs: (T, S, target counts, source counts, guesses[B, 4, 4], n)"""
    import torch
    dev = torch.device("cuda:0")
    n = NAZ * 64
    T = torch.zeros(B, 3, n, device=dev)
    S = torch.zeros(B, 3, n, device=dev)
    far, empty = roles(B)
    tcnt, scnt = [n] * B, [COUNTS[(k + 1) % 3] for k in range(B)]
    for k in range(B):
        t, s, _ = synth.make_pair(first_id + k, NAZ, device=dev)
        T[k] = t.T
        S[k] = s.T
    if far is not None:
        scnt[far] = 5000
        idx = torch.arange(n, device=dev)
        S[far, 0, idx % 512 >= NEAR] += 500.0        # all but the first NEAR points of every work item: half a kilometre off the grid
        tcnt[empty] = 0
    G = np.stack([synth.default_guess() for _ in range(B)]).astype(np.float32)
    G[::2, 0, 3] += 0.3                              # uneven iteration counts
    torch.cuda.synchronize()
    return T, S, tcnt, scnt, G, n


def align(batch, waves, order, score_only):
    T, S, tcnt, scnt, G, n = batch
    eng = ndt.Engine(ndt.default_params(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7, variant=0))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, 2)           # the one-launch align whatever the batch size
    eng.set_option(ndt.OPT_F32_SUM_ORDER, order)
    eng.set_option(ndt.OPT_SCORE_ONLY_LAST_SWEEP, score_only)
    eng.set_option(ndt.OPT_SWEEP_WAVES, waves)
    assert eng.get_option(ndt.OPT_SWEEP_WAVES) == waves
    eng.batch_bind_device(T.data_ptr(), tcnt, n, S.data_ptr(), scnt, n)
    eng.batch_build_targets()
    eng.profile_enable(True)
    eng.profile_reset()
    res = eng.batch_align(G)
    pr = eng.profile_get()
    rows = eng.partial_rows()
    incs = [eng.get_incremental(k) for k in range(len(scnt))]
    eng.close()
    return res, rows, incs, pr


@pytest.mark.parametrize("score_only", [0, 1])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 9])
def test_two_and_three_waves_leave_the_same_words(B, order, score_only):
    batch = make_batch(7000 + 16 * B, B)
    r2, rows2, inc2, p2 = align(batch, 2, order, score_only)
    r3, rows3, inc3, p3 = align(batch, 3, order, score_only)
    # both through the one-launch align, each with the body it was told to take
    assert p2["update_launches"] == 0 and p3["update_launches"] == 0 and p2["async_fallbacks"] == 0 and p3["async_fallbacks"] == 0
    assert (p2["async_waves_per_simd"], p3["async_waves_per_simd"]) == (2, 3)
    assert (p2["async_launch_slots"], p3["async_launch_slots"]) == (2 * n_cu(), 3 * n_cu())
    for k, (x, y) in enumerate(zip(r2, r3)):
        assert same(x, y), (k, x, y)
    for (l0, q0), (l1, q1) in zip(inc2, inc3):
        assert np.array_equal(l0, l1) and np.array_equal(q0, q1)
    assert p2["sweep_hits"] == p3["sweep_hits"] and p2["score_only_sweeps"] == p3["score_only_sweeps"]
    assert score_only or p2["score_only_sweeps"] == 0
    # the rows: four per 2,048-point chunk of the batch's longest source, 44 words each.  A score-only last sweep defines a row's score and
    # hit count alone (the other words are whatever the sweep before it left, or the allocation held)
    assert rows2.shape == rows3.shape == (B, 4 * -(-max(batch[3]) // 2048), 44)
    w = [0, 43] if score_only else list(range(44))
    assert np.array_equal(rows2[:, :, w].view(np.uint64), rows3[:, :, w].view(np.uint64))
    far, empty = roles(B)
    if far is not None:
        # the far source: every item has hits, fewer than 64, all from its first 128 points, and more than 256 points -- so they sit in the
        # queue over a whole super-tile and leave it through the partial drain of the older staging half, in both bodies
        hits = rows3[far, :10, 43]
        assert r3[far]["hits_last"] > 0 and hits.max() < 64 and (hits > 0).any(), hits
        assert np.all(rows3[far, 10:, 43] == 0)
        assert r3[empty]["hits_last"] == 0 and np.all(rows3[empty, :, 43] == 0)
    assert all(r["hits_last"] > 64 for k, r in enumerate(r3) if k not in (far, empty))     # the others: full batches


@pytest.mark.parametrize("order,score_only", [(0, 1), (1, 0), (1, 1), (0, 0)])
def test_stream_of_three_batches_is_the_same_with_two_and_three_waves(order, score_only):
    kw = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7, variant=0)
    made = [make_batch(7100 + 16 * k, B) for k, B in enumerate((9, 3, 1))]
    n = made[0][5]
    got = {}
    for waves in (2, 3):
        eng = ndt.Engine(ndt.default_params(**kw))
        for o, v in ((ndt.OPT_STREAM_THRESHOLD, 2), (ndt.OPT_F32_SUM_ORDER, order), (ndt.OPT_SCORE_ONLY_LAST_SWEEP, score_only), (ndt.OPT_SWEEP_WAVES, waves)):
            eng.set_option(o, v)
        eng.profile_enable(True)
        eng.stream_begin(3, 9, n, n)
        ids = [eng.stream_submit(T.data_ptr(), tcnt, n, S.data_ptr(), scnt, n, colmajor(G)) for T, S, tcnt, scnt, G, _ in made]
        res = [eng.stream_collect(i, len(m[3])) for i, m in zip(ids, made)]
        pr = eng.profile_get()
        eng.stream_end()
        eng.close()
        assert pr["async_waves_per_simd"] == waves and pr["stream_launch_slots"] + pr["stream_reserved_slots"] == waves * n_cu()
        assert pr["async_fallbacks"] == 0
        got[waves] = res
    for bi, (a, b) in enumerate(zip(got[2], got[3])):
        for k, (x, y) in enumerate(zip(a, b)):
            assert same(x, y), (bi, k, x, y)
    # ... and both equal the synchronous batch align (whose rows the test above compares)
    for bi, m in enumerate(made):
        ref = align(m, 2, order, score_only)[0]
        for k, (x, y) in enumerate(zip(ref, got[3][bi])):
            assert same(x, y), (bi, k, x, y)


def waves_taken(kw, naz, opts=(), pairs=2):
    """(waves per SIMD, workgroups) of the persistent launch that aligned `pairs` small pairs; (0, 0): no such launch was made"""
    import torch
    dev = torch.device("cuda:0")
    n = naz * 64
    T = torch.zeros(pairs, 3, n, device=dev)
    S = torch.zeros(pairs, 3, n, device=dev)
    for k in range(pairs):
        t, s, _ = synth.make_pair(7200 + k, naz, device=dev)
        T[k] = t.T
        S[k] = s.T
    torch.cuda.synchronize()
    eng = ndt.Engine(ndt.default_params(trans_epsilon=0.01, max_iterations=8, **kw))
    eng.set_option(ndt.OPT_ASYNC_ALIGN, 2)
    for o, v in opts:
        eng.set_option(o, v)
    eng.batch_bind_device(T.data_ptr(), [n] * pairs, n, S.data_ptr(), [n] * pairs, n)
    eng.batch_build_targets()
    eng.batch_align(np.stack([synth.default_guess()] * pairs).astype(np.float32))
    pr = eng.profile_get()
    eng.close()
    return pr["async_waves_per_simd"], pr["async_launch_slots"]


def test_the_automatic_choice():
    cu = n_cu()
    omp7 = dict(neighbor_mode=ndt.DIRECT7, variant=0)
    eng = ndt.Engine(ndt.default_params(**omp7))
    assert eng.get_option(ndt.OPT_SWEEP_WAVES) == 0                                                   # automatic is the default
    eng.close()
    # 1 m, 4,096 points: 128 leaves = 8 KB of records by the estimate, far below the 341 KB threshold
    assert waves_taken(dict(resolution=1.0, **omp7), 64) == (3, 3 * cu)
    # 0.5 m, 65,536 points: 8,192 leaves = 512 KB, above it
    assert waves_taken(dict(resolution=0.5, **omp7), 1024) == (2, 2 * cu)
    # ... and what the option says where the estimate would say otherwise
    assert waves_taken(dict(resolution=1.0, **omp7), 64, opts=((ndt.OPT_SWEEP_WAVES, 2),)) == (2, 2 * cu)
    assert waves_taken(dict(resolution=0.5, **omp7), 1024, opts=((ndt.OPT_SWEEP_WAVES, 3),)) == (3, 3 * cu)
    # never: ndt_pca, DIRECT1, KDTREE, the tolerance arithmetic (four waves of its own), the Euler model (the lockstep rounds: no persistent launch)
    for opt in (0, 3):
        o = ((ndt.OPT_SWEEP_WAVES, opt),)
        assert waves_taken(dict(resolution=1.0, neighbor_mode=ndt.DIRECT7, variant=1), 64, opts=o) == (2, 2 * cu)
        assert waves_taken(dict(resolution=1.0, neighbor_mode=ndt.DIRECT1, variant=0), 64, opts=o) == (2, 2 * cu)
        assert waves_taken(dict(resolution=1.0, neighbor_mode=ndt.KDTREE, variant=0), 64, opts=o) == (2, 2 * cu)
        assert waves_taken(dict(resolution=1.0, **omp7), 64, opts=o + ((ndt.OPT_ARITH, 1),)) == (4, 4 * cu)
        assert waves_taken(dict(resolution=1.0, **omp7), 64, opts=o + ((ndt.OPT_POSE_MODEL, 1),)) == (0, 0)


def test_option_values_and_the_stream():
    eng = ndt.Engine(ndt.default_params(neighbor_mode=ndt.DIRECT7))
    for bad in (-1, 1, 4):
        with pytest.raises(ndt.NDTError) as e:
            eng.set_option(ndt.OPT_SWEEP_WAVES, bad)
        assert e.value.code == -2                    # MI355NDT_ERR_BAD_ARG
    eng.set_option(ndt.OPT_SWEEP_WAVES, 3)
    eng.stream_begin(3, 8, 4096, 4096)
    with pytest.raises(ndt.NDTError) as e:
        eng.set_option(ndt.OPT_SWEEP_WAVES, 2)
    assert e.value.code == -7                        # MI355NDT_ERR_STATE
    assert eng.get_option(ndt.OPT_SWEEP_WAVES) == 3
    eng.stream_end()
    eng.set_option(ndt.OPT_SWEEP_WAVES, 0)
    assert eng.get_option(ndt.OPT_SWEEP_WAVES) == 0
    eng.close()
