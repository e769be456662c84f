"""GPU (-m gpu): one engine taken through every workspace growth path in both directions -- batch sizes, cloud sizes, voxel-record layout,
prefilter, fitness, sequence and stream sessions -- gives, step by step, the result words of a fresh engine that runs only that step.
A workspace the engine grew, shrank past or re-allocated must never change a result.  Also: a pose-record request that no submit consumed
ends with its stream session."""
import numpy as np
import pytest

from lv_slam_amd import ndt, synth

pytestmark = pytest.mark.gpu

PRM = dict(resolution=1.0, trans_epsilon=0.01, max_iterations=64, neighbor_mode=ndt.DIRECT7)


def same(a, b):
    """bit for bit, through dicts / lists / tuples of arrays and scalars"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    x, y = np.asarray(a), np.asarray(b)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def fresh(step, **kw):
    e = ndt.Engine(ndt.default_params(**{**PRM, **kw}))
    try:
        return step(e)
    finally:
        e.close()


def host_pairs(first, B, naz, src_frac=1.0):
    """B pairs of naz * 64 target points; sources cut to src_frac of theirs"""
    import torch
    out = []
    for b in range(0, B, 16):
        t, s, _ = synth.make_pairs(list(range(first + b, first + min(b + 16, B))), naz, device="cuda")
        t, s = t.cpu().numpy(), s.cpu().numpy()
        out += [(t[j], s[j][: max(1, int(len(s[j]) * src_frac))].copy()) for j in range(len(t))]
    torch.cuda.synchronize()
    return out


def guesses(B):
    G = np.stack([synth.default_guess() for _ in range(B)]).astype(np.float32)
    G[::3, 0, 3] += 0.3
    return G


def batch_step(pairs):
    def run(e):
        e.batch_reserve(len(pairs), max(len(t) for t, _ in pairs), max(len(s) for _, s in pairs))
        for k, (t, s) in enumerate(pairs):
            e.batch_set_target(k, t)
            e.batch_set_source(k, s)
        return e.batch_align(guesses(len(pairs)))
    return run


def device_batches(first, sizes, naz):
    """(T, S, counts, guesses) per batch, SoA rows [B, 3, n] on the device"""
    import torch
    n = naz * 64
    out, pid = [], first
    for bi, B in enumerate(sizes):
        t, s, _ = synth.make_pairs(list(range(pid, pid + B)), naz, device="cuda")
        pid += B
        T = t.transpose(1, 2).contiguous()
        S = s.transpose(1, 2).contiguous()
        cnt = [n - 517 * ((k + bi) % 4) for k in range(B)]
        out.append((T, S, cnt, guesses(B)))
    torch.cuda.synchronize()
    return out, n


def colmajor(G):
    return np.ascontiguousarray(np.transpose(G, (0, 2, 1))).reshape(len(G), 16)


def stream_step(batches, n, nctx):
    def run(e):
        e.stream_begin(nctx, max(len(b[2]) for b in batches), n, n)
        ids = [e.stream_submit(T.data_ptr(), [n] * len(cnt), n, S.data_ptr(), cnt, n, colmajor(G)) for T, S, cnt, G in batches[:nctx]]
        got = [e.stream_collect(i, len(batches[k][2])) for k, i in enumerate(ids)]
        for k in range(nctx, len(batches)):
            T, S, cnt, G = batches[k]
            got.append(e.stream_collect(e.stream_submit(T.data_ptr(), [n] * len(cnt), n, S.data_ptr(), cnt, n, colmajor(G)), len(cnt)))
        e.stream_end()
        return got
    return run


def test_one_engine_through_every_growth_path_equals_fresh_engines():
    eng = ndt.Engine(ndt.default_params(**PRM))
    checks = []

    def check(name, step, **kw):
        got = step(eng)
        want = fresh(step, **kw)
        assert same(got, want), name
        checks.append(name)

    # batches: pairs, target and source sizes grow, then shrink
    check("batch 8", batch_step(host_pairs(0, 8, 64, 0.5)))
    check("batch 64", batch_step(host_pairs(100, 64, 256, 1.0)))
    small = host_pairs(200, 8, 128, 0.25)
    check("batch 8 again", batch_step(small))

    # resolution and minimum points per voxel change together: another record count per target (re-allocated at exactly that size)
    def regrid(e):
        p = e.get_params()
        p.resolution, p.min_points_per_voxel = 0.75, 4
        e.set_params(p)
        res = batch_step(small)(e)
        p.resolution, p.min_points_per_voxel = PRM["resolution"], 6
        e.set_params(p)
        return res
    check("records per target", regrid)

    # one fitness score, then batched scores over larger targets
    t1, s1 = host_pairs(300, 1, 64)[0]
    T = synth.default_guess()

    def single_fitness(e):
        e.set_target(t1)
        e.set_source(s1)
        return [e.fitness_score(mr, T) for mr in (1.0, float("inf"))]
    check("single fitness", single_fitness)
    big = host_pairs(310, 6, 256)

    def batch_fitness(e):
        e.batch_reserve(len(big), max(len(t) for t, _ in big), max(len(s) for _, s in big))
        for k, (t, s) in enumerate(big):
            e.batch_set_target(k, t)
            e.batch_set_source(k, s)
        return [e.batch_fitness_scores(mr, T) for mr in (1.0, float("inf"))]
    check("batched fitness", batch_fitness)

    # prefilter: small, large, small
    clouds = [host_pairs(400 + k, 1, naz)[0][0] for k, naz in enumerate((32, 1024, 48))]
    for k, c in enumerate(clouds):
        check(f"prefilter {k}", lambda e, c=c: e.prefilter(c, 0.5, 100.0, 0.2))

    # sequences of 5, then 12 frames
    for nf in (5, 12):
        scans, _ = synth.make_sequence(nf, 256, n_beams=32)
        stamps = [0.1 * k for k in range(nf)]
        check(f"sequence {nf}", lambda e, scans=scans, stamps=stamps: e.sequence_run(scans, stamps, keyframe_delta_trans=2.5)[0])

    # two stream sessions: other context counts, batch and cloud sizes
    b1, n1 = device_batches(500, [12, 9, 12, 7], 96)
    check("stream 3 contexts", stream_step(b1, n1, 3))
    b2, n2 = device_batches(600, [20, 20, 13], 160)
    check("stream 2 contexts", stream_step(b2, n2, 2))

    eng.close()
    assert len(checks) == 13


def test_pose_record_request_ends_with_its_stream_session():
    """mi355ndt_stream_pose_records applies to the next submit OF THE SESSION: a request that no submit consumed must not reach a batch of the
    next session, whose pose records would otherwise land in the old (possibly freed) block."""
    import torch
    from lv_slam_amd import dist as shard
    batches, n = device_batches(700, [10], 64)
    T, S, cnt, G = batches[0]
    old = torch.zeros((16, shard.REC_WORDS), device="cuda:0", dtype=torch.int32)
    eng = ndt.Engine(ndt.default_params(**PRM))
    eng.stream_begin(3, 10, n, n)
    eng.stream_pose_records(old.data_ptr(), 16, 0, 1)
    eng.stream_end()
    eng.stream_begin(3, 10, n, n)
    res = eng.stream_collect(eng.stream_submit(T.data_ptr(), [n] * len(cnt), n, S.data_ptr(), cnt, n, colmajor(G)), len(cnt))
    eng.stream_end()
    eng.synchronize()
    torch.cuda.synchronize()
    assert not old.any().item()
    assert same([res], fresh(stream_step(batches, n, 3)))
    eng.close()
