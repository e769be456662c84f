"""The fixed-order reduction of a pair's partial rows (lv_slam_amd/csrc/ndt_update.hpp: chunk_sum, group_sum, wave_sums_total, walk_groups,
store_sums), alone, on the device: the three forms the align routes use -- the block form over four rows per chunk (k_update), the block form
over chunk rows (k_seq_update), the one-wave form with agent-scope loads (the one-launch align's updater) -- against the tree written out
below with plain float64 adds: chunk = ((r0 + r1) + r2) + r3; group = 8 chunks in order; group k goes to wave k % 4, which adds its groups in
ascending order; the four wave sums add in order.  Byte for byte, at chunk counts around every edge of the walkers: a group's edge (7, 8, 9),
the one-wave walker's two-group batch and its remainder (15, 16, 17, 24, 25), a full round of the four waves (31, 32, 33, 40), the chunk-row
walker's four-groups-per-wave batch (127, 128, 129), and 0 / 1.

What the inputs can tell apart (the unmarked test): with up to four groups -- 32 chunks -- every wave owns at most one group, so "by wave" and
"groups in ascending order" are the same expression, and with nine chunks the second group is one chunk, which makes the whole tree the plain
sequential sum.  So: from 33 chunks on, adding the groups in ascending order instead of by wave changes bytes; from 10 to 32 chunks, where
that alternative does not exist, adding the chunks in one sequence instead of by group does."""
import os
import subprocess
import functools
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32, 33, 40, 63, 64, 65, 127, 128, 129)
NACC = 44


def tree(rows, by_wave=True, by_group=True):
    """rows: (chunks, 4, 44) float64 -> the 44 column sums, every add a separately rounded float64 add in the order of the device's tree."""
    zero = np.zeros(NACC, np.float64)
    chunks = [((r[0] + r[1]) + r[2]) + r[3] for r in rows]
    if not by_group:
        total = zero
        for c in chunks:
            total = total + c
        return total
    groups = []
    for g0 in range(0, len(chunks), 8):
        gs = zero
        for c in chunks[g0:g0 + 8]:
            gs = gs + c
        groups.append(gs)
    if not by_wave:
        total = zero
        for gs in groups:
            total = total + gs
        return total
    waves = [zero, zero, zero, zero]
    for k, gs in enumerate(groups):
        waves[k % 4] = waves[k % 4] + gs
    total = zero
    for w in waves:
        total = total + w
    return total


@functools.lru_cache(maxsize=None)
def cases():
    """Per chunk count: rows of both signs with magnitudes spread over 1e-8 .. 1e8 (a sum's low bits then depend on the order of every add)."""
    rng = np.random.default_rng(20251019)
    out = []
    for n in COUNTS:
        rows = rng.choice([-1.0, 1.0], size=(n, 4, NACC)) * 10.0 ** rng.uniform(-8.0, 8.0, size=(n, 4, NACC))
        rows.setflags(write=False)
        out.append(rows)
    return tuple(out)


def as_words(v):
    """the sums as a PairState holds them: 43 doubles and the hit count as the (long long) it is stored as"""
    w = np.ascontiguousarray(v, np.float64).copy().view(np.uint64)
    w[NACC - 1] = v[NACC - 1:].astype(np.int64).view(np.uint64)[0]                                      # (truncates toward zero, as the cast does)
    return w


def test_inputs_tell_the_orders_apart():
    for n, rows in zip(COUNTS, cases()):
        want = tree(rows)
        if n <= 32:
            assert np.array_equal(want.view(np.uint64), tree(rows, by_wave=False).view(np.uint64)), n      # one group per wave: the same expression
        else:
            assert np.any(want.view(np.uint64) != tree(rows, by_wave=False).view(np.uint64)), n
        if n <= 9:
            assert np.array_equal(want.view(np.uint64), tree(rows, by_group=False).view(np.uint64)), n     # the plain sequential sum
        else:
            assert np.any(want.view(np.uint64) != tree(rows, by_group=False).view(np.uint64)), n


@pytest.mark.gpu
def test_every_form_of_the_row_tree_equals_the_numpy_tree(tmp_path):
    import __graft_entry__ as entry
    exe = entry.build_row_tree_check()
    rows = cases()
    chunk_rows = [((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3] for r in rows]                                 # what latency mode's sweep stores
    blob = np.concatenate([np.array([len(COUNTS)], np.float64), np.array(COUNTS, np.float64)] + [r.ravel() for r in rows] + [c.ravel() for c in chunk_rows])
    blob.tofile(tmp_path / "in.f64")
    subprocess.check_call([exe, str(tmp_path / "in.f64"), str(tmp_path / "out.u64")], timeout=120)
    out = np.fromfile(tmp_path / "out.u64", np.uint64).reshape(len(COUNTS), 3, NACC)
    bad = []
    for n, r, o in zip(COUNTS, rows, out):
        want = as_words(tree(r))
        for form, name in enumerate(("block form, four rows per chunk", "block form, chunk rows", "one-wave form")):
            cols = np.nonzero(o[form] != want)[0]
            if len(cols):
                bad.append((n, name, cols.tolist()))
    assert not bad, bad
