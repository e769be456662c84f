"""The two device building blocks under every voxel surface, alone, word for word against numpy: the stable segmented radix sort
(lv_slam_amd/csrc/ndt_segsort.hpp: k_rs_hist, k_rs_scan, k_rs_scatter behind rs_plan, rs_pass, rs_sort_one_segment) and the exclusive scans
that turn head flags into emit positions (ndt_prefilter.hpp: k_pf_scan_totals / _offsets / _apply; ndt_prefilter_batch.hpp:
k_pfb_scan_*, k_pfb_heads).  tests/hip/segsort_check.hip launches the library's own kernels through the library's own host entry points; the
references below are numpy's stable argsort, bincount and cumsum.  Everything is integer work: every comparison is exact.

What the cases are for.  Digit plans: field widths 8 .. 32 give every instantiated digit width (8, 10, 11) at one, two and three passes, and
32 the short last digit with key bit 31 in use.  Geometry: a tile is 4096 positions in four wave shares of 1024, walked in rounds of 64; the
pitches are one round, one share and one round more, one tile and one round either side, and 7 / 8 / 10 / 18 tiles for k_rs_scan's
unrolled-by-eight tile loop with and without remainder; 37 and 4097 end inside a round (the `i < pitch` guards); 7 / 8 / 9 / 17 segments are
xcd_map's edges.  Key patterns: ties (stability), bits above the field (ignored), runs of equal keys that straddle rounds, shares and tiles
(k_rs_hist counts whole runs at their heads), runs that share the first digit and differ in a later one.

Without `first` and without points, one segment goes through rs_sort_one_segment; with `first` it goes through the rs_pass loop, because
rs_sort_one_segment takes position ids only together with points (the points cases cover that route)."""
import os
import subprocess

import numpy as np
import pytest

MAGIC = 0x31435353
GUARD = 64
FILL = 0xA5A5A5A5
TILE = 4096
INT_MAX = 2**31 - 1
PLANS = (8, 10, 11, 16, 20, 22, 24, 30, 31, 32)
PATTERNS = ("uniform", "rand32", "zeros", "ones", "alternating", "descending", "asc_tail", "runs", "runs_shared")
TIE_PATTERNS = ("rand32", "runs", "runs_shared")            # what test_inputs_tell_a_wrong_sort_from_a_right_one puts its conditions on
RUN_LENGTHS = (1, 2, 3, 63, 64, 65, 200, 1023, 1025, 4095, 4097)
ONE_SEGMENT = (64, 1024, 1088, 4032, 4096, 4160, 8256, 28672, 32768, 36928, 69696, 37, 4097)
GEOMETRY = tuple((1, p) for p in ONE_SEGMENT) + tuple((k, p) for p in (4160, 64) for k in (7, 8, 9, 17))
EDGES = (64, 1024, 4096)                                    # the first round, wave-share and tile boundary of a segment


def plan_of(field_bits):
    """(bits, passes): as few passes as 11-bit digits allow, then the narrowest instantiated width that covers the field in that many"""
    passes = max(1, -(-field_bits // 11))
    return next(b for b in (8, 10, 11) if passes * b >= field_bits), passes


def sort_mask(field_bits):
    bits, passes = plan_of(field_bits)
    return (1 << min(32, passes * bits)) - 1


def tiles_of(pitch):
    return -(-pitch // TILE)


# ------------------------------------------------------------------------------------------------------------------------------ the inputs
def run_keys(rng, n, field_bits, shared):
    lengths = np.zeros(0, np.int64)
    while lengths.sum() < n:
        lengths = np.concatenate([lengths, rng.choice(RUN_LENGTHS, size=64)])
    bits, passes = plan_of(field_bits)
    if not shared:
        heads = rng.integers(0, 1 << field_bits, size=len(lengths), dtype=np.uint64)
    else:
        # three consecutive runs share the first digit; a run differs from the one before it only above that digit (inside the field when the
        # plan has a later pass to split them again, else in the bits no pass looks at)
        hi_bits = min(32, field_bits) - bits if passes > 1 else 32 - bits
        low = np.repeat(rng.integers(0, 1 << bits, size=len(lengths) // 3 + 1, dtype=np.uint64), 3)[:len(lengths)]
        step = rng.integers(1, 1 << hi_bits, size=len(lengths), dtype=np.uint64)
        heads = low | ((np.cumsum(step) % np.uint64(1 << hi_bits)) << np.uint64(bits))
    return np.repeat(heads, lengths)[:n].astype(np.uint32)


def segment_keys(rng, pattern, n, field_bits):
    ones = (1 << field_bits) - 1
    if pattern == "uniform":
        k = rng.integers(0, 1 << field_bits, size=n, dtype=np.uint64)
    elif pattern == "rand32":
        k = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    elif pattern == "zeros":
        k = np.zeros(n, np.uint64)
    elif pattern == "ones":                                   # the "not binned" key of a cb-bit field
        k = np.full(n, ones, np.uint64)
    elif pattern == "alternating":
        a = int(rng.integers(0, 1 << field_bits))
        k = np.where(np.arange(n) % 2 == 0, a, a ^ (1 + int(rng.integers(0, ones))) & ones).astype(np.uint64)
    elif pattern == "descending":                             # strictly, as 32-bit words
        k = np.uint64(rng.integers(n, 1 << 32)) - np.arange(n, dtype=np.uint64)
    elif pattern == "asc_tail":                               # as a padded cloud gives
        body = n - n // 5 - 1
        k = np.full(n, ones, np.uint64)
        k[:body] = (np.arange(body, dtype=np.uint64) * np.uint64(ones)) // np.uint64(body)
    elif pattern == "permutation":                            # all keys distinct in one digit
        assert n <= 1 << field_bits <= 1 << 11
        k = rng.permutation(n).astype(np.uint64)
    else:
        k = run_keys(rng, n, field_bits, pattern == "runs_shared").astype(np.uint64)
    k = k.astype(np.uint32)
    if pattern in TIE_PATTERNS:                               # an equal sorted field on either side of the first boundary of every kind
        m = np.uint32(sort_mask(field_bits))
        for e in EDGES:
            if e < n:
                k[e] = (k[e] & ~m) | (k[e - 1] & m)
    return k


def segment_vals(rng, n):
    pool = rng.integers(0, 1 << 32, size=max(2, n // 2), dtype=np.uint64).astype(np.uint32)      # random words, with duplicates
    v = pool[rng.integers(0, len(pool), size=n)]
    for e in EDGES:
        if e < n and v[e] == v[e - 1]:
            v[e] ^= np.uint32(1)
    return v


def sort_case(K, pitch, field_bits, pattern):
    rng = np.random.default_rng([20261019, K, pitch, field_bits, (PATTERNS + ("permutation",)).index(pattern)])
    keys = np.stack([segment_keys(rng, pattern, pitch, field_bits) for _ in range(K)])             # every segment its own keys
    vals = np.stack([segment_vals(rng, pitch) for _ in range(K)])
    return dict(K=K, pitch=pitch, field_bits=field_bits, pattern=pattern, keys=keys, vals=vals)


SORT_GROUPS = {
    "every plan x every pattern, 9 segments of 4160": [(9, 4160, f, p) for f in PLANS for p in PATTERNS],
    "every plan x every pattern, 1 segment of 36928": [(1, 36928, f, p) for f in PLANS for p in PATTERNS],
    "every geometry": [(k, n, f, p) for (k, n) in GEOMETRY for f in (8, 20, 31, 32) for p in ("uniform", "runs")] +
                      [(1, 64, 8, "permutation"), (1, 1088, 11, "permutation"), (9, 1088, 11, "permutation")],
}


def name_of(spec):
    K, pitch, f, pattern = spec
    bits, passes = plan_of(f)
    return f"field {f} ({passes} x {bits} bits), pitch {pitch}, K {K}, {pattern}"


# -------------------------------------------------------------------------------------------------------------------------- the references
def stable_order(keys, field_bits, ties_descending=False):
    """per segment: the order an LSD sort over the plan's digits promises -- by the masked key, ties in input order"""
    masked = keys & np.uint32(sort_mask(field_bits))
    if not ties_descending:
        return np.argsort(masked, axis=1, kind="stable")
    n = keys.shape[1]
    return n - 1 - np.argsort(masked[:, ::-1], axis=1, kind="stable")          # (the wrong sort the inputs must tell apart)


def first_pass_hist(keys, field_bits):
    """hist[b][tile][d] and the digit-major, tile-minor exclusive scan of it per segment"""
    K, pitch = keys.shape
    nb = 1 << plan_of(field_bits)[0]
    tiles = tiles_of(pitch)
    slot = (np.arange(pitch) // TILE) * nb
    hist = np.stack([np.bincount(slot + (keys[b] & np.uint32(nb - 1)), minlength=tiles * nb).reshape(tiles, nb) for b in range(K)])
    flat = hist.transpose(0, 2, 1).reshape(K, -1)
    offs = (np.cumsum(flat, axis=1) - flat).reshape(K, nb, tiles).transpose(0, 2, 1)
    return hist.astype(np.uint32), offs.astype(np.uint32)


def cell_keys(pts, n, grids, cb):
    """rs_cell with separately rounded float32 steps and int32 wrap-around; grids: (min_b[3], mul1, mul2, inv_leaf, status) per segment"""
    K, _, pitch = pts.shape
    out = np.empty((K, pitch), np.uint32)
    for b, (min_b, mul1, mul2, inv_leaf, status) in enumerate(grids):
        x = pts[b]
        fin = np.isfinite(x).all(axis=0)
        xs = np.where(fin, x, np.float32(0))
        t = np.floor(xs * np.float32(inv_leaf)) - np.array(min_b, np.float32)[:, None]
        assert t.dtype == np.float32
        i = t.astype(np.int32).astype(np.int64)
        cell = (i[0] + i[1] * mul1 + i[2] * mul2) & 0xFFFFFFFF
        ok = fin & (np.arange(pitch) < n[b]) & (status == 0)
        out[b] = np.where(ok, cell, (1 << cb) - 1).astype(np.uint32)
    return out


def exscan(v):
    v = np.asarray(v, np.int64)
    return (np.cumsum(v) - v).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------------------ the helper
class Results:
    """the helper's output file: buffer after buffer as [n] [64 guard words] [n words] [64 guard words]"""

    def __init__(self, path):
        self.w = np.fromfile(path, np.uint32)
        self.at = 0

    def buf(self):
        n = int(self.w[self.at])
        lo, body, hi = np.split(self.w[self.at + 1:self.at + 1 + n + 2 * GUARD], [GUARD, GUARD + n])
        assert len(hi) == GUARD, "short result file"
        self.at += 1 + n + 2 * GUARD
        return body, bool((lo == FILL).all() and (hi == FILL).all())

    def done(self):
        return self.at == len(self.w)


def run_helper(tmp_path, mode, cases):
    import __graft_entry__ as entry
    exe = entry.build_segsort_check()
    blob = np.concatenate([np.array([MAGIC, mode, len(cases)], np.uint32)] + [np.ascontiguousarray(p).view(np.uint32).ravel() for c in cases for p in c])
    blob.tofile(tmp_path / "in.u32")
    run = subprocess.run([exe, "run", str(tmp_path / "in.u32"), str(tmp_path / "out.u32")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    return Results(tmp_path / "out.u32")


def u32(*v):
    return np.array(v, np.int64).astype(np.uint32)


def w32(a):
    return np.asarray(a, np.int64).astype(np.uint32).ravel()


def differs(got, want):
    """None, or where the first differing word is"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    if len(got) != len(want):
        return f"{len(got)} words for {len(want)}"
    at = np.nonzero(got != want)[0]
    return None if not len(at) else f"first at {int(at[0])}: {int(got[at[0]]):#x} for {int(want[at[0]]):#x}, {len(at)} words differ"


def report(bad):
    """the mismatches ("case: array: where") counted by case and array, the first dozen in full, then every case by name"""
    cases = list(dict.fromkeys(b.split(": ")[0] for b in bad))
    arrays = sorted({b.split(": ")[1] for b in bad})
    return f"{len(bad)} mismatches in {len(cases)} cases ({', '.join(arrays)}): " + " | ".join(bad[:12]) + " || every case: " + "; ".join(cases)


def read_sort(res, words, bad, name):
    """the six buffers a sort leaves: the pair that holds the result is written whole"""
    bufs = [res.buf() for _ in range(6)]
    if not all(ok for _, ok in bufs):
        bad.append(f"{name}: guard words of {[j for j, (_, ok) in enumerate(bufs) if not ok]} (kA vA kB vB hist offs) written")
    full = [j for j in (0, 2) if len(bufs[j][0]) == words]
    assert len(full) == 1 and len(bufs[full[0] + 1][0]) == words, name
    return bufs[full[0]][0], bufs[full[0] + 1][0]


# ------------------------------------------------------------------------------------------------------------------------- tests without GPU
def test_plan_properties():
    import __graft_entry__ as entry
    exe = entry.build_segsort_check() if os.path.exists(entry.HIPCC) else os.path.join(entry.ROOT, "tests", "hip", "segsort_check")    # (else: prebuilt)
    if not os.path.exists(exe):
        pytest.skip("no hipcc and no prebuilt tests/hip/segsort_check")
    out = subprocess.run([exe, "plan"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    table = [tuple(int(t) for t in line.split()) for line in out.stdout.splitlines()]
    assert [t[0] for t in table] == list(range(34))
    for f, bits, passes in table[1:]:
        assert bits in (8, 10, 11), (f, bits)
        assert passes * bits >= f, (f, bits, passes)
        assert passes == -(-f // 11), (f, passes)
        assert all(passes * b < f for b in (8, 10, 11) if b < bits), (f, bits, passes)              # the narrowest that still covers f
        assert (bits, passes) == plan_of(f)                                                        # (what the references below sort by)
    for f, want in zip(PLANS, ((8, 1), (10, 1), (11, 1), (8, 2), (10, 2), (11, 2), (8, 3), (10, 3), (11, 3), (11, 3))):
        assert table[f][1:] == want


def test_inputs_tell_a_wrong_sort_from_a_right_one():
    """Every runs case and every random-words case: equal sorted fields with different values sit in two rounds of one wave (positions 63 and
    64), in two waves of one tile (1023, 1024) and in two tiles (4095, 4096), wherever the pitch reaches that far, and a sort that breaks
    ties by descending position gives other output words, with position ids and with the carried values."""
    seen = 0
    for specs in SORT_GROUPS.values():
        for spec in specs:
            if spec[3] not in TIE_PATTERNS:
                continue
            c = sort_case(*spec)
            masked = c["keys"] & np.uint32(sort_mask(c["field_bits"]))
            for e in EDGES:
                if e < c["pitch"]:
                    assert np.all(masked[:, e - 1] == masked[:, e]) and np.all(c["vals"][:, e - 1] != c["vals"][:, e]), (name_of(spec), e)
            good, wrong = stable_order(c["keys"], c["field_bits"]), stable_order(c["keys"], c["field_bits"], ties_descending=True)
            assert np.array_equal(np.take_along_axis(c["keys"], good, 1) & np.uint32(sort_mask(c["field_bits"])),
                                  np.take_along_axis(c["keys"], wrong, 1) & np.uint32(sort_mask(c["field_bits"])))
            assert np.any(good != wrong), name_of(spec)
            assert np.any(np.take_along_axis(c["vals"], good, 1) != np.take_along_axis(c["vals"], wrong, 1)), name_of(spec)
            seen += 1
    assert seen == 2 * len(PLANS) * len(TIE_PATTERNS) + len(GEOMETRY) * 4


def test_the_cases_are_the_ones_the_kernels_can_go_wrong_at():
    assert [tiles_of(p) for p in ONE_SEGMENT[:11]] == [1, 1, 1, 1, 1, 2, 3, 7, 8, 10, 18]
    assert [plan_of(f) for f in PLANS] == [(8, 1), (10, 1), (11, 1), (8, 2), (10, 2), (11, 2), (8, 3), (10, 3), (11, 3), (11, 3)]
    positions = sum(2 * k * n for specs in SORT_GROUPS.values() for (k, n, _, _) in specs)
    assert positions < 20_000_000, positions
    c = sort_case(1, 36928, 32, "uniform")
    assert 0.4 < np.mean(c["keys"] >> 31) < 0.6                                                     # key bit 31 in half of the keys
    c = sort_case(9, 4160, 20, "runs")
    assert any(np.any(np.diff(np.nonzero(np.diff(c["keys"][b].astype(np.int64)))[0]) == 1) for b in range(9))   # runs of one among the long ones
    assert len({c["keys"][b].tobytes() for b in range(9)}) == 9


# ----------------------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("group", list(SORT_GROUPS))
def test_sort_equals_numpy_stable_argsort(group, tmp_path):
    specs = SORT_GROUPS[group]
    cases = [sort_case(*s) for s in specs]
    res = run_helper(tmp_path, 1, [(u32(c["K"], c["pitch"], c["field_bits"]), c["keys"], c["vals"]) for c in cases])
    bad = []
    for spec, c in zip(specs, cases):
        K, pitch, f = c["K"], c["pitch"], c["field_bits"]
        order = stable_order(c["keys"], f)
        want_keys = np.take_along_axis(c["keys"], order, 1)
        for first in (True, False):
            name = f"{name_of(spec)}, {'first' if first else 'not first'}"
            got_keys, got_vals = read_sort(res, K * pitch, bad, name)
            want_vals = order.astype(np.uint32) if first else np.take_along_axis(c["vals"], order, 1)
            for what, got, want in (("sorted keys", got_keys, want_keys), ("sorted values", got_vals, want_vals)):
                d = differs(got, want)
                if d:
                    bad.append(f"{name}: {what}: {d}")
            if first:
                (_, ok1), (_, ok2), (hist, ok3), (offs, ok4) = res.buf(), res.buf(), res.buf(), res.buf()
                if not (ok1 and ok2 and ok3 and ok4):
                    bad.append(f"{name}: guard words of the first pass alone written")
                want_hist, want_offs = first_pass_hist(c["keys"], f)
                for what, got, want in (("first-pass hist", hist, want_hist), ("first-pass offs", offs, want_offs)):
                    d = differs(got, want)
                    if d:
                        bad.append(f"{name}: {what}: {d}")
    assert res.done()
    assert not bad, report(bad)


def points_cases():
    rng = np.random.default_rng(20261020)
    third = np.float32(1.0) / np.float32(0.3)
    wide = ((-40, -40, -8), 80, 6400, np.float32(1.0), 0)
    fine = ((-41, -41, -3), 83, 83 * 83, third, 0)            # min_b[2] above the lowest points: negative steps, the cell wraps around
    out = []
    for K, ns, grids in ((3, (4160, 4000, 1), (wide, fine, wide)),
                         (3, (4000, 4160, 4160), (fine, wide[:4] + (2,), fine[:4] + (3,))),      # GRID_OVERFLOW, GRID_CAP: nothing binned
                         (1, (4000,), (fine,))):                                                 # (rs_sort_one_segment with points)
        pitch = 4160
        pts = np.empty((K, 3, pitch), np.float32)
        for b in range(K):
            leaf = np.float32(1.0) / np.float32(grids[b][3])
            span = np.float32(38.0) * leaf
            pts[b] = rng.uniform(-1.0, 1.0, (3, pitch)).astype(np.float32) * np.array([span, span, np.float32(7.0) * leaf], np.float32)[:, None]
            k = rng.integers(-30, 30, size=300).astype(np.float32)
            face = np.where(grids[b][3] == np.float32(1.0), k, k * np.float32(0.3)).astype(np.float32)      # on a cell face, and its two neighbours
            pts[b, 0, 100:400] = np.concatenate([face[:100], np.nextafter(face[100:200], np.float32(np.inf)), np.nextafter(face[200:], np.float32(-np.inf))])
            pts[b, 1, 250:550] = face
            for j, bad_value in enumerate((np.nan, np.inf, -np.inf)):
                at = rng.choice(pitch, size=40, replace=False)
                pts[b, rng.integers(0, 3, size=40), at] = np.float32(bad_value)
        out.append(dict(K=K, pitch=pitch, cb=20, n=ns, grids=grids, pts=pts))
    return out


@pytest.mark.gpu
def test_keys_from_points_and_their_sort(tmp_path):
    cases = points_cases()
    blobs = []
    for c in cases:
        g = [np.concatenate([u32(*mb, m1, m2), np.array([il], np.float32).view(np.uint32), u32(st)]) for (mb, m1, m2, il, st) in c["grids"]]
        blobs.append((u32(c["K"], c["pitch"], c["cb"]), u32(*c["n"]), np.concatenate(g), c["pts"]))
    res = run_helper(tmp_path, 2, blobs)
    bad = []
    for j, c in enumerate(cases):
        name = f"points case {j} (K {c['K']}, n {c['n']})"
        want_keys = cell_keys(c["pts"], c["n"], c["grids"], c["cb"])
        binned = want_keys != (1 << c["cb"]) - 1
        if j == 0:                                            # (the case bins what it is meant to)
            assert binned[0].mean() > 0.9 and binned[1, :4000].mean() > 0.9 and not binned[1, 4000:].any() and binned[2].sum() == 1
            assert np.any(want_keys[1][binned[1]] >> 31)      # wrapped cells
        (keys, ok1), (_, ok2), (_, ok3), (_, ok4), (hist, ok5), (offs, ok6) = tuple(res.buf() for _ in range(6))
        if not (ok1 and ok2 and ok3 and ok4 and ok5 and ok6):
            bad.append(f"{name}: guard words of the first pass alone written")
        want_hist, want_offs = first_pass_hist(want_keys, c["cb"])
        order = stable_order(want_keys, c["cb"])
        got_keys, got_vals = read_sort(res, c["K"] * c["pitch"], bad, name)
        for what, got, want in (("keys from points", keys, want_keys), ("first-pass hist", hist, want_hist), ("first-pass offs", offs, want_offs),
                                ("sorted keys", got_keys, np.take_along_axis(want_keys, order, 1)), ("sorted values", got_vals, order.astype(np.uint32))):
            d = differs(got, want)
            if d:
                bad.append(f"{name}: {what}: {d}")
    assert res.done()
    assert not bad, report(bad)


SCAN_N = (1, 3, 4, 5, 4095, 4096, 4097, 8191, 12293)
SCAN_CHUNKS = (1, 1023, 1024, 1025, 2048, 2049, 3200)        # k_pf_scan_offsets alone: its loop carries `base` past 1024 chunks


@pytest.mark.gpu
def test_scans_equal_numpy_cumsum(tmp_path):
    rng = np.random.default_rng(20261021)
    blobs, want = [], []
    for n in SCAN_N:
        for kind, flags in (("all 0", np.zeros(n, np.int64)), ("all 1", np.ones(n, np.int64)), ("random 0/1", rng.integers(0, 2, n)),
                            ("counts 0..1000", rng.integers(0, 1001, n))):
            blobs.append((u32(0, n), w32(flags)))
            sums = np.add.reduceat(flags, np.arange(0, n, TILE))
            want.append((f"scan of {n} flags, {kind}", [("totals", exscan(sums)), ("pos", exscan(flags))]))
    for nchunks in SCAN_CHUNKS:
        totals = rng.integers(0, 4097, nchunks)
        blobs.append((u32(1, nchunks), w32(totals)))
        want.append((f"k_pf_scan_offsets alone, {nchunks} chunks", [("totals", exscan(totals))]))
    for K in (1, 7, 9):
        for chunks in (1, 2, 3):
            for rp, overflow in ((TILE * chunks, True), (TILE * chunks - 192, True), (TILE * chunks - 192, False)):
                flags = rng.integers(0, 2, (K, rp))
                total = flags.sum(axis=1)
                ids = rng.permutation(K) + 10
                # slots: five words to spare, exactly full (no overflow), one word short (overflow: clouds 0, 3, 6)
                out_pitch = np.array([total[b] + (5, 0, -1 if overflow else 0)[(b + 2 * overflow) % 3] for b in range(K)])
                short = [b for b in range(K) if total[b] > out_pitch[b]]
                assert len(short) == (0 if not overflow else 1 if K == 1 else 3) and out_pitch.min() > 0
                if len(short) == 3:                           # the smallest id belongs to the middle one: neither the first nor the last to raise it
                    j = min(short, key=lambda b: ids[b])
                    ids[[short[1], j]] = ids[[j, short[1]]]
                over = [int(ids[b]) for b in short]
                items = np.stack([out_pitch, rng.integers(0, rp + 1, K), ids], axis=1)
                blobs.append((u32(2, K, chunks, rp), w32(items), w32(flags)))
                sums = np.stack([np.add.reduceat(flags[b], np.arange(0, rp, TILE)) for b in range(K)])
                want.append((f"per-cloud scan, K {K}, {chunks} chunks, rp {rp}, {'overflow' if overflow else 'no overflow'}",
                             [("mm", None), ("res", u32(*total, min(over) if over else INT_MAX, INT_MAX)),
                              ("totals", np.stack([exscan(s) for s in sums])), ("pos", np.stack([exscan(f) for f in flags]))]))
    res = run_helper(tmp_path, 3, blobs)
    bad = []
    for name, arrays in want:
        for what, w in arrays:
            got, ok = res.buf()
            if not ok:
                bad.append(f"{name}: guard words of {what} written")
            d = None if w is None else differs(got, w)
            if d:
                bad.append(f"{name}: {what}: {d}")
    assert res.done()
    assert not bad, report(bad)


@pytest.mark.gpu
def test_heads_equal_the_two_branches_of_pf_is_head(tmp_path):
    rng = np.random.default_rng(20261022)
    none = 0x7FFFFFFF
    blobs, want = [], []
    for K, rp, ns, status in ((3, 4160, (4160, 4000, 1), (0, 2, 0)), (9, 100, (100, 99, 64, 63, 1, 0, 37, 100, 65), (0, 0, 1, 0, 2, 0, 0, 0, 0)),
                              (1, 4097, (4097,), (0,))):
        for downsample in (1, 0):
            keys = np.empty((K, rp), np.uint32)
            for b in range(K):                                # sorted voxel keys in short runs, then the not-binned tail
                k = np.sort(rng.integers(0, max(2, ns[b] // 3), ns[b])).astype(np.uint32)
                keys[b] = np.concatenate([k, np.full(rp - ns[b], none, np.uint32)])
            keep = rng.integers(0, 2, (K, rp))
            blobs.append((u32(K, rp, downsample), w32(np.stack([ns, status], axis=1)), keys, w32(keep)))
            run_head = (keys != none) & np.concatenate([np.ones((K, 1), bool), keys[:, 1:] != keys[:, :-1]], axis=1)
            kept = (np.arange(rp)[None, :] < np.array(ns)[:, None]) & (keep != 0)
            ds = np.array([downsample and s == 0 for s in status], bool)[:, None]
            want.append((f"heads, K {K}, rp {rp}, downsample {downsample}",
                         [("k_pfb_heads, every grid usable", (run_head if downsample else kept).astype(np.uint32)),
                          ("k_pfb_heads", np.where(ds, run_head, kept).astype(np.uint32))]))
    res = run_helper(tmp_path, 4, blobs)
    bad = []
    for name, arrays in want:
        for what, w in arrays:
            got, ok = res.buf()
            if not ok:
                bad.append(f"{name}: guard words of {what} written")
            d = differs(got, w)
            if d:
                bad.append(f"{name}: {what}: {d}")
    assert res.done()
    assert not bad, report(bad)
