"""CPU: the item table of a fitness launch (fit_item_table, lv_slam_amd/csrc/ndt_fit_items.hpp).  The builder is compiled into a host
program of its own (tests/cpp/fit_items_main.cpp) with -fsanitize=address,undefined, run on each list of block counts, and its output is
read here: which workgroup serves which block of which pair (fit_item of ndt_fitness.hpp, restated below), where its partial lands, and
how evenly the eight groups are loaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = 8            # ints per item: pair, block0, part0, n_src, n_tgt, ring_max, first, count

# (block counts, who takes part)
CASES = {
    "one_pair_of_ten": ([10], None),
    "one_block": ([1], None),
    "one_big_eight_small": ([64, 3, 3, 3, 3, 3, 3, 3, 3], None),
    "271_full_size": ([256] * 271, None),
    "zeros_and_non_takers": ([5, 0, 300, 7, 0, 12, 1, 40, 0], [1, 1, 1, 0, 1, 1, 0, 1, 0]),
}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fit_items") / "fit_items_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "lv_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fit_items_main.cpp"), "-o", exe])
    return exe


def part0_of(nblk):
    """the first partial slot of every pair, as the host lays them out: back to back over all pairs, takers of this launch or not"""
    out, at = [], 0
    for n in nblk:
        out.append(at)
        at += n
    return out


def table(program, nblk, takes):
    takes = takes or [1] * len(nblk)
    part0 = part0_of(nblk)
    text = f"{len(nblk)}\n" + "".join(f"{n} {t} {p}\n" for n, t, p in zip(nblk, takes, part0))
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stderr        # a sanitizer report ends the program with a message
    nums = [int(x) for x in out.stdout.split()]
    gmax, size, t = nums[0], nums[1], nums[2:]
    assert len(t) == size and size >= 16 and (size - 16) % INTS == 0
    items = [tuple(t[16 + INTS * k:16 + INTS * (k + 1)]) for k in range((size - 16) // INTS)]
    return gmax, t[:16], items, takes, part0


def fit_item(gstart, items, L):
    """fit_item (ndt_fitness.hpp) for workgroup L: (pair, block within the pair, partial slot) or None"""
    g, s = L & 7, L >> 3
    lo, hi = gstart[g], gstart[g + 1]
    if lo >= hi:
        return None
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if items[mid][1] <= s:
            lo = mid
        else:
            hi = mid
    pair, block0, part0, _, _, _, first, count = items[lo]
    if s - block0 >= count:
        return None
    bx = first + (s - block0)
    return pair, bx, part0 + bx


@pytest.mark.parametrize("name", list(CASES))
def test_every_block_once_in_one_group_at_its_slot_and_groups_even(program, name):
    nblk, takes = CASES[name]
    gmax, gstart, items, takes, part0 = table(program, nblk, takes)
    takers = [i for i, n in enumerate(nblk) if n > 0 and takes[i]]
    total = sum(nblk[i] for i in takers)
    cap = max(1, -(-total // 8))
    assert gstart[0] == 0 and gstart[8] == len(items) and all(gstart[g] <= gstart[g + 1] for g in range(8)) and gstart[9:] == [0] * 7
    # every piece lies within one group, the group's pieces back to back from block 0; no piece longer than cap; what tail() gave
    load = []
    for g in range(8):
        at = 0
        for pair, block0, p0, n_src, n_tgt, ring_max, first, count in items[gstart[g]:gstart[g + 1]]:
            assert block0 == at and 1 <= count <= cap and 0 <= first and first + count <= nblk[pair]
            assert pair in takers and p0 == part0[pair] and (n_src, n_tgt, ring_max) == (nblk[pair] * 256 - 3, 1000 + pair, 7)
            at += count
        load.append(at)
    assert gmax == max(load) and sum(load) == total
    # the groups are even to within the largest uncut item
    b = min(cap, max(nblk[i] for i in takers))
    assert max(load) - min(load) <= b, (load, b)
    # the launch: 8 * gmax workgroups; every (pair, block) of a taker is served by exactly one, at slot part0 + block
    seen = {}
    for L in range(8 * gmax):
        got = fit_item(gstart, items, L)
        if got is None:
            continue
        pair, bx, slot = got
        assert (pair, bx) not in seen and slot == part0[pair] + bx
        seen[(pair, bx)] = L & 7
    assert sorted(seen) == [(i, k) for i in takers for k in range(nblk[i])]
    # a pair of more than cap blocks is cut into consecutive pieces of cap blocks, the last one shorter; no other pair is cut
    for i in takers:
        pieces = sorted((it[6], it[7]) for it in items if it[0] == i)
        assert pieces == [(f, min(cap, nblk[i] - f)) for f in range(0, nblk[i], cap)]


def test_271_equal_pairs_are_not_cut_and_sit_where_the_uncut_rule_put_them(program):
    nblk, _ = CASES["271_full_size"]
    gmax, gstart, items, takes, part0 = table(program, nblk, None)
    # the rule before pairs could be cut: a whole pair to the least loaded group, in index order; the groups' pairs listed back to back
    load, group = [0] * 8, []
    for n in nblk:
        g = load.index(min(load))
        group.append(g)
        load[g] += n
    want_start, want = [], []
    for g in range(8):
        want_start.append(len(want))
        at = 0
        for i, n in enumerate(nblk):
            if group[i] == g:
                want.append((i, at, part0[i]))
                at += n
    assert gstart[:9] == want_start + [len(want)] and gmax == max(load)
    assert [it[:3] for it in items] == want
    assert all((it[6], it[7]) == (0, 256) for it in items)
