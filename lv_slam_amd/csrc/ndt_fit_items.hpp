// ndt_fit_items.hpp -- the item table of one fitness launch (FitItem / fit_item, ndt_fitness.hpp).  Host only, no HIP types: a plain
// C++ program can include it (tests/test_fit_items_cpu.py does).
#pragma once
#include <algorithm>
#include <array>
#include <vector>

#define FIT_ITEM_INTS 8                // ints per item: {pair, block0, part0, n_src, n_tgt, ring_max, first, count}

// 16 ints of group starts, then the items group by group.  Item i of N (a pair, an edge; nblk[i] blocks of 256 points) takes part iff
// takes(i).  Group g is the workgroups of one XCD; an item goes to the least loaded of the eight groups, in index order, so that its blocks
// share one L2 with its target points and index.  A launch of few items would leave XCDs idle that way: with `total` blocks in the launch
// and cap = max(1, ceil(total / 8)), an item of more than `cap` blocks is cut into consecutive pieces of `cap` blocks (the last one shorter)
// and the pieces are dealt like items.  A piece covers blocks first .. first + count - 1 of its pair; block0 = the piece's first block
// within its group; tail(i) gives {n_src, n_tgt, ring_max}.  A block's partial slot is part0[i] + its index within the PAIR, so the block
// partials and the order the host sums them in do not depend on the cut.
template <typename Takes, typename Tail>
static void fit_item_table(int N, const std::vector<int>& nblk, const std::vector<int>& part0, Takes takes, Tail tail, std::vector<int>& t, int& group_max) {
  struct Piece { int item, first, count, group; };
  long long total = 0;
  for (int i = 0; i < N; i++) if (nblk[(size_t)i] > 0 && takes(i)) total += nblk[(size_t)i];
  const int cap = (int)std::max(1ll, (total + 7) / 8);
  int load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<Piece> pieces;
  for (int i = 0; i < N; i++) {
    if (nblk[(size_t)i] <= 0 || !takes(i)) continue;
    for (int first = 0; first < nblk[(size_t)i]; first += cap) {
      int g = 0;
      for (int k = 1; k < 8; k++) if (load[k] < load[g]) g = k;
      const int count = std::min(cap, nblk[(size_t)i] - first);
      pieces.push_back({i, first, count, g});
      load[g] += count;
    }
  }
  t.assign(16, 0);
  for (int g = 0; g < 8; g++) {
    t[(size_t)g] = (int)((t.size() - 16) / FIT_ITEM_INTS);
    int blk = 0;
    for (const Piece& p : pieces) {
      if (p.group != g) continue;
      const std::array<int, 3> x = tail(p.item);
      t.insert(t.end(), {p.item, blk, part0[(size_t)p.item], x[0], x[1], x[2], p.first, p.count});
      blk += p.count;
    }
  }
  t[8] = (int)((t.size() - 16) / FIT_ITEM_INTS);
  group_max = *std::max_element(load, load + 8);
}
