// The item table of a fitness launch (lv_slam_amd/csrc/ndt_fit_items.hpp) as a host program, for tests/test_fit_items_cpu.py, which builds it
// with -fsanitize=address,undefined.  stdin: N, then N lines "nblk takes part0".  stdout: group_max, the table's length, the table.
#include <cstdio>
#include "ndt_fit_items.hpp"

int main() {
  int N = 0;
  if (std::scanf("%d", &N) != 1 || N < 0) return 2;
  std::vector<int> nblk((size_t)N), takes((size_t)N), part0((size_t)N);
  for (int i = 0; i < N; i++)
    if (std::scanf("%d %d %d", &nblk[(size_t)i], &takes[(size_t)i], &part0[(size_t)i]) != 3) return 2;
  std::vector<int> t;
  int group_max = 0;
  fit_item_table(N, nblk, part0, [&](int i) { return takes[(size_t)i] != 0; },
                 [&](int i) { return std::array<int, 3>{nblk[(size_t)i] * 256 - 3, 1000 + i, 7}; }, t, group_max);
  std::printf("%d %zu\n", group_max, t.size());
  for (int v : t) std::printf("%d\n", v);
  return 0;
}
