// tests/cpp/sweep_matrix_main.cpp -- the predicates that say which sweep and align kernels exist (lv_slam_amd/csrc/ndt_sweep_exists.hpp: sweep_exists,
// euler_sweep_exists, lean_exists, all derived from the one table of rows) as a table, for tests/test_sweep_entries_cpu.py.  No HIP, no device.  Each predicate is
// asked over a box that is wider than what it accepts, so that a row that should not exist is seen too.
//   const <SWEEP_IT_BATCH>
//   sweep <pca> <K> <ord> <it> <0 / 1>
//   euler <K> <ord> <0 / 1>
//   lean  <pca> <K> <ord> <0 / 1>
// With the argument `tags`, the table's own predicates instead, over every tag of a box wider still, and the gated family's wrapper:
//   tag    <pca> <K> <it> <ord> <pm> <gate> <0 / 1>     sweep_exists(SweepTag)
//   align  <pca> <K> <ord> <lean> <0 / 1>               align_exists(AlignTag)
//   ground <K> <ord> <0 / 1>
#include <cstdio>
#include <cstring>
#include "ndt_sweep_exists.hpp"
#include "ndt_sweep_waves.hpp"

int main(int argc, char** argv) {
  const int Ks[] = {0, 1, 2, 6, 7, 8, 13, 25, 26, 27, 28};
  const int its[] = {0, 1, 2, 3, 4, 8, 16};
  if (argc > 1 && !std::strcmp(argv[1], "tags")) {
    for (int pca = 0; pca < 2; pca++)
      for (int K : Ks)
        for (int ord = -1; ord <= 3; ord++) {
          for (int it : its)
            for (int pm = -1; pm <= 3; pm++)
              for (int gate = 0; gate < 2; gate++)
                std::printf("tag %d %d %d %d %d %d %d\n", pca, K, it, ord, pm, gate, sweep_exists(SweepTag{pca != 0, K, it, ord, pm, gate != 0}) ? 1 : 0);
          for (int lean = 0; lean < 2; lean++) std::printf("align %d %d %d %d %d\n", pca, K, ord, lean, align_exists(AlignTag{pca != 0, K, ord, lean != 0}) ? 1 : 0);
          if (!pca) std::printf("ground %d %d %d\n", K, ord, ground_sweep_exists(K, ord) ? 1 : 0);
        }
    return 0;
  }
  std::printf("const %d\n", SWEEP_IT_BATCH);
  for (int pca = 0; pca < 2; pca++)
    for (int K : Ks)
      for (int ord = -1; ord <= 3; ord++) {
        for (int it : its) std::printf("sweep %d %d %d %d %d\n", pca, K, ord, it, sweep_exists(pca != 0, K, ord, it) ? 1 : 0);
        std::printf("lean %d %d %d %d\n", pca, K, ord, lean_exists(pca != 0, K, ord) ? 1 : 0);
        if (!pca) std::printf("euler %d %d %d\n", K, ord, euler_sweep_exists(K, ord) ? 1 : 0);
      }
  return 0;
}
