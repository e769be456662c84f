// grid_state_main.cpp -- lv_slam_amd/csrc/ndt_grid_state.hpp as tables, for tests/test_grid_state_cpu.py (built with -fsanitize=address,undefined):
//   extras <search> <variant> <mt_live> <arith> <live>  <cent> <icov64> <kdw> <recs_fast>     grid_extras of every configuration, both flavours
//   serve <a> <b> <0|1>                                    grids_serve(a build for configuration a, what configuration b needs), a, b in 0 .. 31
//   invalid <n>                                            needs (of the 32) a record with every extra made but valid = false serves
// Configuration index: ((search * 2 + variant) * 2 + mt_live) * 2 + arith.
#include <cstdio>
#include <vector>
#include "ndt_grid_state.hpp"

int main() {
  std::vector<GridExtras> cfg;
  for (int search = 0; search < 4; search++)
    for (int variant = 0; variant < 2; variant++)
      for (int mt = 0; mt < 2; mt++)
        for (int arith = 0; arith < 2; arith++) {
          mi355ndt_params p{};
          p.resolution = 1.0f; p.neighbor_mode = search; p.variant = variant; p.trans_epsilon = 0.1;
          p.step_size = mt ? 0.01 : 0.1;           // live iff !(step_size - trans_epsilon / 2 > 0)
          for (int live = 0; live < 2; live++) {
            const GridExtras x = grid_extras(p, arith, live != 0);
            std::printf("extras %d %d %d %d %d  %d %d %d %d\n", search, variant, mt, arith, live, x.cent, x.icov64, x.kdw, x.recs_fast);
          }
          cfg.push_back(grid_extras(p, arith));
        }
  int invalid_served = 0;
  for (size_t a = 0; a < cfg.size(); a++)
    for (size_t b = 0; b < cfg.size(); b++) {
      const GridsBuilt built{true, cfg[a], 1.0f, 8, 1024, false};
      std::printf("serve %zu %zu %d\n", a, b, grids_serve(built, cfg[b]) ? 1 : 0);
    }
  for (const GridExtras& need : cfg) invalid_served += grids_serve(GridsBuilt{false, GridExtras{true, true, true, true}, 1.0f, 8, 1024, true}, need) ? 1 : 0;
  std::printf("invalid %d\n", invalid_served);
  return 0;
}
