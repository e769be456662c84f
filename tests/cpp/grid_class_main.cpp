// grid_class_main.cpp -- the class-taking functions of lv_slam_amd/csrc/ndt_grid_state.hpp (MI355NDT_OPT_NDT_CLASS) as tables, for
// tests/test_ndt_pcl_cpu.py (built with -fsanitize=address,undefined):
//   extras <class> <search> <variant> <mt_live> <arith> <live>  <cent> <icov64> <kdw> <recs_fast>
//   same <n>                   configurations (of the 64 with class 0) whose class-taking answers differ from the class-0 functions'
//   model <class> <pose_model>  <model> <arith of MI355NDT_OPT_ARITH = 1> <leaves rounds> <search run for DIRECT1>
//   refuses <class> <pose_model> <variant> <mt_live>  <0|1>
//   rebuild <0|1>              a build for class 0 / DIRECT7 serves what class 1 / DIRECT7 needs (0: the align rebuilds), and the other way round
#include <cstdio>
#include "ndt_grid_state.hpp"

static mi355ndt_params params(int search, int variant, int mt) {
  mi355ndt_params p{};
  p.resolution = 1.0f; p.neighbor_mode = search; p.variant = variant; p.trans_epsilon = 0.1;
  p.step_size = mt ? 0.01 : 0.1;                 // live iff !(step_size - trans_epsilon / 2 > 0)
  return p;
}

int main() {
  int differ = 0;
  for (int cls = 0; cls < 2; cls++)
    for (int search = 0; search < 4; search++)
      for (int variant = 0; variant < 2; variant++)
        for (int mt = 0; mt < 2; mt++)
          for (int arith = 0; arith < 2; arith++)
            for (int live = 0; live < 2; live++) {
              const mi355ndt_params p = params(search, variant, mt);
              const GridExtras x = grid_extras(p, arith, live != 0, cls), x0 = grid_extras(p, arith, live != 0);
              std::printf("extras %d %d %d %d %d %d  %d %d %d %d\n", cls, search, variant, mt, arith, live, x.cent, x.icov64, x.kdw, x.recs_fast);
              if (cls == 0 && (x.cent != x0.cent || x.icov64 != x0.icov64 || x.kdw != x0.kdw || x.recs_fast != x0.recs_fast)) differ++;
            }
  std::printf("same %d\n", differ);
  for (int cls = 0; cls < 2; cls++)
    for (int pm = 0; pm < 2; pm++) {
      std::printf("model %d %d  %d %d %d %d\n", cls, pm, class_model(cls, pm), model_arith(pm, 1, cls), model_leaves_rounds(pm, cls) ? 1 : 0,
                  class_neighbor_mode(cls, MI355NDT_DIRECT1));
      for (int variant = 0; variant < 2; variant++)
        for (int mt = 0; mt < 2; mt++)
          std::printf("refuses %d %d %d %d  %d\n", cls, pm, variant, mt, model_refuses(params(MI355NDT_DIRECT7, variant, mt), pm, cls) ? 1 : 0);
    }
  const mi355ndt_params d7 = params(MI355NDT_DIRECT7, 0, 0);
  const GridsBuilt by0{true, grid_extras(d7, 0, false, NDT_CLASS_OMP), 1.0f, 8, 1024, false}, by1{true, grid_extras(d7, 0, false, NDT_CLASS_PCL), 1.0f, 8, 1024, false};
  std::printf("rebuild %d\n", grids_serve(by0, grid_extras(d7, 0, false, NDT_CLASS_PCL)) ? 1 : 0);
  std::printf("rebuild %d\n", grids_serve(by1, grid_extras(d7, 0, false, NDT_CLASS_OMP)) ? 1 : 0);
  return 0;
}
