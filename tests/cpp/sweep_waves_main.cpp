// tests/cpp/sweep_waves_main.cpp -- lv_slam_amd/csrc/ndt_sweep_waves.hpp (MI355NDT_OPT_SWEEP_WAVES: the option's values, the launches that have a
// three-wave body, the automatic choice) as tables, for tests/test_sweep_waves_cpu.py.  No HIP, no device.
//   option <in_stream> <value> <return code>
//   exists <pca> <K> <ord> <0 / 1>
//   bytes  <resolution> <min_points_per_voxel> <points> <estimated record bytes>
//   choice <option> <variant> <neighbor_mode> <ord> <resolution> <points> <waves>
//   const  <L2 bytes> <pairs in flight> <threshold bytes> <points per m^2> <record bytes>
#include <cstdio>
#include "ndt_sweep_waves.hpp"

int main() {
  for (int in_stream = 0; in_stream < 2; in_stream++)
    for (int v = -2; v <= 5; v++) std::printf("option %d %d %d\n", in_stream, v, sweep_waves_option_rc(in_stream != 0, v));
  const int Ks[] = {1, 7, 26, 27};
  for (int pca = 0; pca < 2; pca++)
    for (int K : Ks)
      for (int ord = 0; ord < 3; ord++) std::printf("exists %d %d %d %d\n", pca, K, ord, lean_exists(pca != 0, K, ord) ? 1 : 0);
  mi355ndt_params prm{};                            // (only resolution, min_points_per_voxel, variant and neighbor_mode are read)
  const float res[] = {0.25f, 0.5f, 1.0f, 2.0f};
  const size_t pts[] = {0, 4096, 65536, 131072, 1000000};
  for (float r : res)
    for (int mp : {1, 6, 1000})
      for (size_t n : pts) {
        prm.resolution = r; prm.min_points_per_voxel = mp;
        std::printf("bytes %g %d %zu %zu\n", (double)r, mp, n, est_record_bytes(prm, n));
      }
  prm.min_points_per_voxel = 6;                     // the reference's default
  for (int opt : {0, 2, 3})
    for (int variant = 0; variant < 2; variant++)
      for (int mode = 0; mode < 4; mode++)
        for (int ord = 0; ord < 3; ord++)
          for (float r : res)
            for (size_t n : pts) {
              prm.variant = variant; prm.neighbor_mode = mode; prm.resolution = r;
              std::printf("choice %d %d %d %d %g %zu %d\n", opt, variant, mode, ord, (double)r, n, sweep_waves_choice(opt, prm, ord, n));
            }
  std::printf("const %zu %d %zu %g %zu\n", LEAN_L2_BYTES, LEAN_PAIRS_IN_FLIGHT, LEAN_REC_BYTES_MAX, LEAN_PTS_PER_M2, LEAN_REC_BYTES);
  return 0;
}
