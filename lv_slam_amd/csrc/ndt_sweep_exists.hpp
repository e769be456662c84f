// ndt_sweep_exists.hpp -- which instantiations of k_sweep / k_align_async exist: the predicates the host's dispatcher (ndt_host_sweep.hpp) is
// guarded by.  Nothing of HIP in this file: it compiles into the library's host side and into tests/cpp/sweep_matrix_main.cpp, which prints the
// predicates as a table for tests/test_sweep_entries_cpu.py to hold the tests' configuration lists and the two text lists to.
#pragma once

// The instantiations of k_sweep / k_align_async that exist, by (ndt_pca, cells probed, sum order / arithmetic ORD, tiles per item IT):
//   * K = 1 / 7 / 26 / 27 (neighbor_K); ndt_pca + KDTREE (K = 27) has the literal kernel k_sweep_pca_kd instead
//   * ORD = 0 / 1: the two f32 sum orders; ORD = 2, the tolerance arithmetic, for DIRECT1 / DIRECT7 alone (fast_served)
//   * IT = 8: batch-mode items (and the one-launch align, which has no other); IT = 1 / 2: latency mode's fine items, DIRECT1 / DIRECT7 alone
// ndt_ord1_list.hpp and ndt_fast_list.hpp spell out the ORD = 1 and ORD = 2 rows of this predicate as text (explicit instantiation needs
// that): a change here is a change there.
// k_align_async alone has a fourth tag: <false, 7, ORD, true>, ORD = 0 / 1, the lean item body at three waves per SIMD (lean_exists, ndt_sweep_waves.hpp;
// launch_async picks it when the launch's AsyncLaunch::lean says so).
// Under MI355NDT_OPT_POSE_MODEL = 1: k_sweep<false, K, 8, false, ORD, 1> for the four K and ORD = 0 / 1 (euler_sweep_exists, launch_sweep_euler).
// Under MI355NDT_OPT_NDT_CLASS = 1: k_sweep<false, 27, 8, false, 0, 2> alone (the radius search, the f64 evaluation: launch_sweep).
// Under MI355NDT_OPT_GROUND_CLASS = 1 / 2: k_sweep<false, K, 8, false, ORD, 0, true>, the gated probe stage, for the DIRECT searches and ORD = 0 / 1
// (ground_sweep_exists, launch_sweep_ground; the ORD = 1 rows are spelled out in ndt_ground_list.hpp).  Class 3 runs the ungated rows.
constexpr int SWEEP_IT_BATCH = 8;
constexpr bool ground_sweep_exists(int K, int ord) { return (K == 1 || K == 7 || K == 26) && (ord == 0 || ord == 1); }
constexpr bool euler_sweep_exists(int K, int ord) { return (K == 1 || K == 7 || K == 26 || K == 27) && (ord == 0 || ord == 1); }
constexpr bool sweep_exists(bool pca, int K, int ord, int it) {
  if ((K != 1 && K != 7 && K != 26 && K != 27) || (pca && K == 27)) return false;
  if (ord < 0 || ord > 2 || (it != SWEEP_IT_BATCH && it != 1 && it != 2)) return false;
  return (K == 1 || K == 7) || (ord != 2 && it == SWEEP_IT_BATCH);
}
