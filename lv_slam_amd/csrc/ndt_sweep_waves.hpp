// ndt_sweep_waves.hpp -- MI355NDT_OPT_SWEEP_WAVES: which values the option takes and when, which launches have a three-wave body at all, and the
// automatic choice between two and three waves per SIMD.  Nothing of HIP in this file: it compiles into the library's host side
// (ndt_host_life.hpp: the option; ndt_host_sweep.hpp: async_lean, the per-launch decision) and into tests/cpp/sweep_waves_main.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include "mi355_ndt.h"
#include "ndt_sweep_exists.hpp"    // lean_exists: the LEAN rows of the table of align kernels

// mi355ndt_set_option(MI355NDT_OPT_SWEEP_WAVES, value): 0 = automatic, 2, 3; not while a stream is open (its launches' geometry, its reserve and
// its hand-over threshold were sized at mi355ndt_stream_begin)
static inline int sweep_waves_option_rc(bool in_stream, int value) {
  if (in_stream) return MI355NDT_ERR_STATE;
  return (value == 0 || value == 2 || value == 3) ? MI355NDT_OK : MI355NDT_ERR_BAD_ARG;
}

// k_align_async<false, 7, ORD, true>, ORD = 0 / 1, is the exact ndt_omp / DIRECT7 launch with the lean item body (SweepTune, ndt_sweep.hpp): 168
// registers, three workgroups per CU, 768 slots instead of 512.  `ord`: 0 / 1 = the f32 sum orders, 2 = the tolerance arithmetic.  The lockstep
// rounds (hence the Euler model and MI355NDT_OPT_NDT_CLASS = 1, which never leave them) have no such body.  lean_exists(pca, K, ord)
// (ndt_sweep_exists.hpp) says whether the table has the row.

// The lean body pays for the third wave with the mid-evaluation record prefetch, so a batch's records have to come out of L2.  What the host
// knows without a readback:
//   * records of a target ~ points / (LEAN_PTS_PER_M2 x leaf^2) leaves x 64 B, at most points / min_points_per_voxel leaves.  A scan paints
//     surfaces: the points of a leaf grow with its face.  32 per m^2 sits between the two leaf statistics the project has (65,536-point
//     headline scans at 1 m: 1,422 leaves, 43 points per leaf; the prefiltered 53 k-point scans: 1,842, 27) and errs to more leaves for
//     denser scans -- towards two waves, the body every configuration ran before.  (The stream's build plan knows the grids' volume, not
//     how much of it is occupied: no help here.)
//   * an XCD's 4 MB L2 serves the pairs its waves have in flight -- two 65,536-point pairs at two waves per SIMD, three at three (a pair's
//     sweep is 128 items, an XCD has 256 / 384 waves) -- and most of it goes to their point streams (786 KB a pair), bitmaps and rows:
//     the records of the pairs in flight get a quarter.  Threshold: 4 MB / 4 / 3 pairs = 341 KB of records per pair.
// Config 3 (1 m, 65,536 points): 2,048 leaves = 128 KB: three waves.  Config 5 (0.5 m, 131,072 points): 16,384 leaves = 1 MB: two.
constexpr size_t LEAN_L2_BYTES = (size_t)4 << 20;
constexpr int LEAN_PAIRS_IN_FLIGHT = 3;
constexpr size_t LEAN_REC_BYTES_MAX = LEAN_L2_BYTES / 4 / LEAN_PAIRS_IN_FLIGHT;
constexpr double LEAN_PTS_PER_M2 = 32.0;
constexpr size_t LEAN_REC_BYTES = 64;              // sizeof(VoxelRec)
static inline size_t est_record_bytes(const mi355ndt_params& prm, size_t tgt_pts) {
  const double by_face = (double)tgt_pts / (LEAN_PTS_PER_M2 * (double)prm.resolution * (double)prm.resolution);
  const double by_count = (double)tgt_pts / (double)std::max(1, prm.min_points_per_voxel);
  return (size_t)(std::min(by_face, by_count) * (double)LEAN_REC_BYTES);
}
// Waves per SIMD of a persistent launch's exact item body: `option` = MI355NDT_OPT_SWEEP_WAVES, `ord` = the arithmetic of the launch's sweeps,
// `tgt_pts` = the largest target of the batch (a stream: of the batch the launch starts).  Measured (docs/experiments.md 10o): config 3 streamed, three
// waves against two on one box, +4.6 % registrations/s, ten times the run-to-run spread.
static inline int sweep_waves_choice(int option, const mi355ndt_params& prm, int ord, size_t tgt_pts) {
  if (!lean_exists(prm.variant == MI355NDT_VARIANT_PCA, prm.neighbor_mode == MI355NDT_DIRECT7 ? 7 : 0, ord) || option == 2) return 2;
  if (option == 3) return 3;
  return est_record_bytes(prm, tgt_pts) <= LEAN_REC_BYTES_MAX ? 3 : 2;
}
