// mi355_ndt.hip -- MI355X (gfx950) NDT scan-matching engine behind the C-ABI of include/mi355_ndt.h.
//
// What runs where (all on the GPU; the host only enqueues):
//   target build  : k_minmax -> k_griddesc -> radix sort (cell from the points, input order) -> k_mark (+ run heads)
//                   -> k_rank (+ run starts by voxel id) -> k_leafsum -> k_voxels          (VoxelGridCovariance::applyFilter,
//                   include/ndt_omp/voxel_grid_covariance_omp_impl.hpp:48-370)
//   GICP          : k_gc_cov -> [k_gc_match -> (k_gc_cost -> k_gc_cost_final)*]*   (pclomp::GeneralizedIterativeClosestPoint, gicp_omp_impl.hpp; the
//                   BFGS optimiser and the outer loop on the host: ndt_gicp.hpp, gicp_bfgs.hpp, ndt_host_gicp.hpp)
//   GICP batch    : k_gc_cov per cloud -> [table copy -> k_gc_match_batch -> k_gc_cost_batch -> k_gc_cost_final_batch]*, one round for all
//                   candidates of a loop check (gicp_lockstep.hpp, ndt_host_gicp_batch.hpp)
//   ICP           : [k_icp_step -> k_icp_final]*, one round trip per iteration (pcl::IterativeClosestPoint; the 3x3 SVD, the criteria and
//                   the loop on the host: ndt_icp.hpp, icp_outer.hpp, ndt_host_icp.hpp); the batch: [table copy -> k_icp_step_batch ->
//                   k_icp_final_batch]* for all candidates of a loop check (ndt_host_icp_batch.hpp)
//   search        : [index build] -> [k_knn_keys -> radix sort per item] -> k_kf_knn (ring walk) + k_kf_knn (exhaustive): exact k-nearest and
//                   radius search over resident keyframes, one launch chain and one wait per call (ndt_knn.hpp, ndt_host_knn.hpp)
//   align         : k_init_state -> k_sweep -> [k_update -> k_sweep]*      (computeTransformation +
//                   computeDerivatives + computeStepLengthMT, include/ndt_omp/ndt_omp_impl2.hpp:87-188, 196-305, 841-1003;
//                   step_size <= eps/2 only: [k_update -> k_hessian -> k_update -> k_sweep]*, impl2:622-714, 920-1000)
// Build: __graft_entry__.build() compiles three translation units side by side and links them: this file, mi355_ndt_ord1.hip (the kernel
// instantiations of the second f32 sum order) and mi355_ndt_fast.hip (those of the tolerance arithmetic), each its ORD's rows of the one table
// of sweep and align kernels (ndt_sweep_exists.hpp); -DNDT_SINGLE_TU builds everything from this file alone.
// Kernels live in ndt_build.hpp / ndt_sweep.hpp / ndt_update.hpp (the Newton control they call: ndt_newton.hpp) / ndt_hessian.hpp / ndt_upload.hpp / ndt_pose_record.hpp / ndt_pose_scores.hpp / ndt_fitness.hpp / ndt_prefilter.hpp / ndt_prefilter_batch.hpp / ndt_prefilter_approx.hpp / ndt_keyframe.hpp / ndt_kffitness.hpp / ...; the host side of the
// C-ABI lives in ndt_engine.hpp and the ndt_host_*.hpp headers listed at the end of this file, one per surface.  It stays ONE translation unit
// (the non-template kernels of the headers would collide across units).  Data layout in HBM: DESIGN.md.  Built with -ffp-contract=off: every
// f32/f64 step of the reference recipe is a separately rounded operation.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>
#include <algorithm>
#include <cmath>
#include <mutex>
#include <atomic>
#include <thread>
#include <sched.h>
#include <fstream>
#include <chrono>
#include <memory>
#include <map>
#include <array>
#include <type_traits>

#include "mi355_ndt.h"
#include "ndt_math.hpp"
#include "ndt_types.hpp"
#include "ndt_build.hpp"
#include "ndt_segsort.hpp"
#include "ndt_sweep.hpp"
#include "ndt_newton.hpp"
#include "ndt_update.hpp"
#include "ndt_upload.hpp"
#include "ndt_pose_record.hpp"
#include "ndt_hessian.hpp"
#include "ndt_sweep_kd.hpp"
#include "ndt_fitness.hpp"
#include "ndt_prefilter.hpp"
#include "ndt_prefilter_batch.hpp"
#include "ndt_prefilter_approx.hpp"
#include "ndt_mapcloud.hpp"
#include "ndt_keyframe.hpp"
#include "ndt_kffitness.hpp"
#include "ndt_outlier.hpp"
#include "ndt_outlier_batch.hpp"
#include "ndt_knn.hpp"
#include "ndt_gicp.hpp"
#include "gicp_bfgs.hpp"
#include "gicp_lockstep.hpp"
#include "ndt_icp.hpp"
#include "icp_outer.hpp"
#include "ndt_sequence.hpp"
#include "ndt_async.hpp"
#include "ndt_hostmem.hpp"
#include "ndt_grid_state.hpp"
#include "ndt_sweep_waves.hpp"
#include "ndt_pose_scores.hpp"
#ifndef NDT_SINGLE_TU      // the ORD = 1 / 2 rows of the table come from mi355_ndt_ord1.hip / mi355_ndt_fast.hip (built side by side with this file)
#define NDT_TU ELSEWHERE
#define NDT_TU_X extern template
NDT_KERNELS_OF_TU
NDT_POSE_SCORE_KERNELS_OF_TU   // (no rows of the table: the pose scores' own list, ndt_pose_scores.hpp)
#endif

// ------------------------------------------------------------------------------------ host side, in dependency order
// Every mi355ndt_* function is declared extern "C" by mi355_ndt.h, so the definitions below need no linkage block of their own.
#include "ndt_engine.hpp"          // the handle, the session, the decisions shared by several surfaces
#include "ndt_host_life.hpp"       // create / destroy / params / options
#include "ndt_host_upload.hpp"     // reserve, bind, host-cloud uploads
#include "ndt_host_profile.hpp"    // ev_*, mi355ndt_profile_*
#include "ndt_host_build.hpp"      // target build
#include "ndt_host_sweep.hpp"      // the table's kernel lookup, launch_sweep, launch_async
#include "ndt_host_align.hpp"      // batch align, single-registration surface
#include "ndt_host_hooks.hpp"      // parity hooks and getters
#include "ndt_host_fitness.hpp"    // fitness scores, calculateScore
#include "ndt_host_pose_scores.hpp" // many start poses per pair scored in one call
#include "ndt_host_voxel.hpp"      // the scratch and the steps shared by the four voxel surfaces below
#include "ndt_host_prefilter.hpp"  // prefilter
#include "ndt_host_mapcloud.hpp"   // map cloud
#include "ndt_host_keyframe.hpp"   // window map, keyframe store, consumers by id
#include "ndt_host_kffitness.hpp"  // fitness scores of edges between keyframes, information matrices
#include "ndt_host_outlier.hpp"    // outlier removal over the prefilter result and over batch slots
#include "ndt_host_knn.hpp"        // k-nearest and radius search over resident keyframes
#include "ndt_host_gicp.hpp"       // GICP: covariances, correspondences, cost, BFGS driver, align
#include "ndt_host_gicp_batch.hpp" // GICP: all candidates of a loop check in one lockstep batch
#include "ndt_host_icp.hpp"        // ICP: correspondences, align (the estimate, the criteria and the loop: icp_outer.hpp)
#include "ndt_host_icp_batch.hpp"  // ICP: all candidates of a loop check in one batch, one loop on the calling thread
#include "ndt_host_sequence.hpp"   // latency mode, sequence run
#include "ndt_host_stream.hpp"     // stream mode
