// ndt_pose_scores.hpp -- mi355ndt_batch_score_poses: the score and the hit count of one computeDerivatives sweep (ndt_omp_impl2.hpp:196-305)
// for many (pair of the bound batch, pose) items in two launches.  No gradient, no Hessian, no PairState: an item names its pair's source
// rows, point count and grid, and its pose comes from a table of the call's own.
//   k_pose_scores<PCA, K, ORD>  every (item, 512-point row) is one sweep_item in its score-only form -- the probe stage, the hit queue, the
//                               64-hit batches, the ndt_pca suffix weights, eval_score and score_row_store of ndt_sweep.hpp, nothing restated --
//                               and leaves the score and the hit count of its row;
//   k_pose_score_rows           adds an item's rows in the update's row tree (ndt_update.hpp: reduce_pair_rows) and writes scores[e], hits[e].
// So an item's two words are what k_sweep + k_update leave in PairState::score / hits for the same pair at the same pose, bit for bit.
// These kernels are no rows of the table of sweep and align kernels (ndt_sweep_exists.hpp): they have the short row list below.
#pragma once
#include "ndt_types.hpp"
#include "ndt_sweep.hpp"
#include "ndt_update.hpp"
#include "ndt_sweep_exists.hpp"

// One item of a call, in the caller's order.  `row0`: where the item's rows start in the call's row buffer, in doubles.
struct PoseItem { long long row0; int pair, n, grid, n_rows; };
// The items of one pair, sorted together: `count` items order[first .. first + count) of n_rows rows each; the segment's work (count * n_rows
// sweep items) starts at `work0` of the call's flat work order.
struct PoseSeg { long long work0; int first, count, n_rows, pad; };
#define POSE_WORDS 12                    // T as the sweep reads it: 3 x 4 row-major
// A score-only row is two words: the score (word 0) and the hit count (word 43 = NACC - 1) of a 44-double stride that sweep_item and the row
// tree both assume.  Items of one pair are laid out POSE_LACE to a block of n_rows + 1 strides, item k of a block starting 2 k doubles in: its
// score words then sit at offset 2 k of every stride and its hit words at offset 2 k - 1 of the next one (k = 0: at 43 of the same), all distinct.
// 22 items share the memory one would take: the call's rows of 2,025 items of 100 k points are 6 MB, not 140.
#define POSE_LACE (NACC / 2)
static_assert(NACC % 2 == 0 && COL_SCORE == 0 && COL_HITS == NACC - 1, "the lacing of score-only rows");

// The kernel's rows: R(PCA, K, ORD).  ndt_pca + KDTREE has order-dependent weights and a kernel of its own (ndt_sweep_kd.hpp): not served.
#define NDT_POSE_SCORE_ROWS(R)                                                                             \
  R(false, 1, 0) R(true, 1, 0) R(false, 7, 0) R(true, 7, 0) R(false, 26, 0) R(true, 26, 0) R(false, 27, 0) \
  R(false, 1, 1) R(true, 1, 1) R(false, 7, 1) R(true, 7, 1) R(false, 26, 1) R(true, 26, 1) R(false, 27, 1)
#define NDT_POSE_SCORE_ARGS_T (const float*, size_t, const GridDesc*, const BitWord*, const VoxelRec*, const float*, const PoseItem*, const int*, const PoseSeg*, int, \
                               long long, const float*, double*, SweepConst)
// the translation units split these rows by ORD as they split the table's (NDT_IF_ROW_IN_TU)
#define NDT_POSE_SCORE_ROW_OF_TU(PCA, K, ORD) NDT_IF_ROW_IN_TU(NDT_TU, ORD)(NDT_TU_X __global__ void k_pose_scores<PCA, K, ORD> NDT_POSE_SCORE_ARGS_T;)
#define NDT_POSE_SCORE_KERNELS_OF_TU NDT_POSE_SCORE_ROWS(NDT_POSE_SCORE_ROW_OF_TU)

// Waves per SIMD the kernel is register-allocated for.  A score-only item carries one f64 lane sum where k_sweep carries 43, and no second batch
// in flight (eval_score runs the prefetch hook first); what bounds the occupancy is then the LDS of an item's hit queue, weight queue and
// staged points: 57 KB a workgroup for DIRECT1, 41 / 73 KB for DIRECT7 (ndt_omp / ndt_pca), 21 / 37 KB for the 26- and 27-cell searches, of
// 160 KB a CU.  The bound asked of the register allocator is what that LDS admits, four at the most; the launch is sized by the runtime's
// occupancy answer (DESIGN.md 8 has every instantiation's registers and LDS).
static constexpr int pose_score_wpe(bool pca, int K) { return K == 1 ? 2 : (K == 7 ? (pca ? 2 : 3) : 4); }
template <bool PCA, int K>
struct PoseScoreTune { static constexpr int WPE = pose_score_wpe(PCA, K); };

// Work item w of the call's flat order belongs to the segment s with segs[s].work0 <= w < segs[s + 1].work0; inside it the rows go round the
// segment's items -- w - work0 = row * count + item -- so that waves side by side move the same 512 points by different poses.  XCD x (workgroup
// L runs on XCD L % 8) takes the x-th eighth of the order, its waves statically: with eight pairs of one size or more a pair's clouds and
// grid are read through one L2 as in k_sweep; with fewer pairs than XCDs a pair is shared by neighbouring XCDs, none of which idles.  Which wave
// runs a work item is no part of its row.  No atomics, no control block: nothing to clear between calls.
template <bool PCA, int K, int ORD>
__global__ void __launch_bounds__(SWEEP_THREADS, (PoseScoreTune<PCA, K>::WPE))
k_pose_scores(const float* __restrict__ src, size_t pitch, const GridDesc* __restrict__ gd, const BitWord* __restrict__ words,
              const VoxelRec* __restrict__ recs, const float* __restrict__ cent, const PoseItem* __restrict__ items, const int* __restrict__ order,
              const PoseSeg* __restrict__ segs, int n_segs, long long total_work, const float* __restrict__ poses, double* rows, SweepConst sc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __shared__ double exp_tab[64];                   // 2^(j/64) for ndtm::exp_f32arg
  if (threadIdx.x < 64) exp_tab[threadIdx.x] = ndtm::c_exp2_64[threadIdx.x];
  __syncthreads();                                 // (the only block barrier of the kernel: the four waves are independent from here on)
  const int xcd = blockIdx.x & 7;
  const int xw = (int)(gridDim.x >> 3) * WAVES;                            // waves per XCD (the grid is a multiple of 8)
  const int wx = __builtin_amdgcn_readfirstlane((int)(blockIdx.x >> 3) * WAVES + wv);
  const long long lo = total_work * xcd / 8, hi = total_work * (xcd + 1) / 8;
  Timeline tl;
  int s = 0;
#pragma unroll 1
  for (long long w = lo + wx; w < hi; w += xw) {
    while (s + 1 < n_segs && w >= segs[s + 1].work0) s++;                  // (wave-uniform; a wave's work indices ascend)
    const PoseSeg sg = segs[s];
    const long long local = w - sg.work0;
    const int r = (int)(local / sg.count);
    const int e = order[sg.first + (int)(local % sg.count)];
    const PoseItem it = items[e];
    // the pose words are wave-uniform: lane k loads word k once per work item, sweep_item reads them with v_readlane into scalar registers
    // (the nine words of Rj that follow them in a PairState are not needed for a score: 0)
    unsigned pose_w = 0;
    if (lane < POSE_WORDS) pose_w = __float_as_uint(poses[(size_t)e * POSE_WORDS + lane]);
    // (rows_per_pair = 0: the row of work item `r` is rows + it.row0 + r * NACC whatever the pair's slot)
    sweep_item<PCA, K, SWEEP_IT_BATCH, false, ORD, true, true>(it.pair, r, src, pitch, nullptr, gd, words, recs, rows + it.row0, 0, sc, cent, nullptr, exp_tab,
                                                               pose_w, it.n, it.grid, tl);
  }
}

// One block per item: the item's rows through the row tree the update uses, the two live columns alone.
NDT_KERNEL void __launch_bounds__(UPD_THREADS)
k_pose_score_rows(const PoseItem* __restrict__ items, const double* __restrict__ rows, double* __restrict__ scores, long long* __restrict__ hits) {
  __shared__ double sm[UPD_WAVES][NACC];
  const PoseItem it = items[blockIdx.x];
  const int lane = threadIdx.x & 63;
  const int nchunks = (it.n + CHUNK_PTS - 1) / CHUNK_PTS;
  const double v = reduce_pair_rows<false>(rows + it.row0, nchunks, sums_live(lane, false, true), sm);
  if (threadIdx.x == COL_SCORE) scores[blockIdx.x] = v;
  if (threadIdx.x == COL_HITS) hits[blockIdx.x] = (long long)v;
}
