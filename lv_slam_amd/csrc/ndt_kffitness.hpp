// ndt_kffitness.hpp -- the spatial index over a resident cloud, and the fitness scores of graph edges between resident keyframes
// (mi355ndt_keyframe_fitness_scores): InformationMatrixCalculator::calc_fitness_score
// (src/global_graph/information_matrix_calculator.cpp:53-87) for E edges in one launch.
//
// A cloud that is searched -- a keyframe by the fitness scores or by GICP, a GICP host cloud, the prefilter result by the outlier removal --
// owns ONE index (CloudIndex, ndt_engine.hpp), built by whichever surface searches it first (kfi_build_rows, ndt_host_kffitness.hpp) and, for
// a keyframe, kept until it is released: one block of device memory holding
//   KfiHead            the cell lattice over the cloud's finite points (k_kfi_grid: the cell rule below; status != GRID_OK = no lattice) and
//                      the number of searchable points (three finite coordinates), in 128 bytes
//   BitWord words[]    occupancy of 64 cells + rank of the first, the layout k_fit_mark / k_fit_rank write and fit_rank reads (ndt_fitness.hpp)
//   unsigned runs[]    sorted position of the first point of the k-th occupied cell; runs[n_occ] = number of binned points
//   float sorted[3][pitch]  x, y, z of the points IN CELL ORDER: a row of a ring face is one contiguous run of floats per coordinate, where
//                      the batch surface gathers every point through its id (the index lives as long as the cloud; the copy pays once)
//   unsigned ids[pitch]     the input position of the point at each sorted position (the k-NN lists' and GICP's (d2, id) tie rules; results by id)
// The kernels take it as a KfiView, made by kfi_view (ndt_host_kffitness.hpp) and by nothing else.
// No NDT leaves: no sums, no eigen decomposition, no inverse covariances.  The build reuses the engine's kernels as they are -- k_minmax
// (ordered-int extremes), the segmented radix sort whose first pass computes the cell keys from the points (rs_pass), k_fit_mark / k_fit_rank /
// k_fit_runs -- on a one-target "batch".
//
// The fitness search is the batch surface's block of queries (fit_ring_block, ndt_fitness.hpp) with the points read in cell order instead of
// by id.  It is exact for any cell size (fit_rings: ring by ring, stop when no unvisited ring can beat the best or be within max_range), so
// the cell rule is about speed only: start from MI355NDT_OPT_KF_FITNESS_CELL_MM and double the cell until the lattice has at most
// `max_cells` cells; a cloud that does not get there within KFI_MAX_DOUBLINGS doublings (a stray point at 1e12 m) has no lattice and is
// searched exhaustively over its unsorted rows (fit_tiles).
#pragma once
#include "ndt_types.hpp"
#include "ndt_build.hpp"
#include "ndt_fitness.hpp"

#define KFI_CELL_BITS      22            // key field of the index build's sort: every cell index + the all-ones "not binned" value
#define KFI_MAX_CELLS      (1 << 21)     // cap of a keyframe's lattice (32,770 BitWords = 512 KB at the cap)
#define KFI_MAX_DOUBLINGS  6             // the cell is coarsened up to 64 x the option's size before the keyframe counts as not indexable
static_assert(KFI_MAX_CELLS < (1 << KFI_CELL_BITS) - 1, "the all-ones key is no cell");

// extremes cleared (k_minmax's all-zero "no finite point yet"), the point count where k_minmax and the sort's key pass read it
__global__ void k_kfi_begin(unsigned* mm, int* cnt, int n) {
  if (threadIdx.x < 6) mm[threadIdx.x] = 0u;
  if (threadIdx.x == 6) *cnt = n;
}

// the block's header: the lattice, then the cloud's searchable points (k_kfi_gather counts them at the end of the build)
struct KfiHead { GridDesc gd; int n_fin; };
static_assert(offsetof(KfiHead, gd) == 0 && sizeof(KfiHead) <= 128, "the index block's header");

// One cloud's index as the kernels take it (kfi_view, ndt_host_kffitness.hpp): the block's parts, then the cloud's own rows
// ([3][pitch], n points, input order), which the exhaustive walk reads when there is no lattice.
struct KfiView {
  const GridDesc* gd; const BitWord* words; const unsigned* runs; const float* sorted; const unsigned* ids;
  const float* rows; unsigned pitch; int n;
  __device__ __forceinline__ int n_fin() const { return reinterpret_cast<const KfiHead*>(gd)->n_fin; }
};

// the cell rule over one cloud's six extreme words (k_kfi_grid below; k_olb_grid for K clouds at once, ndt_outlier_batch.hpp)
__device__ __forceinline__ GridDesc kfi_cell_rule(const unsigned* __restrict__ mm, float cell0, int max_cells) {
  GridDesc g;
  memset(&g, 0, sizeof g);
  g.leaf = cell0;
  g.inv_leaf = 1.0f / cell0;
  if (mm[0] == 0u) {
    g.status = GRID_EMPTY;
  } else {
    float mn[3], mx[3];
    for (int a = 0; a < 3; a++) { mn[a] = ord2f(mm_dec_min(mm[a])); mx[a] = ord2f(mm_dec_max(mm[3 + a])); }
    g.status = GRID_CAP;
    float leaf = cell0;
    for (int k = 0; k <= KFI_MAX_DOUBLINGS; k++, leaf *= 2.0f) {
      const float inv = 1.0f / leaf;
      if (grid_too_big((mx[0] - mn[0]) * inv, (mx[1] - mn[1]) * inv, (mx[2] - mn[2]) * inv)) continue;
      int lo[3], hi[3];
      for (int a = 0; a < 3; a++) { lo[a] = (int)floorf(mn[a] * inv); hi[a] = (int)floorf(mx[a] * inv); }
      const long long nc = (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
      if (nc > (long long)max_cells) continue;
      for (int a = 0; a < 3; a++) { g.min_b[a] = lo[a]; g.max_b[a] = hi[a]; g.div_b[a] = hi[a] - lo[a] + 1; }
      g.leaf = leaf; g.inv_leaf = inv;
      g.mul1 = g.div_b[0];
      g.mul2 = g.div_b[0] * g.div_b[1];
      g.ncells = (int)nc;
      g.nwords = (int)((nc + 63) >> 6) + 1;       // + one all-zero word, as the target grids have (k_fit_rank leaves n_occ in it)
      g.status = GRID_OK;
      break;
    }
  }
  return g;
}
// ... for one cloud; stat_out[0] = the status, for the host (two words per index built in a call, fetched with the call's results; the
// second: the searchable points, cleared here for k_kfi_gather)
__global__ void k_kfi_grid(const unsigned* __restrict__ mm, float cell0, int max_cells, KfiHead* head, int* stat_out) {
  const GridDesc g = kfi_cell_rule(mm, cell0, max_cells);
  head->gd = g;
  stat_out[0] = g.status;
  stat_out[1] = 0;
}

// the points and their ids in cell order (positions past the binned points hold the not-binned points and the padding: never read,
// runs[n_occ] ends the last run).  vals is a permutation of 0 .. pitch - 1 whatever the lattice's status, so every point passes here once:
// the searchable ones are counted, one integer atomic per block into the header (zeroed by the host) and one into the host's word.
__global__ void __launch_bounds__(256) k_kfi_gather(const float* __restrict__ rows, size_t pitch, int n, const unsigned* __restrict__ vals,
                                                    float* __restrict__ sorted, unsigned* __restrict__ ids, KfiHead* head, int* stat_out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  bool fin = false;
  if (i < pitch) {
    const unsigned v = vals[i];
    const float x = rows[v], y = rows[pitch + v], z = rows[2 * pitch + v];
    ids[i] = v;
    sorted[i] = x; sorted[pitch + i] = y; sorted[2 * pitch + i] = z;
    fin = v < (unsigned)n && finite3(x, y, z);
  }
  const int c = __syncthreads_count(fin);
  if (threadIdx.x == 0 && c) { atomicAdd(&head->n_fin, c); atomicAdd(stat_out + 1, c); }
}

// One scored edge.  src: the rows of keyframe ids2[e] (moved by T); tgt: keyframe ids1[e], the searched side.
struct KfEdge {
  const float* src;
  KfiView tgt;
  float T[16];                                    // relpose.cast<float>(), column-major
  unsigned spitch;
};

// The launch is k_fitness_batch's: a flat grid over (edge, 256-point block) items, workgroup L serving group L % 8 -- the workgroups of one
// XCD -- so that an edge's blocks share one L2 with its index and its cloud1 points (FitItem / fit_item, ndt_fitness.hpp; .pair = the edge).
// The block body is k_fitness_batch's too (fit_ring_block); only the point accessor differs, contiguous in cell order here.  An edge's
// partials are therefore those of a one-pair engine, because the nearest distance is a minimum over the same points whatever the lattice and
// the visiting order.  The lattice's cell size is known on the device only (the index may be built by this call): ring_max is taken here.
// An edge whose searched keyframe has no lattice leaves its partials to k_kf_fitness_brute.
__global__ void __launch_bounds__(256) k_kf_fitness(const FitItem* __restrict__ items, const int* __restrict__ gstart, const KfEdge* __restrict__ edges,
                                                    float max_range, double max_range_d, double* partial) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const KfEdge& e = edges[it.pair];
  const GridDesc& g = *e.tgt.gd;
  if (g.status != GRID_OK) return;
  const float* X = e.tgt.sorted;
  const size_t tpitch = e.tgt.pitch;
  fit_ring_block(e.src, e.spitch, it.n_src, e.T, g, e.tgt.words, e.tgt.runs, fit_ring_max(max_range_d, g.leaf), max_range, bx,
                 [=](const float (&q)[3], unsigned j) { return fit_d2(q, X[j], X[tpitch + j], X[2 * tpitch + j]); },
                 partial + 2 * ((size_t)it.part0 + bx));
}

// the edges whose searched keyframe has no lattice, in a launch of their own (a keyframe without a finite point: no target point at all)
__global__ void __launch_bounds__(256) k_kf_fitness_brute(const FitItem* __restrict__ items, const int* __restrict__ gstart, const KfEdge* __restrict__ edges,
                                                          float max_range, double* partial) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const KfEdge& e = edges[it.pair];
  const int status = e.tgt.gd->status;
  if (status == GRID_OK) return;
  fitness_brute_block(e.src, e.spitch, it.n_src, e.tgt.rows, e.tgt.pitch, status == GRID_EMPTY ? 0 : it.n_tgt, e.T, max_range, bx,
                      partial + 2 * ((size_t)it.part0 + bx));
}
