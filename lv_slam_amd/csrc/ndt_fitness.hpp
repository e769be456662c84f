// ndt_fitness.hpp -- getFitnessScore(max_range) for the loop-closure caller.
#pragma once
#include "ndt_types.hpp"
#include "ndt_fit_items.hpp"

// ------------------------------------------------------------------------------------ fitness score (loop-closure caller)
// pcl::Registration::getFitnessScore(max_range) as used by include/global_graph/loop_detector.hpp:249-262, same recipe as
// the in-tree InformationMatrixCalculator::calc_fitness_score (src/global_graph/information_matrix_calculator.cpp:53-87):
// move the source by the final pose (f32), exact nearest target point per source point, and average the SQUARED
// distances that are <= max_range (the comparison really is squared distance vs max_range in the reference).
// Three surfaces serve it -- one pair (mi355ndt_fitness_score_T, the B = 1 case of the batch), a batch (mi355ndt_batch_fitness_scores),
// edges between resident keyframes (ndt_kffitness.hpp) -- and everything a score is made of is stated once, here:
//   fit_query         a source point moved by the transform, and whether it counts
//   fit_d2            the squared distance to a target point
//   fit_rings         the exact 1-NN over an occupied-cell index: cells are visited ring by ring around the query's cell and the search stops
//                     once the best distance cannot be beaten by an unvisited ring (fit_ring_max: the rings that cover sqrt(max_range))
//   fit_ring_block    one 256-point block of queries through fit_rings; the two index layouts differ in the point accessor only
//   fit_tiles         the exhaustive walk over a cloud without a lattice, through LDS tiles (also ndt_outlier.hpp, ndt_gicp.hpp)
//   fitness_brute_block   one 256-point block of queries through fit_tiles, for a target without a grid
//   fit_block_score   the `best <= max_range` tail and the deterministic block reduction every block ends with
// so a pair's block partials are the same words whichever surface made them.

// deterministic block reduction of the 256 lanes' (squared distance, inlier) terms: shuffle-xor inside each wave, then the four wave sums
// in wave order; out[0] = sum, out[1] = count.
__device__ __forceinline__ void fit_block_reduce(double sum, unsigned long long cnt, double* out) {
  for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o); cnt += __shfl_xor(cnt, o); }
  __shared__ double rs[4];
  __shared__ unsigned long long rc[4];
  if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = sum; rc[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = ((rs[0] + rs[1]) + rs[2]) + rs[3];
    out[1] = (double)(rc[0] + rc[1] + rc[2] + rc[3]);
  }
}

// a lane's term -- `best` = the squared distance of its query's nearest target point, live = it has a query -- and the block's reduction
__device__ __forceinline__ void fit_block_score(bool live, float best, float max_range, double* out) {
  double sum = 0.0;
  unsigned long long cnt = 0;
  if (live && best <= max_range) { sum = (double)best; cnt = 1; }
  fit_block_reduce(sum, cnt, out);
}

// query i of the source rows: the point moved by the column-major transform; false (q = 0) past the end of the cloud or when not finite
__device__ __forceinline__ bool fit_query(const float* __restrict__ src, size_t spitch, int n_src, int i, const float* __restrict__ Tcm, float (&q)[3]) {
  q[0] = q[1] = q[2] = 0.f;
  if (i >= n_src) return false;
  const float px = src[i], py = src[spitch + i], pz = src[2 * spitch + i];
#pragma unroll
  for (int a = 0; a < 3; a++) q[a] = ((Tcm[0 * 4 + a] * px + Tcm[1 * 4 + a] * py) + Tcm[2 * 4 + a] * pz) + Tcm[3 * 4 + a];   // PCL 1.8 scalar form
  return finite3(q[0], q[1], q[2]);
}

// squared distance from the query to (x, y, z)
__device__ __forceinline__ float fit_d2(const float (&q)[3], float x, float y, float z) {
  const float dx = q[0] - x, dy = q[1] - y, dz = q[2] - z;
  return (dx * dx + dy * dy) + dz * dz;                                            // FLANN L2_Simple accumulation order
}

// rings needed to cover sqrt(max_range) (+1 cell of slack).  A query outside the grid may sit further away than the grid is wide:
// fit_rings clamps its cell to 2^29 cells from the grid's origin, so 2^30 rings reach every target cell from anywhere.
__host__ __device__ inline int fit_ring_max(double max_range, float leaf) {
  const double rr = sqrt(max_range < 1e30 ? max_range : 1e30) / (double)leaf + 2.0;
  return rr > (double)(1 << 30) ? (1 << 30) : (int)rr;
}

// The exhaustive walk over a cloud that has no lattice to search (GRID_OVERFLOW, GRID_CAP: a stray point at 1e12 m): the rows staged through
// LDS 256 points at a time, visit(x, y, z, id) for every finite point (a non-finite one is in no tree), id = its input position.  The WHOLE
// workgroup of BLOCK threads calls it (256, or one wave: OL_LANES); a lane without a live query masks itself inside `visit`.
template <int BLOCK, typename Visit>
__device__ __forceinline__ void fit_tiles(const float* __restrict__ rows, size_t pitch, int n, Visit visit) {
  __shared__ float tx[256], ty[256], tz[256];
  constexpr int U = 256 / BLOCK;
  for (int j0 = 0; j0 < n; j0 += 256) {
    float x[U], y[U], z[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int j = j0 + u * BLOCK + (int)threadIdx.x;
      x[u] = y[u] = z[u] = __int_as_float(0x7fc00000);                             // past the end: NaN, skipped below
      if (j < n) { x[u] = rows[j]; y[u] = rows[pitch + j]; z[u] = rows[2 * pitch + j]; }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; u++) { const int k = u * BLOCK + (int)threadIdx.x; tx[k] = x[u]; ty[k] = y[u]; tz[k] = z[u]; }
    __syncthreads();
    for (int k = 0; k < 256; k++)
      if (finite3(tx[k], ty[k], tz[k])) visit(tx[k], ty[k], tz[k], (unsigned)(j0 + k));
  }
}

// The score for a target that has no voxel grid -- pcl::Registration::getFitnessScore searches a kd-tree over the target CLOUD and does not
// care.  (block `blk` of one pair: source points blk * 256 .. blk * 256 + 255)
__device__ __forceinline__ void fitness_brute_block(const float* __restrict__ src, size_t spitch, int n_src,
                                                    const float* __restrict__ tgt, size_t tpitch, int n_tgt,
                                                    const float* __restrict__ Tcm, float max_range, int blk, double* out) {
  float q[3];
  const bool live = fit_query(src, spitch, n_src, blk * 256 + threadIdx.x, Tcm, q);
  float best = __int_as_float(0x7f800000);
  fit_tiles<256>(tgt, tpitch, n_tgt, [&](float x, float y, float z, unsigned) {
    if (!live) return;
    const float d2 = fit_d2(q, x, y, z);
    best = d2 < best ? d2 : best;
  });
  fit_block_score(live, best, max_range, out);
}


// ------------------------------------------------------------------------------------ the occupied-cell index
// A dense first / last position per grid cell would cost 8 B per cell, gigabytes over a batch.  The search reads an index of the OCCUPIED
// cells instead, built by the first fitness call after a target build, in pools of its own:
//   words[gd.word_off + w]   (BitWord, the NDT bitmap's layout and offsets, not its pool): occupancy of cells 64w .. 64w + 63 -- every cell
//                            holding a target point, whatever min_points says -- and `prefix` = occupied cells before them (rank);
//   runs[b * (pitch + 1) + k]: sorted position (d_vals_b segment) of the first point of the pair's k-th occupied cell; runs[n_occ] = the
//                            number of binned points.
// Cells are sorted by linear index, so the occupied cells of a cell range [a, e) are ranks rank(a) .. rank(e) - 1 and their points the
// sorted positions runs[rank(a)] .. runs[rank(e)] - 1: one row of a ring face costs two word reads however long it is.
__device__ __forceinline__ unsigned fit_rank(const BitWord* __restrict__ W, unsigned c) {
  const BitWord w = W[c >> 6];
  return w.prefix + (unsigned)__popcll(w.bits & ((1ull << (c & 63)) - 1ull));
}

// occupancy bits: every run head of a pair's sorted segment sets its cell's bit.  The lanes of a wave hold ascending cells, so the lanes
// that share a word are contiguous: a segmented OR across them leaves one atomicOr per (wave, word) instead of one per cell.
__global__ void __launch_bounds__(256) k_fit_mark(const unsigned* __restrict__ keys, size_t pitch, const GridDesc* __restrict__ gd, BitWord* words, int cb) {
  const int b = blockIdx.y;
  if (gd[b].status != GRID_OK) return;
  const unsigned cmask = (1u << cb) - 1u;
  const unsigned* K = keys + (size_t)b * pitch;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  unsigned cell = cmask;
  bool head = false;
  if (i < pitch) {
    cell = K[i] & cmask;
    head = cell != cmask && (i == 0 || (K[i - 1] & cmask) != cell);
  }
  const unsigned w = cell >> 6;                   // (not binned: cmask >> 6, at or above every real word, and no bit)
  unsigned long long bits = head ? 1ull << (cell & 63) : 0ull;
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long vb = __shfl_down(bits, o);
    const unsigned vw = __shfl_down(w, o);
    if (lane + o < 64 && vw == w) bits |= vb;
  }
  const unsigned wp = __shfl_up(w, 1);
  if (bits && (lane == 0 || wp != w)) atomicOr(&words[gd[b].word_off + w].bits, bits);
}

// rank of every word: exclusive popcount prefix over the pair's words (one block per pair; the trailing all-zero word gets n_occ)
__global__ void __launch_bounds__(1024) k_fit_rank(const GridDesc* __restrict__ gd, BitWord* words) {
  __shared__ unsigned sm[17];
  const int b = blockIdx.x;
  if (gd[b].status != GRID_OK) return;
  BitWord* W = words + gd[b].word_off;
  const int nw = gd[b].nwords;
  unsigned base = 0;
  for (int w0 = 0; w0 < nw; w0 += 1024) {
    const int w = w0 + threadIdx.x;
    const unsigned c = w < nw ? (unsigned)__popcll(W[w].bits) : 0u;
    unsigned tot;
    const unsigned ex = block_exscan<1024>(c, &tot, sm);
    if (w < nw) W[w].prefix = base + ex;
    base += tot;
  }
}

// run starts by rank; the end of the last run closes the table
__global__ void __launch_bounds__(256) k_fit_runs(const unsigned* __restrict__ keys, size_t pitch, const GridDesc* __restrict__ gd,
                                                  const BitWord* __restrict__ words, unsigned* runs, int cb) {
  const int b = blockIdx.y;
  if (gd[b].status != GRID_OK) return;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= pitch) return;
  const unsigned cmask = (1u << cb) - 1u;
  const unsigned* K = keys + (size_t)b * pitch;
  const unsigned cell = K[i] & cmask;
  if (cell == cmask) return;
  const bool head = i == 0 || (K[i - 1] & cmask) != cell;
  const bool last = i + 1 == pitch || (K[i + 1] & cmask) == cmask;
  if (!head && !last) return;
  const unsigned k = fit_rank(words + gd[b].word_off, cell);
  unsigned* R = runs + (size_t)b * (pitch + 1);
  if (head) R[k] = (unsigned)i;
  if (last) R[k + 1] = (unsigned)i + 1u;
}

// One item of a launch: `count` consecutive blocks of one scored pair, from the pair's block `first` on -- the whole pair unless the launch is
// so small that a pair is cut to spread over the XCDs (fit_item_table, ndt_fit_items.hpp).  The launch is a flat grid over (item, 256-point
// block): workgroup L serves group g = L % 8 (the workgroups that share an XCD, cdna_hip_programming.md 5.5 T1) and the (L / 8)-th block
// of that group's items, which are listed back to back (block0 = the item's first block within its group).  A pair's blocks therefore
// share one XCD's L2 with its target points and index.  part0 = the pair's first partial slot; the host sums a pair's partials in block order.
struct FitItem { int pair, block0, part0, n_src, n_tgt, ring_max, first, count; };
static_assert(sizeof(FitItem) == FIT_ITEM_INTS * sizeof(int), "the table's layout");

// this workgroup's item and bx = its block within the PAIR; false: the workgroup is past its group's last block
__device__ __forceinline__ bool fit_item(const FitItem* __restrict__ items, const int* __restrict__ gstart, FitItem& it, int& bx) {
  const int g = blockIdx.x & 7, s = blockIdx.x >> 3;
  int lo = gstart[g], hi = gstart[g + 1];
  if (lo >= hi) return false;
  while (hi - lo > 1) {                           // last item of the group with block0 <= s
    const int mid = (lo + hi) >> 1;
    if (items[mid].block0 <= s) lo = mid; else hi = mid;
  }
  it = items[lo];
  bx = it.first + (s - it.block0);
  return s - it.block0 < it.count;
}

// The ring walk over an occupied-cell index: the query's cell, the rings r_first .. r_last around it, the stopping rule.  visit(j0, j1)
// takes the sorted positions j0 .. j1 - 1 of one row's (or one cell's) points and lowers `best`, the squared distance of the nearest point
// so far, which the walk reads to stop.  Shared by fit_ring_block (k_fitness_batch, k_kf_fitness), knn_fill (ndt_outlier.hpp) and k_gc_match (ndt_gicp.hpp).
// The query's cell is taken relative to the grid and clamped to +-2^29 cells: a query further out than that (a stray source point at
// 1e12 m) still sees every target cell in rings r_first .. r_first + extent, and (r - 1) * leaf stays a lower bound of its distances.
// r_first = the distance from the query's cell to the grid box in cells (0 inside): rings closer than that are empty.  Every point in
// ring >= r lies more than (r - 1) * leaf away (`reach`, with 0.1 % of a cell of slack for the binning's rounding).
template <typename Visit>
__device__ __forceinline__ void fit_rings(const float (&q)[3], const GridDesc& g, const BitWord* __restrict__ W, const unsigned* __restrict__ R,
                                          const int ring_max, const float max_range, const float& best, Visit visit) {
  int cq[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float cf = floorf(q[a] * g.inv_leaf);
    const long long ci = cf >= 1.0e9f ? 1000000000ll : (cf <= -1.0e9f ? -1000000000ll : (long long)cf);
    const long long cl = ci - (long long)g.min_b[a];
    cq[a] = (int)(cl > (1ll << 29) ? (1ll << 29) : (cl < -(1ll << 29) ? -(1ll << 29) : cl));
  }
  const int c0 = cq[0], c1 = cq[1], c2 = cq[2];
  const int o0 = c0 < 0 ? -c0 : (c0 >= g.div_b[0] ? c0 - g.div_b[0] + 1 : 0);
  const int o1 = c1 < 0 ? -c1 : (c1 >= g.div_b[1] ? c1 - g.div_b[1] + 1 : 0);
  const int o2 = c2 < 0 ? -c2 : (c2 >= g.div_b[2] ? c2 - g.div_b[2] + 1 : 0);
  const int r_first = max(o0, max(o1, o2));
  const int r_last = min(ring_max, r_first + max(g.div_b[0], max(g.div_b[1], g.div_b[2])) + 1);
  for (int r = r_first; r <= r_last; r++) {
    const float reach = ((float)(r - 1) - 1e-3f) * g.leaf;
    if (r > 1 && (best <= reach * reach || reach * reach > max_range)) break;
    const int z0 = max(c2 - r, 0), z1 = min(c2 + r, g.div_b[2] - 1);
    const int y0 = max(c1 - r, 0), y1 = min(c1 + r, g.div_b[1] - 1);
    const int x0 = max(c0 - r, 0), x1 = min(c0 + r, g.div_b[0] - 1);
    if (x0 > x1) continue;                    // (the ring misses the grid's x extent)
    for (int z = z0; z <= z1; z++) {
      const bool zface = (z == c2 - r || z == c2 + r);
      for (int y = y0; y <= y1; y++) {
        const bool yface = (y == c1 - r || y == c1 + r);
        const unsigned row = (unsigned)(y * g.mul1 + z * g.mul2);
        if (zface || yface) {                 // the whole row x0 .. x1: its occupied cells are one rank interval
          const unsigned k0 = fit_rank(W, row + (unsigned)x0), k1 = fit_rank(W, row + (unsigned)x1 + 1u);
          if (k0 != k1) visit(R[k0], R[k1]);
        } else {                              // interior row: the two x faces only
#pragma unroll
          for (int f = 0; f < 2; f++) {
            const int x = f ? c0 + r : c0 - r;
            if (x < x0 || x > x1) continue;
            const unsigned c = row + (unsigned)x;
            const BitWord w = W[c >> 6];
            if ((w.bits >> (c & 63)) & 1ull) {
              const unsigned k = w.prefix + (unsigned)__popcll(w.bits & ((1ull << (c & 63)) - 1ull));
              visit(R[k], R[k + 1]);
            }
          }
        }
      }
    }
  }
}

// One 256-point block of queries against an occupied-cell index: query -> rings -> `best <= max_range` -> block reduction.
// d2_at(q, j) = the squared distance (fit_d2) from q to the point at sorted position j: the one thing the index layouts differ in.
template <typename D2At>
__device__ __forceinline__ void fit_ring_block(const float* __restrict__ src, size_t spitch, int n_src, const float* __restrict__ Tcm,
                                               const GridDesc& g, const BitWord* __restrict__ W, const unsigned* __restrict__ R,
                                               int ring_max, float max_range, int blk, D2At d2_at, double* out) {
  float q[3];
  const bool live = fit_query(src, spitch, n_src, blk * 256 + threadIdx.x, Tcm, q);
  float best = __int_as_float(0x7f800000);
  if (live)
    fit_rings(q, g, W, R, ring_max, max_range, best, [&](unsigned j0, unsigned j1) {
      for (unsigned j = j0; j < j1; j++) {
        const float d2 = d2_at(q, j);
        best = d2 < best ? d2 : best;
      }
    });
  fit_block_score(live, best, max_range, out);
}

// every pair with a grid: the batch's index, the target points by id through `vals`.  The nearest distance is a minimum over a set of
// points, so it does not depend on the order they are visited in.
__global__ void __launch_bounds__(256) k_fitness_batch(const FitItem* __restrict__ items, const int* __restrict__ gstart,
                                                       const float* __restrict__ src, size_t spitch, const float* __restrict__ tgt, size_t tpitch,
                                                       const unsigned* __restrict__ vals, const GridDesc* __restrict__ gd,
                                                       const BitWord* __restrict__ words, const unsigned* __restrict__ runs,
                                                       const float* __restrict__ Tcm, int Tstride, float max_range, double* partial) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const int b = it.pair;
  const GridDesc& g = gd[b];
  const float* X = tgt + (size_t)b * 3 * tpitch;
  const unsigned* V = vals + (size_t)b * tpitch;
  fit_ring_block(src + (size_t)b * 3 * spitch, spitch, it.n_src, Tcm + (size_t)b * Tstride, g, words + g.word_off, runs + (size_t)b * (tpitch + 1),
                 it.ring_max, max_range, bx, [=](const float (&q)[3], unsigned j) {
                   const unsigned pi = V[j];
                   return fit_d2(q, X[pi], X[tpitch + pi], X[2 * tpitch + pi]);
                 }, partial + 2 * ((size_t)it.part0 + bx));
}

// the pairs without a grid (GRID_OVERFLOW / GRID_CAP), in a launch of their own
__global__ void __launch_bounds__(256) k_fitness_brute_batch(const FitItem* __restrict__ items, const int* __restrict__ gstart,
                                                             const float* __restrict__ src, size_t spitch, const float* __restrict__ tgt, size_t tpitch,
                                                             const float* __restrict__ Tcm, int Tstride, float max_range, double* partial) {
  FitItem it;
  int bx;
  if (!fit_item(items, gstart, it, bx)) return;
  const int b = it.pair;
  fitness_brute_block(src + (size_t)b * 3 * spitch, spitch, it.n_src, tgt + (size_t)b * 3 * tpitch, tpitch, it.n_tgt,
                      Tcm + (size_t)b * Tstride, max_range, bx, partial + 2 * ((size_t)it.part0 + bx));
}
