// ndt_icp.hpp -- the device stages of pcl::IterativeClosestPoint as the loop-closure factory sets it up for registration_method = ICP
// (src/global_graph/registrations.cpp:21-29): point-to-point ICP, correspondences by the nearest target point, the rigid estimate by
// TransformationEstimationSVD.  PCL itself is restated from memory (parity unpinned); tools/icp_ref.py restates all of it.
// One iteration is one device round trip: the host (icp_outer.hpp, ndt_host_icp.hpp) runs the 3x3 SVD and the convergence criteria.
//
// 1. k_icp_step -- one iteration's device half, lane i = point i of the working cloud W (the surface's or the slot's own buffer: a keyframe
//    source is never written).  `moves` f32 products in front of the search, each coordinate ((a*x + b*y) + c*z) + d:
//      2: W[i] = T (G in[i])       mi355ndt_icp_correspondences: a fresh working cloud from the source rows
//      1: W[i] = T in[i]           the align: the first launch moves the source rows by the guess, launch k + 1 moves W (in = W) by the
//                                  transformation iteration k estimated -- the move is fused into the next matching, W is cumulative
//      0: W as it is
//    then the exact 1-NN of W[i] over the target's one index: fit_rings over the lattice (GRID_OK) with `range` = the f32 just above
//    corr_dist_threshold^2 (+inf for the default), fit_tiles over the rows when the lattice gave GRID_CAP.  What the engine fixes:
//      * a tie goes to the lower point id (gc_nearer; PCL's kd-tree order is not observable);
//      * d2 = (dx*dx + dy*dy) + dz*dz in f32 (fit_d2);
//      * kept iff (double)d2 <= corr_dist_threshold^2 (PCL discards on >);
//      * a point that is not finite, or whose moved copy is not finite, matches nothing.
//    idx[i] = the target id or -1, d2[i] = the squared distance (0 where unmatched), *m += matches (an integer atomic per wave).  Sixteen
//    f64 terms per matched lane, f64 products of the f32 coordinates, p = W[i], q = the target point:
//      [0..2] p   [3..5] q   [6 + 3 r + c] q_r * p_c   [15] d2
//    (Eigen's own centroid and covariance sums are f32 and vectorised in an order nobody can observe) into the fixed tree of ndt_gicp.hpp
//    (gc_chunk_tree<16>): 256 points per chunk, 64 lanes by shuffle-xor, four wave sums in wave order.
// 2. k_icp_final -- gc_slot_tree<16> over the chunks' partials (chunk c into slot c % 256, the slots by halving) into the record in mapped
//    host memory: 16 sums, m; the match counter is cleared for the next step.  No float atomics anywhere.
// 3. k_icp_step_batch / k_icp_final_batch -- the same two bodies for every slot of mi355ndt_icp_batch_align that has not ended, one launch
//    each: one table in device memory, a workgroup belongs to one slot, found by bisection over the slots' first chunks (k_gc_match_batch).
#pragma once
#include "ndt_gicp.hpp"

#define ICP_SUMS 16
#define ICP_REC  18                      // doubles of the result record: 16 sums, m, one spare

struct IcpStep {
  float G[16], T[16];                              // column-major; moves = 2: G then T, 1: T
  double thr2;                                     // corr_dist_threshold^2 (inf when it overflows)
  float range;                                     // nothing further than this (the f32 just above thr2) can match: the ring walk may stop there
  int moves;
};

__device__ __forceinline__ void icp_move(const float* M, float (&q)[3]) {
  const float x = q[0], y = q[1], z = q[2];
#pragma unroll
  for (int r = 0; r < 3; r++) q[r] = ((M[0 * 4 + r] * x + M[1 * 4 + r] * y) + M[2 * 4 + r] * z) + M[3 * 4 + r];
}

// the per-thread body of the step kernels: points chunk * 256 .. + 255 of one working cloud.  The WHOLE workgroup calls it (fit_tiles, the
// ballot, the tree); k_icp_step and k_icp_step_batch instantiate this one copy, which is what makes their bytes equal.  `in` may be W.
__device__ __forceinline__ void icp_step_body(const float* in, float* W, size_t pitch, int n, const KfiView& tgt, const IcpStep& a,
                                              int* __restrict__ idx, float* __restrict__ d2, double* __restrict__ part, int* m, int chunk) {
  const GridDesc& g = *tgt.gd;
  const size_t tpitch = tgt.pitch;
  const int i = chunk * GC_CHUNK + threadIdx.x;
  float q[3] = {0.f, 0.f, 0.f};
  bool live = false;
  if (i < n) {
    q[0] = in[i]; q[1] = in[pitch + i]; q[2] = in[2 * pitch + i];
    live = finite3(q[0], q[1], q[2]);
    if (a.moves == 2) icp_move(a.G, q);
    if (a.moves >= 1) {
      icp_move(a.T, q);
      W[i] = q[0]; W[pitch + i] = q[1]; W[2 * pitch + i] = q[2];
    }
    live = live && finite3(q[0], q[1], q[2]);
  }
  float best = __int_as_float(0x7f800000);
  unsigned bid = 0xFFFFFFFFu;
  if (g.status == GRID_OK) {
    const float* X = tgt.sorted;
    const unsigned* ids = tgt.ids;
    if (live)
      fit_rings(q, g, tgt.words, tgt.runs, 1 << 30, a.range, best, [&](unsigned j0, unsigned j1) {
        for (unsigned t = j0; t < j1; t++) gc_nearer(fit_d2(q, X[t], X[tpitch + t], X[2 * tpitch + t]), ids[t], best, bid);
      });
  } else if (g.status == GRID_CAP) {               // no lattice: exhaustive (a target without a finite point: nothing)
    fit_tiles<256>(tgt.rows, tpitch, tgt.n, [&](float x, float y, float z, unsigned t) {
      if (live) gc_nearer(fit_d2(q, x, y, z), t, best, bid);
    });
  }
  const bool matched = live && bid != 0xFFFFFFFFu && (double)best <= a.thr2;
  const unsigned long long b = __ballot(matched);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(m, __popcll(b));
  if (i < n) { idx[i] = matched ? (int)bid : -1; d2[i] = matched ? best : 0.f; }
  double v[ICP_SUMS];
#pragma unroll
  for (int k = 0; k < ICP_SUMS; k++) v[k] = 0.0;
  if (matched) {
    const float* Y = tgt.rows;
    const double t[3] = {(double)Y[bid], (double)Y[tpitch + bid], (double)Y[2 * tpitch + bid]};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      v[r] = (double)q[r];
      v[3 + r] = t[r];
#pragma unroll
      for (int c = 0; c < 3; c++) v[6 + 3 * r + c] = t[r] * (double)q[c];
    }
    v[15] = (double)best;
  }
  gc_chunk_tree<ICP_SUMS>(v, part, chunk);
}

__global__ void __launch_bounds__(GC_CHUNK) k_icp_step(const float* in, float* W, size_t pitch, int n, KfiView tgt, IcpStep a,
                                                       int* __restrict__ idx, float* __restrict__ d2, double* __restrict__ part, int* m) {
  icp_step_body(in, W, pitch, n, tgt, a, idx, d2, part, m, (int)blockIdx.x);
}

// one cloud's chunk partials -> its record: rec[0 .. 15] = the sums, rec[16] = m; the counter is cleared for the next step
__device__ __forceinline__ void icp_final_body(const double* __restrict__ part, int n_chunks, int* m, double* rec) {
  gc_slot_tree<ICP_SUMS>(part, n_chunks, rec);
  if (threadIdx.x == 0) { rec[ICP_SUMS] = (double)*m; rec[ICP_SUMS + 1] = 0.0; *m = 0; }
}

__global__ void __launch_bounds__(256) k_icp_final(const double* __restrict__ part, int n_chunks, int* m, double* rec) {
  icp_final_body(part, n_chunks, m, rec);
}

// ---- the batch round (mi355ndt_icp_batch_align, ndt_host_icp_batch.hpp) ---------------------------------------------------
// every slot has its own W, idx, d2, partials, counter and record; the table is copied in-stream per round
struct IcpSlot {
  const float* in; float* W;                       // the rows this step reads (the slot's source, or W) and the slot's working cloud
  int* idx; float* d2; int* m; double* part;
  double* rec;                                     // the slot's record in mapped host memory (the device's view)
  unsigned pitch; int n, chunk0, n_chunks;         // chunk0: the slot's first workgroup in the step kernel's grid
  IcpStep step;
};

// the entry whose chunks hold workgroup `wg`: the last one with chunk0 <= wg (every entry has at least one chunk)
__device__ __forceinline__ const IcpSlot& icp_slot_of(const IcpSlot* __restrict__ tab, int n, int wg) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].chunk0 <= wg) lo = mid; else hi = mid - 1;
  }
  return tab[lo];
}

__global__ void __launch_bounds__(GC_CHUNK) k_icp_step_batch(const IcpSlot* __restrict__ tab, int n_entries, KfiView tgt) {
  const IcpSlot& e = icp_slot_of(tab, n_entries, (int)blockIdx.x);
  icp_step_body(e.in, e.W, e.pitch, e.n, tgt, e.step, e.idx, e.d2, e.part, e.m, (int)blockIdx.x - e.chunk0);
}

__global__ void __launch_bounds__(256) k_icp_final_batch(const IcpSlot* __restrict__ tab) {
  const IcpSlot& e = tab[blockIdx.x];
  icp_final_body(e.part, e.n_chunks, e.m, e.rec);
}

// the working cloud, moved by the last estimate when one is pending (the align's last move has no matching behind it to be fused into):
// x, y, z records of 12 B
__global__ void __launch_bounds__(256) k_icp_out(const float* __restrict__ W, size_t pitch, int n, IcpStep a, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float q[3] = {W[i], W[pitch + i], W[2 * pitch + i]};
  if (a.moves) icp_move(a.T, q);
#pragma unroll
  for (int r = 0; r < 3; r++) out[3 * (size_t)i + r] = q[r];
}
